"""The shared-activation GEMV for 33 .. 64 rows on wide matrices (awq_repacked_sharedx_wide.hip), forced through
variant=RP_SHARED_X_WIDE, against the oracle's float64 exact sums: every strip width at its raggedest, K edges, ldx > K, bias,
determinism, the refusals and the automatic route."""
import pytest
import torch

from oracle import c_oracle
from sglang_awq_amd import _lib, synth
from tests.util import assert_gemm_close, to_np, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SXW = getattr(_lib, "RP_SHARED_X_WIDE", 2)


@pytest.fixture(scope="module")
def ops():
    from sglang_awq_amd import ops as _ops

    _lib.load()
    return _ops


def _case(ops, M, K, N, g, dt="f16"):
    qw, s, qz = synth.make_awq_weights(K, N, g, dt, "A", seed=M + K + N)
    x = synth.make_activations(M, K, dt, "A", seed=M + K + 1)
    packed = ops.awq_repack(*[to_torch(a, DEV) for a in (qw, s, qz)])
    return qw, s, qz, x, packed


def _check(ops, M, K, N, g, variant=SXW):
    qw, s, qz, x, packed = _case(ops, M, K, N, g)
    y = ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=variant)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    assert_gemm_close(to_np(y), exact, "f16", what=f"shared-x wide M={M} K={K} N={N} g={g}")


# G - 1 full strips and one column group more: the last strip overlaps its neighbour; 11 k-blocks: ragged last chunk
@pytest.mark.parametrize("G", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("M", [33, 48, 49, 64])
def test_every_strip_width_ragged(ops, M, G):
    _check(ops, M, 1408, 4096 * (G - 1) + 16, 128)


# one k-block | exactly one chunk, g = K | both buffers reused, a group spanning k-blocks; at an odd and an even strip width
@pytest.mark.parametrize("K,g", [(128, 128), (512, 512), (2048, 256)])
@pytest.mark.parametrize("N", [8208, 22016])
@pytest.mark.parametrize("M", [33, 64])
def test_k_edges(ops, M, N, K, g):
    _check(ops, M, K, N, g)


@pytest.mark.parametrize("M", [33, 64])
def test_operator_edges(ops, M):
    """x as a column slice of a wider tensor (ldx > K); bias after the rounding; run-to-run identical."""
    K, N, g = 1408, 8208, 128
    _, _, _, x, packed = _case(ops, M, K, N, g)
    dx = to_torch(x, DEV)
    y = ops.awq_gemm_repacked(dx, packed, K, N, g, variant=SXW)
    wide = torch.full((M, K + 264), 7.0, dtype=torch.float16, device=DEV)
    wide[:, 8:8 + K] = dx
    assert torch.equal(ops.awq_gemm_repacked(wide[:, 8:8 + K], packed, K, N, g, variant=SXW), y)
    b = to_torch(synth.make_bias(N, "f16", 3), DEV)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, bias=b, variant=SXW), y + b)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, variant=SXW), y)


@pytest.mark.parametrize("M,N,g,dt", [(32, 8208, 128, "f16"), (65, 8208, 128, "f16"), (33, 4096, 128, "f16"), (33, 8208, 128, "bf16"),
                                      (33, 8208, 64, "f16")])
def test_refuses_outside_its_domain(ops, M, N, g, dt):
    K = 256
    _, _, _, x, packed = _case(ops, M, K, N, g, dt)
    with pytest.raises(_lib.AwqHipError, match=f"status {_lib.ERR_BAD_VARIANT}"):
        ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=SXW)


def test_auto_route_at_33_rows(ops):
    _check(ops, 33, 128, 8208, 128, variant=_lib.RP_AUTO)

"""The shared-activation decode GEMV (awq_repacked_sharedx.hip), forced through variant=RP_SHARED_X, against the oracle's
float64 exact sums: chunk / strip / wave-split edges, the epilogues, the refusals and the automatic route."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from sglang_awq_amd import _lib, synth
from tests.util import assert_gemm_close, to_np, to_torch, ulp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SX = _lib.RP_SHARED_X
SMALL = (1408, 48, 128)


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


# one k-block and one column group | 11 k-blocks: ragged last chunk, G = 1 | NG = 257: G = 2, one-group last strip, g = 256 |
# G = 6, g = K | G = 3 with a ragged last strip, both x buffers reused | 86 k-blocks
@pytest.mark.parametrize("K,N,g", [(128, 16, 128), SMALL, (2048, 4112, 256), (1024, 22016, 1024), (4096, 11008, 128), (11008, 4096, 128)])
@pytest.mark.parametrize("M", [17, 25, 32])
def test_sharedx_vs_exact_sum(ops, M, K, N, g):
    qw, s, qz, x, packed = _case(ops, M, K, N, g)
    y = ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=SX)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    assert_gemm_close(to_np(y), exact, "f16", what=f"shared-x M={M} K={K} N={N} g={g}")


@pytest.mark.parametrize("M", [1, 16, 17, 32])
def test_sharedx_edges_small_shape(ops, M):
    """One row tile (M <= 16) and two; x as a column slice of a wider tensor (ldx > K); bias after the rounding; run-to-run identical."""
    K, N, g = SMALL
    qw, s, qz, x, packed = _case(ops, M, K, N, g)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    dx = to_torch(x, DEV)
    y = ops.awq_gemm_repacked(dx, packed, K, N, g, variant=SX)
    assert_gemm_close(to_np(y), exact, "f16", what=f"shared-x M={M}")
    wide = torch.full((M, K + 264), 7.0, dtype=torch.float16, device=DEV)
    wide[:, 8:8 + K] = dx
    assert torch.equal(ops.awq_gemm_repacked(wide[:, 8:8 + K], packed, K, N, g, variant=SX), y)
    b = to_torch(synth.make_bias(N, "f16", 3), DEV)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, bias=b, variant=SX), y + b)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, variant=SX), y)


@pytest.mark.parametrize("M,g,dt", [(17, 128, "bf16"), (17, 64, "f16"), (33, 128, "f16")])
def test_sharedx_refuses_outside_its_domain(ops, M, g, dt):
    K, N = 256, 64
    _, _, _, x, packed = _case(ops, M, K, N, g, dt)
    with pytest.raises(_lib.AwqHipError, match=f"status {_lib.ERR_BAD_VARIANT}"):
        ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=SX)
    assert _lib.load().awq_gemm_repacked_ex(None, K, None, None, None, None, 0, M, K, N, g, 0, 7, None) == _lib.ERR_BAD_VARIANT


@pytest.mark.parametrize("K,N", [(4096, 2112), (1024, 22016)])
@pytest.mark.parametrize("M", [17, 32])
def test_sharedx_silu_epilogue(ops, M, K, N):
    from sglang_awq_amd import aux_ops

    g = 128
    qw, s, qz = synth.make_awq_weights(K, N, g, "f16", "A", seed=M * 5 + K + N)
    x = synth.make_activations(M, K, "f16", "A", seed=M + K + 2)
    packed_il = ops.awq_repack(*aux_ops.interleave_gate_up(*[to_torch(a, DEV) for a in (qw, s, qz)]))
    r = aux_ops.gemv_repacked_fused(packed_il, K, N, g, x=to_torch(x, DEV), silu_mul=True, variant=SX)
    assert r is not None
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    gu = exact.astype(np.float16)
    gate, up = gu[:, :N // 2].astype(np.float32), gu[:, N // 2:]
    want = ((gate / (1.0 + np.exp(-gate))).astype(np.float16) * up).astype(np.float64)
    got = to_np(r[0]).astype(np.float64)
    tol = 2.0 * ulp(want, "f16") + 2e-3 * (1.0 + np.abs(exact[:, N // 2:]))
    assert got.shape == (M, N // 2) and np.all(np.abs(got - want) <= tol), f"worst {np.abs(got - want).max():.3e}"
    assert float((got != want).mean()) < 0.05


def test_auto_route_at_32_rows(ops):
    M, K, N, g = 32, 4096, 11008, 128
    qw, s, qz, x, packed = _case(ops, M, K, N, g)
    y = ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=_lib.RP_AUTO)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    assert_gemm_close(to_np(y), exact, "f16", what="auto route, 32 rows")

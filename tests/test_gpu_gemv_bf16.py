"""The straight-line bf16 decode GEMV for 1 .. 16 rows (awq_repacked_gemv_bf16.hip), forced through variant=RP_GEMV_BF16: one-hot rows
bit-equal to awq_dequantize, the oracle's float64 exact sums at every strip width and staging-chunk count, K edges (empty and ragged
waves, the one-row long form), ldx > K, bias, determinism, the refusals and the automatic route."""
import pytest
import torch

from oracle import c_oracle
from sglang_awq_amd import _lib, synth
from tests.util import assert_gemm_close, to_np, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RP = getattr(_lib, "RP_GEMV_BF16", 7)


@pytest.fixture(scope="module")
def ops():
    from sglang_awq_amd import ops as _ops

    _lib.load()
    return _ops


def _case(ops, M, K, N, g, dt="bf16", pattern="A"):
    qw, s, qz = synth.make_awq_weights(K, N, g, dt, pattern, seed=M + K + N)
    x = synth.make_activations(M, K, dt, "A", seed=M + K + 1)
    dev = [to_torch(a, DEV) for a in (qw, s, qz)]
    return qw, s, qz, x, ops.awq_repack(*dev), dev


def _check(ops, M, K, N, g, variant=RP):
    qw, s, qz, x, packed, _ = _case(ops, M, K, N, g)
    y = ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=variant)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    assert_gemm_close(to_np(y), exact, "bf16", what=f"bf16 GEMV M={M} K={K} N={N} g={g}")


# N = 8208: three-group strips, the last overlapping.  K = 1408: 11 k-blocks, one per wave, five waves own nothing; K = 2176: 17
# k-blocks, two per wave, wave 8 has one real and one ragged k-block, the waves behind it none; (2048, 256): a group spans two
# k-blocks.  32 hot positions, M at a time: position i looks at k-block 3 i % KB, k-step (i / 8 + i) % 4, position i % 32 of the k-step
# (all eight nibble positions of a dword, every k % 32); the first four sit on the first row of K and on both sides of the boundary
# between the k-blocks of waves 0 and 1 (twice), the last on the last row of K.
@pytest.mark.parametrize("K,g", [(1408, 128), (2176, 128), (2048, 256)])
@pytest.mark.parametrize("M", [1, 16])
def test_one_hot_rows_reproduce_dequantize(ops, M, K, g):
    N, KB = 8208, K // 128
    edge = 128 * ((KB + 15) // 16)
    _, _, _, _, packed, dev = _case(ops, M, K, N, g, pattern="F")
    W = ops.awq_dequantize(*dev)
    ks = [(128 * (3 * i % KB) + 32 * ((i // 8 + i) % 4) + i % 32) % K for i in range(32)]
    ks[:4], ks[-1] = [0, edge - 1, edge, edge - 1], K - 1
    for i in range(0, 32, M):
        x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        x[torch.arange(M), torch.tensor(ks[i:i + M])] = 1.0
        assert torch.equal(ops.awq_gemm_repacked(x, packed, K, N, g, variant=RP), W[ks[i:i + M]])


# G - 1 full strips and one column group more (G = 1: five lone column groups); one row: the one-row form, 5 / 16 rows: 2 / 4 staging loads
@pytest.mark.parametrize("G", range(1, 9))
@pytest.mark.parametrize("M", [1, 5, 16])
def test_every_strip_width_ragged(ops, M, G):
    _check(ops, M, 1408, 4096 * (G - 1) + 16 if G > 1 else 72, 128)


# one k-block, fifteen empty waves | one group | the deepest straight-line form three-group strips have at that row count, ragged:
# five k-blocks per wave at one row (65 k-blocks), two at sixteen (31) | the one-row long form: the deepest three-group strips hold,
# eight k-blocks per wave, ragged (127), and nine k-blocks per wave on one-group strips, ragged (129)
@pytest.mark.parametrize("M,K,N,g", [(1, 128, 8208, 128), (16, 128, 8208, 128), (1, 4096, 8208, 4096), (16, 4096, 8208, 4096),
                                     (1, 8320, 8208, 128), (16, 3968, 8208, 128), (1, 16256, 8208, 128), (1, 16512, 72, 128)])
def test_k_edges(ops, M, K, N, g):
    _check(ops, M, K, N, g)


def test_operator_edges(ops):
    """x as a column slice of a wider tensor (ldx > K); bias after the rounding; run-to-run identical."""
    M, K, N, g = 16, 1408, 8208, 128
    _, _, _, x, packed, _ = _case(ops, M, K, N, g)
    dx = to_torch(x, DEV)
    y = ops.awq_gemm_repacked(dx, packed, K, N, g, variant=RP)
    wide = torch.full((M, K + 264), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, 8:8 + K] = dx
    assert torch.equal(ops.awq_gemm_repacked(wide[:, 8:8 + K], packed, K, N, g, variant=RP), y)
    b = to_torch(synth.make_bias(N, "bf16", 3), DEV)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, bias=b, variant=RP), y + b)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, variant=RP), y)


# fp16 tensors | g = 64 | 17 rows | N past 32768 | a row stride that is no multiple of 8
@pytest.mark.parametrize("M,N,g,dt,pad", [(16, 8208, 128, "f16", 0), (16, 8208, 64, "bf16", 0), (17, 8208, 128, "bf16", 0),
                                          (16, 32784, 128, "bf16", 0), (16, 8208, 128, "bf16", 4)])
def test_refuses_outside_its_domain(ops, M, N, g, dt, pad):
    K = 256
    _, _, _, x, packed, _ = _case(ops, M, K, N, g, dt)
    dx = torch.zeros(M, K + pad, dtype=to_torch(x).dtype, device=DEV)[:, :K]
    with pytest.raises(_lib.AwqHipError, match=f"status {_lib.ERR_BAD_VARIANT}"):
        ops.awq_gemm_repacked(dx, packed, K, N, g, variant=RP)


# one routed cell per row bucket (awq_dispatch.h: gemv_bf16_wins): one row on three-group strips, 2 .. 8 rows on two-group strips,
# 9 .. 16 rows on one-group strips
@pytest.mark.parametrize("M,N", [(1, 8208), (8, 4112), (16, 72)])
def test_auto_route(ops, M, N):
    _check(ops, M, 1408, N, 128, variant=_lib.RP_AUTO)

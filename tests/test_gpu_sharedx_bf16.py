"""The bf16 shared-activation GEMV for 1 .. 64 rows (awq_repacked_sharedx_bf16.hip), forced through variant=RP_SHARED_X_BF16:
one-hot rows bit-equal to awq_dequantize, the oracle's float64 exact sums at every strip width and row-tile count, K edges, ldx > K,
bias, determinism, the refusals and the automatic route."""
import pytest
import torch

from oracle import c_oracle
from sglang_awq_amd import _lib, synth
from tests.util import assert_gemm_close, to_np, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SXB = getattr(_lib, "RP_SHARED_X_BF16", 3)


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


def _check(ops, M, K, N, g, variant=SXB):
    qw, s, qz, x, packed, _ = _case(ops, M, K, N, g)
    y = ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=variant)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    assert_gemm_close(to_np(y), exact, "bf16", what=f"shared-x bf16 M={M} K={K} N={N} g={g}")


# K = 1408: 11 k-blocks, a ragged last chunk at 4 and at 8 k-blocks per chunk; N = 8208: three-group strips, the last overlapping.
# Row i looks at k-block 3 i % 11, k-step (i / 8 + i) % 4, position i % 32 of the k-step (all eight positions of a dword from 16 rows,
# every k % 32 from 64); the first four rows sit on both sides of the chunk boundaries at 512 and 1024, the last on the last row of K.
@pytest.mark.parametrize("M,K,g", [(16, 1408, 128), (32, 1408, 128), (48, 1408, 128), (64, 1408, 128), (32, 2048, 256)])
def test_one_hot_rows_reproduce_dequantize(ops, M, K, g):
    N = 8208
    _, _, _, _, packed, dev = _case(ops, M, K, N, g, pattern="F")
    W = ops.awq_dequantize(*dev)
    ks = [(128 * (3 * i % 11) + 32 * ((i // 8 + i) % 4) + i % 32) % K for i in range(M)]
    ks[:4], ks[-1] = [511, 512, 1023, 1024], K - 1
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    x[torch.arange(M), torch.tensor(ks)] = 1.0
    assert torch.equal(ops.awq_gemm_repacked(x, packed, K, N, g, variant=SXB), W[ks])


# G - 1 full strips and one column group more (G = 1: five lone column groups); one launch up to 32 rows, two above where the strip width has them
@pytest.mark.parametrize("G,M", [(G, M) for G in range(1, 9) for M in [17, 32] + [1] * (G in (1, 6)) + [33, 64] * (G >= 3) + [48, 49] * (G in (3, 8))])
def test_every_strip_width_ragged(ops, M, G):
    _check(ops, M, 1408, 4096 * (G - 1) + 16 if G > 1 else 72, 128)


# one k-block | half a chunk, g = K | both buffers reused, a group spanning k-blocks
@pytest.mark.parametrize("K,g", [(128, 128), (512, 512), (2048, 256)])
@pytest.mark.parametrize("M", [32, 64])
def test_k_edges(ops, M, K, g):
    _check(ops, M, K, 8208, g)


@pytest.mark.parametrize("M", [32, 64])
def test_operator_edges(ops, M):
    """x as a column slice of a wider tensor (ldx > K); bias after the rounding; run-to-run identical."""
    K, N, g = 1408, 8208, 128
    _, _, _, x, packed, _ = _case(ops, M, K, N, g)
    dx = to_torch(x, DEV)
    y = ops.awq_gemm_repacked(dx, packed, K, N, g, variant=SXB)
    wide = torch.full((M, K + 264), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, 8:8 + K] = dx
    assert torch.equal(ops.awq_gemm_repacked(wide[:, 8:8 + K], packed, K, N, g, variant=SXB), y)
    b = to_torch(synth.make_bias(N, "bf16", 3), DEV)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, bias=b, variant=SXB), y + b)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, variant=SXB), y)


# fp16 tensors | g = 64 | 65 rows | 33 rows on a narrow matrix | N past 32768 | a row stride that is no multiple of 8
@pytest.mark.parametrize("M,N,g,dt,pad", [(32, 8208, 128, "f16", 0), (32, 8208, 64, "bf16", 0), (65, 8208, 128, "bf16", 0),
                                          (33, 4096, 128, "bf16", 0), (32, 32784, 128, "bf16", 0), (32, 8208, 128, "bf16", 4)])
def test_refuses_outside_its_domain(ops, M, N, g, dt, pad):
    K = 256
    _, _, _, x, packed, _ = _case(ops, M, K, N, g, dt)
    dx = torch.zeros(M, K + pad, dtype=to_torch(x).dtype, device=DEV)[:, :K]
    with pytest.raises(_lib.AwqHipError, match=f"status {_lib.ERR_BAD_VARIANT}"):
        ops.awq_gemm_repacked(dx, packed, K, N, g, variant=SXB)


# one routed cell per row range: 1 .. 16 rows on a five-group strip, 17 .. 32, 33 .. 48 and 49 .. 64 on three-group strips
@pytest.mark.parametrize("M,N", [(8, 16400), (32, 8208), (33, 8208), (64, 8208)])
def test_auto_route(ops, M, N):
    _check(ops, M, 1408, N, 128, variant=_lib.RP_AUTO)

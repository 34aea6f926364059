"""The hand-pipelined fp16 MFMA tiles for group sizes 32 / 64 (awq_repacked_prefill_sg.hip), forced through variant=RP_TILES_SG_WIDE /
_NARROW on N = 488 (31 column groups, the last half full: one 256-wide tile + 192-wide tiles of 12 and 3 groups, or four 128-wide
tiles, the last of 7 groups): one-hot rows bit-equal to awq_dequantize, the oracle's float64 exact sums, ldx > K, bias, determinism,
the refusals, the planned form and the automatic route."""
import pytest
import torch

from oracle import c_oracle
from sglang_awq_amd import _lib, synth
from tests.util import assert_gemm_close, to_np, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 488
WIDE, NARROW = getattr(_lib, "RP_TILES_SG_WIDE", 9), getattr(_lib, "RP_TILES_SG_NARROW", 10)
both = pytest.mark.parametrize("variant", [WIDE, NARROW])
groups = pytest.mark.parametrize("g", [32, 64])


@pytest.fixture(scope="module")
def ops():
    from sglang_awq_amd import ops as _ops

    _lib.load()
    return _ops


def _case(ops, M, K, N, g, dt="f16", pattern="A"):
    qw, s, qz = synth.make_awq_weights(K, N, g, dt, pattern, seed=M + K + N)
    x = synth.make_activations(M, K, dt, "A", seed=M + K + 1)
    dev = [to_torch(a, DEV) for a in (qw, s, qz)]
    return qw, s, qz, x, ops.awq_repack(*dev), dev


def _check(ops, M, K, N, g, variant):
    qw, s, qz, x, packed, _ = _case(ops, M, K, N, g)
    y = ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=variant)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    assert_gemm_close(to_np(y), exact, "f16", what=f"small-group tiles variant={variant} M={M} K={K} N={N} g={g}")


# Two row tiles, the second ragged; five k-blocks, so both LDS buffers are reused.  Row i looks at k-block i % 5, k-step (i / 5) % 4,
# position i % 32 of the k-step (160 rows: every k-block with every k-step — at g = 32 each its own quantisation group, scales differing
# per group in family "F" — and every position); the first ten rows sit on k = 0, on both sides of every k-block boundary and on K - 1.
@both
@groups
def test_one_hot_rows_reproduce_dequantize(ops, variant, g):
    M, K = 160, 640
    _, _, _, _, packed, dev = _case(ops, M, K, N, g, pattern="F")
    W = ops.awq_dequantize(*dev)
    ks = [128 * (i % 5) + 32 * ((i // 5) % 4) + i % 32 for i in range(M)]
    ks[:10] = [0, 127, 128, 255, 256, 383, 384, 511, 512, K - 1]
    x = torch.zeros(M, K, dtype=torch.float16, device=DEV)
    x[torch.arange(M), torch.tensor(ks)] = 1.0
    assert torch.equal(ops.awq_gemm_repacked(x, packed, K, N, g, variant=variant), W[ks])


# a second row tile of one row | one k-block: prologue and epilogue only | fewer rows than a tile | three row tiles
@both
@groups
@pytest.mark.parametrize("M,K", [(129, 640), (128, 128), (33, 256), (257, 640)])
def test_sums_against_exact(ops, variant, g, M, K):
    _check(ops, M, K, N, g, variant)


@both
@groups
def test_operator_edges(ops, variant, g):
    """x as a column slice of a wider tensor (ldx > K); bias after the rounding; run-to-run identical."""
    M, K = 129, 640
    _, _, _, x, packed, _ = _case(ops, M, K, N, g)
    dx = to_torch(x, DEV)
    y = ops.awq_gemm_repacked(dx, packed, K, N, g, variant=variant)
    wide = torch.full((M, K + 264), 7.0, dtype=torch.float16, device=DEV)
    wide[:, 8:8 + K] = dx
    assert torch.equal(ops.awq_gemm_repacked(wide[:, 8:8 + K], packed, K, N, g, variant=variant), y)
    b = to_torch(synth.make_bias(N, "f16", 3), DEV)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, bias=b, variant=variant), y + b)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, variant=variant), y)


# g = 128 | bf16 tensors | a row stride that is no multiple of 8
@both
@pytest.mark.parametrize("g,dt,pad", [(128, "f16", 0), (64, "bf16", 0), (64, "f16", 4)])
def test_refuses_outside_its_domain(ops, variant, g, dt, pad):
    M, K = 129, 256
    _, _, _, x, packed, _ = _case(ops, M, K, N, g, dt)
    dx = torch.zeros(M, K + pad, dtype=to_torch(x).dtype, device=DEV)[:, :K]
    with pytest.raises(_lib.AwqHipError, match=f"status {_lib.ERR_BAD_VARIANT}"):
        ops.awq_gemm_repacked(dx, packed, K, N, g, variant=variant)


# With the round constants of awq_dispatch.h (0.84 / 0.65 / 0.02), three row tiles on N = 32648 (2041 column groups) plan as 85 column
# tiles of 256 (255 workgroups: one round) and 57 of 192 for the remaining 681 groups (171 workgroups: one round): 1 + 0.84 + 0.02 =
# 1.86 against 2 for 128 x 3 wide tiles, 3 x 0.84 = 2.52 for 192-wide tiles alone and 3 x 0.65 = 1.95 for 768 128-wide ones: both regions run.
def test_planned_form_runs_both_regions(ops):
    _check(ops, 257, 128, 32648, 32, _lib.RP_TILES_SG)


# from 33 rows on a narrow and on a wide matrix, through the route AWQLinearMethod.apply and the op's cached copy take
@pytest.mark.parametrize("M,n", [(64, N), (129, N), (65, 8208)])
def test_auto_route(ops, M, n):
    _check(ops, M, 640, n, 64, _lib.RP_AUTO)

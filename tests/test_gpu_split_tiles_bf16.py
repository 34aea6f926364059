"""The bf16 MFMA tiles with K split over workgroups (awq_repacked_prefill_bf16.hip, SPLIT form + pf_splitk_reduce_kernel), forced through
variant=RP_SPLIT_BF16_WIDE / _NARROW on N = 488 (31 column groups, the last half full: two 256-wide or four 128-wide column tiles): one-hot
rows bit-equal to awq_dequantize, the oracle's float64 exact sums, ldx > K, bias, determinism (also after another shape used the scratch),
the refusals, the planned form and the automatic route.  Slices: S = min(256 / tiles, 8, (K / 128) / 4) of ceil((K / 128) / S) k-blocks."""
import pytest
import torch

from oracle import c_oracle
from sglang_awq_amd import _lib, synth
from tests.test_gpu_tiles_bf16 import DEV, N, _case, ops  # noqa: F401  (the same helpers and fixture)
from tests.util import assert_gemm_close, to_np, to_torch

pytestmark = pytest.mark.gpu
PLANNED, WIDE, NARROW = (getattr(_lib, "RP_SPLIT_BF16" + s, v) for s, v in (("", 11), ("_WIDE", 12), ("_NARROW", 13)))
both = pytest.mark.parametrize("variant", [WIDE, NARROW])


def _check(ops, M, K, N, g, variant):
    qw, s, qz, x, packed, _ = _case(ops, M, K, N, g)
    y = ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g, variant=variant)
    _, exact = c_oracle.gemm(x, qw, s, qz, want_exact=True)
    assert_gemm_close(to_np(y), exact, "bf16", what=f"bf16 split tiles variant={variant} M={M} K={K} N={N} g={g}")
    return y


# 21 k-blocks: five slices of 5, 5, 5, 5 and 1.  A single non-zero product makes every fp32 slice sum exact.  Row i looks at k-block
# i % 21 (every slice), k-step (i / 21) % 4, position i % 32 of the k-step; the first ten rows sit on k = 0, on both sides of every slice
# boundary and on k = K - 1.
@both
def test_one_hot_rows_reproduce_dequantize(ops, variant):
    M, K, g = 160, 2688, 128
    _, _, _, _, packed, dev = _case(ops, M, K, N, g, pattern="F")
    W = ops.awq_dequantize(*dev)
    ks = [128 * (i % 21) + 32 * ((i // 21) % 4) + i % 32 for i in range(M)]
    ks[:10] = [0, 639, 640, 1279, 1280, 1919, 1920, 2559, 2560, K - 1]
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    x[torch.arange(M), torch.tensor(ks)] = 1.0
    assert torch.equal(ops.awq_gemm_repacked(x, packed, K, N, g, variant=variant), W[ks])


# two slices of 5 and 4, a second row tile of one row | slices starting at k-blocks 5, 10, 15, inside a quantisation group of 3 |
# a last slice of one k-block: prologue and epilogue only | g = K, three row tiles, the minimum of two slices of four k-blocks
@both
@pytest.mark.parametrize("M,K,g", [(129, 1152, 128), (65, 2304, 384), (200, 2688, 128), (257, 1024, 1024)])
def test_sums_against_exact(ops, variant, M, K, g):
    _check(ops, M, K, N, g, variant)


@both
def test_operator_edges(ops, variant):
    """x as a column slice of a wider tensor (ldx > K); bias after the rounding; identical run to run, also after another shape has
    left its partial tiles in the same scratch."""
    M, K, g = 129, 1152, 128
    _, _, _, x, packed, _ = _case(ops, M, K, N, g)
    dx = to_torch(x, DEV)
    y = ops.awq_gemm_repacked(dx, packed, K, N, g, variant=variant)
    wide = torch.full((M, K + 264), 7.0, dtype=torch.bfloat16, device=DEV)
    wide[:, 8:8 + K] = dx
    assert torch.equal(ops.awq_gemm_repacked(wide[:, 8:8 + K], packed, K, N, g, variant=variant), y)
    b = to_torch(synth.make_bias(N, "bf16", 3), DEV)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, bias=b, variant=variant), y + b)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, variant=variant), y)
    _check(ops, 200, 2688, N, g, variant)
    assert torch.equal(ops.awq_gemm_repacked(dx, packed, K, N, g, variant=variant), y)


# fp16 tensors | g = 64 | five k-blocks: one slice | a row stride that is no multiple of 8
@both
@pytest.mark.parametrize("K,g,dt,pad", [(1152, 128, "f16", 0), (1152, 64, "bf16", 0), (640, 128, "bf16", 0), (1152, 128, "bf16", 4)])
def test_refuses_outside_its_domain(ops, variant, K, g, dt, pad):
    M = 129
    _, _, _, x, packed, _ = _case(ops, M, K, N, g, dt)
    dx = torch.zeros(M, K + pad, dtype=to_torch(x).dtype, device=DEV)[:, :K]
    with pytest.raises(_lib.AwqHipError, match=f"status {_lib.ERR_BAD_VARIANT}"):
        ops.awq_gemm_repacked(dx, packed, K, N, g, variant=variant)


# 32 k-blocks in eight slices of 4 on 128 x 128 tiles (8 of them).  The automatic route takes the same plan: route::split_tiles_bf16_wins
# (awq_dispatch.h) routes matrices from 32 k-blocks deep — the shallowest measured (profiles/kbench_split_tiles_bf16_ab.txt), so K = 4096 is
# the smallest routed K — with at most 64 wide tiles (here 4; every measured cell with that few won), and the shim asks
# awq_gemm_repacked_workspace_bytes, which wants the scratch from 65 rows.
def test_planned_form_and_auto_route(ops):
    M, K, g = 129, 4096, 128
    y = _check(ops, M, K, N, g, PLANNED)
    _, _, _, x, packed, _ = _case(ops, M, K, N, g)
    assert _lib.load().awq_gemm_repacked_workspace_bytes(M, K, N, g, _lib.DTYPE_BF16) > 0
    assert torch.equal(ops.awq_gemm_repacked(to_torch(x, DEV), packed, K, N, g), y)

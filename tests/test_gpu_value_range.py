"""Value range and non-finite parity of every kernel on the quantized GEMM path.

The other GPU files vary shape; this one varies VALUES, over one table with a row per kernel at the smallest shape that reaches it:
  a. scaled one-hot rows (x = c e_k with c at both ends of the storage dtype's range): bit-equal to c * awq_dequantize, rounded once;
  b. y(2^p x) == 2^p y(x) bit for bit wherever both sides are normal and finite;
  c. scales at both ends of their range against the oracle (fp16) or against the unscaled run (bf16: exact powers of two);
  d. a NaN row, a single +inf, a NaN scale column, a scale of 65504: the poisoned outputs have the IEEE class float64 gives them, every
     other output keeps its bits;
  e. a call that leaves NaN partial tiles in the per-stream scratch does not change what a later, smaller call through it returns.
Shapes: N % 16 == 8 (a half-filled last column group) and M one past a row-tile boundary wherever the kernel's domain allows."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import awq_ref, c_oracle
from sglang_awq_amd import _lib, synth
from tests.util import assert_gemm_close, to_np, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}

Row = namedtuple("Row", "label dt M K N g how")
RP, NOWS, CK, OP = "repacked", "repacked, no workspace", "checkpoint", "op"
L = _lib

# how: (RP, variant) ops.awq_gemm_repacked(variant=) — RP_AUTO takes the per-stream scratch exactly where awq_gemm_repacked_workspace_bytes
# asks for it (ops.py: awq_gemm_repacked) | (NOWS,) the same dispatcher through the C entry without a workspace, awq_gemm_repacked, as
# test_gpu_round3.py calls it | (CK, variant) ops.awq_gemm_variant on the checkpoint tensors | (OP,) torch.ops.sgl_kernel.awq_gemm.
# Below: NG = ceil(N / 16) column groups, KB = K / 128 k-blocks, G = ceil(NG / 256) strip width.
ROWS = [
    # ---- forced variants (awq_capi.hip:318-349 awq_gemm_repacked_ex)
    # gemv_sharedx_kernel, two row tiles (awq_capi.hip:349)
    Row("sharedx", "f16", 17, 640, 264, 128, (RP, L.RP_SHARED_X)),
    # gemv_sharedx_wide_kernel, three row tiles; its launcher wants G >= 3 (awq_repacked_sharedx_wide.hip:231): NG = 513
    Row("sharedx_wide", "f16", 33, 256, 8200, 128, (RP, L.RP_SHARED_X_WIDE)),
    # gemv_sharedx_bf16_kernel: one row tile, two, and 33 .. 64 rows as two launches (G >= 3: awq_repacked_sharedx_bf16.hip:382)
    Row("sharedx_bf16_1_16", "bf16", 3, 640, 264, 128, (RP, L.RP_SHARED_X_BF16)),
    Row("sharedx_bf16_17_32", "bf16", 17, 640, 264, 128, (RP, L.RP_SHARED_X_BF16)),
    Row("sharedx_bf16_33_64", "bf16", 33, 256, 8200, 128, (RP, L.RP_SHARED_X_BF16)),
    # gemm_repacked_pipelined_bf16_kernel: planned (31 column groups, one row round: 128-wide tiles win the round model,
    # awq_repacked_prefill_bf16.hip:492-493), 256-wide + 192-wide remainder, 128-wide (awq_repacked_prefill_bf16.hip:476-502)
    Row("tiles_bf16", "bf16", 129, 384, 488, 128, (RP, L.RP_TILES_BF16)),
    Row("tiles_bf16_wide", "bf16", 129, 384, 488, 128, (RP, L.RP_TILES_BF16_WIDE)),
    Row("tiles_bf16_narrow", "bf16", 129, 384, 488, 128, (RP, L.RP_TILES_BF16_NARROW)),
    # gemv_bf16_kernel, the 2 .. 16-row form and the one-row form (constants as (s, s / 16, -z s) in LDS): 5 k-blocks on 16 waves, so
    # eleven waves run the past-K path of awq_repacked_gemv_bf16.hip:46-48
    Row("gemv_bf16", "bf16", 5, 640, 264, 128, (RP, L.RP_GEMV_BF16)),
    Row("gemv_bf16_one_row", "bf16", 1, 640, 264, 128, (RP, L.RP_GEMV_BF16)),
    # gemm_repacked_pipelined_sg_kernel, g = 32 and 64 (awq_repacked_prefill_sg.hip:313)
    Row("tiles_sg_g32", "f16", 129, 384, 488, 32, (RP, L.RP_TILES_SG)),
    Row("tiles_sg_wide_g32", "f16", 129, 384, 488, 32, (RP, L.RP_TILES_SG_WIDE)),
    Row("tiles_sg_narrow_g32", "f16", 129, 384, 488, 32, (RP, L.RP_TILES_SG_NARROW)),
    Row("tiles_sg_g64", "f16", 129, 384, 488, 64, (RP, L.RP_TILES_SG)),
    Row("tiles_sg_wide_g64", "f16", 129, 384, 488, 64, (RP, L.RP_TILES_SG_WIDE)),
    Row("tiles_sg_narrow_g64", "f16", 129, 384, 488, 64, (RP, L.RP_TILES_SG_NARROW)),
    # gemm_repacked_pipelined_bf16_kernel, SPLIT form + pf_splitk_reduce_kernel<bf16>: K >= 1024 for two slices of four k-blocks
    # (awq_repacked_prefill_bf16.hip:530-555); 9 k-blocks: slices of 5 and 4
    Row("split_bf16", "bf16", 129, 1152, 488, 128, (RP, L.RP_SPLIT_BF16)),
    Row("split_bf16_wide", "bf16", 129, 1152, 488, 128, (RP, L.RP_SPLIT_BF16_WIDE)),
    Row("split_bf16_narrow", "bf16", 129, 1152, 488, 128, (RP, L.RP_SPLIT_BF16_NARROW)),
    # ---- the older fp16 kernels, g = 128, by the automatic route (awq_capi.hip:41-157 repacked_dispatch; <= 32 rows: :67-85 ->
    # gemv_one_launch :31-39 -> launch_gemv_repacked, awq_repacked.hip:189-273)
    # gemv_repacked_kernel, one row tile: KB = 5 < kRp2MinKBlocks and under 12 MiB, so neither rp2 condition of awq_repacked.hip:244-245
    # holds; 8 waves, straight-line T = 1 (:229-235)
    Row("gemv_repacked_1tile", "f16", 5, 640, 264, 128, (RP, L.RP_AUTO)),
    # two row tiles (M > 16, awq_repacked.hip:204): below kSharedXMinRows[1] = 24 (awq_dispatch.h:118), loop form T = 0 (:232-233) ...
    Row("gemv_repacked_2tiles", "f16", 17, 640, 264, 128, (RP, L.RP_AUTO)),
    # ... and straight-line T = 4 (KB = 32 on 8 waves, awq_repacked.hip:232; the scratch is offered at K >= 2048, rps_plan refuses
    # KB < kRpsMinKBlocks, awq_repacked_splitk.hip:128)
    Row("gemv_repacked_2tiles_t4", "f16", 17, 4096, 264, 128, (RP, L.RP_AUTO)),
    # rounds mode: NG = 2049 -> G = 9 > kOneStripMaxGroups (awq_repacked.hip:212-214)
    Row("gemv_repacked_rounds", "f16", 5, 128, 32776, 128, (RP, L.RP_AUTO)),
    # gemv_rp2_kernel, short form: KB = 16 >= kRp2MinKBlocks (awq_repacked.hip:244-247), G T = 1
    Row("gemv_rp2", "f16", 5, 2048, 264, 128, (RP, L.RP_AUTO)),
    # the same with a ragged last wave: KB = 17, T = 2, wave 8 holds one k-block and one past K, waves 9 .. 15 only k-blocks past K
    # (awq_repacked_gemv.h: "ragged last wave")
    Row("gemv_rp2_ragged", "f16", 5, 2176, 264, 128, (RP, L.RP_AUTO)),
    # long form: one row, T = ceil(KB / 16) = 9 > 8 (rp2_fits_long, awq_repacked_gemv.h:577, :607-617).  The narrowest strip needs KB >= 129,
    # so K = 16512 is the smallest K that reaches it; N is kept small instead
    Row("gemv_rp2_long", "f16", 1, 16512, 136, 128, (RP, L.RP_AUTO)),
    # gemv_rp3_kernel: 13 .. 16 rows, G <= 2, KB >= 16 (awq_repacked.hip:255) where rp2 has no instantiation: M T = 13 x 3 staging
    # chunks > 8 per lane (rp2_chunks, awq_repacked_gemv.h:578)
    Row("gemv_rp3", "f16", 13, 4224, 264, 128, (RP, L.RP_AUTO)),
    # gemv_rps_kernel: 9 .. 32 rows with the scratch, KB >= 64, 8 <= NG <= 256 (awq_capi.hip:70-73, awq_repacked_splitk.hip:117-141); NG = 9
    # gives five strips, the last overlapping its neighbour, in eight slices; sharedx_wins takes 17 rows up on NG <= 80 (awq_dispatch.h:128-129)
    Row("gemv_rps", "f16", 11, 8192, 136, 128, (RP, L.RP_AUTO)),
    # passes of the 32-row GEMV (awq_capi.hip:142-155): gemv_passes_max(1536, 264) = 2 (awq_dispatch.h:75-81), 33 rows = a pass of 32
    # (gemv_sharedx_kernel from 24 rows) and one of 1 (gemv_repacked_kernel).  With a scratch the split-K tiles below come first
    # (awq_capi.hip:137-140), and ops.awq_gemm_repacked offers it wherever that plan exists: only the entry without one gets here
    Row("gemv_passes", "f16", 33, 1536, 264, 128, (NOWS,)),
    # gemm_repacked_ksplit_kernel: 97 rows up, <= 64 wide tiles (awq_capi.hip:141); KB = 4 < 8 leaves no split-K plan, so no scratch
    # (awq_repacked_prefill.hip:507-509)
    Row("ksplit", "f16", 129, 512, 264, 128, (RP, L.RP_AUTO)),
    # gemm_repacked_pipelined_kernel (awq_capi.hip:156 -> awq_repacked.hip:132-135 -> awq_repacked_prefill.hip:521-567): 85 tiles of 256
    # and 57 of 192 on three row tiles (NG = 2041, the plan of tests/test_gpu_tiles_bf16.py with the same round constants) ...
    Row("pipelined_256_192", "f16", 257, 128, 32648, 128, (RP, L.RP_AUTO)),
    # ... and 128-wide tiles: one round of five beats one of three 192-wide (0.65 < 0.84, awq_repacked_prefill.hip:547-548); 33 rows is
    # past gemv_passes_max(512, 520) = 1 pass and below kKsplitMinRows
    Row("pipelined_128", "f16", 33, 512, 520, 128, (RP, L.RP_AUTO)),
    # gemm_repacked_pipelined_kernel, PfSplit form + pf_splitk_reduce_kernel<fp16> (awq_capi.hip:137-140, pf_split_plan
    # awq_repacked_prefill.hip:464-495): four wide tiles, KB = 8 -> two slices of four k-blocks on 128 x 128 tiles
    Row("pf_split", "f16", 129, 1024, 264, 128, (RP, L.RP_AUTO)),
    # gemv_rpx_kernel: bf16 with g = 64 and fp16 with g = 32 are not repacked_fast (awq_repacked.hip:151-153, :191-201), 16 rows a launch
    Row("gemv_rpx_bf16_g64", "bf16", 17, 640, 264, 64, (RP, L.RP_AUTO)),
    Row("gemv_rpx_f16_g32", "f16", 17, 640, 264, 32, (RP, L.RP_AUTO)),
    # gemm_rpx_tiled_kernel: bf16, g = 64, 33 rows up (awq_capi.hip:113 -> awq_repacked.hip:134)
    Row("gemm_rpx_tiled_bf16_g64", "bf16", 33, 640, 264, 64, (RP, L.RP_AUTO)),
    # ---- checkpoint-layout kernels (awq_capi.hip:222-228)
    Row("generic_f16", "f16", 17, 256, 72, 64, (CK, L.GEMM_GENERIC)),
    Row("generic_bf16", "bf16", 17, 256, 72, 64, (CK, L.GEMM_GENERIC)),
    # skinny: M <= 16, N % 32 == 0 (awq_gemm_skinny.hip:338-342), so no half-filled column group
    Row("skinny_f16", "f16", 5, 1024, 288, 128, (CK, L.GEMM_SKINNY)),
    Row("skinny_bf16", "bf16", 5, 1024, 288, 128, (CK, L.GEMM_SKINNY)),
    Row("tiled_f16", "f16", 129, 384, 264, 128, (CK, L.GEMM_TILED)),
    Row("tiled_bf16", "bf16", 129, 384, 264, 128, (CK, L.GEMM_TILED)),
    # ---- the op without a cached copy, 33 rows up: awq_repack into the front of the workspace, then repacked_dispatch with what lies
    # behind it (awq_capi.hip:233-244) — the split-K tiles of the pf_split row
    Row("op_on_the_fly", "f16", 65, 1024, 264, 128, (OP,)),
]
ROW = {r.label: r for r in ROWS}
by_row = pytest.mark.parametrize("row", ROWS, ids=[r.label for r in ROWS])

# (row label, family) -> the arithmetic reason a pair is left out; at most one pair in ten
SKIP = {}


def test_route_table_is_well_formed():
    assert len(ROW) == len(ROWS)
    assert len(SKIP) * 10 <= len(ROWS) * 5
    for r in ROWS:
        assert r.K % 128 == 0 and r.K % r.g == 0 and r.N % 8 == 0 and r.K * r.N <= 4.4e6 and r.K <= 16512


@pytest.fixture(scope="module")
def ops():
    from sglang_awq_amd import ops as _ops   # raises if the HIP library is missing: no fallback

    _lib.load()
    _ops.awq_gemm_cache_enable(False)        # the op row wants the on-the-fly re-layout, never a cached copy
    return _ops


# ------------------------------------------------------------------------------------------------------------------------ helpers
class Weights:
    """Checkpoint tensors on the host and on the device, and the repacked copy where the layout exists for the shape."""

    def __init__(self, ops, qw, s, qz):
        self.qw, self.s, self.qz = qw, s, qz
        self.dev = [to_torch(a, DEV) for a in (qw, s, qz)]
        self._ops, self._packed, self._w64 = ops, None, None

    @property
    def packed(self):
        if self._packed is None:
            self._packed = self._ops.awq_repack(*self.dev)
            assert self._packed is not None
        return self._packed

    def w64(self, dt):
        """awq_dequantize on the GPU (bit-exact by test_gpu_parity.py), in float64."""
        if self._w64 is None:
            self._w64 = awq_ref.to_f64(to_np(self._ops.awq_dequantize(*self.dev)), dt)
        return self._w64


def pow2(a, dt, e):
    """storage array x 2^e, rounded once into the storage dtype (exact while the result is normal)."""
    with np.errstate(over="ignore"):
        return awq_ref.from_f64(awq_ref.to_f64(a, dt) * 2.0 ** e, dt)


def weights(ops, row, family="A", scale_exp=0, K=None):
    K = row.K if K is None else K
    qw, s, qz = synth.make_awq_weights(K, row.N, row.g, row.dt, family, seed=K + row.N + row.g)
    return Weights(ops, qw, pow2(s, row.dt, scale_exp) if scale_exp else s, qz)


def activations(row, clipped=False, M=None, K=None):
    """Family "A" (N(0, 1)); clipped: |x| >= 2^-6, so that x 2^-8 stays normal in fp16."""
    M, K = row.M if M is None else M, row.K if K is None else K
    x = synth.rand_normal((M, K), M + K + 1, 5)
    if clipped:
        x = np.where(x < 0, -1.0, 1.0) * np.maximum(np.abs(x), 2.0 ** -6)
    return synth.cast(x, row.dt)


def run(ops, row, x, w):
    """x: [M, K] device tensor with exactly the row's M (the route depends on it)."""
    M, K = x.shape
    kind = row.how[0]
    if kind == RP:
        return ops.awq_gemm_repacked(x, w.packed, K, row.N, row.g, variant=row.how[1])
    if kind == CK:
        return ops.awq_gemm_variant(x, *w.dev, row.how[1])
    if kind == OP:
        assert ops.awq_gemm_cache_info()["entries"] == 0
        return torch.ops.sgl_kernel.awq_gemm(x, *w.dev, 1)
    assert kind == NOWS and x.is_contiguous()
    y = torch.empty((M, row.N), dtype=x.dtype, device=x.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = _lib.load().awq_gemm_repacked(vp(x), K, vp(w.packed), None, vp(y), M, K, row.N, row.g, {"f16": 0, "bf16": 1}[row.dt],
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "awq_gemm_repacked")
    return y


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def klass(v):
    """0 finite, +1 / -1 the infinities, 2 NaN."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isnan(v), 2, np.where(np.isinf(v), np.sign(v), 0)).astype(np.int8)


def normal_finite(v, dt):
    return np.isfinite(v) & (np.abs(v) >= 2.0 ** {"f16": -14, "bf16": -126}[dt])


def skip_if_listed(row, family):
    if (row.label, family) in SKIP:
        pytest.skip(SKIP[(row.label, family)])


# ------------------------------------------------------------------------------------------------------------------------ a. one-hot
ONE_HOT_C = {"f16": (2.0 ** -16, 2.0 ** 15), "bf16": (2.0 ** -120, 2.0 ** 125)}


def one_hot_ks(row):
    """First and last k, both sides of k-block boundaries — those at every half, third, quarter, fifth and eighth of the k-blocks, where
    the split-K routes cut their slices — then a stride through every position of a k-step; a whole number of M-row batches, at most 4."""
    K, KB = row.K, row.K // 128
    cuts = sorted({128 * ((j * KB + d - 1) // d) for d in (2, 3, 4, 5, 8) for j in range(1, d)} - {0, K})
    ks = [0, K - 1] + [k for b in cuts for k in (b - 1, b)]
    want = row.M if row.M >= 8 else min(4 * row.M, 8) if row.M > 1 else 8
    ks = ks[:max(want, row.M) - 1] if len(ks) >= want else ks + [(37 * i + 5) % K for i in range(want - 1 - len(ks))]
    while (len(ks) + 1) % row.M:
        ks.append((53 * len(ks) + 11) % K)
    return ks


@by_row
def test_a_scaled_one_hot_rows(ops, row):
    """Row i of x is c e_k(i): every output is ONE product, so it must be c W[k, n] rounded once — subnormal results at the small c, +-inf
    of the right sign (never the largest finite value) at the large c wherever |c W| rounds past it.  The last row holds -0.0 in place of c:
    it must come out as zeros.  The sign of those zeros is not pinned: a route that starts its accumulator at +0 returns +0, one that
    starts from the first product may return -0 under a negative weight, and both add nothing; the comparison is on values (0.0 == -0.0)."""
    skip_if_listed(row, "a")
    w = weights(ops, row, "F")
    W = w.w64(row.dt)
    ks = one_hot_ks(row)
    R = len(ks) + 1
    for c in ONE_HOT_C[row.dt]:
        x = torch.zeros(R, row.K, dtype=torch.float64)
        x[torch.arange(R - 1), torch.tensor(ks)] = c
        x[R - 1, ks[0]] = -0.0
        x = x.to(TDT[row.dt]).to(DEV)
        assert float(x[0, ks[0]]) == c and torch.signbit(x[R - 1, ks[0]])
        with np.errstate(over="ignore"):
            want = awq_ref.from_f64(W[ks] * c, row.dt)
        wf = awq_ref.to_f64(want, row.dt)
        if c > 1:
            assert np.isinf(wf).any() and np.isfinite(wf).any(), "the large c was meant to overflow some outputs and not others"
        else:
            assert ((wf != 0) & ~normal_finite(wf, row.dt)).any(), "the small c was meant to give subnormal outputs"
        y = torch.cat([run(ops, row, x[i:i + row.M], w) for i in range(0, R, row.M)])
        got = to_np(y)
        diff = np.argwhere(got[:R - 1].view(np.uint16) != want.view(np.uint16))
        assert diff.size == 0, (f"{row.label} c=2^{int(np.log2(c))}: {len(diff)} of {want.size} outputs are not c W rounded once; first at row {diff[0][0]} "
                                f"(k={ks[diff[0][0]]}) col {diff[0][1]}: got {awq_ref.to_f64(got, row.dt)[tuple(diff[0])]!r}, want {wf[tuple(diff[0])]!r}")
        assert torch.equal(y[R - 1].float(), torch.zeros(row.N, device=DEV)), f"{row.label} c=2^{int(np.log2(c))}: the -0.0 row is not zero"


# ------------------------------------------------------------------------------------------------------------------------ b. x * 2^p
POW = {"f16": (8, -6), "bf16": (100, -100)}
# The share of outputs left out (either side subnormal or overflowing) was computed with the oracle on the CPU for these seeds: fp16 p = -6
# leaves out |y| < 2^-8, at most 0.51 % (gemv_repacked_rounds, K = 128, where |y| is smallest; pipelined_256_192 0.43 %, every other row
# under 0.3 %); fp16 p = +8 and both bf16 cases under 0.01 %.
MAX_LEFT_OUT = 0.01


@by_row
def test_b_power_of_two_activations(ops, row):
    """Scaling x by 2^p scales every product and every fp32 partial sum exactly: y(2^p x) must be 2^p y(x) bit for bit wherever both are
    normal and finite in the storage dtype."""
    skip_if_listed(row, "b")
    w = weights(ops, row, "A")
    x = activations(row, clipped=True)
    y0 = awq_ref.to_f64(to_np(run(ops, row, to_torch(x, DEV), w)), row.dt)
    assert np.isfinite(y0).all()
    for p in POW[row.dt]:
        xp = pow2(x, row.dt, p)
        assert np.array_equal(awq_ref.to_f64(xp, row.dt), awq_ref.to_f64(x, row.dt) * 2.0 ** p), "2^p x must be exact"
        yp = awq_ref.to_f64(to_np(run(ops, row, to_torch(xp, DEV), w)), row.dt)
        want = y0 * 2.0 ** p
        keep = normal_finite(y0, row.dt) & normal_finite(want, row.dt) & (np.abs(want) < {"f16": 65520.0, "bf16": 2.0 ** 128}[row.dt])
        left_out = 1.0 - keep.mean()
        assert left_out < MAX_LEFT_OUT, f"{row.label} p={p}: {left_out:.4f} of the outputs fall outside the normal range"
        bad = keep & (yp != want)
        assert not bad.any(), (f"{row.label} p={p}: {bad.sum()} of {keep.sum()} outputs are not 2^p y(x); first at {tuple(np.argwhere(bad)[0])}: "
                               f"{yp[tuple(np.argwhere(bad)[0])]!r} against {want[tuple(np.argwhere(bad)[0])]!r}")


# ------------------------------------------------------------------------------------------------------------------------ c. scales
@by_row
def test_c_scale_range(ops, row):
    """fp16: scales 2^-8 down (0.005 .. 0.02 becomes 1.9e-5 .. 7.8e-5, on both sides of the smallest normal 6.1e-5) with x 2^8 up, and
    scales 2^8 up with x 2^-8 down: outputs at unit scale, against the oracle's exact sums at the standard bound.  bf16: scales 2^+-100
    with x 2^-+100, every factor an exact power of two that stays normal: bit-identical to the unscaled run."""
    skip_if_listed(row, "c")
    x = activations(row, clipped=True)
    if row.dt == "f16":
        for e in (-8, 8):
            w = weights(ops, row, "A", scale_exp=e)
            xe = pow2(x, "f16", -e)
            y = run(ops, row, to_torch(xe, DEV), w)
            _, exact = c_oracle.gemm(xe, w.qw, w.s, w.qz, want_exact=True)
            assert_gemm_close(to_np(y), exact, "f16", what=f"{row.label} scales x 2^{e}, x x 2^{-e}")
        return
    y0 = run(ops, row, to_torch(x, DEV), weights(ops, row, "A"))
    assert torch.isfinite(y0).all()
    for e in (100, -100):
        w = weights(ops, row, "A", scale_exp=e)
        y = run(ops, row, to_torch(pow2(x, "bf16", -e), DEV), w)
        n = int((y.view(torch.int16) != y0.view(torch.int16)).sum())
        assert n == 0, f"{row.label} scales x 2^{e}, x x 2^{-e}: {n} of {y.numel()} outputs differ from the unscaled run"


# ------------------------------------------------------------------------------------------------------------------------ d. non-finite
def poisoned_rows(M):
    return sorted({0, M - 1, min(15, M - 1)})


@by_row
def test_d_nonfinite_rows(ops, row):
    """A row of NaN poisons exactly that row of y; a single +inf at x[r, k] makes row r +-inf by the sign of W[k, n] and NaN where
    W[k, n] == 0, as float64 gives it.  Every other row keeps its bits.  k sits in the first k-block for the first row (kernels that
    feed padding k-blocks re-read it), in the last one for the last row, in the middle otherwise."""
    skip_if_listed(row, "d-rows")
    w = weights(ops, row, "A")
    W = w.w64(row.dt)
    x = to_torch(activations(row), DEV)
    clean = run(ops, row, x, w)
    assert torch.isfinite(clean).all()
    others = lambda r: torch.arange(row.M, device=DEV) != r      # noqa: E731
    for r in poisoned_rows(row.M):
        xp = x.clone()
        xp[r, :] = float("nan")
        y = run(ops, row, xp, w)
        assert torch.isnan(y[r]).all(), f"{row.label}: NaN row {r}: {int((~torch.isnan(y[r])).sum())} outputs of that row are not NaN"
        assert same_bits(y[others(r)], clean[others(r)]), f"{row.label}: NaN row {r} changed another row"
    for r in poisoned_rows(row.M):
        k = 5 if r == 0 else row.K - 3 if r == row.M - 1 else row.K // 2 + 1
        xp = x.clone()
        xp[r, k] = float("inf")
        y = run(ops, row, xp, w)
        with np.errstate(invalid="ignore"):
            want = klass(awq_ref.to_f64(to_np(xp[r:r + 1]), row.dt) @ W)[0]
        assert set(np.unique(want)) <= {-1, 1, 2}
        got = klass(awq_ref.to_f64(to_np(y[r:r + 1]), row.dt))[0]
        assert np.array_equal(got, want), (f"{row.label}: +inf at x[{r}, {k}]: {int((got != want).sum())} of {row.N} outputs of that row have another "
                                           f"class than float64 gives (first col {int(np.argmax(got != want))}: {got[np.argmax(got != want)]} against {want[np.argmax(got != want)]})")
        assert same_bits(y[others(r)], clean[others(r)]), f"{row.label}: +inf at x[{r}, {k}] changed another row"


@by_row
def test_d_nonfinite_scale_columns(ops, row):
    """The scale of one column NaN in every group: exactly that column of y is NaN.  fp16: a column with scale 65504, whose W is +-inf, 0 or
    +-65504 as awq_dequantize gives it: the column has the class of the float64 product.  Every other column keeps its bits."""
    skip_if_listed(row, "d-columns")
    base = weights(ops, row, "A")
    xn = activations(row)
    x = to_torch(xn, DEV)
    clean = run(ops, row, x, base)
    N = row.N
    cases = [(n0, float("nan")) for n0 in sorted({0, N - 1, 16 * ((N - 1) // 16)})] + ([(N - 2, 65504.0)] if row.dt == "f16" else [])
    for n0, value in cases:
        s = base.s.copy()
        s[:, n0] = awq_ref.from_f64(np.array([value]), row.dt)[0]
        w = Weights(ops, base.qw, s, base.qz)
        y = run(ops, row, x, w)
        keep = torch.arange(N, device=DEV) != n0
        assert same_bits(y[:, keep], clean[:, keep]), f"{row.label}: scale {value} in column {n0} changed another column"
        with np.errstate(invalid="ignore", over="ignore"):
            want = klass(awq_ref.to_f64(xn, row.dt) @ w.w64(row.dt)[:, n0])
        assert (want == 2).all() if np.isnan(value) else (want != 0).all()
        got = klass(awq_ref.to_f64(to_np(y[:, n0].contiguous()), row.dt))
        assert np.array_equal(got, want), (f"{row.label}: scale {value} in column {n0}: {int((got != want).sum())} of {row.M} outputs of that column have "
                                           f"another class than float64 gives (first row {int(np.argmax(got != want))}: {got[np.argmax(got != want)]} against {want[np.argmax(got != want)]})")


# ------------------------------------------------------------------------------------------------------------------------ e. stale scratch
# every row whose route writes fp32 partial tiles (or the re-laid-out weight) into the per-stream scratch, with a smaller M and another K that
# take the same route through the same bytes: (row, M2, K2)
SCRATCH = [("pf_split", 33, 1536), ("gemv_rps", 9, 8320), ("split_bf16", 65, 2304), ("split_bf16_wide", 65, 2304), ("split_bf16_narrow", 65, 2304),
           ("op_on_the_fly", 33, 1536), ("skinny_f16", 3, 1536), ("skinny_bf16", 3, 1536)]


@pytest.mark.parametrize("label,M2,K2", SCRATCH, ids=[s[0] for s in SCRATCH])
def test_e_stale_scratch(ops, label, M2, K2):
    """A call on NaN activations leaves NaN partial tiles in the scratch, which persists between calls; a later call with fewer rows and
    another K reads none of them: its result is the one the same call gave before."""
    row = ROW[label]
    skip_if_listed(row, "e")
    small = row._replace(M=M2, K=K2)
    w2 = weights(ops, small, "A")
    x2 = to_torch(activations(small), DEV)
    before = run(ops, small, x2, w2)
    assert torch.isfinite(before).all()
    w = weights(ops, row, "A")
    y = run(ops, row, torch.full((row.M, row.K), float("nan"), dtype=TDT[row.dt], device=DEV), w)
    assert torch.isnan(y).all()
    assert same_bits(run(ops, small, x2, w2), before), f"{label}: NaN partial tiles of an earlier call leaked into M={M2} K={K2}"
    _, exact = c_oracle.gemm(to_np(x2), w2.qw, w2.s, w2.qz, want_exact=True)
    assert_gemm_close(to_np(before), exact, row.dt, what=f"{label} M={M2} K={K2}")

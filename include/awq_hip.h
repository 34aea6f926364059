/*
 * awq_hip.h — C ABI of the MI355X (gfx950) AWQ int4 quantized-linear kernels.
 *
 * This is the drop-in boundary for ONE path of kvcache-ai/sglang_awq: the operator pair that
 * AWQLinearMethod.apply() runs (python/sglang/srt/layers/quantization/awq.py:434-451).
 * Plain pointers and sizes only; no torch types; nothing here allocates, frees or synchronises.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer on the GPU that owns `stream`; tensors are dense row-major;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); the call only
 *     enqueues kernels on it — safe inside hipGraph stream capture (model_runner.py:2765-2771
 *     replays the captured decode graph, so the op may not sync or allocate);
 *   - dtype: AWQ_DTYPE_F16 / AWQ_DTYPE_BF16 / AWQ_DTYPE_F32 is the dtype of scales, activations
 *     and outputs (the reference op returns `scales.dtype`, awq_kernel.cu:198-199);
 *   - return value: 0 on success, a negative AWQ_ERR_* code otherwise (never throws, never aborts);
 *   - AWQ tensor format (AutoAWQ "GEMM" layout, consumed as stored on disk):
 *       qweight int32 [K, N/8]   logical column 8c+j in nibble {0,4,1,5,2,6,3,7}[j] of word c
 *       qzeros  int32 [K/g, N/8] same nibble order
 *       scales  dtype [K/g, N]
 *       W[k,n] = (q[k,n] - z[k/g,n]) * s[k/g,n], one rounding in `dtype`.
 */
#ifndef AWQ_HIP_H_
#define AWQ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AWQ_HIP_ABI_VERSION 2

enum awq_dtype { AWQ_DTYPE_F16 = 0, AWQ_DTYPE_BF16 = 1, AWQ_DTYPE_F32 = 2 };

enum awq_status {
  AWQ_OK = 0,
  AWQ_ERR_NULL_POINTER = -1,
  AWQ_ERR_BAD_SHAPE = -2,     /* N % 8 != 0, K % g != 0, non-positive dims, ldx < K */
  AWQ_ERR_BAD_DTYPE = -3,
  AWQ_ERR_BAD_SPLIT_K = -4,   /* split_k_iters not a power of two in [1, 32] (awq_triton.py:307-308) */
  AWQ_ERR_WORKSPACE = -5,     /* workspace missing / smaller than awq_gemm_workspace_bytes() */
  AWQ_ERR_MISALIGNED = -6,    /* a pointer is not 16-byte aligned (the op's uint4 loads: awq_kernel.cu:142,161) */
  AWQ_ERR_BAD_VARIANT = -7,
  AWQ_ERR_LAUNCH = -100       /* hipGetLastError() != hipSuccess after the launch */
};

/* ABI / build identification. */
int awq_hip_abi_version(void);
const char* awq_hip_build_info(void);               /* e.g. "gfx950 hipcc 7.2 ..." (static string) */
const char* awq_hip_status_string(int status);      /* static string for an awq_status value */

/*
 * awq_dequantize — replaces the op `sgl_kernel::awq_dequantize`
 *   schema   sgl-kernel/csrc/common_extension.cc:126-127
 *   host     sgl-kernel/csrc/gemm/awq_kernel.cu:186-221,  kernel :126-184
 *   python   sgl-kernel/python/sgl_kernel/gemm.py:8-11
 * out[K, N] (dtype) <- dequantise(qweight, scales, qzeros); bit-exact with the reference
 * (integer unpack exact, (q - z) exact, one round-to-nearest-even multiply).
 * group_size = K / scales.size(0) as the reference infers it (awq_kernel.cu:189).
 */
int awq_dequantize(const int32_t* qweight, const void* scales, const int32_t* qzeros, void* out,
                   int64_t K, int64_t N, int64_t group_size, int dtype, void* stream);

/*
 * awq_gemm — the fused dequantise + GEMM the north star names `sgl_kernel.awq_gemm`; argument
 * order and meaning follow the only fused GEMM in the reference,
 *   awq_gemm_triton(input, qweight, scales, qzeros, split_k_iters)  awq_triton.py:284-339
 * and the numerics follow what AWQLinearMethod.apply computes (awq.py:446-447): W is rounded to
 * `dtype` element by element exactly as awq_dequantize would, products are accumulated in fp32,
 * the sum is rounded once to `dtype`.
 *
 *   x [M, K] with row stride `ldx` elements (ldx >= K; lets a row-parallel rank pass its K-slice
 *   of a wider activation without a copy: linear.py:1395-1399), y [M, N] dense.
 *   split_k_iters: power of two in [1, 32] (validated like the reference); a HINT — the kernel
 *   picks its own K partition; results do not depend on it and are run-to-run deterministic.
 *   workspace: device scratch of at least awq_gemm_workspace_bytes(...) bytes, 16-byte aligned,
 *   zero-filled ONCE when allocated (arrival counters live in it and every call leaves them
 *   zero again).  It may be shared by successive calls on one stream, not by concurrent streams.
 *   For M > 32 (fp16, K % 128 == 0, g % 128 == 0) awq_gemm_workspace_bytes() also
 *   covers one re-laid-out copy of the weight: the call then repacks on the fly and runs the kernel
 *   of awq_gemm_repacked; with less workspace it keeps to the checkpoint-layout kernels.
 *   bias (may be NULL): [N] in `dtype`, added AFTER the sum is rounded to `dtype`, with a second
 *   rounding — the reference's in-place `out.add_(bias)` (awq.py:449-450).
 */
size_t awq_gemm_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int dtype);

int awq_gemm(const void* x, int64_t ldx, const int32_t* qweight, const void* scales,
             const int32_t* qzeros, const void* bias, void* y, void* workspace, size_t workspace_bytes,
             int64_t M, int64_t K, int64_t N, int64_t group_size, int dtype, int split_k_iters,
             void* stream);

/*
 * Same as awq_gemm with the kernel variant forced (tests and A/B benchmarks).  variant:
 *   AWQ_GEMM_AUTO     the heuristic awq_gemm uses
 *   AWQ_GEMM_GENERIC  any shape / dtype, VALU, no MFMA
 *   AWQ_GEMM_SKINNY   M <= 32: dequantised tiles fed straight from registers to MFMA,
 *                     K split over waves and workgroups, in-launch deterministic reduction
 *   AWQ_GEMM_TILED    large M: LDS-staged MFMA tiles
 * `tune` packs variant-specific knobs (0 = defaults); see csrc/awq_capi.hip.
 * Returns AWQ_ERR_BAD_VARIANT if the variant cannot run the given shape.
 */
enum awq_gemm_variant { AWQ_GEMM_AUTO = 0, AWQ_GEMM_GENERIC = 1, AWQ_GEMM_SKINNY = 2, AWQ_GEMM_TILED = 3 };

int awq_gemm_ex(const void* x, int64_t ldx, const int32_t* qweight, const void* scales,
                const int32_t* qzeros, const void* bias, void* y, void* workspace, size_t workspace_bytes,
                int64_t M, int64_t K, int64_t N, int64_t group_size, int dtype, int split_k_iters,
                int variant, int64_t tune, void* stream);

/*
 * Optional one-time re-layout for decode.  The reference re-lays AWQ weights out only for
 * its NVIDIA Marlin path (sgl-kernel/csrc/gemm/marlin/awq_marlin_repack.cu:13-253, called from
 * AWQMarlinLinearMethod.process_weights_after_loading); its plain AWQ method keeps the checkpoint layout
 * (awq.py:429-432).  awq_repack writes an MFMA-fragment-major copy of (qweight, qzeros, scales) into
 * `packed` (awq_repacked_bytes() bytes, 16-byte aligned); awq_gemm_repacked then computes the same result as
 * awq_gemm — same per-element rounding, fp32 accumulation, bias epilogue — from that copy: for M <= 32 a
 * streaming GEMV (linear weight stream, no cross-workgroup reduction, no workspace), for larger M an MFMA-bound
 * tiled kernel whose B fragments go from the copy straight to registers (an M <= 32 call whose reduction scratch
 * would not fit returns AWQ_ERR_BAD_VARIANT: use awq_gemm).
 * Supported: fp16 or bf16 (the dtype of the scales the copy is made from = the dtype of x and y), K % 128 == 0, group_size a
 * multiple of 128 or one of 32 / 64 (the group sizes of the reference's Triton path, awq_triton.py:250); otherwise
 * awq_repacked_bytes returns 0 and the other two return AWQ_ERR_BAD_VARIANT (callers keep using awq_gemm).  The hand-tuned kernels
 * (straight-line / loop-form GEMV, hand-pipelined prefill tiles) exist for fp16 with group_size % 128 == 0; bf16 and the small
 * groups run compiler-scheduled kernels on the same layout.
 */
size_t awq_repacked_bytes(int64_t K, int64_t N, int64_t group_size, int dtype);

int awq_repack(const int32_t* qweight, const void* scales, const int32_t* qzeros, void* packed, int64_t K,
               int64_t N, int64_t group_size, int dtype, void* stream);

int awq_gemm_repacked(const void* x, int64_t ldx, const void* packed, const void* bias, void* y, int64_t M,
                      int64_t K, int64_t N, int64_t group_size, int dtype, void* stream);

/*
 * awq_gemm_repacked with an optional scratch buffer (>= awq_gemm_repacked_workspace_bytes(), 16-byte aligned, its first 4096 bytes
 * zero-filled ONCE when allocated — arrival counters, left at zero by every call — one buffer per stream of execution, the same rules
 * as awq_gemm's).  Two routes use it:
 *   9 .. 32 rows on a narrow matrix (N <= 8192): the one-strip-per-workgroup GEMV re-reads all of x in every workgroup; with the scratch
 *     that case runs wide strips with K split across workgroups (fp32 partials summed in fixed order by the last workgroup to arrive);
 *   33 rows and up where the MFMA tiling leaves most CUs without a tile (narrow or deep matrices, up to a few hundred rows): the tile
 *     kernel runs with K split over workgroups, fp32 partial tiles go to the scratch and a second small launch adds them in slice order,
 *     adds the bias and rounds once (11008 x 4096 at 128 rows: 89 -> 26 us).  fp16 from 33 rows; bf16 (group_size % 128 == 0) from 65
 *     rows — up to 64 rows bf16 uses no scratch and the query returns 0.
 * Both are deterministic; sums agree with the no-workspace routes to fp32 rounding, not bit for bit.  The same holds for the
 * shared-activation GEMV (AWQ_RP_SHARED_X below) against the kernels it replaces at 17 .. 32 rows: same per-element rounding of W, fp32
 * accumulation and one final rounding, another fp32 summation order.  workspace == NULL or too small:
 * exactly awq_gemm_repacked.  awq_gemm_repacked_workspace_bytes returns 0 where the scratch would not be used (at most 4096 + 32 MiB).
 */
size_t awq_gemm_repacked_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t group_size, int dtype);

int awq_gemm_repacked_ws(const void* x, int64_t ldx, const void* packed, const void* bias, void* y, void* workspace,
                         size_t workspace_bytes, int64_t M, int64_t K, int64_t N, int64_t group_size, int dtype, void* stream);

/*
 * Same as awq_gemm_repacked_ws with the decode kernel forced (tests and A/B benchmarks).  variant:
 *   AWQ_RP_AUTO      exactly awq_gemm_repacked_ws
 *   AWQ_RP_SHARED_X  1 <= M <= 32, fp16, group_size % 128 == 0, N <= 32768, ldx % 8 == 0, x 16-byte aligned: one strip of column
 *                    groups per workgroup; the activations are loaded once per workgroup into LDS in MFMA operand order and shared
 *                    by all its waves, which split the strip's (k-block, column group) units.  No workspace is used.
 *   AWQ_RP_SHARED_X_WIDE  33 <= M <= 64, fp16, group_size % 128 == 0, 8192 < N <= 32768 (strips of 3 .. 8 column groups),
 *                    ldx % 8 == 0, ldx < 2^24, x 16-byte aligned, K / 128 < 4096: the same split with every dequantised weight
 *                    fragment multiplied into three (M <= 48) or four row tiles and every activation fragment into two column
 *                    groups.  No workspace is used.
 *   AWQ_RP_SHARED_X_BF16  bf16, group_size % 128 == 0, ldx % 8 == 0, x 16-byte aligned, K / 128 < 4096: the bf16 form of
 *                    AWQ_RP_SHARED_X, its dequantisation kept in fp32.  1 <= M <= 32 on N <= 32768: one launch (one row tile up to
 *                    16 rows, two above); 33 <= M <= 64 on 8192 < N <= 32768: two launches of it (rows 0 .. 31, then the rest).
 *                    Every weight is the bf16 awq_dequantize produces (for normal scales of magnitude >= 2^-122; see
 *                    awq_repacked_sharedx_bf16.hip).  No workspace is used.  Not built: a bf16 form of AWQ_RP_SHARED_X_WIDE (three /
 *                    four row tiles in one launch) gave wrong sums on the MI355X for a reason not found.
 *                    AWQ_RP_SHARED_X and AWQ_RP_SHARED_X_WIDE refuse bf16; this variant refuses fp16.
 *   AWQ_RP_TILES_BF16  any M >= 1, bf16, group_size % 128 == 0, ldx % 8 == 0, x 16-byte aligned, spans inside 32-bit buffer
 *                    offsets (ldx < 2^22): the hand-pipelined bf16 MFMA tiles (awq_repacked_prefill_bf16.hip), planned as the
 *                    automatic route runs them: 128 x 256 tiles for whole rounds of the CUs + 128 x 192 tiles for the remaining
 *                    columns, or 128 x 128 tiles where that is cheaper.  Every weight is the bf16 awq_dequantize produces (normal
 *                    scales of magnitude >= 2^-122).  No workspace is used.
 *   AWQ_RP_TILES_BF16_WIDE  the same kernel and domain: floor(ceil(N / 16) / 16) whole 256-wide column tiles in one launch, the
 *                    remaining column groups in 192-wide tiles in a second.
 *   AWQ_RP_TILES_BF16_NARROW  the same kernel and domain: 128 x 128 tiles everywhere, one launch.
 *                    The three refuse fp16 and group sizes 32 / 64.
 *   AWQ_RP_GEMV_BF16  1 <= M <= 16, bf16, group_size % 128 == 0, N <= 32768 (one strip of at most 8 column groups per
 *                    workgroup), ldx % 8 == 0, x 16-byte aligned, K / 128 < 4096: the straight-line decode GEMV in bf16
 *                    (awq_repacked_gemv_bf16.hip) — 16 waves, x and the (scale | zero) words staged once per wave through
 *                    wave-private LDS, a ring of two weight loads per wave, dequantisation kept in fp32 (as
 *                    AWQ_RP_SHARED_X_BF16) with its per-column constants precomputed into LDS in the one-row form.  ceil(K / 2048) k-blocks per
 *                    wave: at most 16 units (strip width x k-blocks per wave) with at most 8 k-blocks per wave, at one row up to 32
 *                    units with at most 16; M x k-blocks per wave <= 32; the staging area within 144 KiB of LDS (16 rows: K <= 4096,
 *                    at K > 2048 on strips of at most 5 column groups).  Every weight is the bf16 awq_dequantize produces
 *                    (normal scales of magnitude >= 2^-122).  No workspace is used.  Refuses fp16 and group sizes 32 / 64.
 *                    Error precedence differs from the other variants here: fp16, M > 16 or group_size % 128 != 0 return
 *                    AWQ_ERR_BAD_VARIANT before the pointer and shape checks (that part of the domain needs no pointer), so such a call
 *                    is a refused variant even with NULL arguments.
 *   AWQ_RP_TILES_SG  any M >= 1, fp16, group_size 32 or 64, ldx % 8 == 0, x 16-byte aligned, spans inside 32-bit buffer offsets
 *                    (ldx < 2^22): the hand-pipelined MFMA tiles for the small groups (awq_repacked_prefill_sg.hip), planned as the
 *                    automatic route runs them: 128 x 256 tiles for whole rounds of the CUs + 128 x 192 tiles for the remaining
 *                    columns, or 128 x 128 tiles where that is cheaper.  Every k-step of 32 rows dequantises with the (scale | zero)
 *                    word of its own quantisation group; every weight is the fp16 awq_dequantize produces.  No workspace is used.
 *   AWQ_RP_TILES_SG_WIDE  the same kernel and domain: floor(ceil(N / 16) / 16) whole 256-wide column tiles in one launch, the
 *                    remaining column groups in 192-wide tiles in a second.
 *   AWQ_RP_TILES_SG_NARROW  the same kernel and domain: 128 x 128 tiles everywhere, one launch.
 *                    The three refuse bf16 and group sizes that are multiples of 128.
 *   AWQ_RP_SPLIT_BF16  any M >= 1, bf16, group_size % 128 == 0, N % 4 == 0, ldx % 8 == 0, x 16-byte aligned, spans inside 32-bit
 *                    buffer offsets, and a 16-byte aligned workspace behind whose 4096-byte head at least two M x N fp32 slices fit:
 *                    the bf16 MFMA tiles with K split over S workgroups per tile (awq_repacked_prefill_bf16.hip) and a second launch
 *                    that adds the fp32 partial tiles in slice order, rounds once and adds the bias.  S = min(256 / tiles, 8,
 *                    (K / 128) / 4, slices the workspace holds); fewer than two slices (K < 1024, or more than 128 tiles): refused.
 *                    128 x 128 tiles while there are few of them, 128 x 256 beyond, as the automatic route plans it — but wherever
 *                    the domain allows, not only where it measured faster.  This is the one forced variant that uses the workspace.
 *   AWQ_RP_SPLIT_BF16_WIDE  the same kernel and domain on 128 x 256 tiles.
 *   AWQ_RP_SPLIT_BF16_NARROW  the same kernel and domain on 128 x 128 tiles.
 *                    The three refuse fp16, group sizes 32 / 64 and a missing, misaligned or too small workspace.
 * Returns AWQ_ERR_BAD_VARIANT for an unknown variant or a shape / dtype outside the variant's domain; nothing is launched then.
 * (Enumerators are only ever added: an added variant does not move AWQ_HIP_ABI_VERSION.)
 */
enum awq_repacked_variant {
  AWQ_RP_AUTO = 0, AWQ_RP_SHARED_X = 1, AWQ_RP_SHARED_X_WIDE = 2, AWQ_RP_SHARED_X_BF16 = 3,
  AWQ_RP_TILES_BF16 = 4, AWQ_RP_TILES_BF16_WIDE = 5, AWQ_RP_TILES_BF16_NARROW = 6, AWQ_RP_GEMV_BF16 = 7,
  AWQ_RP_TILES_SG = 8, AWQ_RP_TILES_SG_WIDE = 9, AWQ_RP_TILES_SG_NARROW = 10,
  AWQ_RP_SPLIT_BF16 = 11, AWQ_RP_SPLIT_BF16_WIDE = 12, AWQ_RP_SPLIT_BF16_NARROW = 13
};

int awq_gemm_repacked_ex(const void* x, int64_t ldx, const void* packed, const void* bias, void* y, void* workspace,
                         size_t workspace_bytes, int64_t M, int64_t K, int64_t N, int64_t group_size, int dtype, int variant,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AWQ_HIP_H_ */

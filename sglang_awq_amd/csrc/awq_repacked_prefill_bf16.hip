// bf16 tile GEMM on the MFMA-fragment-major layout, software-pipelined by hand (gfx950): the bf16 sibling of
// gemm_repacked_pipelined_kernel (awq_repacked_prefill.hip), reached as AWQ_RP_TILES_BF16 / _WIDE / _NARROW.  Before it every bf16
// batch of more than 64 rows (and the 33 .. 64-row cells the bf16 GEMV is not routed in) ran gemm_rpx_tiled_kernel
// (awq_repacked_ext.hip): compiler-scheduled, 128 x 256 tiles only, ~29 VALU per dword through fp16.
//
// What carried over from the fp16 kernel unchanged: workgroup tile 128 x (64 NJ) — NJ = 4 / 3 / 2 column groups per wave: 128 x 256,
// 128 x 192 (remainder region) and 128 x 128 tiles — four waves of 8 row tiles x NJ column groups; accumulators tied in the AGPR
// file (inline-asm MFMA, "+a"; the s_nop guard before the compiler-scheduled reads); B never touches LDS (a wave dequantises the
// dwords of its own columns and reuses every fragment for 8 row tiles); x through two XOR-swizzled 32 KiB LDS buffers
// (v_mfma_f32_16x16x32_bf16 takes its A operand in the lane order of the f16 form); one barrier per k-block inside its last k-step;
// every global load of the loop a buffer load with an SGPR base; XCD-aware tile order in super-rows of 4 row tiles; the output tile
// through the idle x buffers, 16 bytes per lane.
//
// What is new: the dequantisation pipeline.  Every W element must be the bf16 awq_dequantize produces: (q - z) exact, exact fp32
// product with the scale, one round-to-nearest-even.  The dword goes through the fp16 magic words straight into mixed-precision fmas:
//   t0 = (w & 0x000f000f) | 0x64006400         halves 1024 + q      (k0, k1)        t2: the same of w >> 8   (k4, k5)
//   t1 = (w & 0x00f000f0) | 0x64006400         halves 1024 + 16 q   (k2, k3)        t3: the same of w >> 8   (k6, k7)
//   v_fma_mix_f32 (op_sel picks the half):  (1024 + q) s - (1024 + z) s   resp.   (1024 + 16 q) (s / 16) - (64 + z) s
//   v_cvt_pk_bf16_f32 per k-pair.
// 1 shift + 4 v_and_or_b32 + 8 v_fma_mix_f32 + 4 v_cvt_pk_bf16_f32 = 17 VALU per dword (the fp32 route of awq_repacked_sharedx_bf16.hip:
// 18; through fp16: 29).  s has an 8-bit significand, 1024 + q / 1024 + z 11 bits, so both products are exact in fp32 and so is their
// difference (q - z) s (at most 13 significant bits): the fma's one rounding returns it exactly, the conversion is the one RNE.  As in
// the bf16 GEMV this holds for normal scales whose s / 16 is normal too (|s| >= 2^-122); q = z gives +0 where the generic form gives
// -0 under a negative scale.  Per (column, k-block) the constants s, s / 16, -(1024 + z) s and -(64 + z) s cost 4 VALU from the
// (bf16 scale | fp16(1024 + zero)) word: shift, v_fma_mix_f32 of the word's high half, fma with 960 s, multiply.
//
// Slot table.  An MFMA 16x16x32 holds the matrix pipe for 16 cycles and the issue port for 8: two VALU ops ride free behind each
// (fp16: 13 ops per dword in 7 stages, 3 of a fragment's 16 slots left for passengers).  Per k-block and wave at NJ = 4: 128 MFMAs =
// 256 free VALU slots; wanted are 16 x 17 = 272 dequantisation ops + 4 x 4 = 16 constant ops = 288, so 32 of the 128 MFMAs carry a
// third VALU op (by this count 32 x 4 of 2048 cycles, 6 %, if everything else hides; not measured separately):
//   behind MFMA (row tile) 0: w8 = w >> 8, t0      1: t1, t2      2: t3, a0 = mix(t0.lo)      3: a1 = mix(t0.hi), b0 = mix(t1.lo)
//               4: b1, f0 = cvt_pk(a0, a1)         5: c0, c1 (t2) 6: d0 = mix(t3.lo), f1 = cvt_pk(b0, b1)
//               7: d1, f2 = cvt_pk(c0, c1), f3 = cvt_pk(d0, d1)                                  <- the third op, once per fragment
//   constants of the next k-block, one op each behind MFMAs 0 .. 3 (the third op there): column group 0 during fragment (d, j) =
//   (2, NJ - 1), group j + 1 during (3, j) — each ready one fragment before the first dequantisation stage that reads it (stage 2).
// The passengers that are not VALU keep the fp16 kernel's places: the 8 LDS reads of the next k-step's x fragments behind the MFMAs
// of every j = 1 fragment; the 8 LDS writes of the next x tile behind every fourth MFMA of (1, 2) (1, 3) (2, 0) (2, 1) (NJ = 3: MFMAs
// 0, 3, 6 of (1, 2) (2, 0) (2, 2); NJ = 2: every second MFMA of (1, 0) (2, 0)); the request for the tile after it behind them; the
// barrier behind the first MFMA of (3, 0).
//
// AWQ-MoE form (template parameters MOE, EPI at NJ = 4; awq_aux_moe_gemm_blocks with bf16): 128-row blocks of expert-sorted (token,
// expert) pairs, the expert chosen per row tile, x rows gathered and output rows scattered through row_map — see PfbMoe below.  Only the
// tile order, the x offsets and the epilogue differ from the dense form (198 / 199 VGPRs + 128 AGPRs, zero scratch, as the dense 199).
// 64-row tiles (MI = 4) would need a slot table of their own (17 ops behind 4 MFMAs) and are not built.
//
// Split-K form (template parameter SPLIT at NJ = 2 / 4, dense; AWQ_RP_SPLIT_BF16 / _WIDE / _NARROW and, from 65 rows with a workspace,
// the automatic route): under-filled launches cut K over workgroups, fp32 partial tiles go to the workspace and a second launch adds
// them — see PfbSplit below and pfb_split_plan.  The loop body is the unsplit one: only where K starts and ends, the tile order and
// the epilogue differ (198 VGPRs + 128 AGPRs / 141 + 64, zero scratch).
#include <cstdlib>

#include "awq_prefill_common.h"

namespace awq {

typedef __bf16 pfb_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float pfb_float2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void pfb_mfma_tied(float4_t& acc, const u32x4_t& a, const u32x4_t& b) {
  asm("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}

// fmaf((float)half HI of t, m, c): one v_fma_mix_f32, in the operand form hipcc itself emits for that expression.  Inline asm because
// left to itself hipcc turns the two halves of a word into 2 v_cvt_f32_f16 + 1 v_pk_fma_f32 (same values, 12 ops per dword instead of 8).
template <int HI>
__device__ __forceinline__ float pfb_mix(uint32_t t, float m, float c) {
  float d;
  if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(d) : "v"(t), "v"(m), "v"(c));
  else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(t), "v"(m), "v"(c));
  return d;
}

__device__ __forceinline__ uint32_t pfb_pack(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((pfb_float2_t){lo, hi}, pfb_bf16x2_t));
}

// constants of one (column, quantisation group) from its (bf16 scale | fp16(1024 + zero)) word, in four one-op stages
struct PfbZs { float s, s16, c1024, c64; };       // s, s / 16, -(1024 + z) s, -(64 + z) s
template <int S>
__device__ __forceinline__ void pfb_zs_stage(PfbZs& u, uint32_t zw) {
  if constexpr (S == 0) u.s = __builtin_bit_cast(float, zw << 16);
  if constexpr (S == 1)                                                      // fmaf((float)high half, -s, 0); exact: 11 x 8 bits
    asm("v_fma_mix_f32 %0, %1, -%2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(u.c1024) : "v"(zw), "v"(u.s));
  if constexpr (S == 2) u.c64 = __builtin_fmaf(960.f, u.s, u.c1024);         // exact: -(64 + z) s has 7 x 8 bits
  if constexpr (S == 3) u.s16 = u.s * 0.0625f;
}
__device__ __forceinline__ PfbZs pfb_zs_unpack(uint32_t zw) {
  PfbZs u;
  pfb_zs_stage<0>(u, zw); pfb_zs_stage<1>(u, zw); pfb_zs_stage<2>(u, zw); pfb_zs_stage<3>(u, zw);
  return u;
}

struct PfbPipe {           // one dword on its way to becoming a fragment
  uint32_t w, w8, t0, t1, t2, t3;
  float a0, a1, b0, b1, c0, c1, d0, d1;
  u32x4_t f;
};

template <int S>
__device__ __forceinline__ void pfb_stage(PfbPipe& p, const PfbZs& z) {
  const uint32_t magic = kMagicF16;
  if constexpr (S == 0) { p.w8 = p.w >> 8; p.t0 = and_or(p.w, kLoNib, magic); }
  if constexpr (S == 1) { p.t1 = and_or(p.w, kHiNib, magic); p.t2 = and_or(p.w8, kLoNib, magic); }
  if constexpr (S == 2) { p.t3 = and_or(p.w8, kHiNib, magic); p.a0 = pfb_mix<0>(p.t0, z.s, z.c1024); }
  if constexpr (S == 3) { p.a1 = pfb_mix<1>(p.t0, z.s, z.c1024); p.b0 = pfb_mix<0>(p.t1, z.s16, z.c64); }
  if constexpr (S == 4) { p.b1 = pfb_mix<1>(p.t1, z.s16, z.c64); p.f[0] = pfb_pack(p.a0, p.a1); }
  if constexpr (S == 5) { p.c0 = pfb_mix<0>(p.t2, z.s, z.c1024); p.c1 = pfb_mix<1>(p.t2, z.s, z.c1024); }
  if constexpr (S == 6) { p.d0 = pfb_mix<0>(p.t3, z.s16, z.c64); p.f[1] = pfb_pack(p.b0, p.b1); }
  if constexpr (S == 7) { p.d1 = pfb_mix<1>(p.t3, z.s16, z.c64); p.f[2] = pfb_pack(p.c0, p.c1); p.f[3] = pfb_pack(p.d0, p.d1); }
}

// the same operations in one piece (prologue: the first fragment of k-block 0)
__device__ __forceinline__ u32x4_t pfb_dequant(uint32_t w, const PfbZs& z) {
  PfbPipe p;
  p.w = w;
  pfb_stage<0>(p, z); pfb_stage<1>(p, z); pfb_stage<2>(p, z); pfb_stage<3>(p, z);
  pfb_stage<4>(p, z); pfb_stage<5>(p, z); pfb_stage<6>(p, z); pfb_stage<7>(p, z);
  return p.f;
}

constexpr int kPfbThreads = 256;
constexpr int kPfbRowBlock = 4;       // row tiles per super-row of the tile order (as PF_ROW_BLOCK of the fp16 kernel)

// NJ = column groups (16 columns) per wave: 4 -> 128 x 256 tiles, 3 -> 128 x 192, 2 -> 128 x 128.  A launch covers the column groups
// [cg_base, cg_base + ng_region) of the matrix (the host cuts N into regions: launch_gemm_repacked_tiles_bf16).
//
// MOE (AWQ-MoE prefill, NJ = 4; awq_aux_moe_gemm_blocks with bf16): the rows are (token, expert) pairs grouped by expert into 128-row
// blocks (awq_aux_moe_align_blocks_n); row tile t takes its weights from expert block_expert[t] (expert_stride bytes apart; < 0: unused
// tile, the workgroup leaves before any barrier), its row r reads activation row row_map[128 t + r] / x_div and writes output row
// row_map[128 t + r] (-1 = padding: reads row 0, stores nothing), the fp32 sums multiplied by slot_scale[pair] before the one rounding.
// Plain tile order (the row tiles of a super-row would belong to different experts).  EPI = 1: the column groups alternate gate / up
// and act = bf16(bf16(silu(bf16 gate)) * bf16 up) is written, N / 2 wide.  The slot table and the main loop are those of the dense form.
struct PfbMoe {
  const int* row_map;
  const int* block_expert;
  const float* slot_scale;
  long long expert_stride;
  int x_div;
};

// Split-K over workgroups for under-filled launches (SPLIT; dense form, NJ = 2 / 4; 65 rows up, a workspace given): the launch has
// tiles x S workgroups, slice s owns the k-blocks [s kb_per, min(K / 128, (s + 1) kb_per)) and everything that walks K starts at its first
// one; the look-ahead of a slice's last k-block is clamped to the slice as the unsplit kernel clamps it to the matrix.  A workgroup writes
// its fp32 partial tile to part[slice][M][N] with plain stores; pf_splitk_reduce_kernel<bf16> (a second launch: the kernel boundary orders
// them) adds the slices in slice order, rounds once and adds the bias.  A template parameter, so the unsplit forms compile as before.
struct PfbSplit {
  float* part;
  int S;
  int kb_per;
};

template <int NJ, bool MOE = false, int EPI = 0, bool SPLIT = false>
__global__ __launch_bounds__(kPfbThreads, 1) void gemm_repacked_pipelined_bf16_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                                                       const u32x4_t* __restrict__ qw_r,
                                                                                       const uint32_t* __restrict__ zs_r,
                                                                                       const void* __restrict__ bias, void* __restrict__ y,
                                                                                       int M, int K, int N, int g, int NG, int nbx, int nby,
                                                                                       int cg_base, int ng_region, PfbMoe moe, PfbSplit split) {
  static_assert(NJ >= 2 && NJ <= 4, "128 x 128 .. 128 x 256 tiles");
  static_assert(!SPLIT || (!MOE && NJ != 3), "split-K: dense 128 x 128 / 128 x 256 tiles");
  static_assert(!MOE || NJ == 4, "expert blocks run 128 x 256 tiles");
  static_assert(!EPI || MOE, "SiLU-mul epilogue: whole (gate, up) pairs per wave, MoE form only");
  extern __shared__ __attribute__((aligned(16))) unsigned char As[];      // 2 x 32 KiB
  constexpr int MI = 8, BM = kPfBM, AL = 8;           // row tiles per wave; rows per workgroup tile; x-tile chunks (16 B) per thread
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave-uniform: every weight / scale address is an SGPR base + a lane offset
  const int q = lane >> 4, r = lane & 15;
  const int KBT = K / 128, groups = K / g, kpg = g / 128;

  const int ntile = nbx * nby, nwg = SPLIT ? ntile * split.S : ntile, bid = blockIdx.x;
  const int xcd = bid & 7, qd = nwg >> 3, rem = nwg & 7;
  const int logical_all = (xcd < rem ? xcd * (qd + 1) : rem * (qd + 1) + (xcd - rem) * qd) + (bid >> 3);
  const int slice = SPLIT ? logical_all / ntile : 0, logical = SPLIT ? logical_all - slice * ntile : logical_all;
  const int k0 = SPLIT ? slice * split.kb_per : 0;                  // this workgroup's k-blocks: [k0, k0 + KB)
  const int KB = SPLIT ? (KBT - k0 < split.kb_per ? KBT - k0 : split.kb_per) : KBT;
  // the 32 tiles an XCD runs together cover 4 row tiles x 8 column tiles: x and weights each shared in its L2 (see the fp16 kernel)
  const int sb_tiles = kPfbRowBlock * nbx, sb = logical / sb_tiles, in_sb = logical - sb * sb_tiles;
  const int rows_sb = nby - sb * kPfbRowBlock < kPfbRowBlock ? nby - sb * kPfbRowBlock : kPfbRowBlock;
  int bm = (sb * kPfbRowBlock + in_sb % rows_sb) * BM;
  int cg_tile = cg_base + (in_sb / rows_sb) * (4 * NJ) + wn * NJ;             // this wave's first column group
  const int cg_end = cg_base + ng_region < NG ? cg_base + ng_region : NG;
  if constexpr (MOE || SPLIT) {                         // plain order: the column tiles of an expert's row tile together / few tiles per slice
    bm = (logical / nbx) * BM;
    cg_tile = cg_base + (logical % nbx) * (4 * NJ) + wn * NJ;
  }
  if constexpr (MOE) {
    const int eid = moe.block_expert[bm / BM];          // uniform over the workgroup, read before any barrier
    if (eid < 0) return;
    qw_r = (const u32x4_t*)((const unsigned char*)qw_r + (long long)eid * moe.expert_stride);
    zs_r = (const uint32_t*)((const unsigned char*)zs_r + (long long)eid * moe.expert_stride);
  }

  __amdgpu_buffer_rsrc_t rw[NJ];                       // this wave's column groups: [KB][64 lanes] dwordx4
  uint32_t zoff_s[NJ];                                 // byte offset of the group's first scale word in zs_r
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = cg_tile + j;
    const int cgj = c < cg_end ? c : cg_end - 1;       // clamped: groups outside the region are never stored
    rw[j] = __builtin_amdgcn_make_buffer_rsrc((void*)(qw_r + ((size_t)cgj * KBT + k0) * 64), 0, KB * 1024, kPfRsrcFlags);
    zoff_s[j] = (uint32_t)cgj * (uint32_t)groups * 64u;
  }
  const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)zs_r, 0, 0x7fffffff, kPfRsrcFlags);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (MOE ? (size_t)0 : (size_t)bm * ldx) + (size_t)k0 * 128), 0, 0x7fffffff, kPfRsrcFlags);
  const int lane16 = lane * 16, r4 = r * 4;

  u32x4_t a_st[AL];
  u32x4_t w_cur[NJ], w_nxt[NJ];
  uint32_t zs_nxt[NJ];
  PfbZs zu[NJ], zu_nxt[NJ];

  // this thread's AL rows / chunks of the x tile: byte offsets from the tile's first row (rows >= M re-read row M - 1: never stored)
  uint32_t xoff[AL];
#pragma unroll
  for (int i = 0; i < AL; ++i) {
    const int c = tid + kPfbThreads * i;
    const int row = c >> 4, chunk = c & 15;
    int mr = bm + row < M ? row : M - 1 - bm;
    if constexpr (MOE) {                               // byte offsets from x itself (below 2 GiB: the host's guard)
      const int pr = moe.row_map[bm + row];
      mr = pr >= 0 ? pr / moe.x_div : 0;
    }
    xoff[i] = (uint32_t)((size_t)mr * ldx + chunk * 8) * 2u;
  }
  auto load_a = [&](int kb) {
#pragma unroll
    for (int i = 0; i < AL; ++i) a_st[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, xoff[i], kb * 256, 0);
  };
  auto store_a1 = [&](int buf, int i) {
    const int c = tid + kPfbThreads * i;
    *(u32x4_t*)(As + buf * (BM * 256) + pfp_off(c >> 4, c & 15)) = a_st[i];
  };
  auto load_b = [&](u32x4_t (&w)[NJ], uint32_t (&zs)[NJ], int kb, int grp) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      w[j] = __builtin_amdgcn_raw_buffer_load_b128(rw[j], lane16, kb * 1024, 0);
      zs[j] = __builtin_amdgcn_raw_buffer_load_b32(rz, r4, zoff_s[j] + grp * 64, 0);
    }
  };

  float4_t acc[MI][NJ];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[mi][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

  // prologue: x tile 0 into LDS, k-block 0's weights / scales in registers, its first fragment dequantised (k-blocks counted from k0)
  load_a(0);
  int grp_n = SPLIT ? k0 / kpg : 0, cnt_n = SPLIT ? k0 - grp_n * kpg : 0;   // quantisation group of the next k-block, counted up (no division in the loop)
  load_b(w_cur, zs_nxt, 0, grp_n);
#pragma unroll
  for (int i = 0; i < AL; ++i) store_a1(0, i);
#pragma unroll
  for (int j = 0; j < NJ; ++j) zu[j] = pfb_zs_unpack(zs_nxt[j]);
  u32x4_t frag = pfb_dequant(w_cur[0][0], zu[0]);
  load_a(KB > 1 ? 1 : 0);                              // tile 1 travels while block 0 computes
  __syncthreads();
  u32x4_t af[MI], af_n[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) af[mi] = *(const u32x4_t*)(As + pfp_off(mi * 16 + r, q));

  // One barrier per k-block, in the middle of its last k-step: by then every wave has read all it needs from the current x buffer (the
  // d = 3 fragments are fetched during d = 2) and has written its share of the next tile into the other buffer (during d = 1 / 2).
  for (int kb = 0; kb < KB; ++kb) {
    const int nxt = kb + 1 < KB ? kb + 1 : kb;         // clamped, unconditional prefetch (no branch between load and use)
    const unsigned char* Ab = As + (kb & 1) * (BM * 256);
    const int nbuf = (kb + 1) & 1;
    const unsigned char* An = As + nbuf * (BM * 256);
    const int nx2 = kb + 2 < KB ? kb + 2 : KB - 1;
    if (kb + 1 < KB && ++cnt_n == kpg) { cnt_n = 0; ++grp_n; }
    load_b(w_nxt, zs_nxt, nxt, grp_n);
    __builtin_amdgcn_sched_barrier(0);

#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        // the fragment after (d, j): (d, j + 1), then (d + 1, 0), then k-block kb + 1's (0, 0)
        PfbPipe p;
        PfbZs zn;
        if (j < NJ - 1) { p.w = w_cur[j + 1][d]; zn = zu[j + 1]; }
        else if (d < 3) { p.w = w_cur[0][d + 1]; zn = zu[0]; }
        else { uint32_t w0 = w_nxt[0][0]; pin_here(w0); p.w = w0; zn = zu_nxt[0]; }
        // whose constants are unpacked behind MFMAs 0 .. 3 of this fragment (-1: nobody's)
        const int zj = (d == 2 && j == NJ - 1) ? 0 : (d == 3 && j < NJ - 1) ? j + 1 : -1;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          pfb_mfma_tied(acc[mi][j], af[mi], frag);
          switch (mi) {                                  // (compile-time after unrolling)
            case 0: pfb_stage<0>(p, zn); if (zj >= 0) { pin_here(zs_nxt[zj]); pfb_zs_stage<0>(zu_nxt[zj], zs_nxt[zj]); } break;
            case 1: pfb_stage<1>(p, zn); if (zj >= 0) pfb_zs_stage<1>(zu_nxt[zj], zs_nxt[zj]); break;
            case 2: pfb_stage<2>(p, zn); if (zj >= 0) pfb_zs_stage<2>(zu_nxt[zj], zs_nxt[zj]); break;
            case 3: pfb_stage<3>(p, zn); if (zj >= 0) pfb_zs_stage<3>(zu_nxt[zj], zs_nxt[zj]); break;
            case 4: pfb_stage<4>(p, zn); break;
            case 5: pfb_stage<5>(p, zn); break;
            case 6: pfb_stage<6>(p, zn); break;
            default: pfb_stage<7>(p, zn); break;
          }
          // passengers (read in the order 7 .. 0: the first consumer, row tile 0, then waits for the youngest read — one s_waitcnt per
          // k-step; the same for the x-tile registers written to LDS youngest first)
          if (d < 3 && j == 1) af_n[MI - 1 - mi] = *(const u32x4_t*)(Ab + pfp_off((MI - 1 - mi) * 16 + r, (d + 1) * 4 + q));   // next k-step's x fragments
          if constexpr (NJ == 4) {
            if (((d == 1 && j >= 2) || (d == 2 && j <= 1)) && (mi & 3) == 0) store_a1(nbuf, AL - 1 - (((d - 1) * 4 + j - 2) * 2 + (mi >> 2)));
            if (d == 2 && j == 2 && mi == 0) load_a(nx2);
          } else {
            const int slot = NJ == 3 ? ((d == 1 && j == 2) ? 0 : (d == 2 && j == 0) ? 1 : (d == 2 && j == 2) ? 2 : -1)
                                     : ((d == 1 && j == 0) ? 0 : (d == 2 && j == 0) ? 1 : -1);     // (compile-time after unrolling)
            constexpr int PER = NJ == 3 ? 3 : 2, CNT = (MI + PER - 1) / PER;
            if (slot >= 0 && mi % PER == 0 && slot * CNT + mi / PER < AL) store_a1(nbuf, AL - 1 - (slot * CNT + mi / PER));
            if (d == 2 && j == NJ - 1 && mi == MI - 1) load_a(nx2);
          }
          if (d == 3 && j == 0 && mi == 0) __syncthreads();
          if (d == 3 && j == 1) af_n[MI - 1 - mi] = *(const u32x4_t*)(An + pfp_off((MI - 1 - mi) * 16 + r, q));    // next k-block's first fragments
          __builtin_amdgcn_sched_barrier(0);
        }
        frag = p.f;
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) af[mi] = af_n[mi];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) { w_cur[j] = w_nxt[j]; zu[j] = zu_nxt[j]; }
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs' results must have left the pipe before the (compiler-scheduled) reads below

  // the output tile: rounded (and biased, second rounding) exactly as store_output<bf16> does, parked wave-privately in the idle x
  // buffers 64 rows at a time, stored as 16 bytes per lane (8 lanes per 128-byte row run of a 64-column wave)
  if constexpr (MOE) {
    // the same route with the routed weight on the fp32 sums and, EPI = 1, SiLU-mul over the wave's (gate, up) pairs of groups at the
    // rounding points of the bf16 GEMV's epilogue; every lane then stores 16 bytes of its pair's output row (rows scatter by pair index)
    constexpr int WO = EPI == 1 ? NJ * 8 : NJ * 16;                            // output columns of this wave
    const int width = EPI == 1 ? N / 2 : N;
    const int n_wave = EPI == 1 ? (cg_tile >> 1) * 16 : cg_tile * 16;          // first output column of this wave
    __syncthreads();
    uint16_t* const tw = (uint16_t*)As + (size_t)wn * (64 * WO);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rl = mi * 16 + 4 * q + i;
          const int pr = moe.row_map[bm + half * 64 + rl];
          const float sc = (pr >= 0 && moe.slot_scale) ? moe.slot_scale[pr] : 1.f;
          if constexpr (EPI == 1) {
#pragma unroll
            for (int j = 0; j < NJ; j += 2) {
              const float xg = round_to_dtype<AWQ_DTYPE_BF16>(acc[half * 4 + mi][j][i] * sc);
              const float up = round_to_dtype<AWQ_DTYPE_BF16>(acc[half * 4 + mi][j + 1][i] * sc);
              tw[rl * WO + (j >> 1) * 16 + r] = float_to_bf16_bits(round_to_dtype<AWQ_DTYPE_BF16>(xg / (1.f + __expf(-xg))) * up);
            }
          } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j) tw[rl * WO + j * 16 + r] = float_to_bf16_bits(acc[half * 4 + mi][j][i] * sc);
          }
        }
      // (a wave's LDS accesses complete in order: no barrier between its own writes and reads)
#pragma unroll
      for (int p = 0; p < WO / 8; ++p) {
        const int f = (p * 64 + lane) * 8;
        const int row = f / WO, col = f - row * WO;
        const int pr = moe.row_map[bm + half * 64 + row];
        const int n = n_wave + col;
        // (a 16-column output group is complete or absent: cg_end and N / width are multiples of what a group covers; width % 8 == 0)
        const bool in = EPI == 1 ? (cg_tile + 2 * (col >> 4) + 1 < cg_end) : (cg_tile + (col >> 4) < cg_end);
        if (pr >= 0 && in && n < width) *(u32x4_t*)((uint16_t*)y + (size_t)pr * width + n) = *(const u32x4_t*)(tw + f);
      }
    }
    return;
  }
  constexpr int WC = NJ * 16;
  __syncthreads();                                     // every wave has read its last x fragments: the buffers are free
  if constexpr (SPLIT) {
    // fp32 partial tile -> part[slice][M][N], no bias, no rounding: wave-private through the idle x buffers 64 rows at a time (64 rows x
    // WC floats: 16 KiB per wave at NJ = 4, the four waves' the whole 64 KiB), every lane stores 16 bytes of a 256- / 128-byte row run
    float* const tp = (float*)As + (size_t)wn * (64 * WC);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) tp[(mi * 16 + 4 * q + i) * WC + j * 16 + r] = acc[half * 4 + mi][j][i];
      // (a wave's LDS accesses complete in order: no barrier between its own writes and reads)
#pragma unroll
      for (int p = 0; p < WC / 4; ++p) {
        const int f = (p * 64 + lane) * 4;
        const int row = f / WC, col = f - row * WC;
        const int m = bm + half * 64 + row, cg = cg_tile + (col >> 4), n = cg * 16 + (col & 15);
        const float4_t v = *(const float4_t*)(tp + f);
        if (m < M && cg < cg_end && n < N) *(float4_t*)(split.part + ((size_t)slice * M + m) * N + n) = v;      // (N % 4 == 0: the host's guard)
      }
    }
    return;
  }
  uint16_t* const tw = (uint16_t*)As + (size_t)wn * (64 * WC);
  const bool n_ok8 = (N % 8) == 0;                     // (16-byte stores need 8-column alignment; otherwise element stores below)
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int n = (cg_tile + j) * 16 + r;
          tw[(mi * 16 + 4 * q + i) * WC + j * 16 + r] = output_bits16<AWQ_DTYPE_BF16>(acc[half * 4 + mi][j][i], (cg_tile + j < cg_end && n < N) ? bias : nullptr, n);
        }
    // (a wave's LDS accesses complete in order: no barrier between its own writes and reads)
#pragma unroll
    for (int p = 0; p < WC / 8; ++p) {
      const int f = (p * 64 + lane) * 8;
      const int row = f / WC, col = f - row * WC;
      const int m = bm + half * 64 + row, cg = cg_tile + (col >> 4), n = cg * 16 + (col & 15);
      if (m < M && cg < cg_end && n < N) {
        if (n_ok8) {
          *(u32x4_t*)((uint16_t*)y + (size_t)m * N + n) = *(const u32x4_t*)(tw + f);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) if (n + e < N) ((uint16_t*)y)[(size_t)m * N + n + e] = tw[f + e];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
template <int NJ>
static int pfb_launch_region(const GemmArgs& a, const u32x4_t* qw_r, const uint32_t* zs_r, int NG, int cg_base, int ng_region) {
  const int nbx = (ng_region + 4 * NJ - 1) / (4 * NJ), nby = (a.M + kPfBM - 1) / kPfBM;
  const size_t lds = 2 * kPfBM * 256;
  static unsigned long long opted[2] = {0ull, 0ull};
  if (!opt_in_dynamic_lds((const void*)gemm_repacked_pipelined_bf16_kernel<NJ>, (int)lds, opted)) return AWQ_ERR_LAUNCH;
  hipLaunchKernelGGL((gemm_repacked_pipelined_bf16_kernel<NJ>), dim3(nbx * nby), dim3(kPfbThreads), lds, a.stream, (const uint16_t*)a.x, a.ldx,
                     qw_r, zs_r, a.bias, a.y, a.M, a.K, a.N, a.g, NG, nbx, nby, cg_base, ng_region, PfbMoe{nullptr, nullptr, nullptr, 0ll, 1}, PfbSplit{nullptr, 1, 0});
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

// AWQ-MoE over expert-sorted 128-row blocks: `num_blocks` row tiles x ceil(NG / 16) column tiles of 256 (the remainder tile is clamped)
template <int EPI>
static int pfb_launch_moe(const GemmArgs& a, const u32x4_t* qw_r, const uint32_t* zs_r, int NG, int num_blocks, const PfbMoe& moe) {
  const int nbx = (NG + 15) / 16, nby = num_blocks;
  const size_t lds = 2 * kPfBM * 256;
  static unsigned long long opted[2] = {0ull, 0ull};
  if (!opt_in_dynamic_lds((const void*)gemm_repacked_pipelined_bf16_kernel<4, true, EPI>, (int)lds, opted)) return AWQ_ERR_LAUNCH;
  hipLaunchKernelGGL((gemm_repacked_pipelined_bf16_kernel<4, true, EPI>), dim3(nbx * nby), dim3(kPfbThreads), lds, a.stream, (const uint16_t*)a.x,
                     a.ldx, qw_r, zs_r, nullptr, a.y, num_blocks * kPfBM, a.K, a.N, a.g, NG, nbx, nby, 0, NG, moe, PfbSplit{nullptr, 1, 0});
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

// The caller (awq_aux_moe_gemm_blocks) has checked that every activation row read starts below 2 GiB from a.x and that the grid fits.
int launch_gemm_repacked_moe_tiles_bf16(const GemmArgs& a, const void* packed_experts, const int* row_map, const int* block_expert,
                                        int num_blocks, const float* slot_scale, long long expert_stride, int x_div, bool silu_mul) {
  if (a.dtype != AWQ_DTYPE_BF16 || a.g % 128 || !repacked_supported(a.K, a.N, a.g, a.dtype) || a.ldx < a.K || a.ldx % 8 ||
      (((uintptr_t)a.x) & 15) || !pipelined_addressable(a) || num_blocks < 1 || x_div < 1)
    return AWQ_ERR_BAD_VARIANT;
  const int NG = rp_groups(a.N);
  if (silu_mul && (a.N % 32 || (NG & 1))) return AWQ_ERR_BAD_VARIANT;
  const u32x4_t* qw_r = (const u32x4_t*)packed_experts;
  const uint32_t* zs_r = (const uint32_t*)packed_experts + (size_t)NG * (a.K / 128) * 256;
  const PfbMoe moe = {row_map, block_expert, slot_scale, expert_stride, x_div};
  return silu_mul ? pfb_launch_moe<1>(a, qw_r, zs_r, NG, num_blocks, moe) : pfb_launch_moe<0>(a, qw_r, zs_r, NG, num_blocks, moe);
}

// width 0: the planned form — N cut into a region of 256-wide tiles that fills whole rounds of the 256 CUs and a remainder of 192-wide
// tiles, or 128 x 128 tiles everywhere where the round model (route::kTilesBf16*) says they are cheaper; 256: floor(NG / 16) whole
// 256-wide column tiles, the remaining column groups in 192-wide tiles; 128: 128 x 128 tiles everywhere.
int launch_gemm_repacked_tiles_bf16(const GemmArgs& a, const void* packed, int width) {
  if (a.dtype != AWQ_DTYPE_BF16 || a.g % 128 || !repacked_supported(a.K, a.N, a.g, a.dtype) || a.M < 1 || a.ldx < a.K || a.ldx % 8 ||
      (((uintptr_t)a.x) & 15) || !pipelined_addressable(a))
    return AWQ_ERR_BAD_VARIANT;                          // fp16, g in {32, 64}, unaligned x, spans past the 32-bit buffer offsets
  if (a.norm_h != nullptr || a.moe_slots != 0 || a.silu_mul) return AWQ_ERR_BAD_VARIANT;
  const int NG = rp_groups(a.N);
  const u32x4_t* qw_r = (const u32x4_t*)packed;
  const uint32_t* zs_r = (const uint32_t*)packed + (size_t)NG * (a.K / 128) * 256;
  if (width == 128) return pfb_launch_region<2>(a, qw_r, zs_r, NG, 0, NG);
  int gA = (NG / 16) * 16;
  if (width == 0) {
    // cost in rounds of the 256 CUs, as launch_gemm_repacked_pipelined counts it: ceil(tiles_A / 256) + kTilesBf16Round192
    // ceil(tiles_B / 256) (+ a little for the second launch); the smallest wins, ties go to fewer launches / wider tiles
    const int nby = (a.M + kPfBM - 1) / kPfBM, nA_max = (NG + 15) / 16;
    int best_nA = nA_max;
    double best = 1e30;
    for (int nA = nA_max; nA >= 0; --nA) {
      const int rest = NG - 16 * nA > 0 ? NG - 16 * nA : 0;
      const int nB = (rest + 11) / 12;
      if (nA == 0 && nB == 0) continue;
      const double cost = (double)((nA * nby + 255) / 256) + route::kTilesBf16Round192 * (double)((nB * nby + 255) / 256) +
                          (nA > 0 && nB > 0 ? route::kTilesBf16SecondLaunch : 0.0);
      if (cost < best - 1e-9) { best = cost; best_nA = nA; }
    }
    const double cost2 = route::kTilesBf16Round128 * (double)((((NG + 7) / 8) * nby + 255) / 256);
    if (cost2 < best - 1e-9) return pfb_launch_region<2>(a, qw_r, zs_r, NG, 0, NG);
    gA = best_nA * 16 < NG ? best_nA * 16 : NG;
  } else if (width != 256) {
    return AWQ_ERR_BAD_VARIANT;
  }
  if (gA > 0) {
    const int rc = pfb_launch_region<4>(a, qw_r, zs_r, NG, 0, gA);
    if (rc) return rc;
  }
  if (gA < NG) return pfb_launch_region<3>(a, qw_r, zs_r, NG, gA, NG - gA);
  return AWQ_OK;
}

// ------------------------------------------------------------------------------------------------ split-K form
// tiles x S workgroups write fp32 partial tiles into the workspace (behind its 4096-byte counter head, which is left alone), a second
// launch adds them in slice order, rounds once to bf16 and adds the bias: deterministic, no counters, no in-launch hand-off.
template <int NJ>
static int pfb_launch_split(const GemmArgs& a, const u32x4_t* qw_r, const uint32_t* zs_r, int NG, int S, int kb_per) {
  const int nbx = (NG + 4 * NJ - 1) / (4 * NJ), nby = (a.M + kPfBM - 1) / kPfBM;
  const size_t lds = 2 * kPfBM * 256;
  static unsigned long long opted[2] = {0ull, 0ull};
  if (!opt_in_dynamic_lds((const void*)gemm_repacked_pipelined_bf16_kernel<NJ, false, 0, true>, (int)lds, opted)) return AWQ_ERR_LAUNCH;
  float* part = (float*)((char*)a.workspace + kPfSplitHead);
  hipLaunchKernelGGL((gemm_repacked_pipelined_bf16_kernel<NJ, false, 0, true>), dim3(nbx * nby * S), dim3(kPfbThreads), lds, a.stream,
                     (const uint16_t*)a.x, a.ldx, qw_r, zs_r, nullptr, a.y, a.M, a.K, a.N, a.g, NG, nbx, nby, 0, NG,
                     PfbMoe{nullptr, nullptr, nullptr, 0ll, 1}, PfbSplit{part, S, kb_per});
  const size_t MN = (size_t)a.M * a.N;
  const unsigned blocks = (unsigned)((MN / 4 + 255) / 256 < 2048 ? (MN / 4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(pf_splitk_reduce_kernel<AWQ_DTYPE_BF16>, dim3(blocks), dim3(256), 0, a.stream, (const float*)part, a.bias, a.y, S, MN, a.N);
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

// The plan: false = outside the domain (fp16, g in {32, 64}, no / misaligned / too small a workspace, N % 4, ldx % 8, spans past the
// 32-bit buffer offsets) or fewer than two slices.  S = min(256 / tiles: fill the chip once, kPfSplitMaxSlices, slices of at least
// kPfSplitMinBlocks k-blocks, what the workspace holds), then evened out: ceil(KBT / ceil(KBT / S)) slices, the last one the shortest.
// width 0: 128 x 128 tiles while there are at most kPfSplitBf16NarrowTilesMax (deep matrices: ...Deep) of them (the other width where that one cannot split);
// 128 / 256: that width.  Where it pays is not decided here: route::split_tiles_bf16_wins (awq_capi.hip: repacked_dispatch).
static bool pfb_split_plan(const GemmArgs& a, int width, int* NJ_out, int* S_out, int* kb_per_out) {
  if (a.dtype != AWQ_DTYPE_BF16 || a.g % 128 || !repacked_supported(a.K, a.N, a.g, a.dtype) || a.M < 1 || a.ldx < a.K || a.ldx % 8 ||
      (((uintptr_t)a.x) & 15) || !pipelined_addressable(a) || a.N % 4)
    return false;
  if (a.norm_h != nullptr || a.moe_slots != 0 || a.silu_mul) return false;
  if (!a.workspace || (((uintptr_t)a.workspace) & 15) || a.workspace_bytes <= kPfSplitHead) return false;
  if (width != 0 && width != 128 && width != 256) return false;
  const int NG = rp_groups(a.N), KBT = a.K / 128, nby = (a.M + kPfBM - 1) / kPfBM;
  const size_t slice_bytes = (size_t)a.M * a.N * sizeof(float);
  const size_t s_ws = (a.workspace_bytes - kPfSplitHead) / slice_bytes;
  const int narrow_max = KBT >= route::kPfSplitBf16DeepBlocks ? route::kPfSplitBf16NarrowTilesMaxDeep : route::kPfSplitBf16NarrowTilesMax;
  const int first = width == 128 ? 2 : width == 256 ? 4 : (((NG + 7) / 8) * nby <= narrow_max ? 2 : 4);
  for (int pass = 0; pass < (width ? 1 : 2); ++pass) {
    const int nj = pass == 0 ? first : 6 - first;
    const int tiles = ((NG + 4 * nj - 1) / (4 * nj)) * nby;
    int S = 256 / tiles;
    if (S > route::kPfSplitMaxSlices) S = route::kPfSplitMaxSlices;
    if ((size_t)S > s_ws) S = (int)s_ws;
    if (S > KBT / route::kPfSplitMinBlocks) S = KBT / route::kPfSplitMinBlocks;
    if (S < 2) continue;
    const int kb_per = (KBT + S - 1) / S;
    *NJ_out = nj; *S_out = (KBT + kb_per - 1) / kb_per; *kb_per_out = kb_per;
    return *S_out >= 2;
  }
  return false;
}

int launch_gemm_repacked_split_tiles_bf16(const GemmArgs& a, const void* packed, int width) {
  int NJ = 0, S = 0, kb_per = 0;
  if (!pfb_split_plan(a, width, &NJ, &S, &kb_per)) return AWQ_ERR_BAD_VARIANT;
  const int NG = rp_groups(a.N);
  const u32x4_t* qw_r = (const u32x4_t*)packed;
  const uint32_t* zs_r = (const uint32_t*)packed + (size_t)NG * (a.K / 128) * 256;
  return NJ == 4 ? pfb_launch_split<4>(a, qw_r, zs_r, NG, S, kb_per) : pfb_launch_split<2>(a, qw_r, zs_r, NG, S, kb_per);
}

}  // namespace awq

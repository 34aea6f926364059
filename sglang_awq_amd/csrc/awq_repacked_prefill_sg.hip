// fp16 tile GEMM for the small quantisation groups (group_size 32 / 64) on the MFMA-fragment-major layout, software-pipelined by hand
// (gfx950): the small-group sibling of gemm_repacked_pipelined_kernel (awq_repacked_prefill.hip), reached as AWQ_RP_TILES_SG / _WIDE /
// _NARROW.  Before it g in {32, 64} ran gemm_rpx_tiled_kernel (awq_repacked_ext.hip) from 33 rows: compiler-scheduled, 128 x 256 tiles
// only.
//
// What carried over from the g % 128 kernel unchanged: workgroup tile 128 x (64 NJ) — NJ = 4 / 3 / 2 column groups per wave: 128 x 256,
// 128 x 192 (remainder region) and 128 x 128 tiles — four waves of 8 row tiles x NJ column groups; accumulators tied in the AGPR file
// (inline-asm v_mfma_f32_16x16x32_f16, "+a"; the s_nop guard before the compiler-scheduled reads); B never touches LDS; x through two
// XOR-swizzled 32 KiB LDS buffers; one barrier per k-block inside its last k-step; every global load of the loop a buffer load with an
// SGPR descriptor and a scalar k offset; XCD-aware tile order in super-rows of 4 row tiles; the output tile through the idle x buffers,
// rounded once (the bias adds a second rounding), 16 bytes per lane.
//
// What is new: a 128-row k-block spans GS = 128 / g quantisation groups.  K-step d of column group j dequantises with the word
// zs[j][d GS / 4] of zs_r[NG][K / g][16], so the per-word constants of the g % 128 kernel (the splats s2 and z1024 and z64 =
// (1024 + z) - 960: 3 ops per word, once per k-block there) would have to be made GS times per k-block: 48 ops at GS = 4 on top of
// the 16 x 13 = 208 of the dequantisation, all 256 slots full before any LDS address arithmetic.
//
// Constants scheme: no splat registers.  The packed-fp16 ops select the half of the (scale | fp16(1024 + zero)) word they need for both
// lanes through op_sel / op_sel_hi, so the word itself is the operand:
//   d = t - z1024     v_pk_add_f16 d, t, zs  op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]     (both lanes subtract the word's high half)
//   f = d * s         v_pk_mul_f16 f, d, zs  op_sel:[0,0] op_sel_hi:[1,0]                                (both lanes multiply by its low half)
//   z64 = z1024 - 960 v_pk_add_f16 z64, zs, c  op_sel:[1,0] op_sel_hi:[1,1]  with c = (-960, -960)       (high half into both lanes: a plain splat)
// z64 stays one op per fragment (the fma of the odd k-pairs takes it as a plain operand) and lives for three stages only, so a
// fragment costs 14 ops whatever GS is (at GS = 2 z64 is made twice per word: the slot is free and no register outlives its fragment).
// The per-element operations and their order are those of rp_dequant / rpx_dequant — (1024 + q) - (1024 + z) resp.
// fma(1024 + 16 q, 1 / 16, -(64 + z)), then one multiplication by the scale — so every W element is the fp16 awq_dequantize produces.
//
// Slot table.  An MFMA 16x16x32 holds the matrix pipe for 16 cycles and the issue port for 8: two VALU ops ride free behind each.
//   per k-block and wave      MFMAs   free slots   dequantisation          constants      third ops
//   NJ = 4                     128      256        16 x 14 = 224           (in the 14)        0
//   NJ = 3                      96      192        12 x 14 = 168                              0
//   NJ = 2                      64      128         8 x 14 = 112                              0
//   behind MFMA (row tile) 0: w8 = w >> 8, t0      1: t1, t2      2: t3, d0 = t0 - z1024      3: d2 = t2 - z1024, z64
//               4: d1 = fma(t1, 1/16, -z64), d3 = fma(t3, 1/16, -z64)      5: f0 = d0 s, f1 = d1 s      6: f2 = d2 s, f3 = d3 s      7: -
// No MFMA carries a third VALU op.  The passengers that are not VALU keep the g % 128 kernel's places: the 8 LDS reads of the next
// k-step's x fragments behind the MFMAs of every j = 1 fragment; the 8 LDS writes of the next x tile behind every fourth MFMA of (1, 2)
// (1, 3) (2, 0) (2, 1) (NJ = 3: MFMAs 0, 3, 6 of (1, 2) (2, 0) (2, 2); NJ = 2: every second MFMA of (1, 0) (2, 0)); the request for the
// tile after it behind them; the barrier behind the first MFMA of (3, 0).
//
// Scale loads: GS dword buffer loads per (column group, k-block), 64 bytes apart (lane offset 4 r, scalar offset (kb GS + s) 64),
// issued at the top of the k-block before the one that uses them, beside its weight loads; 2 x GS x NJ words live across the loop.
// Resources (tools/rp_resources.py; VGPRs + AGPRs, scratch 0 in all six): NJ = 4: 199 + 128 (GS = 2) / 212 + 128 (GS = 4); NJ = 3:
// 178 + 96 / 188 + 96; NJ = 2: 141 + 64 / 149 + 64 — every instantiation is built, g = 32 keeps its 256-wide tiles.
#include <cstdlib>

#include "awq_prefill_common.h"

namespace awq {

// the three packed-fp16 ops that read a half of the zs word for both lanes (see the header)
__device__ __forceinline__ uint32_t pfs_sub_z(uint32_t t, uint32_t zs) {
  uint32_t d;
  asm("v_pk_add_f16 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(t), "v"(zs));
  return d;
}
__device__ __forceinline__ uint32_t pfs_mul_s(uint32_t d, uint32_t zs) {
  uint32_t f;
  asm("v_pk_mul_f16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(f) : "v"(d), "v"(zs));
  return f;
}
__device__ __forceinline__ half2_t pfs_z64(uint32_t zs, uint32_t neg960) {
  uint32_t z;
  asm("v_pk_add_f16 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(z) : "v"(zs), "v"(neg960));      // exact: (1024 + z) - 960
  return as_h2(z);
}

struct PfsPipe {           // one dword on its way to becoming a fragment
  uint32_t w, w8, t0, t1, t2, t3, d0, d2;
  half2_t z64, d1, d3;
  u32x4_t f;
};

template <int S>
__device__ __forceinline__ void pfs_stage(PfsPipe& p, uint32_t zs, uint32_t neg960) {
  const half2_t sixteenth = {(half_t)0.0625f, (half_t)0.0625f};
  const uint32_t magic = kMagicF16;
  if constexpr (S == 0) { p.w8 = p.w >> 8; p.t0 = and_or(p.w, kLoNib, magic); }
  if constexpr (S == 1) { p.t1 = and_or(p.w, kHiNib, magic); p.t2 = and_or(p.w8, kLoNib, magic); }
  if constexpr (S == 2) { p.t3 = and_or(p.w8, kHiNib, magic); p.d0 = pfs_sub_z(p.t0, zs); }
  if constexpr (S == 3) { p.d2 = pfs_sub_z(p.t2, zs); p.z64 = pfs_z64(zs, neg960); }
  if constexpr (S == 4) { p.d1 = __builtin_elementwise_fma(as_h2(p.t1), sixteenth, -p.z64); p.d3 = __builtin_elementwise_fma(as_h2(p.t3), sixteenth, -p.z64); }
  if constexpr (S == 5) { p.f[0] = pfs_mul_s(p.d0, zs); p.f[1] = pfs_mul_s(as_u32(p.d1), zs); }
  if constexpr (S == 6) { p.f[2] = pfs_mul_s(p.d2, zs); p.f[3] = pfs_mul_s(as_u32(p.d3), zs); }
}

// the same operations in one piece (prologue: the first fragment of k-block 0)
__device__ __forceinline__ u32x4_t pfs_dequant(uint32_t w, uint32_t zs, uint32_t neg960) {
  PfsPipe p;
  p.w = w;
  pfs_stage<0>(p, zs, neg960); pfs_stage<1>(p, zs, neg960); pfs_stage<2>(p, zs, neg960); pfs_stage<3>(p, zs, neg960);
  pfs_stage<4>(p, zs, neg960); pfs_stage<5>(p, zs, neg960); pfs_stage<6>(p, zs, neg960);
  return p.f;
}

constexpr int kPfsThreads = 256;
constexpr int kPfsRowBlock = 4;       // row tiles per super-row of the tile order (as PF_ROW_BLOCK of the g % 128 kernel)

// NJ = column groups (16 columns) per wave: 4 -> 128 x 256 tiles, 3 -> 128 x 192, 2 -> 128 x 128.  GS = quantisation groups per
// k-block: 2 (g = 64) or 4 (g = 32).  A launch covers the column groups [cg_base, cg_base + ng_region) of the matrix (the host cuts N
// into regions: launch_gemm_repacked_tiles_sg).
template <int NJ, int GS>
__global__ __launch_bounds__(kPfsThreads, 1) void gemm_repacked_pipelined_sg_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                                                     const u32x4_t* __restrict__ qw_r,
                                                                                     const uint32_t* __restrict__ zs_r,
                                                                                     const void* __restrict__ bias, void* __restrict__ y,
                                                                                     int M, int K, int N, int NG, int nbx, int nby,
                                                                                     int cg_base, int ng_region) {
  static_assert(NJ >= 2 && NJ <= 4, "128 x 128 .. 128 x 256 tiles");
  static_assert(GS == 2 || GS == 4, "group size 64 or 32");
  extern __shared__ __attribute__((aligned(16))) unsigned char As[];      // 2 x 32 KiB
  constexpr int MI = 8, BM = kPfBM, AL = 8;           // row tiles per wave; rows per workgroup tile; x-tile chunks (16 B) per thread
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave-uniform: every weight / scale address is an SGPR base + a lane offset
  const int q = lane >> 4, r = lane & 15;
  const int KB = K / 128, groups = KB * GS;

  const int nwg = nbx * nby, bid = blockIdx.x;
  const int xcd = bid & 7, qd = nwg >> 3, rem = nwg & 7;
  const int logical = (xcd < rem ? xcd * (qd + 1) : rem * (qd + 1) + (xcd - rem) * qd) + (bid >> 3);
  // the 32 tiles an XCD runs together cover 4 row tiles x 8 column tiles: x and weights each shared in its L2 (see the g % 128 kernel)
  const int sb_tiles = kPfsRowBlock * nbx, sb = logical / sb_tiles, in_sb = logical - sb * sb_tiles;
  const int rows_sb = nby - sb * kPfsRowBlock < kPfsRowBlock ? nby - sb * kPfsRowBlock : kPfsRowBlock;
  const int bm = (sb * kPfsRowBlock + in_sb % rows_sb) * BM;
  const int cg_tile = cg_base + (in_sb / rows_sb) * (4 * NJ) + wn * NJ;       // this wave's first column group
  const int cg_end = cg_base + ng_region < NG ? cg_base + ng_region : NG;

  __amdgpu_buffer_rsrc_t rw[NJ];                       // this wave's column groups: [KB][64 lanes] dwordx4
  uint32_t zoff_s[NJ];                                 // byte offset of the group's first scale word in zs_r
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = cg_tile + j;
    const int cgj = c < cg_end ? c : cg_end - 1;       // clamped: groups outside the region are never stored
    rw[j] = __builtin_amdgcn_make_buffer_rsrc((void*)(qw_r + (size_t)cgj * KB * 64), 0, KB * 1024, kPfRsrcFlags);
    zoff_s[j] = (uint32_t)cgj * (uint32_t)groups * 64u;
  }
  const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)zs_r, 0, 0x7fffffff, kPfRsrcFlags);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (size_t)bm * ldx), 0, 0x7fffffff, kPfRsrcFlags);
  const int lane16 = lane * 16, r4 = r * 4;
  uint32_t neg960 = 0xe380e380u;                       // (-960, -960); kept in a register: not an inline constant
  pin_here(neg960);

  u32x4_t a_st[AL];
  u32x4_t w_cur[NJ], w_nxt[NJ];
  uint32_t zs_cur[NJ][GS], zs_nxt[NJ][GS];

  // this thread's AL rows / chunks of the x tile: byte offsets from the tile's first row (rows >= M re-read row M - 1: never stored)
  uint32_t xoff[AL];
#pragma unroll
  for (int i = 0; i < AL; ++i) {
    const int c = tid + kPfsThreads * i;
    const int row = c >> 4, chunk = c & 15;
    const int mr = bm + row < M ? row : M - 1 - bm;
    xoff[i] = (uint32_t)((size_t)mr * ldx + chunk * 8) * 2u;
  }
  auto load_a = [&](int kb) {
#pragma unroll
    for (int i = 0; i < AL; ++i) a_st[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, xoff[i], kb * 256, 0);
  };
  auto store_a1 = [&](int buf, int i) {
    const int c = tid + kPfsThreads * i;
    *(u32x4_t*)(As + buf * (BM * 256) + pfp_off(c >> 4, c & 15)) = a_st[i];
  };
  // the weights and the GS scale words per column group of k-block kb (groups kb GS .. kb GS + GS - 1, 64 bytes apart)
  auto load_b = [&](u32x4_t (&w)[NJ], uint32_t (&zs)[NJ][GS], int kb) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      w[j] = __builtin_amdgcn_raw_buffer_load_b128(rw[j], lane16, kb * 1024, 0);
#pragma unroll
      for (int s = 0; s < GS; ++s) zs[j][s] = __builtin_amdgcn_raw_buffer_load_b32(rz, r4 + s * 64, zoff_s[j] + kb * (GS * 64), 0);
    }
  };

  float4_t acc[MI][NJ];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[mi][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

  // prologue: x tile 0 into LDS, k-block 0's weights / scale words in registers, its first fragment dequantised
  load_a(0);
  load_b(w_cur, zs_cur, 0);
#pragma unroll
  for (int i = 0; i < AL; ++i) store_a1(0, i);
  u32x4_t frag = pfs_dequant(w_cur[0][0], zs_cur[0][0], neg960);
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
    load_b(w_nxt, zs_nxt, nxt);
    __builtin_amdgcn_sched_barrier(0);

#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        // the fragment after (d, j): (d, j + 1), then (d + 1, 0), then k-block kb + 1's (0, 0); its word is that of its own k-step
        PfsPipe p;
        uint32_t zn;
        if (j < NJ - 1) { p.w = w_cur[j + 1][d]; zn = zs_cur[j + 1][(d * GS) / 4]; }
        else if (d < 3) { p.w = w_cur[0][d + 1]; zn = zs_cur[0][((d + 1) * GS) / 4]; }
        else { uint32_t w0 = w_nxt[0][0], z0 = zs_nxt[0][0]; pin_here(w0); pin_here(z0); p.w = w0; zn = z0; }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          mfma_tied(acc[mi][j], af[mi], frag);
          switch (mi) {                                  // (compile-time after unrolling)
            case 0: pfs_stage<0>(p, zn, neg960); break;
            case 1: pfs_stage<1>(p, zn, neg960); break;
            case 2: pfs_stage<2>(p, zn, neg960); break;
            case 3: pfs_stage<3>(p, zn, neg960); break;
            case 4: pfs_stage<4>(p, zn, neg960); break;
            case 5: pfs_stage<5>(p, zn, neg960); break;
            case 6: pfs_stage<6>(p, zn, neg960); break;
            default: break;
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
    for (int j = 0; j < NJ; ++j) {
      w_cur[j] = w_nxt[j];
#pragma unroll
      for (int s = 0; s < GS; ++s) zs_cur[j][s] = zs_nxt[j][s];
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs' results must have left the pipe before the (compiler-scheduled) reads below

  // the output tile: rounded (and biased, second rounding) exactly as store_output<fp16> does, parked wave-privately in the idle x
  // buffers 64 rows at a time, stored as 16 bytes per lane (8 lanes per 128-byte row run of a 64-column wave)
  constexpr int WC = NJ * 16;
  __syncthreads();                                     // every wave has read its last x fragments: the buffers are free
  half_t* const tw = (half_t*)As + (size_t)wn * (64 * WC);
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
          half_t h = (half_t)acc[half * 4 + mi][j][i];
          if (bias && cg_tile + j < cg_end && n < N) h = h + ((const half_t*)bias)[n];
          tw[(mi * 16 + 4 * q + i) * WC + j * 16 + r] = h;
        }
    // (a wave's LDS accesses complete in order: no barrier between its own writes and reads)
#pragma unroll
    for (int p = 0; p < WC / 8; ++p) {
      const int f = (p * 64 + lane) * 8;
      const int row = f / WC, col = f - row * WC;
      const int m = bm + half * 64 + row, cg = cg_tile + (col >> 4), n = cg * 16 + (col & 15);
      if (m < M && cg < cg_end && n < N) {
        if (n_ok8) {
          *(u32x4_t*)((half_t*)y + (size_t)m * N + n) = *(const u32x4_t*)(tw + f);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) if (n + e < N) ((half_t*)y)[(size_t)m * N + n + e] = tw[f + e];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
template <int NJ, int GS>
static int pfs_launch_gs(const GemmArgs& a, const u32x4_t* qw_r, const uint32_t* zs_r, int NG, int cg_base, int ng_region) {
  const int nbx = (ng_region + 4 * NJ - 1) / (4 * NJ), nby = (a.M + kPfBM - 1) / kPfBM;
  const size_t lds = 2 * kPfBM * 256;
  static unsigned long long opted[2] = {0ull, 0ull};
  if (!opt_in_dynamic_lds((const void*)gemm_repacked_pipelined_sg_kernel<NJ, GS>, (int)lds, opted)) return AWQ_ERR_LAUNCH;
  hipLaunchKernelGGL((gemm_repacked_pipelined_sg_kernel<NJ, GS>), dim3(nbx * nby), dim3(kPfsThreads), lds, a.stream, (const uint16_t*)a.x, a.ldx,
                     qw_r, zs_r, a.bias, a.y, a.M, a.K, a.N, NG, nbx, nby, cg_base, ng_region);
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

template <int NJ>
static int pfs_launch_region(const GemmArgs& a, const u32x4_t* qw_r, const uint32_t* zs_r, int NG, int cg_base, int ng_region) {
  return a.g == 64 ? pfs_launch_gs<NJ, 2>(a, qw_r, zs_r, NG, cg_base, ng_region) : pfs_launch_gs<NJ, 4>(a, qw_r, zs_r, NG, cg_base, ng_region);
}

// width 0: the planned form — N cut into a region of 256-wide tiles that fills whole rounds of the 256 CUs and a remainder of 192-wide
// tiles, or 128 x 128 tiles everywhere where the round model (route::kTilesSg*) says they are cheaper; 256: floor(NG / 16) whole
// 256-wide column tiles, the remaining column groups in 192-wide tiles; 128: 128 x 128 tiles everywhere.
int launch_gemm_repacked_tiles_sg(const GemmArgs& a, const void* packed, int width) {
  if (a.dtype != AWQ_DTYPE_F16 || (a.g != 32 && a.g != 64) || !repacked_supported(a.K, a.N, a.g, a.dtype) || a.M < 1 || a.ldx < a.K ||
      a.ldx % 8 || (((uintptr_t)a.x) & 15) || !pipelined_addressable(a))
    return AWQ_ERR_BAD_VARIANT;                          // bf16, g % 128 == 0, unaligned x, spans past the 32-bit buffer offsets
  if (a.norm_h != nullptr || a.moe_slots != 0 || a.silu_mul) return AWQ_ERR_BAD_VARIANT;
  const int NG = rp_groups(a.N);
  const u32x4_t* qw_r = (const u32x4_t*)packed;
  const uint32_t* zs_r = (const uint32_t*)packed + (size_t)NG * (a.K / 128) * 256;
  if (width == 128) return pfs_launch_region<2>(a, qw_r, zs_r, NG, 0, NG);
  int gA = (NG / 16) * 16;
  if (width == 0) {
    // cost in rounds of the 256 CUs, as launch_gemm_repacked_pipelined counts it: ceil(tiles_A / 256) + kTilesSgRound192
    // ceil(tiles_B / 256) (+ a little for the second launch); the smallest wins, ties go to fewer launches / wider tiles
    const int nby = (a.M + kPfBM - 1) / kPfBM, nA_max = (NG + 15) / 16;
    int best_nA = nA_max;
    double best = 1e30;
    for (int nA = nA_max; nA >= 0; --nA) {
      const int rest = NG - 16 * nA > 0 ? NG - 16 * nA : 0;
      const int nB = (rest + 11) / 12;
      if (nA == 0 && nB == 0) continue;
      const double cost = (double)((nA * nby + 255) / 256) + route::kTilesSgRound192 * (double)((nB * nby + 255) / 256) +
                          (nA > 0 && nB > 0 ? route::kTilesSgSecondLaunch : 0.0);
      if (cost < best - 1e-9) { best = cost; best_nA = nA; }
    }
    const double cost2 = route::kTilesSgRound128 * (double)((((NG + 7) / 8) * nby + 255) / 256);
    if (cost2 < best - 1e-9) return pfs_launch_region<2>(a, qw_r, zs_r, NG, 0, NG);
    gA = best_nA * 16 < NG ? best_nA * 16 : NG;
  } else if (width != 256) {
    return AWQ_ERR_BAD_VARIANT;
  }
  if (gA > 0) {
    const int rc = pfs_launch_region<4>(a, qw_r, zs_r, NG, 0, gA);
    if (rc) return rc;
  }
  if (gA < NG) return pfs_launch_region<3>(a, qw_r, zs_r, NG, gA, NG - gA);
  return AWQ_OK;
}

}  // namespace awq

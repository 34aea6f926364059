// Shared-activation decode GEMV in bf16 on the MFMA-fragment-major layout (layout: awq_repacked.hip and awq_repacked_ext.hip; bf16,
// group size a multiple of 128): the bf16 sibling of gemv_sharedx_kernel (awq_repacked_sharedx.hip, one or two row tiles), reached as
// AWQ_RP_SHARED_X_BF16 for 1 .. 32 rows in one launch and 33 .. 64 rows in two.  Before it a bf16 batch ran gemv_rpx_kernel
// (awq_repacked_ext.hip: every wave fetches its own x fragments from global memory, strips of at most 4 column groups, 16 rows per
// launch — two passes over the whole weight from 17 rows) and, from 33 rows, under-filled 128 x 256 tiles.
//
// What carried over from the fp16 kernels unchanged: a workgroup owns a strip of G column groups for all of K (nothing shared
// between workgroups, no workspace, safe under graph capture); x crosses the memory system once per workgroup and waits in two LDS
// buffers in MFMA A-operand order — v_mfma_f32_16x16x32_bf16 takes its A operand in the lane order of the f16 form — with the
// r ^ (4 d + q) bank swizzle; x loads issued two chunk bodies ahead (two register sets); one barrier per chunk, all trip counts
// functions of K alone; the weight ring re-issued the moment a unit has arrived, before it is dequantised; rows >= M and k-blocks past
// K written as zeros without touching memory (ldx > K is fine); the fixed-order reduction through LDS over the x buffers;
// store_output<bf16>: one rounding of the fp32 sum, then the bias with a second rounding.  No folded norm (fp16 only).
//
// AWQ-MoE form (template parameters EPI, ROWMAP; one row tile; awq_aux_moe_gemv_blocks with bf16): a second grid dimension of
// expert-sorted 16-row blocks, the loader and the final reduction indirected through row_map, the routed weight on the fp32 sums,
// and the SiLU-mul epilogue over (gate, up) pairs of column groups — see SxbMoe below.  The chunk loop is the dense one: same LDS
// (sxb_lds(G, 1)), same barriers; the dense instantiations compile to the same registers as before it existed.
//
// Dequantisation.  Every W element is the bf16 awq_dequantize produces: (q - z) exact, times the scale as an exact fp32 product,
// one round-to-nearest-even to bf16 (the statement of it: rpx_dequant<AWQ_DTYPE_BF16>, awq_repacked_ext.hip).  The generic form
// goes through fp16: per dword 4 v_and_or_b32 + shift, 2 subtracts, 2 fmas, 8 v_cvt_f32_f16, 8 multiplies, 4 v_cvt_pk_bf16_f32.
// Here the dword stays in fp32 throughout:
//   lo = w & 0x0f0f0f0f          bytes (k0, k4, k1, k5) = q
//   hi = w & 0xf0f0f0f0          bytes (k2, k6, k3, k7) = 16 q   (no shift: the 16 goes into the scale)
//   v_cvt_f32_ubyte0..3 of both; per k-pair one packed fma  (q, q') * s - z s   resp.  (16 q, 16 q') * (s / 16) - z s;
//   v_cvt_pk_bf16_f32 per k-pair.
// 2 + 8 + 4 + 4 = 18 VALU per dword.  s, s / 16 and -z s come once per unit from the (bf16 scale | fp16(1024 + zero)) word.  z is a
// 4-bit integer and s has an 8-bit significand, so z s is exact in fp32; with q also 4-bit, (q - z) s has at most 13 significant
// bits, so the fma's single rounding returns it exactly — the same value as the exact product of the generic form.  This argument
// is for NORMAL scales whose s / 16 is normal too (|s| >= 2^-122): for subnormal or near-subnormal bf16 scales neither s / 16 nor the
// fma's result need be exact and the kernel is not held to bit equality with awq_dequantize there.  q = z gives +0 where the
// generic form gives -0 under a negative scale; both add nothing to the sum.
// -DSXB_DEQUANT_F16=1 builds the generic sequence into the same kernels (A/B; profiles/kbench_sharedx_bf16_ab.txt).
//
// Split.  The (S, U) table of the fp16 kernel (sx_slots / sx_units, restated below as sxb_slots / sxb_units) was rechecked under
// bf16's register use, not assumed: a unit's dequantisation holds 8 fp32 values + 2 masked words where fp16 holds 4 packed words, the
// per-unit constants are 3 registers either way.  At G = 8 bf16 takes U = 2 where fp16 takes 4: four units per chunk hold 2 x 4 x
// vectors per lane beside the fp32 dequantisation and spilled 12 bytes per lane at the 128 VGPRs of a 16-wave workgroup.  Resources,
// and the three / four-row-tile form that is not shipped: the comment above sxb_go below.
#include <type_traits>

#include "awq_repacked_gemv.h"

#ifndef SXB_DEQUANT_F16
#define SXB_DEQUANT_F16 0     // 1: A/B build, the dequantisation through fp16 (rpx_dequant<AWQ_DTYPE_BF16> with the unit's constants hoisted)
#endif

namespace awq {

typedef __bf16 sxb_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float sxb_float2_t __attribute__((ext_vector_type(2)));

// per-unit constants from the (bf16 scale | fp16(1024 + zero)) word of this lane's column
struct SxbUnit {
  float s;                    // the scale
  float s16;                  // fp32 route: s / 16;  fp16 route: bits of half2(1024 + z, 1024 + z)
  float nzs;                  // fp32 route: -z s;    fp16 route: bits of half2(64 + z, 64 + z)
};

__device__ __forceinline__ SxbUnit sxb_unit(uint32_t zw) {
  SxbUnit u;
  u.s = __builtin_bit_cast(float, zw << 16);
#if SXB_DEQUANT_F16
  const half2_t c960 = {(half_t)960.f, (half_t)960.f};
  const half2_t zh = as_h2(zw);
  const half2_t z1024 = __builtin_shufflevector(zh, zh, 1, 1);
  u.s16 = __builtin_bit_cast(float, z1024);
  u.nzs = __builtin_bit_cast(float, z1024 - c960);         // exact: (1024 + z) - 960
#else
  u.s16 = u.s * 0.0625f;
  u.nzs = -(float)((zw >> 16) & 15u) * u.s;                 // fp16(1024 + z) = 0x6400 | z: z sits in the low mantissa bits; exact product
#endif
  return u;
}

__device__ __forceinline__ uint32_t sxb_pack(sxb_float2_t p) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(p, sxb_bf16x2_t)); }

// 8 weights of one column (one dword) -> the 4 packed bf16 k-pairs of an MFMA B fragment
__device__ __forceinline__ u32x4_t sxb_dequant(uint32_t w, const SxbUnit& u) {
#if SXB_DEQUANT_F16
  const half2_t sixteenth = {(half_t)0.0625f, (half_t)0.0625f};
  const half2_t z1024 = __builtin_bit_cast(half2_t, u.s16), z64 = __builtin_bit_cast(half2_t, u.nzs);
  const uint32_t magic = kMagicF16;
  const uint32_t w8 = w >> 8;
  half2_t d[4];                                            // (q - z), exact small integers in fp16
  d[0] = as_h2(and_or(w, kLoNib, magic)) - z1024;
  d[1] = __builtin_elementwise_fma(as_h2(and_or(w, kHiNib, magic)), sixteenth, -z64);
  d[2] = as_h2(and_or(w8, kLoNib, magic)) - z1024;
  d[3] = __builtin_elementwise_fma(as_h2(and_or(w8, kHiNib, magic)), sixteenth, -z64);
  u32x4_t f;
#pragma unroll
  for (int t = 0; t < 4; ++t) f[t] = sxb_pack((sxb_float2_t){(float)d[t][0] * u.s, (float)d[t][1] * u.s});   // exact products, one RNE rounding each
  return f;
#else
  // nibble of k-element e sits at bit {0, 16, 4, 20, 8, 24, 12, 28}[e] (the order rp_dequant reads: k-pair t = halves of w >> 4 t)
  const uint32_t lo = w & 0x0f0f0f0fu, hi = w & 0xf0f0f0f0u;
  const sxb_float2_t S = {u.s, u.s}, S16 = {u.s16, u.s16}, Z = {u.nzs, u.nzs};
  const sxb_float2_t q0 = {(float)(lo & 0xffu), (float)((lo >> 16) & 0xffu)};     // (k0, k1)
  const sxb_float2_t q1 = {(float)(hi & 0xffu), (float)((hi >> 16) & 0xffu)};     // 16 (k2, k3)
  const sxb_float2_t q2 = {(float)((lo >> 8) & 0xffu), (float)(lo >> 24)};        // (k4, k5)
  const sxb_float2_t q3 = {(float)((hi >> 8) & 0xffu), (float)(hi >> 24)};        // 16 (k6, k7)
  return (u32x4_t){sxb_pack(__builtin_elementwise_fma(q0, S, Z)), sxb_pack(__builtin_elementwise_fma(q1, S16, Z)),
                   sxb_pack(__builtin_elementwise_fma(q2, S, Z)), sxb_pack(__builtin_elementwise_fma(q3, S16, Z))};
#endif
}

__device__ __forceinline__ float4_t sxb_mfma(const u32x4_t& a, const u32x4_t& b, float4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// Waves per column group (k-block slots of a chunk) and units per wave and chunk, by strip width G; C = S U <= 8 keeps two 32-row
// buffers at 128 KiB.  The fp16 table except at G = 8 (U = 2, not 4: see the header): with these every instantiation below has zero
// scratch (NW = S G waves -> 128 VGPRs at 16 waves, 168 at 9 .. 12, 256 at 8); a larger S needs more than 16 waves or a chunk of more
// than 8 k-blocks.
constexpr int sxb_slots(int G) { return G <= 2 ? 8 : G <= 4 ? 4 : G == 5 ? 3 : 2; }
constexpr int sxb_units(int G) { return G <= 2 ? 1 : G == 6 ? 4 : 2; }
constexpr size_t sxb_lds(int G, int MT) {
  const size_t x2 = (size_t)2 * MT * 16 * sxb_slots(G) * sxb_units(G) * 256, red = (size_t)sxb_slots(G) * G * MT * 1024;
  return x2 > red ? x2 : red;
}

// ROWMAP (AWQ-MoE, one row tile): grid row b serves the (token, expert) pairs row_map[16 b .. 16 b + 15] (sorted by expert, -1 =
// padding) with the weights of expert block_expert[b] (< 0: unused block, the workgroup leaves before any barrier); row i of the block
// is activation row row_map[16 b + i] / x_div (padding: zeros, no load) and output row row_map[16 b + i] (padding: no store), the fp32
// sums multiplied by slot_scale[pair] before their one rounding.  EPI = 1 (ROWMAP only, G even so that every strip starts on a gate
// group): the column groups alternate gate / up and act = bf16(bf16(silu(bf16 gate)) * bf16 up) is written, N / 2 wide.
struct SxbMoe {
  const int* row_map;
  const int* block_expert;
  const float* slot_scale;
  long long expert_stride;
  int x_div;
};

template <int G, int MT, bool NT, int EPI = 0, bool ROWMAP = false>
__global__ __launch_bounds__(sxb_slots(G) * G * 64) void gemv_sharedx_bf16_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                                                 const u32x4_t* __restrict__ qw_r,
                                                                                 const uint32_t* __restrict__ zs_r,
                                                                                 const void* __restrict__ bias, void* __restrict__ y,
                                                                                 int M, int K, int N, int groups, int gmul, int gshift,
                                                                                 int NG, SxbMoe moe) {
  static_assert(!ROWMAP || MT == 1, "an expert block is one row tile");
  static_assert(!EPI || (ROWMAP && G % 2 == 0), "SiLU-mul: whole (gate, up) pairs of column groups per strip");
  constexpr int S = sxb_slots(G), U = sxb_units(G), C = S * U, NW = S * G, NTH = NW * 64;
  constexpr int ROWS = MT * 16, PIECES = ROWS * C * 16, PL = (PIECES + NTH - 1) / NTH;
  constexpr int BUF = ROWS * C * 256;                      // bytes of one x buffer
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, r = lane & 15;
  const int KB = K / 128, NCH = (KB + C - 1) / C;          // workgroup-uniform: every wave runs NCH chunk bodies
  int cg0 = blockIdx.x * G;
  if (cg0 + G > NG) cg0 = NG - G;                          // last strip overlaps its neighbour (same values written twice)
  const int c = wave % G, slot = wave / G;                 // this wave's column group and k-block slot
  const int* rows = nullptr;
  int xrow[PL];                                            // ROWMAP: activation row of this thread's piece i (-1: padding)
  if constexpr (ROWMAP) {
    const int eid = moe.block_expert[blockIdx.y];
    if (eid < 0) return;                                   // unused block (uniform over the workgroup)
    qw_r = (const u32x4_t*)((const unsigned char*)qw_r + (long long)eid * moe.expert_stride);
    zs_r = (const uint32_t*)((const unsigned char*)zs_r + (long long)eid * moe.expert_stride);
    rows = moe.row_map + (size_t)blockIdx.y * 16;
    M = 16;
#pragma unroll
    for (int i = 0; i < PL; ++i) {
      const int id = i * NTH + tid;
      const int p = id < PIECES ? rows[id / (C * 16)] : -1;
      xrow[i] = p >= 0 ? p / moe.x_div : -1;
    }
  }
  const u32x4_t* const wbase = qw_r + (size_t)(cg0 + c) * KB * 64 + lane;
  const uint32_t* const zbase = zs_r + (size_t)(cg0 + c) * groups * 16 + r;

  // ---- cooperative x loader: global -> registers (issue), registers -> LDS (park); piece p = (row p / 16C, 16-byte column p % 16C)
  auto x_issue = [&](int ch, u32x4_t (&xv)[PL]) {
#pragma unroll
    for (int i = 0; i < PL; ++i) {
      const int id = i * NTH + tid;
      const int row = id / (C * 16), kk = id - row * (C * 16);
      xv[i] = (u32x4_t){0u, 0u, 0u, 0u};
      if constexpr (ROWMAP) {
        if (xrow[i] >= 0 && ch * C + (kk >> 4) < KB) xv[i] = *(const u32x4_t*)(x + (size_t)xrow[i] * ldx + (size_t)ch * (C * 128) + kk * 8);
      } else {
        const bool in = id < PIECES && row < M && ch * C + (kk >> 4) < KB;
        if (in) xv[i] = *(const u32x4_t*)(x + (size_t)row * ldx + (size_t)ch * (C * 128) + kk * 8);
      }
    }
  };
  auto x_park = [&](int b, const u32x4_t (&xv)[PL]) {
#pragma unroll
    for (int i = 0; i < PL; ++i) {
      const int id = i * NTH + tid;
      const int row = id / (C * 16), kk = id - row * (C * 16);
      const int j = kk & 15;                               // 16-byte piece of the k-block: k-step d = j >> 2, quarter q = j & 3
      const int e = (((kk >> 4) * 4 + (j >> 2)) * MT + (row >> 4)) * 64 + (j & 3) * 16 + ((row & 15) ^ j);
      if (PIECES % NTH == 0 || id < PIECES) *(u32x4_t*)(smem + (size_t)b * BUF + (size_t)e * 16) = xv[i];
    }
  };

  // ---- weight ring: unit n of this wave = k-block (n / U) C + slot U + n % U
  u32x4_t wb[2];
  uint32_t zb[2];
  auto w_issue = [&](int n, auto SL) {
    constexpr int sl = decltype(SL)::value;
    const int kb = (n / U) * C + slot * U + n % U;
    if (kb < KB) {                                         // wave-uniform
      const u32x4_t* p = wbase + (size_t)kb * 64;
      wb[sl] = NT ? __builtin_nontemporal_load(p) : *p;    // streamed once: keep it out of the caches' way
      zb[sl] = zbase[(size_t)((kb * gmul) >> gshift) * 16];   // quantisation group kb / (g / 128), kb < 4096
    }
  };

  float4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (float4_t){0.f, 0.f, 0.f, 0.f};

  u32x4_t xs[2][PL];                                       // x chunks in flight: two register sets, a chunk travels for two chunk bodies
  auto chunk = [&](int ch, auto BP, auto SP) __attribute__((always_inline)) {
    constexpr int b = decltype(BP)::value, sp = decltype(SP)::value;
    if (ch + 2 < NCH) x_issue(ch + 2, xs[b]);              // workgroup-uniform; set b gave up chunk ch at the end of the previous body
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int kbl = slot * U + j;
      if (ch * C + kbl < KB) {                             // wave-uniform; units past K are skipped, the barrier below is not
        u32x4_t w = (sp + j) % 2 ? wb[1] : wb[0];
        const uint32_t zw = (sp + j) % 2 ? zb[1] : zb[0];
        asm volatile("" : "+v"(w));                        // the unit has arrived (the wait sits here) ...
        if ((sp + j) % 2) w_issue(ch * U + j + 2, std::integral_constant<int, 1>{});   // ... its replacement leaves at once
        else w_issue(ch * U + j + 2, std::integral_constant<int, 0>{});
        const SxbUnit un = sxb_unit(zw);
        const u32x4_t* xl = (const u32x4_t*)(smem + (size_t)b * BUF) + (size_t)kbl * 4 * MT * 64;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const u32x4_t frag = sxb_dequant(w[d], un);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {                // the dequantised fragment is shared by both row tiles
            const u32x4_t xa = xl[(d * MT + mt) * 64 + q * 16 + (r ^ (4 * d + q))];
            acc[mt] = sxb_mfma(xa, frag, acc[mt]);
          }
        }
      }
    }
    if (ch + 1 < NCH) x_park(b ^ 1, xs[b ^ 1]);            // chunk ch + 1, on its way since the start of the previous body
    __syncthreads();                                       // chunk ch + 1 is in its buffer; everyone is done reading chunk ch
  };

  w_issue(0, std::integral_constant<int, 0>{});
  w_issue(1, std::integral_constant<int, 1>{});
  x_issue(0, xs[0]);
  if (1 < NCH) x_issue(1, xs[1]);
  x_park(0, xs[0]);
  __syncthreads();
  for (int ch = 0; ch < NCH; ch += 2) {                    // two chunks per trip: buffer and ring slot are compile-time
    chunk(ch, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    if (ch + 1 < NCH) chunk(ch + 1, std::integral_constant<int, 1>{}, std::integral_constant<int, U % 2>{});
  }

  // ---- D[m = 4 q + i][n = r] per wave and row tile -> LDS (over the x buffers: the last chunk's barrier is behind every read),
  // added over the S waves of a column group in wave order
  float4_t* const red4 = (float4_t*)smem;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) red4[(wave * MT + mt) * 64 + lane] = acc[mt];
  __syncthreads();
  const float* const red = (const float*)smem;
  const int SW = 16 * G;
  if constexpr (EPI == 1) {
    // strip = G / 2 (gate, up) pairs of column groups (cg0 is even: G and NG are); output column 16 (pair index) + r of act[pairs, N / 2].
    // Rounding points of the fp16 epilogue (gemv_rp3_kernel) in bf16: gate and up each rounded, silu in fp32 on the rounded gate and
    // rounded, the product rounded.
    const int SH = 8 * G, I = N / 2;
    for (int idx = tid; idx < 16 * SH; idx += NTH) {
      const int m = idx / SH, col = idx - m * SH;
      const int pair = col >> 4, r16 = col & 15;
      const int n = (cg0 / 2 + pair) * 16 + r16;
      const int orow = rows[m];
      if (n >= I || orow < 0) continue;
      const int e = (((m & 15) >> 2) * 16 + r16) * 4 + (m & 3);
      float gv = red[(size_t)(2 * pair) * 256 + e], uv = red[(size_t)(2 * pair + 1) * 256 + e];
#pragma unroll
      for (int s = 1; s < S; ++s) {
        gv += red[(size_t)(s * G + 2 * pair) * 256 + e];
        uv += red[(size_t)(s * G + 2 * pair + 1) * 256 + e];
      }
      if (moe.slot_scale != nullptr) { const float sc = moe.slot_scale[orow]; gv *= sc; uv *= sc; }
      const float xg = round_to_dtype<AWQ_DTYPE_BF16>(gv);
      const float act = round_to_dtype<AWQ_DTYPE_BF16>(xg / (1.f + __expf(-xg))) * round_to_dtype<AWQ_DTYPE_BF16>(uv);
      ((uint16_t*)y)[(size_t)orow * I + n] = float_to_bf16_bits(act);
    }
  } else {
    for (int idx = tid; idx < M * SW; idx += NTH) {
      const int m = idx / SW, col = idx - m * SW;
      const int n = cg0 * 16 + col;
      if (n >= N) continue;
      int orow = m;
      if constexpr (ROWMAP) { orow = rows[m]; if (orow < 0) continue; }
      const int cc = col >> 4, e = (((m >> 4) * 64) + ((m & 15) >> 2) * 16 + (col & 15)) * 4 + (m & 3);
      float v = red[(size_t)cc * MT * 256 + e];
#pragma unroll
      for (int s = 1; s < S; ++s) v += red[(size_t)(s * G + cc) * MT * 256 + e];
      if constexpr (ROWMAP) { if (moe.slot_scale != nullptr) v *= moe.slot_scale[orow]; }
      store_output<AWQ_DTYPE_BF16>(y, (size_t)orow * N + n, v, bias, n);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// Every instantiation (G = 1 .. 8, one or two row tiles, either load policy) has zero scratch: 62 .. 162 VGPRs, 72 .. 120 of the 128
// where the workgroup has 16 waves (tools/rp_resources.py).  The AWQ-MoE instantiations (G = 1, 2, 3, 4, 6, 8; SiLU-mul on the even
// ones) take 0 .. 6 registers more than their dense width (66 .. 100 VGPRs), zero scratch too.
//
// 33 .. 64 rows (8192 < N <= 32768 only) run as two launches of this kernel: rows 0 .. 31 on two row tiles, then the rest.  The
// bf16 form of gemv_sharedx_wide_kernel (three / four row tiles per dequantised fragment, a wave owning two column groups) was
// written and is NOT shipped: on the MI355X its second column group of every wave column came out wrong on random activations at
// three row tiles (one-hot rows passed), and the four-row-tile form failed its one-hot check in 5 of 30 identical runs; both
// compiled without scratch (118 and 126 .. 128 VGPRs).  The cause was not found, so neither is built; the two launches stream and
// dequantise the weight twice, as the fp16 route did before gemv_sharedx_wide_kernel.

struct SxbLaunch {
  const u32x4_t* qw_r;
  const uint32_t* zs_r;
  int gmul, gshift, NG, nwg;
};

template <int G, int MT, bool NT>
static int sxb_go(const GemmArgs& a, const SxbLaunch& l) {
  constexpr size_t lds = sxb_lds(G, MT);
  static_assert(lds <= (size_t)kRpMaxLds, "x buffers past the CU's LDS");
  auto kern = gemv_sharedx_bf16_kernel<G, MT, NT>;
  if (lds > 64 * 1024) {                                   // opt in to more of the CU's 160 KiB of LDS, once per device
    static unsigned long long opted[2] = {0ull, 0ull};
    if (!opt_in_dynamic_lds((const void*)kern, kRpMaxLds, opted)) return AWQ_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(l.nwg), dim3(sxb_slots(G) * G * 64), lds, a.stream, (const uint16_t*)a.x, a.ldx, l.qw_r, l.zs_r, a.bias, a.y,
                     a.M, a.K, a.N, a.K / a.g, l.gmul, l.gshift, l.NG, SxbMoe{nullptr, nullptr, nullptr, 0ll, 1});
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

// the AWQ-MoE form: (strips, blocks) workgroups of one row tile
template <int G, int EPI>
static int sxb_go_moe(const GemmArgs& a, const SxbLaunch& l, int num_blocks, const SxbMoe& moe, bool nt) {
  constexpr size_t lds = sxb_lds(G, 1);
  static_assert(lds <= 64 * 1024, "no opt-in needed at one row tile");
  const dim3 grid(l.nwg, num_blocks), block(sxb_slots(G) * G * 64);
  if (nt)
    hipLaunchKernelGGL((gemv_sharedx_bf16_kernel<G, 1, true, EPI, true>), grid, block, lds, a.stream, (const uint16_t*)a.x, a.ldx, l.qw_r, l.zs_r,
                       nullptr, a.y, 16, a.K, a.N, a.K / a.g, l.gmul, l.gshift, l.NG, moe);
  else
    hipLaunchKernelGGL((gemv_sharedx_bf16_kernel<G, 1, false, EPI, true>), grid, block, lds, a.stream, (const uint16_t*)a.x, a.ldx, l.qw_r, l.zs_r,
                       nullptr, a.y, 16, a.K, a.N, a.K / a.g, l.gmul, l.gshift, l.NG, moe);
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

// a.M <= 32
template <int G>
static int sxb_go_rows(const GemmArgs& a, const SxbLaunch& l, bool nt) {
  if (a.M > 16) return nt ? sxb_go<G, 2, true>(a, l) : sxb_go<G, 2, false>(a, l);
  return nt ? sxb_go<G, 1, true>(a, l) : sxb_go<G, 1, false>(a, l);
}

template <int G>
static int sxb_go_g(const GemmArgs& a, const SxbLaunch& l, bool nt) {
  if (a.M <= 32) return sxb_go_rows<G>(a, l, nt);
  GemmArgs c = a;                                          // 33 .. 64 rows: rows 0 .. 31, then the rest
  c.M = 32;
  const int rc = sxb_go_rows<G>(c, l, nt);
  if (rc) return rc;
  c.M = a.M - 32;
  c.x = (const char*)a.x + (size_t)32 * a.ldx * 2;
  c.y = (char*)a.y + (size_t)32 * a.N * 2;
  return sxb_go_rows<G>(c, l, nt);
}

int launch_gemv_repacked_sharedx_bf16(const GemmArgs& a, const void* packed) {
  if (a.dtype != AWQ_DTYPE_BF16 || a.g % 128 || !repacked_supported(a.K, a.N, a.g, a.dtype) || a.M < 1 || a.M > 64 || a.ldx < a.K ||
      a.ldx % 8 || (((uintptr_t)a.x) & 15))
    return AWQ_ERR_BAD_VARIANT;                            // fp16, g in {32, 64}, more than 64 rows
  if (a.norm_h != nullptr || a.moe_slots != 0 || a.silu_mul) return AWQ_ERR_BAD_VARIANT;
  int G, nwg;
  if (!gemv_strip_geometry(a.K, a.N, &G, &nwg)) return AWQ_ERR_BAD_VARIANT;   // N > 32768: rounds mode
  if (a.K / 128 >= 4096 || a.g / 128 >= 4096) return AWQ_ERR_BAD_VARIANT;
  if (a.M > 32 && G <= 2) return AWQ_ERR_BAD_VARIANT;      // 33 rows up: wide matrices only (narrow ones have the split-K routes)
  SxbLaunch l;
  l.NG = rp_groups(a.N);
  l.nwg = nwg;
  l.qw_r = (const u32x4_t*)packed;
  l.zs_r = (const uint32_t*)packed + (size_t)l.NG * (a.K / 128) * 256;
  const int gk = a.g / 128;                                // k-blocks per quantisation group; kb / gk as a multiply-shift, exact for kb < 4096
  int lg = 0;
  while ((1 << lg) < gk) ++lg;
  l.gshift = 12 + lg;
  l.gmul = (int)(((1ll << l.gshift) + gk - 1) / gk);
  const bool nt = (size_t)a.K * a.N / 2 >= route::kStreamedMinBytes;
  switch (G) {
    case 1: return sxb_go_g<1>(a, l, nt);
    case 2: return sxb_go_g<2>(a, l, nt);
    case 3: return sxb_go_g<3>(a, l, nt);
    case 4: return sxb_go_g<4>(a, l, nt);
    case 5: return sxb_go_g<5>(a, l, nt);
    case 6: return sxb_go_g<6>(a, l, nt);
    case 7: return sxb_go_g<7>(a, l, nt);
    case 8: return sxb_go_g<8>(a, l, nt);
    default: return AWQ_ERR_BAD_VARIANT;
  }
}

// AWQ-MoE over expert-sorted 16-row blocks (awq_aux_moe_gemv_blocks, bf16).  Strip width: a launch holds many blocks (one per active
// expert at least) and every workgroup stages all 16 rows of its block, so — the fp16 launcher's reasoning — the widest strip the
// matrix has, not one strip per CU: 8 column groups (16 waves, 32 KiB of x buffers), else 6 / 4 / 2; an odd 3 or 1 only without
// SiLU-mul, whose strips must start on a gate group.  All of these have zero scratch (tools/rp_resources.py).  Activation rows are
// addressed with 64-bit offsets: no limit on num_blocks x ldx here.
int launch_gemv_repacked_sharedx_bf16_moe(const GemmArgs& a, const void* packed_experts, const int* row_map, const int* block_expert,
                                          int num_blocks, const float* slot_scale, long long expert_stride, int x_div, bool silu_mul) {
  if (a.dtype != AWQ_DTYPE_BF16 || a.g % 128 || !repacked_supported(a.K, a.N, a.g, a.dtype) || a.ldx < a.K || a.ldx % 8 ||
      (((uintptr_t)a.x) & 15) || num_blocks < 1 || num_blocks > 65535 || x_div < 1)
    return AWQ_ERR_BAD_VARIANT;
  if (a.K / 128 >= 4096 || a.g / 128 >= 4096) return AWQ_ERR_BAD_VARIANT;
  SxbLaunch l;
  l.NG = rp_groups(a.N);
  if (silu_mul && (a.N % 32 || (l.NG & 1))) return AWQ_ERR_BAD_VARIANT;
  const int G = l.NG >= 8 ? 8 : l.NG >= 6 ? 6 : l.NG >= 4 ? 4 : (l.NG == 3 && !silu_mul) ? 3 : l.NG >= 2 ? 2 : 1;
  if (silu_mul && (G & 1)) return AWQ_ERR_BAD_VARIANT;
  l.nwg = (l.NG + G - 1) / G;
  l.qw_r = (const u32x4_t*)packed_experts;
  l.zs_r = (const uint32_t*)packed_experts + (size_t)l.NG * (a.K / 128) * 256;
  const int gk = a.g / 128;                                // kb / gk as a multiply-shift, exact for kb < 4096 (as the dense launcher)
  int lg = 0;
  while ((1 << lg) < gk) ++lg;
  l.gshift = 12 + lg;
  l.gmul = (int)(((1ll << l.gshift) + gk - 1) / gk);
  const SxbMoe moe = {row_map, block_expert, slot_scale, expert_stride, x_div};
  const bool nt = (size_t)a.K * a.N / 2 >= route::kStreamedMinBytes;      // per expert, as the dense launcher decides per matrix
  if (silu_mul) {
    switch (G) {
      case 2: return sxb_go_moe<2, 1>(a, l, num_blocks, moe, nt);
      case 4: return sxb_go_moe<4, 1>(a, l, num_blocks, moe, nt);
      case 6: return sxb_go_moe<6, 1>(a, l, num_blocks, moe, nt);
      default: return sxb_go_moe<8, 1>(a, l, num_blocks, moe, nt);
    }
  }
  switch (G) {
    case 1: return sxb_go_moe<1, 0>(a, l, num_blocks, moe, nt);
    case 2: return sxb_go_moe<2, 0>(a, l, num_blocks, moe, nt);
    case 3: return sxb_go_moe<3, 0>(a, l, num_blocks, moe, nt);
    case 4: return sxb_go_moe<4, 0>(a, l, num_blocks, moe, nt);
    case 6: return sxb_go_moe<6, 0>(a, l, num_blocks, moe, nt);
    default: return sxb_go_moe<8, 0>(a, l, num_blocks, moe, nt);
  }
}

}  // namespace awq

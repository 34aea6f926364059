// Shared-activation GEMV for 33 .. 64 rows on wide matrices (8192 < N <= 32768: strips of G = 3 .. 8 column groups) on the
// MFMA-fragment-major layout (layout: awq_repacked.hip; fp16, group size a multiple of 128).
//
// gemv_sharedx_kernel (awq_repacked_sharedx.hip) multiplies a dequantised weight fragment into two row tiles; 33 .. 64 rows ran as
// two passes of it, every pass streaming and dequantising the whole weight again.  Here a fragment is dequantised once and
// multiplied into MT = 3 (33 .. 48 rows) or 4 (49 .. 64 rows) row tiles.  What carried over unchanged: a workgroup owns a strip
// of G column groups for all of K (no workspace, nothing shared between workgroups, safe under graph capture); x crosses the
// memory system once per workgroup and waits in two LDS buffers in v_mfma_f32_16x16x32_f16 A-operand order with the bank swizzle
// of the 32-row kernel; loads of chunk i + 2 are issued before chunk i is multiplied (two register sets); one barrier per chunk;
// two weight loads in flight per wave that never wait for x; rp_dequant; fixed-order reduction through LDS over the x
// buffers; rows >= M and k-blocks past K written as zeros without touching memory (ldx > K is fine).
//
// What four row tiles change:
//
// Chunk geometry.  Two 64-row buffers fit the CU's LDS only at C = 4 k-blocks per chunk (2 x 64 x 4 x 256 B = 128 KiB); C = 4 is
// used at three row tiles as well (96 KiB; C = 5 would fit but divides into no even wave split).  A chunk is 1024 MT 16-byte
// pieces, so the loader's PL <= 4 pieces per thread and set (today's 4 + 4 staging registers) needs 1024 threads at MT = 4: every
// instantiation runs 16 waves, PL = MT, each wave load reading 1 KiB of one row.  The (S, U) tables of sx_slots / sx_units do not
// apply: S = 4 k-block slots, U = 1 unit per wave and chunk for every G.
//
// LDS read traffic.  In the 32-row kernel every MFMA fetches its own 1 KiB A fragment.  A CU's four SIMDs retire four 16x16x32
// MFMAs per 16 cycles (the matrix pipe is held 16 cycles per instruction), i.e. would ask LDS for 4 KiB per 16 cycles = 256 B /
// clock: all of the read rate CDNA4 documents for ds_read_b128 (256 B / clock / CU, twice CDNA3's 128), before the loader's
// writes and any bank conflict.  With MT = 4 that is 16 KiB of reads per 1 KiB of weights and the reads, not the dequantisation,
// would bound the loop.  So a wave owns TWO column groups of the same k-block: one x fragment feeds two MFMAs (128 B / clock at
// full MFMA rate), the accumulators double to 2 x MT x 4 floats.  The strip has NC = ceil(G / 2) wave columns; with odd G the
// last column has a single group: it loads that one and runs the same straight-line body with zeros as the second operand
// (a separate one-group body put every odd-G instantiation into scratch).  Wave w < 4 NC multiplies: column w % NC, k-block slot w / NC; waves 4 NC .. 15 (G <= 6) only
// carry x.  Only this structure is built (the unpaired form is the 32-row kernel's, whose LDS traffic is the argument above).
//
// Weight ring.  One unit pair (two 1 KiB loads + their zs words) in flight per wave, re-issued the moment it has arrived, before
// it is dequantised; two pairs in flight do not fit 128 VGPRs beside 2 x MT x 4 accumulators and 2 x MT x 4 staging registers.
// Resources: MT = 4 123 .. 125 VGPRs, MT = 3 103 .. 104, scratch 0 in all 24 instantiations (tools/rp_resources.py).
//
// Barrier cadence.  A chunk body is one unit pair per wave: 8 dequantised fragments and 8 MT MFMAs (512 matrix-pipe cycles at
// MT = 4) between barriers, against 16 MFMAs per k-block in the removed barrier-per-k-block attempt; the x loads keep their lead of
// two chunk bodies.  All trip counts are functions of K alone: every wave executes every barrier.
//
// Epilogues: plain and bias through store_output (one rounding to fp16, then the bias with a second rounding).  Sums differ from
// the passes of the 32-row kernel in fp32 summation order only.
#include <type_traits>

#include "awq_repacked_gemv.h"

namespace awq {

constexpr int kSxwChunk = 4;        // k-blocks per chunk = k-block slots per wave column
constexpr int kSxwWaves = 16;
constexpr size_t sxw_lds(int G, int MT) {
  const size_t x2 = (size_t)2 * MT * 16 * kSxwChunk * 256, red = (size_t)kSxwChunk * ((G + 1) / 2) * 2 * MT * 1024;
  return x2 > red ? x2 : red;
}

template <int G, int MT, bool NT>
__global__ __launch_bounds__(kSxwWaves * 64) void gemv_sharedx_wide_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                                          const u32x4_t* __restrict__ qw_r,
                                                                          const uint32_t* __restrict__ zs_r,
                                                                          const void* __restrict__ bias, void* __restrict__ y, int M,
                                                                          int K, int N, int groups, int gmul, int gshift, int NG) {
  constexpr int C = kSxwChunk, NC = (G + 1) / 2, NTH = kSxwWaves * 64;
  constexpr int ROWS = MT * 16, PL = MT;                   // ROWS C 16 pieces of 16 bytes per chunk = PL per thread exactly
  constexpr int BUF = ROWS * C * 256;                      // bytes of one x buffer
  static_assert(ROWS * C * 16 == PL * NTH && PL <= 4, "loader pieces per thread");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, r = lane & 15;
  const int KB = K / 128, NCH = (KB + C - 1) / C;          // workgroup-uniform: every wave runs NCH chunk bodies
  int cg0 = blockIdx.x * G;
  if (cg0 + G > NG) cg0 = NG - G;                          // last strip overlaps its neighbour (same values written twice)
  const bool mul = wave < C * NC;                          // wave-uniform: this wave multiplies (the others only carry x)
  const int wc = wave % NC, slot = wave / NC;              // wave column (column groups 2 wc, 2 wc + 1) and k-block slot
  const bool two = G % 2 == 0 || 2 * wc + 1 < G;           // wave-uniform: the column has a second group
  const u32x4_t* const wbase = qw_r + (size_t)(cg0 + 2 * wc) * KB * 64 + lane;
  const uint32_t* const zbase = zs_r + (size_t)(cg0 + 2 * wc) * groups * 16 + r;

  // ---- cooperative x loader: global -> registers (issue), registers -> LDS (park).  Piece i of a wave = the 1 KiB of row
  // 16 i + wave that lies in the chunk, lane l its 16-byte column l: row and row tile are wave-uniform, the per-lane parts of
  // both addresses (one 32-bit offset each) are the same for every piece and chunk.
  const uint32_t xoff = (uint32_t)wave * (uint32_t)ldx * 2u + lane * 16;   // M ldx < 2^30 (launcher)
  const int pj = lane & 15;                                // 16-byte piece of the k-block: k-step d = pj >> 2, quarter q = pj & 3
  const uint32_t poff = (uint32_t)((((lane >> 4) * 4 + (pj >> 2)) * MT) * 64 + (pj & 3) * 16 + (wave ^ pj)) * 16;
  auto x_issue = [&](int ch, u32x4_t (&xv)[PL]) {
#pragma unroll
    for (int i = 0; i < PL; ++i) {
      xv[i] = (u32x4_t){0u, 0u, 0u, 0u};
      const char* rowp = (const char*)x + ((size_t)(16 * i) * ldx + (size_t)ch * (C * 128)) * 2;   // uniform
      if (16 * i + wave < M && ch * C + (lane >> 4) < KB) xv[i] = *(const u32x4_t*)(rowp + xoff);
    }
  };
  auto x_park = [&](int b, const u32x4_t (&xv)[PL]) {
#pragma unroll
    for (int i = 0; i < PL; ++i) *(u32x4_t*)(smem + b * BUF + i * 1024 + poff) = xv[i];   // entry (kb, d, row tile i, q, wave ^ pj)
  };

  // ---- weight ring: unit pair n of this wave = k-block n C + slot of its one or two column groups
  u32x4_t wb[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};     // a single-group column never loads [1]: it multiplies zeros into
  uint32_t zb[2] = {0u, 0u};                               // accumulators nobody reads, on the same straight-line body
  auto w_issue = [&](int n) {
    const int kb = n * C + slot;
    if (mul && kb < KB) {                                  // wave-uniform
      const u32x4_t* p = wbase + (size_t)kb * 64;
      const uint32_t* z = zbase + (size_t)((kb * gmul) >> gshift) * 16;   // quantisation group kb / (g / 128), kb < 4096
      wb[0] = NT ? __builtin_nontemporal_load(p) : *p;  // streamed once: keep it out of the caches' way
      zb[0] = z[0];
      if (two) {
        wb[1] = NT ? __builtin_nontemporal_load(p + (size_t)KB * 64) : p[(size_t)KB * 64];
        zb[1] = z[(size_t)groups * 16];
      }
    }
  };

  float4_t acc[2][MT];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[p][mt] = (float4_t){0.f, 0.f, 0.f, 0.f};
  const half2_t c960 = {(half_t)960.f, (half_t)960.f};

  // one unit pair: the column groups of k-block `slot` of the chunk in buffer b; every x fragment feeds both MFMAs
  auto multiply = [&](const u32x4_t* xl, int next) {
    constexpr int P = 2;
    u32x4_t w[P];
    uint32_t zw[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      w[p] = wb[p];
      zw[p] = zb[p];
      asm volatile("" : "+v"(w[p]));                       // the unit has arrived (the wait sits here) ...
    }
    w_issue(next);                                         // ... its replacement leaves at once
    half2_t s2[P], z1024[P], z64[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const half2_t zh = as_h2(zw[p]);
      s2[p] = __builtin_shufflevector(zh, zh, 0, 0);
      z1024[p] = __builtin_shufflevector(zh, zh, 1, 1);
      z64[p] = z1024[p] - c960;                            // exact: (1024 + z) - 960
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      u32x4_t frag[P];
#pragma unroll
      for (int p = 0; p < P; ++p) frag[p] = rp_dequant(w[p][d], z1024[p], z64[p], s2[p]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {                    // a dequantised fragment is shared by every row tile, an x fragment by both groups
        const u32x4_t xa = xl[(d * MT + mt) * 64 + q * 16 + (r ^ (4 * d + q))];
#pragma unroll
        for (int p = 0; p < P; ++p)
          acc[p][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, xa), __builtin_bit_cast(half8_t, frag[p]), acc[p][mt], 0, 0, 0);
      }
    }
  };

  u32x4_t xs[2][PL];                                       // x chunks in flight: two register sets, a chunk travels for two chunk bodies
  auto chunk = [&](int ch, auto BP) {
    constexpr int b = decltype(BP)::value;                 // buffer = chunk parity
    if (ch + 2 < NCH) x_issue(ch + 2, xs[b]);              // workgroup-uniform; set b gave up chunk ch at the end of the previous body
    if (mul && ch * C + slot < KB) {                       // wave-uniform; units past K are skipped, the barrier below is not
      const u32x4_t* xl = (const u32x4_t*)(smem + (size_t)b * BUF) + (size_t)slot * 4 * MT * 64;
      multiply(xl, ch + 1);
    }
    if (ch + 1 < NCH) x_park(b ^ 1, xs[b ^ 1]);            // chunk ch + 1, on its way since the start of the previous body
    __syncthreads();                                       // chunk ch + 1 is in its buffer; everyone is done reading chunk ch
  };

  w_issue(0);
  x_issue(0, xs[0]);
  if (1 < NCH) x_issue(1, xs[1]);
  x_park(0, xs[0]);
  __syncthreads();
  for (int ch = 0; ch < NCH; ch += 2) {                    // two chunks per trip: the buffer is compile-time
    chunk(ch, std::integral_constant<int, 0>{});
    if (ch + 1 < NCH) chunk(ch + 1, std::integral_constant<int, 1>{});
  }

  // ---- D[m = 4 q + i][n = r] per multiplying wave, group and row tile -> LDS (over the x buffers: the last chunk's barrier is
  // behind every read), added over the 4 slots of a wave column in slot order
  float4_t* const red4 = (float4_t*)smem;
  if (mul) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red4[((wave * 2 + p) * MT + mt) * 64 + lane] = acc[p][mt];
  }
  __syncthreads();
  const float* const red = (const float*)smem;
  const int SW = 16 * G;
  for (int idx = tid; idx < M * SW; idx += NTH) {
    const int m = idx / SW, col = idx - m * SW;
    const int n = cg0 * 16 + col;
    if (n >= N) continue;
    const int cc = col >> 4, e = (((m >> 4) * 64) + ((m & 15) >> 2) * 16 + (col & 15)) * 4 + (m & 3);
    float v = red[(size_t)(cc >> 1) * 2 * MT * 256 + (size_t)(cc & 1) * MT * 256 + e];
#pragma unroll
    for (int s = 1; s < C; ++s) v += red[(size_t)((s * NC + (cc >> 1)) * 2 + (cc & 1)) * MT * 256 + e];
    store_output<AWQ_DTYPE_F16>(y, (size_t)m * N + n, v, bias, n);
  }
}

template <int G, int MT, bool NT>
static int sxw_go(const GemmArgs& a, const void* packed, int NG, int nwg) {
  const u32x4_t* qw_r = (const u32x4_t*)packed;
  const uint32_t* zs_r = (const uint32_t*)packed + (size_t)NG * (a.K / 128) * 256;
  const int gk = a.g / 128;                                // k-blocks per quantisation group; kb / gk as a multiply-shift, exact for kb < 4096
  int lg = 0;
  while ((1 << lg) < gk) ++lg;
  const int gshift = 12 + lg, gmul = (int)(((1ll << gshift) + gk - 1) / gk);
  constexpr size_t lds = sxw_lds(G, MT);
  static_assert(lds <= (size_t)kRpMaxLds, "x buffers past the CU's LDS");
  auto kern = gemv_sharedx_wide_kernel<G, MT, NT>;
  static unsigned long long opted[2] = {0ull, 0ull};       // 96 / 128 KiB: opt in to more of the CU's 160 KiB of LDS, once per device
  if (!opt_in_dynamic_lds((const void*)kern, kRpMaxLds, opted)) return AWQ_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(kSxwWaves * 64), lds, a.stream, (const uint16_t*)a.x, a.ldx, qw_r, zs_r, a.bias, a.y, a.M, a.K,
                     a.N, a.K / a.g, gmul, gshift, NG);
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

template <int G>
static int sxw_go_g(const GemmArgs& a, const void* packed, int NG, int nwg, bool four, bool nt) {
  if (four) return nt ? sxw_go<G, 4, true>(a, packed, NG, nwg) : sxw_go<G, 4, false>(a, packed, NG, nwg);
  return nt ? sxw_go<G, 3, true>(a, packed, NG, nwg) : sxw_go<G, 3, false>(a, packed, NG, nwg);
}

int launch_gemv_repacked_sharedx_wide(const GemmArgs& a, const void* packed) {
  if (!repacked_fast(a.K, a.N, a.g, a.dtype) || a.M < 33 || a.M > 64 || a.ldx < a.K || a.ldx % 8 || (((uintptr_t)a.x) & 15))
    return AWQ_ERR_BAD_VARIANT;                            // bf16, g in {32, 64}, rows outside 33 .. 64
  if (a.norm_h != nullptr || a.moe_slots != 0) return AWQ_ERR_BAD_VARIANT;
  int G, nwg;
  if (!gemv_strip_geometry(a.K, a.N, &G, &nwg)) return AWQ_ERR_BAD_VARIANT;   // N > 32768: rounds mode
  if (G <= 2 || a.ldx >= (1 << 24) || a.K / 128 >= 4096 || a.g / 128 >= 4096) return AWQ_ERR_BAD_VARIANT;   // narrow matrices have the split-K routes; 32-bit x offsets
  const int NG = rp_groups(a.N);
  const bool four = a.M > 48;
  const bool nt = (size_t)a.K * a.N / 2 >= route::kStreamedMinBytes;
  switch (G) {
    case 3: return sxw_go_g<3>(a, packed, NG, nwg, four, nt);
    case 4: return sxw_go_g<4>(a, packed, NG, nwg, four, nt);
    case 5: return sxw_go_g<5>(a, packed, NG, nwg, four, nt);
    case 6: return sxw_go_g<6>(a, packed, NG, nwg, four, nt);
    case 7: return sxw_go_g<7>(a, packed, NG, nwg, four, nt);
    case 8: return sxw_go_g<8>(a, packed, NG, nwg, four, nt);
    default: return AWQ_ERR_BAD_VARIANT;
  }
}

}  // namespace awq

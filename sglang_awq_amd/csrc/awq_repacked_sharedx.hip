// Shared-activation decode GEMV for up to 32 rows on the MFMA-fragment-major layout (layout: awq_repacked.hip; fp16,
// group size a multiple of 128).
//
// gemv_repacked_kernel<.., MT = 2> lets every wave fetch the activation fragments of its own k-blocks from L2: eight 16 row x 64 B
// loads beside every G weight loads, 262 KB of x against 98 KB of weights per workgroup on 4096 x 12288.  Here x crosses the
// memory system once per workgroup and waits in LDS in the order v_mfma_f32_16x16x32_f16 wants its A operand.
//
// Work split.  A workgroup owns a strip of G column groups for all of K (the strip rule of launch_gemv_repacked): nothing is
// shared between workgroups, no workspace, no counters.  K is walked in chunks of C = S U consecutive k-blocks.  A unit is one
// (k-block, column group) pair = one 1 KiB wave load of weights.  The workgroup has S G waves; wave w owns column group w % G
// and the U consecutive k-blocks (w / G) U .. + U - 1 of every chunk, so its accumulators cover one column group (two row tiles
// x 4 floats).  (S, U) per strip width: sx_slots / sx_units below; waves whose k-blocks lie past K in the ragged last chunk skip
// their units but execute every barrier (all trip counts are functions of K alone).
//
// x in LDS.  Two buffers of [k-block 0..C-1][d 0..3][row tile][lane] x 16 B: entry (kb, d, mt, lane (q, r)) holds row 16 mt + r,
// k = 128 kb + 32 d + 8 q .. + 7 — the A fragment of the MFMA at k-step d — so a consumer fetches a fragment with one
// lane-consecutive ds_read_b128.  The loader (all waves) walks the chunk in 16-byte pieces, thread t taking pieces t, t + threads,
// ..: piece p = (row p / 16C, 16-byte column p % 16C), so 16C consecutive lanes read 256 C contiguous bytes of one row.  Written
// straight to the layout above, the 16 pieces of one (row, k-block) would all land on bank group r (entries 256 B apart): the
// entry index of row r is therefore stored as r ^ (4 d + q), distinct for those 16 lanes, and still a permutation of the 16
// entries of a (d, q) for the reader.  Rows >= M and k-blocks past K are written as zeros without touching memory.
// The loads of chunk i + 2 are issued before chunk i is multiplied (two register sets: a chunk is in flight for two chunk bodies,
// one was not enough to cover an L2 round trip beside the weight stream); chunk i + 1 is parked in the other buffer after chunk
// i's units, followed by the one workgroup barrier of the chunk.
//
// Weights never wait for x: each wave keeps two unit loads (weights + the unit's (scale | 1024 + zero) word per column) in flight
// across chunk boundaries; the load that replaces a unit leaves the moment the unit has arrived, before it is dequantised.
// Dequantisation is rp_dequant (awq_repacked_gemv.h): every W element rounded to fp16 exactly as awq_dequantize rounds it; one
// dequantised fragment feeds both row tiles.
//
// Reduction: the waves of a column group add their fp32 tiles through LDS (over the x buffers, behind the last barrier) in wave
// order: deterministic.  One rounding to fp16, then the bias with a second rounding; or, on gate / up interleaved copies, the
// SiLU-mul epilogue with the rounding points of gemv_repacked_kernel's.  Sums differ from the per-wave-k-range kernels in fp32
// summation order only.
#include <type_traits>

#include "awq_repacked_gemv.h"

namespace awq {

// waves per column group (k-block slots of a chunk) and units per wave and chunk, by strip width G; C = S U <= 8 keeps two
// 32-row buffers at 128 KiB
constexpr int sx_slots(int G) { return G <= 2 ? 8 : G <= 4 ? 4 : G == 5 ? 3 : 2; }
constexpr int sx_units(int G) { return G <= 2 ? 1 : (G <= 5 || G == 7) ? 2 : 4; }   // (G = 7, 14 waves: 4 would hold 2 x 5 x vectors per lane and spill)
constexpr size_t sx_lds(int G, int MT) {
  const size_t x2 = (size_t)2 * MT * 16 * sx_slots(G) * sx_units(G) * 256, red = (size_t)sx_slots(G) * G * MT * 1024;
  return x2 > red ? x2 : red;
}

template <int G, int MT, bool NT, int EPI>
__global__ __launch_bounds__(sx_slots(G) * G * 64) void gemv_sharedx_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                                           const u32x4_t* __restrict__ qw_r,
                                                                           const uint32_t* __restrict__ zs_r,
                                                                           const void* __restrict__ bias, void* __restrict__ y, int M,
                                                                           int K, int N, int groups, int gmul, int gshift, int NG) {
  constexpr int S = sx_slots(G), U = sx_units(G), C = S * U, NW = S * G, NTH = NW * 64;
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
  const u32x4_t* const wbase = qw_r + (size_t)(cg0 + c) * KB * 64 + lane;
  const uint32_t* const zbase = zs_r + (size_t)(cg0 + c) * groups * 16 + r;

  // ---- cooperative x loader: global -> registers (issue), registers -> LDS (park)
  auto x_issue = [&](int ch, u32x4_t (&xv)[PL]) {
#pragma unroll
    for (int i = 0; i < PL; ++i) {
      const int id = i * NTH + tid;
      const int row = id / (C * 16), kk = id - row * (C * 16);
      const bool in = id < PIECES && row < M && ch * C + (kk >> 4) < KB;
      xv[i] = (u32x4_t){0u, 0u, 0u, 0u};
      if (in) xv[i] = *(const u32x4_t*)(x + (size_t)row * ldx + (size_t)ch * (C * 128) + kk * 8);
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
  const half2_t c960 = {(half_t)960.f, (half_t)960.f};

  u32x4_t xs[2][PL];                                       // x chunks in flight: two register sets, a chunk travels for two chunk bodies
  auto chunk = [&](int ch, auto BP, auto SP) {
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
        const half2_t zh = as_h2(zw);
        const half2_t s2 = __builtin_shufflevector(zh, zh, 0, 0);
        const half2_t z1024 = __builtin_shufflevector(zh, zh, 1, 1);
        const half2_t z64 = z1024 - c960;                  // exact: (1024 + z) - 960
        const u32x4_t* xl = (const u32x4_t*)(smem + (size_t)b * BUF) + (size_t)kbl * 4 * MT * 64;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const u32x4_t frag = rp_dequant(w[d], z1024, z64, s2);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {                // the dequantised fragment is shared by both row tiles
            const u32x4_t xa = xl[(d * MT + mt) * 64 + q * 16 + (r ^ (4 * d + q))];
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, xa), __builtin_bit_cast(half8_t, frag), acc[mt], 0, 0, 0);
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
  auto total = [&](int m, int col) {                       // row m, column col of the strip
    const int cc = col >> 4, e = (((m >> 4) * 64) + ((m & 15) >> 2) * 16 + (col & 15)) * 4 + (m & 3);
    float v = red[(size_t)cc * MT * 256 + e];
#pragma unroll
    for (int s = 1; s < S; ++s) v += red[(size_t)(s * G + cc) * MT * 256 + e];
    return v;
  };
  if constexpr (EPI == 1) {
    // strip = G / 2 (gate, up) pairs of column groups; output column = 16 * (pair index) + r of act[M, N / 2]
    const int SH = 8 * G, I = N / 2;
    for (int idx = tid; idx < M * SH; idx += NTH) {
      const int m = idx / SH, cc = idx - m * SH;
      const int pair = cc >> 4, r16 = cc & 15;
      const int n = (cg0 / 2 + pair) * 16 + r16;
      if (n >= I) continue;
      const float gv = total(m, pair * 32 + r16), uv = total(m, pair * 32 + 16 + r16);
      const float xg = (float)(half_t)gv;                  // the unfused path rounds gate_up to fp16 first
      ((half_t*)y)[(size_t)m * I + n] = (half_t)(xg / (1.f + __expf(-xg))) * (half_t)uv;
    }
  } else {
    const int SW = 16 * G;
    for (int idx = tid; idx < M * SW; idx += NTH) {
      const int m = idx / SW, col = idx - m * SW;
      const int n = cg0 * 16 + col;
      if (n >= N) continue;
      store_output<AWQ_DTYPE_F16>(y, (size_t)m * N + n, total(m, col), bias, n);
    }
  }
}

template <int G, int MT, bool NT, int EPI>
static int sx_go(const GemmArgs& a, const void* packed, int NG, int nwg) {
  const u32x4_t* qw_r = (const u32x4_t*)packed;
  const uint32_t* zs_r = (const uint32_t*)packed + (size_t)NG * (a.K / 128) * 256;
  const int gk = a.g / 128;                                // k-blocks per quantisation group; kb / gk as a multiply-shift, exact for kb < 4096
  int lg = 0;
  while ((1 << lg) < gk) ++lg;
  const int gshift = 12 + lg, gmul = (int)(((1ll << gshift) + gk - 1) / gk);
  constexpr size_t lds = sx_lds(G, MT);
  static_assert(lds <= (size_t)kRpMaxLds, "x buffers past the CU's LDS");
  auto kern = gemv_sharedx_kernel<G, MT, NT, EPI>;
  if (lds > 64 * 1024) {                                   // opt in to more of the CU's 160 KiB of LDS, once per device
    static unsigned long long opted[2] = {0ull, 0ull};
    if (!opt_in_dynamic_lds((const void*)kern, kRpMaxLds, opted)) return AWQ_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(sx_slots(G) * G * 64), lds, a.stream, (const uint16_t*)a.x, a.ldx, qw_r, zs_r, a.bias, a.y, a.M,
                     a.K, a.N, a.K / a.g, gmul, gshift, NG);
  return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
}

template <int G>
static int sx_go_g(const GemmArgs& a, const void* packed, int NG, int nwg, bool two, bool nt, bool silu) {
  if (silu) {
    if constexpr (G % 2 == 0) return two ? sx_go<G, 2, true, 1>(a, packed, NG, nwg) : sx_go<G, 1, true, 1>(a, packed, NG, nwg);
    else return AWQ_ERR_BAD_VARIANT;
  }
  if (two) return nt ? sx_go<G, 2, true, 0>(a, packed, NG, nwg) : sx_go<G, 2, false, 0>(a, packed, NG, nwg);
  return nt ? sx_go<G, 1, true, 0>(a, packed, NG, nwg) : sx_go<G, 1, false, 0>(a, packed, NG, nwg);
}

int launch_gemv_repacked_sharedx(const GemmArgs& a, const void* packed, bool silu_mul) {
  if (!repacked_fast(a.K, a.N, a.g, a.dtype) || a.M < 1 || a.M > 32 || a.ldx < a.K || a.ldx % 8 || (((uintptr_t)a.x) & 15))
    return AWQ_ERR_BAD_VARIANT;                            // bf16, g in {32, 64}, more than 32 rows
  if (a.norm_h != nullptr || a.moe_slots != 0) return AWQ_ERR_BAD_VARIANT;
  int G, nwg;
  if (!gemv_strip_geometry(a.K, a.N, &G, &nwg)) return AWQ_ERR_BAD_VARIANT;   // N > 32768: rounds mode
  const int NG = rp_groups(a.N);
  if (silu_mul) {                                          // whole (gate, up) pairs of 16-column groups per strip
    if (a.N % 32) return AWQ_ERR_BAD_VARIANT;
    if (G & 1) ++G;
    if (G > kRpMaxG || G > NG) return AWQ_ERR_BAD_VARIANT;
    nwg = (NG + G - 1) / G;
  }
  if (a.K / 128 >= 4096 || a.g / 128 >= 4096) return AWQ_ERR_BAD_VARIANT;
  const bool two = a.M > 16;
  const bool nt = (size_t)a.K * a.N / 2 >= route::kStreamedMinBytes;
  switch (G) {
    case 1: return sx_go_g<1>(a, packed, NG, nwg, two, nt, silu_mul);
    case 2: return sx_go_g<2>(a, packed, NG, nwg, two, nt, silu_mul);
    case 3: return sx_go_g<3>(a, packed, NG, nwg, two, nt, silu_mul);
    case 4: return sx_go_g<4>(a, packed, NG, nwg, two, nt, silu_mul);
    case 5: return sx_go_g<5>(a, packed, NG, nwg, two, nt, silu_mul);
    case 6: return sx_go_g<6>(a, packed, NG, nwg, two, nt, silu_mul);
    case 7: return sx_go_g<7>(a, packed, NG, nwg, two, nt, silu_mul);
    case 8: return sx_go_g<8>(a, packed, NG, nwg, two, nt, silu_mul);
    default: return AWQ_ERR_BAD_VARIANT;
  }
}

}  // namespace awq

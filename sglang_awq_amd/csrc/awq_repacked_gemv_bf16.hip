// Straight-line decode GEMV in bf16 for 1 .. 16 rows on the MFMA-fragment-major layout (layout: awq_repacked.hip; bf16, group size a
// multiple of 128), reached as AWQ_RP_GEMV_BF16: the bf16 sibling of gemv_rp2_kernel (awq_repacked_gemv.h).  Before it a bf16 batch of
// 1 .. 16 rows ran gemv_rpx_kernel (awq_repacked_ext.hip: a compiler-scheduled runtime loop, every wave fetching its x fragments
// from global memory, the (scale | zero) words as separate small loads, strips of at most 4 column groups, ~29 VALU per dword
// through fp16) or, on 5- and 6-group strips, gemv_sharedx_bf16_kernel.
//
// What carried over from gemv_rp2_kernel unchanged: one strip of G column groups per workgroup (nothing shared between workgroups, no
// workspace, safe under graph capture); 16 waves, wave w owns k-blocks [w T, w T + T), T = ceil(KB / 16); straight-line code of G T
// units (c-major: a wave's consecutive loads are contiguous); x (M x T x 128 bf16) and the wave's (scale | zero) words fetched by at
// most 8 per-lane-addressed 16-byte loads and parked in wave-private LDS, no barrier; a ring of two 1 KiB non-temporal weight loads
// per wave, the replacement issued the moment a unit has arrived (one row: into a spare register set, before the unit is
// dequantised); the first two issue rounds separated by workgroup barriers; s_setprio falling with progress; fp32 partial sums added
// in wave order through LDS (deterministic); store_output<bf16>: one rounding of the sum, then the bias with a second rounding.
// v_mfma_f32_16x16x32_bf16 takes its A operand in the lane order of the f16 form, so x is staged as raw 16-bit words.
//
// What is new: the dequantisation, and where its constants live.  Every W element must be the bf16 awq_dequantize produces: (q - z)
// exact, the exact fp32 product with the scale, one round-to-nearest-even.  The tree has two bit-exact sequences; kept here is the
// fp32 route of awq_repacked_sharedx_bf16.hip,
//   lo = w & 0x0f0f0f0f          bytes (k0, k4, k1, k5) = q
//   hi = w & 0xf0f0f0f0          bytes (k2, k6, k3, k7) = 16 q   (no shift: the 16 goes into the scale)
//   v_cvt_f32_ubyte0..3 of both; per k-pair one packed fma  (q, q') * s - z s   resp.  (16 q, 16 q') * (s / 16) - z s;
//   v_cvt_pk_bf16_f32 per k-pair,
// 2 + 8 + 4 + 4 = 18 VALU per dword in the disassembly (over all instantiations, per MFMA: 2.2 v_and_b32, 8.2 v_cvt_f32_ubyte0..3, 4.0
// v_pk_fma_f32, 4.1 v_cvt_pk_bf16_f32 — with the masked words opaque to the compiler, see gb_dequant; transparent, clang folds the
// masks into one v_and_b32 per byte in front of a ubyte0 convert: 25 per dword, which measured 0.3 .. 3.3 us slower per launch, 8.53 against 7.70 us on 4096 x 11008 at one row).  The other one — the fp16 magic words fed into v_fma_mix_f32, the sequence of
// awq_repacked_prefill_bf16.hip — counts 17 (1 shift + 4 v_and_or_b32 + 8 v_fma_mix_f32 + 4 v_cvt_pk_bf16_f32), was built into this
// kernel first, and gave WRONG results on the MI355X in the one-row form: hipcc emits v_fma_mix_f32 and the three-operand
// v_and_or_b32 only from inline asm, and the compiler's MFMA hazard recogniser does not see the registers an inline-asm statement
// writes.  With one row only element 0 of a finished column group's accumulator stays live, the allocator hands the other three to
// the next unit's first asm results, and the asm wrote them while the group's last v_mfma_f32_16x16x32_bf16 was still in flight
// (write-after-write; no wait states inserted): the MFMA then overwrote t0, and one-hot rows came out as -(1024 + z) s in randomly
// chosen workgroups.  (The tile kernel ties its accumulators into AGPRs and never reuses them; the 2 .. 16-row form here keeps all
// four elements live and passed.)  One op per dword is not worth hand-placed wait states in a kernel whose register allocation is
// the compiler's, so the sequence that is plain C++ is kept: every instruction is visible to the hazard recogniser.
// Constants: s, s / 16 and -z s per (column, k-block) cost four ops (shift, multiply, bit-field extract + convert, multiply) from
// the (bf16 scale | fp16(1024 + zero)) word.  A GEMV lane meets each (column, k-block) for four dwords only, so that is one op per
// dword.  In the one-row form the staging pass turns every staged word ONCE into (s, s / 16, -z s, 0) and parks them in the
// wave-private LDS area, 16 bytes per (column, k-block) instead of 4: a unit then costs one ds_read_b128 and no constant arithmetic.
// The 2 .. 16-row form keeps the 4-byte words and spends the four ops per unit: its x rows fill the LDS — 16 rows of K = 4096 are
// 128 KiB of the 144 KiB a workgroup may have — and the wider constants would cut the domain to a handful of shapes.
// Exactness: z is a 4-bit integer and s has an 8-bit significand, so z s is exact in fp32; with q also 4-bit, (q - z) s has at most
// 13 significant bits, so the fma's single rounding returns it exactly, the conversion is the one RNE.  As in the other bf16 kernels
// this holds for NORMAL scales whose s / 16 is normal too (|s| >= 2^-122); for subnormal or near-subnormal bf16 scales the kernel is
// not held to bit equality with awq_dequantize.  q = z gives +0 where the generic form gives -0 under a negative scale; both add
// nothing to the sum.
// A k-block past K (ragged last wave, empty waves) re-reads the last valid k-block's weights and x from column 0 (both in bounds) and
// has its staged constants overwritten — with zeros in the one-row form, the word with (scale 0 | 1024) otherwise — by a second,
// predicated LDS store behind the first: every dequantised value is exactly 0, and there is no select on loaded data.  Its staged x
// is overwritten with zeros the same way (0 x NaN and 0 x inf are NaN: a non-finite x[0, 0 .. 127] would reach every row otherwise).
//
// LDS.  One row: [16][16 G] floats of partial sums, then per wave the x row, G T x 16 x 16 bytes of constants and a 64-byte dump
// slot.  2 .. 16 rows: per wave M x rows (T x 128 + 8 halves: rows 16 bytes apart in bank phase), G T x 16 words and a 16-byte dump
// slot; the [16][M][16 G] partial sums go OVER the staging area behind one more workgroup barrier (gemv_rp2_kernel keeps them beside
// it and so has no 16-row form on 8-group strips: 128 KiB of sums alone).  A shape whose area is larger than kRpMaxLds has no
// instantiation: AWQ_ERR_BAD_VARIANT.
#include "awq_repacked_gemv.h"

namespace awq {

typedef __bf16 gb_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float gb_float2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t gb_pack(gb_float2_t p) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(p, gb_bf16x2_t)); }

// (s, s / 16, -z s, 0) of one (bf16 scale | fp16(1024 + zero)) word: fp16(1024 + z) = 0x6400 | z, z sits in the low mantissa bits
__device__ __forceinline__ float4_t gb_consts(uint32_t zw) {
  const float s = __builtin_bit_cast(float, zw << 16);
  return (float4_t){s, s * 0.0625f, -(float)((zw >> 16) & 15u) * s, 0.f};
}

// 8 weights of one column (one dword) -> the 4 packed bf16 k-pairs of an MFMA B fragment: 18 VALU.  Nibble of k-element e sits at bit
// {0, 16, 4, 20, 8, 24, 12, 28}[e] (k-pair t = the halves of w >> 4 t)
__device__ __forceinline__ u32x4_t gb_dequant(uint32_t w, const float4_t& k) {
  // lo / hi are made opaque so that the byte extraction stays IN the convert (v_cvt_f32_ubyte0..3): left transparent, clang folds
  // the two masks into one v_and_b32 per byte in front of a ubyte0 convert (25 VALU per dword in the disassembly instead of 18).
  // The asm statements are empty: no instruction writes a register behind the compiler's back.
  uint32_t lo = w & 0x0f0f0f0fu, hi = w & 0xf0f0f0f0u;
  asm("" : "+v"(lo));
  asm("" : "+v"(hi));
  const gb_float2_t S = {k[0], k[0]}, S16 = {k[1], k[1]}, Z = {k[2], k[2]};
  const gb_float2_t q0 = {(float)(lo & 0xffu), (float)((lo >> 16) & 0xffu)};     // (k0, k1)
  const gb_float2_t q1 = {(float)(hi & 0xffu), (float)((hi >> 16) & 0xffu)};     // 16 (k2, k3)
  const gb_float2_t q2 = {(float)((lo >> 8) & 0xffu), (float)(lo >> 24)};        // (k4, k5)
  const gb_float2_t q3 = {(float)((hi >> 8) & 0xffu), (float)(hi >> 24)};        // 16 (k6, k7)
  return (u32x4_t){gb_pack(__builtin_elementwise_fma(q0, S, Z)), gb_pack(__builtin_elementwise_fma(q1, S16, Z)),
                   gb_pack(__builtin_elementwise_fma(q2, S, Z)), gb_pack(__builtin_elementwise_fma(q3, S16, Z))};
}

// bytes of LDS per (column group, k-block) of a wave's constants and of its dump slot (lanes without a chunk store there)
constexpr int gb_cbytes(bool m1) { return m1 ? 256 : 64; }
constexpr int gb_dump(bool m1) { return m1 ? 64 : 16; }
inline size_t gb_lds(int M, int G, int T) {
  const size_t red = (size_t)16 * M * 16 * G * sizeof(float);
  const size_t stg = (size_t)16 * ((size_t)M * (T * 128 + 8) * 2 + (size_t)G * T * gb_cbytes(M == 1) + gb_dump(M == 1));
  return M == 1 ? red + stg : (red > stg ? red : stg);
}

// CHS: 16-byte staging loads per lane.  M1 (one row): x and zs chunks in one id space, CHS covers both.  Otherwise CHS loads of x
// chunks and one more of the (<= 64) zs chunks.
template <int G, int T, int CHS, bool M1>
__global__ __launch_bounds__(1024) void gemv_bf16_kernel(const uint16_t* __restrict__ x, int64_t ldx, const u32x4_t* __restrict__ qw_r,
                                                         const uint32_t* __restrict__ zs_r, const void* __restrict__ bias,
                                                         void* __restrict__ y, int M, int K, int N, int groups, int gmul, int gshift,
                                                         int NG) {
  constexpr int W = 16, L = G * T, DD = 2 > L ? L : 2;
  constexpr int XS = T * 128 + 8;                          // halves per staged x row (+8: rows 16 B apart in bank phase)
  constexpr int CB = gb_cbytes(M1), DUMP = gb_dump(M1);
  extern __shared__ __attribute__((aligned(16))) float red[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = lane >> 4, r = lane & 15;
  const int KB = K / 128;                                  // quantisation group of k-block kb: (kb * gmul) >> gshift (= kb / (g / 128), kb < 4096)
  int cg0 = blockIdx.x * G;
  if (cg0 + G > NG) cg0 = NG - G;                          // last strip overlaps its neighbour (same values written twice)
  const int kb0 = wave * T;
  if constexpr (M1) M = 1;
  const int xbytes = M * XS * 2;                           // staged x of one wave
  unsigned char* const stg = (unsigned char*)red + (M1 ? (size_t)W * 16 * G * sizeof(float) : 0) + (size_t)wave * (xbytes + L * CB + DUMP);
  const int dump = xbytes + L * CB;

  // staging chunks (16 B): 16 M T chunks of x (row, 8-element column chunk) and NZ = 4 G T chunks of zs words (c, t, 4 columns)
  constexpr int NZ = L * 4, CHT = M1 ? CHS : CHS + 1;
  const int nx = M * T * 16;
  u32x4_t sv[CHT];
  int sdst[CHT];
  auto zs_src = [&](int j) {                               // j in [0, NZ)
    const int c = j / (T * 4), rem = j - c * (T * 4), t = rem >> 2, part = rem & 3;
    int kbz = kb0 + t;
    kbz = kbz < KB ? kbz : KB - 1;
    return (const unsigned char*)(zs_r + ((size_t)(cg0 + c) * groups + ((kbz * gmul) >> gshift)) * 16 + part * 4);
  };
  auto zs_dst = [&](int j) {                               // (c, t, part) -> offset of its 4 columns' constants
    const int c = j / (T * 4), rem = j - c * (T * 4), t = rem >> 2, part = rem & 3;
    return xbytes + ((c * T + t) * 16 + part * 4) * (CB / 16);
  };
  if constexpr (M1) {
    // one id space, lanes take ids lane + 64 i: x chunks first, then zs chunks.  k-blocks past K are whole k-blocks: their x chunks
    // are read from column 0 instead (in bounds), their constants are zeroed after staging
#pragma unroll
    for (int i = 0; i < CHS; ++i) {
      const int id = lane + 64 * i;
      const bool isx = id < T * 16;
      int j = id - T * 16;
      j = j < 0 ? 0 : (j >= NZ ? NZ - 1 : j);
      const bool xin = isx && (kb0 * 128 + id * 8 < K);
      const unsigned char* sx = (const unsigned char*)(x + (xin ? (size_t)kb0 * 128 + id * 8 : 0));
      sv[i] = *(const u32x4_t*)(isx ? sx : zs_src(j));
      sdst[i] = id >= T * 16 + NZ ? dump : isx ? id * 16 : zs_dst(j);
    }
  } else {
#pragma unroll
    for (int i = 0; i < CHS; ++i) {
      const int id = lane + 64 * i;
      const int row = id / (T * 16), cc = id - row * (T * 16);
      const bool xin = id < nx && (kb0 * 128 + cc * 8 < K);
      sv[i] = *(const u32x4_t*)(x + (xin ? (size_t)row * ldx + (size_t)kb0 * 128 + cc * 8 : 0));
      sdst[i] = id < nx ? (row * XS + cc * 8) * 2 : dump;
    }
    static_assert(M1 || NZ <= 64, "the zs chunks of a wave are one load");
    sv[CHS] = *(const u32x4_t*)zs_src(lane < NZ ? lane : NZ - 1);
    sdst[CHS] = lane < NZ ? zs_dst(lane) : dump;
  }
  // weights: wave-uniform base + lane offset; k-blocks past K are clamped (re-read, dequantised to zeros)
  const uint32_t loff = (uint32_t)lane * 16u;
  // DD loads in flight per wave.  One row: DD + 1 register sets, the load that replaces unit i leaves the moment unit i has arrived,
  // before its 4 x (18 VALU + MFMA) are computed (gemv_rp2_kernel: 0-3 % faster at one row, 1 % slower at 4 / 16 rows)
  constexpr int RB = (M1 && DD < L) ? DD + 1 : DD;
  u32x4_t wbuf[RB];
  auto load_w = [&](int i) {
    const int t = i % T, c = i / T;
    int kb = kb0 + t;
    kb = kb < KB ? kb : KB - 1;
    const unsigned char* p = (const unsigned char*)(qw_r + ((size_t)(cg0 + c) * KB + kb) * 64) + loff;
    wbuf[i % RB] = __builtin_nontemporal_load((const u32x4_t*)p);      // streamed once: keep it out of the caches' way
  };
#pragma unroll
  for (int i = 0; i < DD; ++i) {
    load_w(i);
    // the CU's queue holds round k of all sixteen waves before round k + 1 of any: the waves of a SIMD progress together
    __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0);
  }

  // park the staged chunks.  One row: x chunks as they are; zs chunks as the fp32 constants of each of their 4 columns.  Whether
  // load i holds x ids, zs ids or both is known at compile time; a lane of the other kind (or of neither) writes the dump slot.
#pragma unroll
  for (int i = 0; i < CHT; ++i) {
    if constexpr (M1) {
      const int id = lane + 64 * i;
      const bool isx = id < T * 16;
      if (64 * i < T * 16) *(u32x4_t*)(stg + (isx ? sdst[i] : dump)) = sv[i];
      if (64 * i + 64 > T * 16 && 64 * i < T * 16 + NZ) {
        float4_t* const d = (float4_t*)(stg + (isx ? dump : sdst[i]));
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = gb_consts(sv[i][e]);
      }
    } else {
      *(u32x4_t*)(stg + sdst[i]) = sv[i];
    }
  }
  if (kb0 + T > KB) {
    // ragged last wave / empty wave (wave-uniform, rare): a k-block past K must contribute nothing — see the header.  Its staged x
    // (re-read from x[0, 0 .. 127]) is overwritten with zeros as well: 0 x NaN or 0 x inf would otherwise turn every row NaN
#pragma unroll
    for (int i = 0; i < CHS; ++i) {
      const int id = lane + 64 * i;
      if constexpr (M1) {
        if (id < T * 16 && kb0 * 128 + id * 8 >= K) *(u32x4_t*)(stg + id * 16) = (u32x4_t){0u, 0u, 0u, 0u};
      } else {
        const int row = id / (T * 16), cc = id - row * (T * 16);
        if (id < nx && kb0 * 128 + cc * 8 >= K) *(u32x4_t*)(stg + (row * XS + cc * 8) * 2) = (u32x4_t){0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int jj = 0; jj < (NZ + 63) / 64; ++jj) {
      const int j = lane + 64 * jj;
      const int t = (j % (T * 4)) >> 2;
      if (j < NZ && kb0 + t >= KB) {
        if constexpr (M1) {
          float4_t* const d = (float4_t*)(stg + zs_dst(j));
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] = (float4_t){0.f, 0.f, 0.f, 0.f};
        } else {
          *(u32x4_t*)(stg + zs_dst(j)) = (u32x4_t){0x64000000u, 0x64000000u, 0x64000000u, 0x64000000u};
        }
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);

  const uint16_t* x_lds = (const uint16_t*)stg + (M1 ? 0 : (size_t)(r < M ? r : M - 1) * XS);   // (one row: every A row is row 0)
  const unsigned char* c_lds = stg + xbytes + r * (CB / 16);
  float4_t acc[G];
#pragma unroll
  for (int c = 0; c < G; ++c) acc[c] = (float4_t){0.f, 0.f, 0.f, 0.f};
  u32x4_t xa[4];
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int t = i % T, c = i / T;
    if (T > 1 || i == 0) {
#pragma unroll
      for (int d = 0; d < 4; ++d) xa[d] = *(const u32x4_t*)(x_lds + t * 128 + d * 32 + q * 8);
    }
    // issue priority tied to progress: whoever of a SIMD's four waves is behind outranks whoever is ahead, the four finish together
    switch (3 - (i * 4) / L) {
      case 3: __builtin_amdgcn_s_setprio(3); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      default: __builtin_amdgcn_s_setprio(0); break;
    }
    float4_t k;
    if constexpr (M1) k = *(const float4_t*)(c_lds + (c * T + t) * CB);
    else k = gb_consts(*(const uint32_t*)(c_lds + (c * T + t) * CB));
    u32x4_t w = wbuf[i % RB];
    if (RB > DD && i + DD < L) {
      asm volatile("" : "+v"(w));                          // unit i has arrived (the wait sits here) ...
      __builtin_amdgcn_sched_barrier(0);
      load_w(i + DD);                                      // ... its replacement leaves at once, into the spare register set
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const u32x4_t frag = gb_dequant(w[d], k);
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, xa[d]), __builtin_bit_cast(bf16x8_t, frag), acc[c], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (RB == DD && i + DD < L) {
      load_w(i + DD);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __builtin_amdgcn_s_setprio(0);

  // D[m = 4q + i][n = r] per column group -> LDS, summed over the waves in fixed order
  const int SW = 16 * G;
  if constexpr (M1) {
    if (q == 0) {
#pragma unroll
      for (int c = 0; c < G; ++c) red[wave * SW + c * 16 + r] = acc[c][0];
    }
  } else {
    __syncthreads();                                       // the sums go over the staging areas: every wave is done reading its own
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 4 * q + i;
#pragma unroll
      for (int c = 0; c < G; ++c)
        if (m < M) red[((size_t)wave * M + m) * SW + c * 16 + r] = acc[c][i];
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < M * SW; idx += W * 64) {
    const int m = M1 ? 0 : idx / SW, col = idx - m * SW;
    const int n = cg0 * 16 + col;
    if (n >= N) continue;
    float v = red[(size_t)m * SW + col];
#pragma unroll
    for (int w = 1; w < W; ++w) v += red[((size_t)w * M + m) * SW + col];
    store_output<AWQ_DTYPE_BF16>(y, (size_t)m * N + n, v, bias, n);
  }
}

// ------------------------------------------------------------------------------------------------ host
// Instantiations: the (G, T) table of gemv_rp2_kernel — G T <= 16 units with T <= 8 at every row count, up to 32 units with T <= 16
// for one row (the long form) — times those of the staging-chunk counts 1 / 2 / 4 / 8 that some row count 2 .. 16 selects at that T
// (M T <= 32; at T = 8 only 4 and 8).  Every one of them
// compiles without scratch inside the 128 VGPRs of a 1024-thread workgroup (tools/rp_resources.py lists them); gb_fits is where a
// spilling one would be struck out, so that it is neither built nor chosen.
constexpr bool gb_fits(int G, int T, int chunks, bool m1) {
  if (m1) return (rp2_fits(G, T) || rp2_fits_long(G, T)) && chunks == (T * 16 + G * T * 4 + 63) / 64;
  if (!rp2_fits(G, T)) return false;
  for (int M = 2; M <= 16; ++M) {                          // a chunk count no row count selects at this T is not built (rp2_chunks)
    const int n = (M * T * 16 + 63) / 64;
    if ((n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 0) == chunks) return true;
  }
  return false;
}

struct GbLaunch {
  const u32x4_t* qw_r;
  const uint32_t* zs_r;
  int gmul, gshift, NG, nwg, chunks;
  size_t lds;
};

template <int G, int T, int CHS, bool M1>
static int gb_go(const GemmArgs& a, const GbLaunch& l) {
  if constexpr (!gb_fits(G, T, CHS, M1)) {
    return AWQ_ERR_BAD_VARIANT;
  } else {
    auto kern = gemv_bf16_kernel<G, T, CHS, M1>;
    if (l.lds > 64 * 1024) {                               // opt in to more of the CU's 160 KiB of LDS, once per device
      static unsigned long long opted[2] = {0ull, 0ull};
      if (!opt_in_dynamic_lds((const void*)kern, kRpMaxLds, opted)) return AWQ_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(l.nwg), dim3(1024), l.lds, a.stream, (const uint16_t*)a.x, a.ldx, l.qw_r, l.zs_r, a.bias, a.y, a.M, a.K, a.N,
                       a.K / a.g, l.gmul, l.gshift, l.NG);
    return hipGetLastError() == hipSuccess ? AWQ_OK : AWQ_ERR_LAUNCH;
  }
}

template <int G, int T>
static int gb_go_t(const GemmArgs& a, const GbLaunch& l) {
  if (a.M == 1) {
    return gb_go<G, T, (T * 16 + G * T * 4 + 63) / 64, true>(a, l);      // <= 6 loads for G T <= 32, T <= 16
  }
  switch (l.chunks) {
    case 1: return gb_go<G, T, 1, false>(a, l);
    case 2: return gb_go<G, T, 2, false>(a, l);
    case 4: return gb_go<G, T, 4, false>(a, l);
    case 8: return gb_go<G, T, 8, false>(a, l);
    default: return AWQ_ERR_BAD_VARIANT;
  }
}

template <int G>
static int gb_go_g(int T, const GemmArgs& a, const GbLaunch& l) {
  switch (T) {
    case 1: return gb_go_t<G, 1>(a, l);
    case 2: return gb_go_t<G, 2>(a, l);
    case 3: return gb_go_t<G, 3>(a, l);
    case 4: return gb_go_t<G, 4>(a, l);
    case 5: return gb_go_t<G, 5>(a, l);
    case 6: return gb_go_t<G, 6>(a, l);
    case 7: return gb_go_t<G, 7>(a, l);
    case 8: return gb_go_t<G, 8>(a, l);
    case 9: return gb_go_t<G, 9>(a, l);
    case 10: return gb_go_t<G, 10>(a, l);
    case 11: return gb_go_t<G, 11>(a, l);
    case 12: return gb_go_t<G, 12>(a, l);
    case 13: return gb_go_t<G, 13>(a, l);
    case 14: return gb_go_t<G, 14>(a, l);
    case 15: return gb_go_t<G, 15>(a, l);
    case 16: return gb_go_t<G, 16>(a, l);
    default: return AWQ_ERR_BAD_VARIANT;
  }
}

int launch_gemv_repacked_bf16(const GemmArgs& a, const void* packed) {
  if (a.dtype != AWQ_DTYPE_BF16 || a.g % 128 || !repacked_supported(a.K, a.N, a.g, a.dtype) || a.M < 1 || a.M > 16 || a.ldx < a.K ||
      a.ldx % 8 || (((uintptr_t)a.x) & 15))
    return AWQ_ERR_BAD_VARIANT;                            // fp16, g in {32, 64}, more than 16 rows
  if (a.norm_h != nullptr || a.moe_slots != 0 || a.silu_mul) return AWQ_ERR_BAD_VARIANT;
  int G;
  GbLaunch l;
  if (!gemv_strip_geometry(a.K, a.N, &G, &l.nwg)) return AWQ_ERR_BAD_VARIANT;   // N > 32768: rounds mode
  if (a.K / 128 >= 4096 || a.g / 128 >= 4096) return AWQ_ERR_BAD_VARIANT;
  const int T = (a.K / 128 + 15) / 16;
  l.chunks = a.M == 1 ? 1 : rp2_chunks(a.M, G, T);         // 0: more than 8 staging loads per lane
  l.lds = gb_lds(a.M, G, T);
  if (!l.chunks || l.lds > (size_t)kRpMaxLds) return AWQ_ERR_BAD_VARIANT;
  l.NG = rp_groups(a.N);
  l.qw_r = (const u32x4_t*)packed;
  l.zs_r = (const uint32_t*)packed + (size_t)l.NG * (a.K / 128) * 256;
  const int gk = a.g / 128;                                // k-blocks per quantisation group; kb / gk as a multiply-shift, exact for kb < 4096
  int lg = 0;
  while ((1 << lg) < gk) ++lg;
  l.gshift = 12 + lg;
  l.gmul = (int)(((1ll << l.gshift) + gk - 1) / gk);
  switch (G) {
    case 1: return gb_go_g<1>(T, a, l);
    case 2: return gb_go_g<2>(T, a, l);
    case 3: return gb_go_g<3>(T, a, l);
    case 4: return gb_go_g<4>(T, a, l);
    case 5: return gb_go_g<5>(T, a, l);
    case 6: return gb_go_g<6>(T, a, l);
    case 7: return gb_go_g<7>(T, a, l);
    case 8: return gb_go_g<8>(T, a, l);
    default: return AWQ_ERR_BAD_VARIANT;
  }
}

}  // namespace awq

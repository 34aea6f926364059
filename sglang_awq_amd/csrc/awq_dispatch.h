// One place for the (M, K, N) -> kernel choices on the fragment-major layout and the measured crossover points behind them.
// Every threshold the launchers use is a named constant here; the launchers (awq_capi.hip: repacked_dispatch; awq_repacked.hip:
// launch_gemv_repacked; awq_repacked_splitk.hip: rps_plan; awq_repacked_prefill.hip: launch_gemm_repacked_pipelined) only apply them.
// fp16, group size a multiple of 128 unless noted; g in {32, 64} takes the generic kernels of awq_repacked_ext.hip (fp16 from 33 rows: the
// "g 32 / 64" row below), and so does bf16 except in the cells of the four bf16 rows below.
//
//  rows M        matrix                                   kernel                                        measured (us; source)
//  ------------  ---------------------------------------  --------------------------------------------  ------------------------------------------------
//  1..16         >= 16 k-blocks, streamed (>= 12 MiB) or   gemv_rp2_kernel (straight-line, 16 waves)      4096 x 11008 at 1 row 7.0 -> 6.3 (round 2, gemv_lab);
//                small; M T <= 32 staging chunks            ring of 2 loads per wave, x + zs staged once   4096 x 4096 4.39 -> 4.07; 1024 x 8192 (8 k-blocks) stays 8-wave
//  1             17..32 units per wave (G T <= 32, T <= 16) gemv_rp2_kernel, long form                     8192 x 28672 25.9 -> 24.0; 28672 x 8192 26.4 -> 23.9;
//                                                                                                         14336 x 4096 11.2 -> 8.0 (r03_kbench_long_rp2_ab.txt)
//  13..16        strips of <= 2 column groups, deep K      gemv_rp3_kernel (loop form of the ring)        11008 x 4096 at 16 rows 14.4 -> 13.1; 8192 x 1280 10.4 -> 8.5;
//                                                                                                         slower at 6..12 rows and on wide strips (r03_kbench_rp3_ab.txt)
//  9..32         K >= 8192 and N <= 4096, workspace given  gemv_rps_kernel (K split over workgroups)      11008 x 4096 at 12 / 16 / 32 rows 12.2 -> 10.6 / 14.7 -> 11.3 /
//                                                                                                         23.1 -> 17.2; not at K = 4096 or N = 8192 (r02_kbench_splitk_ab.txt)
//  17..32        N <= 32768; from 17 / 24 / 28 rows by strip    gemv_sharedx_kernel (x once per workgroup in    4096 x 22016 at 32 rows 20.7 -> 18.4; 4096 x 4096 10.6 -> 8.6; 11008 x 4096
//                width (kSharedXMinRows), not 5-group strips   LDS in MFMA order, waves split the units)      22.9 -> 19.5; 4096 x 12288 13.6 -> 13.2; 8192 x 1280 17.4 -> 12.6
//                                                                                                         (kbench_sharedx_ab.txt)
//  2..32 (rest)  anything else, N <= 32768                 gemv_repacked_kernel (round 1: 8 / 16 waves,    17..32 rows: two row tiles per fragment, 8 waves
//                                                          straight-line or double-buffered loop)
//  1..32         N > 32768                                 gemv_repacked_kernel, rounds of 3-group strips  8192 x 57344: 145 -> 51 (G = 3; 53 / 54.5 / 60 at G = 2 / 4 / 1)
//  33..64        8192 < N <= 32768 (kSharedXWideMinRows3 / 4:   gemv_sharedx_wide_kernel (x once per workgroup   4096 x 22016 at 64 rows 35.4 -> 23.3 (a 32-row pass: 18.4); 4096 x 12288
//                every strip width 3..8)                       in LDS, 3 / 4 row tiles per fragment, a wave     24.8 -> 17.6 (13.0); 8192 x 28672 75.1 -> 50.2 (38.7)
//                                                              owns two column groups of a k-block)             (kbench_sharedx_wide_ab.txt)
//  bf16 1..64    g % 128 == 0, N <= 32768: 17..32 rows on every   gemv_sharedx_bf16_kernel (the 32-row kernel's   4096 x 22016 at 16 / 32 / 64 rows 20.8 -> 18.7 / 40.8 -> 21.4 / 85.4 -> 41.5;
//                strip width, 1..16 on 5- and 6-group strips,     structure, dequantisation in fp32; 33..64 rows  4096 x 4096 at 32 rows 13.3 -> 9.5 (kbench_sharedx_bf16_ab.txt)
//                33..64 on N > 8192 (kSharedXBf16MinRows); 1..16   as two launches)
//                only where the row below is not routed
//  bf16 1..16    g % 128 == 0, N <= 32768: 1..8 rows on every strip     gemv_bf16_kernel (gemv_rp2_kernel's structure:   4096 x 11008 at 1 row 8.90 -> 7.70 (fp16 6.20); 4096 x 4096 4.95 -> 4.47; 4096 x 22016
//                width, 9..16 rows on G = 1..5 (gemv_bf16_wins);       x + zs staged per wave, ring of two loads;     at 1 / 8 rows 17.6 -> 12.6 / 18.1 -> 13.3; 8192 x 28672 at 1 row 36.6 -> 27.2
//                consulted first                                      dequantisation in fp32, constants in LDS)       (kbench_gemv_bf16_ab.txt)
//  bf16 33..     g % 128 == 0, wherever the bf16 GEMV above is    gemm_repacked_pipelined_bf16_kernel: 128 x 256  4096 x 22016 at 128 / 2048 / 4096 rows 87.5 -> 44.5 / 518 -> 367 / 950 -> 702;
//                not routed (tiles_bf16_wins)                     + 128 x 192 or 128 x 128 tiles, dequantisation  11008 x 4096 at 64 / 2048 rows 215 -> 105 / 226 -> 172
//                                                                 by v_fma_mix_f32 from the fp16 magic words      (kbench_tiles_bf16_ab.txt)
//  bf16 65..     g % 128 == 0, workspace given, >= 32 k-blocks,   the same kernel with K split over workgroups    11008 x 4096 at 65 / 128 / 512 rows 104.9 -> 24.7 / 105.6 -> 26.8 / 105.1 -> 60.2;
//                <= 64 wide tiles, or <= 128 on deep matrices     (SPLIT form) + pf_splitk_reduce_kernel<bf16>;   4096 x 4096 at 128 rows 41.9 -> 20.9; 8192 x 8192 79.6 -> 28.2 at 65 rows
//                or up to 160 rows (split_tiles_bf16_wins);       consulted before the row above                  (kbench_split_tiles_bf16_ab.txt)
//  g 32 / 64     fp16, 33 rows up (tiles_sg_wins)              gemm_repacked_pipelined_sg_kernel: the same      4096 x 22016 at 128 / 2048 / 4096 rows, g = 64: 80.2 -> 41.7 / 448 -> 369 / 825 -> 707;
//  33..                                                          tiles, every k-step its own (scale | zero) word  11008 x 4096 at 64 / 2048 rows, g = 32: 203 -> 98 / 206 -> 173
//                                                                 read through op_sel (no splat registers)        (kbench_tiles_sg_ab.txt)
//  33..160       while passes cost less than the tiles     passes of <= 32 rows of the GEMV                a pass 10.3 / 13.2 / 19.7 / 22.8 us on 4096 x 4096 / x 11008 / x 22016 /
//                (gemv_passes_max: 2..4 passes)                                                           11008 x 4096; under-filled tiles ~1.12 us per k-block: 37-44 / 91 us
//                                                                                                         (r03_kbench_middle_rows_ab.txt: 4096 x 22016 at 128 rows 78.6 -> 44)
//  33..          few wide tiles, workspace given           gemm_repacked_pipelined_kernel with K split     11008 x 4096 at 128 / 256 rows 88.7 -> 26.4 / 88.9 -> 40.5; 8192 x 8192 at 128
//                (pf_split_plan)                           over workgroups + pf_splitk_reduce_kernel       rows 76.4 -> 35.2; 4096 x 11008 at 96 / 128 rows 40.4 -> 27.1 / 38.6 -> 28.2
//                                                                                                         (r03_kbench_split_tiles_ab.txt)
//  97..          <= 64 wide tiles, no workspace            gemm_repacked_ksplit_kernel (128 x 64 tiles)    11008 x 4096 at 256 / 512 rows 142 -> 90 / 97
//  161..         any                                       gemm_repacked_pipelined_kernel: 128 x 256 tiles 2048 x 4096 x 11008: 206.6 -> 200.3 with the wide + narrow
//                                                          for whole rounds + 128 x 192 for the rest,      split; 192 / 256 rows 51.5 -> 43 with 128 x 128 tiles
//                                                          or 128 x 128 when few row tiles                 (r02_kbench_prefill_split_ab.txt, …_nj2_ab.txt)
//  the torch op  M >= 33 without a cached copy             awq_repack into the workspace, then the above   11008 x 4096: M = 64 212 -> 63, M = 256 217 -> 118
//  AWQ-MoE       <= 12 (token, expert) pairs               gemv_rp2_kernel, one grid row per pair          ~17 per pair (E = 8, 4096 / 14336); blocks ~215: cross at ~13
//                more                                      gemv_rp3_kernel on expert-sorted 16-row blocks  (r03_time_moe.txt; threshold in sglang_awq_amd/moe.py)
//  AWQ-MoE bf16  below 32 rows per expert on average       gemv_sharedx_bf16_kernel<G, 1, NT, EPI, ROWMAP>  8 / 64 pairs 222 / 223 (fp16 203 / 211; E = 8, 4096 / 14336); E = 256, 7168 / 2048 at
//                (no slot route)                            on 16-row blocks, strips of 8 / 6 / 4 / 2 groups 2048 pairs 1729 (fp16 1587) (time_moe_bf16.txt)
//  AWQ-MoE bf16  from 32 rows per expert                   gemm_repacked_pipelined_bf16_kernel<4, MOE, EPI>  4096 tokens 3405 (fp16 3259) Mixtral-like; blocks / tiles 554 / 552 at 32 rows per
//                (no 64-row tiles)                          on 128-row blocks                                expert, 613 / 556 at 40; DeepSeek-V3-like 4057 / 3604 at 32 (time_moe_bf16.txt)
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace awq {
namespace route {

// ---- rows -> route (awq_capi.hip: repacked_dispatch)
constexpr int kGemvMaxRows = 32;              // one launch of the streaming GEMV
constexpr int kGemvPassRows = 32;             // rows per pass when a batch runs as passes of the GEMV
constexpr int kGemvPassesMaxRows = 160;       // never more passes than this many rows' worth; fewer where the tiles are cheaper (gemv_passes_max)
// Passes of the 32-row GEMV against one launch of under-filled MFMA tiles (33 .. 160 rows).  Measured: a pass costs about
// 8 us + 0.26 us per MB of packed weight (2.5 x the per-MB term on deep matrices, K > 8192, where the 32-row kernel has no split-K form
// without a workspace); the tile kernel with at most one tile per CU takes about 1.12 us per k-block + 2 us (64 MFMAs per wave and block).
// Returns how many passes may run before the tiles win.
inline int gemv_passes_max(int64_t K, int64_t N) {
  const double mb = (double)K * (double)N / 2.0 / 1.0e6;
  const double t_pass = 8.0 + 0.26 * mb * (K > 8192 ? 2.5 : 1.0);
  const double t_tiles = 1.12 * (double)(K / 128) + 2.0;
  int p = (int)(t_tiles / t_pass + 0.35);
  return p < 1 ? 1 : (p > kGemvPassesMaxRows / kGemvPassRows ? kGemvPassesMaxRows / kGemvPassRows : p);
}
constexpr int kKsplitMinRows = 97;            // 128 x 64 K-split tiles from here ...
constexpr int kKsplitMaxWideTiles = 64;       // ... while the 128 x 256 tiling would give at most this many tiles
constexpr int kSplitKMinRows = 9;             // split-K GEMV (needs a workspace) from here
constexpr int kPfSplitMaxSlices = 8;          // split-K MFMA tiles (under-filled launches, workspace given): at most this many slices ...
constexpr int kPfSplitMinBlocks = 4;          // ... of at least this many k-blocks each
constexpr int kPfSplitMinRows = 33;           // ... from this many rows
constexpr int kPfSplitFewWideTiles = 48;      // ... when the 128 x 256 tiling gives at most this many tiles,
constexpr int kPfSplitDeepBlocks = 64;        // ... or, on matrices at least this many k-blocks deep,
constexpr int kPfSplitMaxWideTiles = 128;     // ... at most this many;
constexpr int kPfSplitNarrowWideTiles = 32;   // ... up to 64 rows only where even fewer (the GEMV passes win on wider matrices there)
constexpr int kPfSplitNarrowTilesMax = 64;    // 128 x 128 tiles while there are at most this many of them, 128 x 256 beyond
constexpr int64_t kRepackOnTheFlyMinM = 33;   // the op re-lays the weight out per call from here (no cached copy)

// ---- the GEMV family (awq_repacked.hip: launch_gemv_repacked)
constexpr size_t kStreamedMinBytes = 12u << 20;   // packed weight bytes from which a matrix is streamed from HBM: 16 waves, non-temporal loads
constexpr int kOneStripMaxGroups = 8;             // strip width (column groups) up to which one strip per CU is used; beyond: rounds
constexpr int kRoundsGroups = 3;                  // strip width in rounds mode
constexpr int kRp2MinKBlocks = 16;                // every one of the 16 waves has a k-block
constexpr int kRp3MinRows = 13;                   // loop form of the ring: from these rows ...
constexpr int kRp3MaxGroups = 2;                  // ... on strips of at most this many column groups

// ---- split-K GEMV plan (awq_repacked_splitk.hip: rps_plan)
constexpr int kRpsMinKBlocks = 64;                // K >= 8192
constexpr int kRpsMaxGroups = 256;                // N <= 4096
constexpr int kRpsStripGroups = 2;

// ---- shared-activation GEMV (awq_repacked_sharedx.hip; awq_capi.hip: repacked_dispatch, awq_repacked_fused.hip)
// First row count at which it measured faster than the two-row-tile gemv_repacked_kernel by more than the spread of repeated runs
// (0.5 %), per strip width G = ceil(ceil(N / 16) / 256); kSharedXNever where it did not (profiles/kbench_sharedx_ab.txt, us old -> new):
//   G = 1 from 24: 4096 x 4096 8.96 -> 8.22, 11008 x 4096 19.5 -> 18.1 (17 rows: 16.0 -> 17.1, not taken)
//   G = 2 from 24: 8192 x 7168 16.9 -> 16.2 (17 rows: 14.4 -> 15.1), 3584 x 8192 10.6 -> 9.9, 4096 x 8192 11.0 -> 10.4
//   G = 3 from 28: 4096 x 12288 13.05 -> 12.85, at 32 rows 13.6 -> 13.2 (24 rows: 12.27 -> 12.33)
//   G = 4 from 17: 4096 x 16384 13.8 -> 13.6;  G = 5 never: 4096 x 20480 at 32 rows 18.0 -> 18.4 (15 waves of 3 k-block slots)
//   G = 6, 7, 8 from 17: 4096 x 22016 17.8 -> 17.4 (32 rows 20.7 -> 18.4), 4096 x 28672 21.7 -> 20.3, 4096 x 32768 23.8 -> 21.6
constexpr int kSharedXMaxRows = 32;               // its x buffers hold two row tiles
constexpr int kSharedXNever = kSharedXMaxRows + 1;
constexpr int kSharedXMinRows[kOneStripMaxGroups + 1] = {kSharedXNever, 24, 24, 28, 17, kSharedXNever, 17, 17, 17};
// Where a workspace makes gemv_rps_kernel available (K >= 8192, N <= 4096) that one stays (11008 x 4096 at 32 rows: 16.7 against 19.5)
// except on matrices of at most this many column groups, from 17 rows (8192 x 1280 at 17 / 32 rows: 12.8 -> 11.2 / 14.2 -> 12.6)
constexpr int kSharedXOverSplitKMaxGroups = 80;
constexpr int kSharedXOverSplitKMinRows = 17;
constexpr int kSharedXSiluGroups = 6;             // SiLU-mul epilogue: measured on 6-group strips only (4096 x 22016 at 17 / 32 rows 17.7 -> 17.3 / 20.6 -> 18.2)
// Pure functions of the shape and of whether a split-K scratch was given: the same call always takes the same route.
inline bool sharedx_wins(int64_t M, int64_t K, int64_t N, bool splitk_scratch) {
  const int64_t NG = (N + 15) / 16, KB = K / 128, G = (NG + 255) / 256;
  if (M > kSharedXMaxRows || G > kOneStripMaxGroups) return false;
  if (splitk_scratch && KB >= kRpsMinKBlocks && NG <= kRpsMaxGroups && NG >= 8)   // rps_plan's domain
    return NG <= kSharedXOverSplitKMaxGroups && M >= kSharedXOverSplitKMinRows;
  return M >= kSharedXMinRows[G];
}
inline bool sharedx_wins_silu(int64_t M, int64_t N) {
  const int64_t NG = (N + 15) / 16;
  return M >= kSharedXMinRows[kSharedXSiluGroups] && M <= kSharedXMaxRows && (NG + 255) / 256 == kSharedXSiluGroups;
}

// ---- shared-activation GEMV for 33 .. 64 rows on wide matrices (awq_repacked_sharedx_wide.hip; awq_capi.hip: repacked_dispatch)
// Routed per (strip width G, row-tile count) where it measured faster than the parent route (passes of the 32-row GEMV or under-filled
// tiles; the same with a workspace: no split-K route applies on these widths) by more than the spread of repeated runs (<= 0.5 us,
// 1.5 %).  Every cell won (profiles/kbench_sharedx_wide_ab.txt, us old -> new at 33 / 48 rows | 49 / 64 rows; a 32-row pass beside it):
//   G = 3  4096 x 12288: 18.8 -> 13.8 / 21.3 -> 15.0 | 23.3 -> 16.6 / 24.8 -> 17.6   (13.0)
//   G = 4  4096 x 16384: 21.9 -> 15.0 / 24.5 -> 16.4 | 27.0 -> 17.3 / 28.3 -> 18.9   (14.9)
//   G = 5  4096 x 20480: 26.1 -> 18.0 / 30.5 -> 19.8 | 32.3 -> 21.6 / 34.2 -> 23.1   (17.6)
//   G = 6  4096 x 22016: 27.7 -> 18.6 / 32.8 -> 20.0 | 34.3 -> 21.8 / 35.4 -> 23.3   (18.4)
//   G = 7  4096 x 28672: 39.0 -> 22.8 / 39.3 -> 24.6 | 39.4 -> 27.4 / 39.5 -> 28.8   (22.1); 8192 x 28672: 59.7 -> 40.0 / 63.7 -> 43.0 | 70.3 -> 47.3 / 75.1 -> 50.2 (38.7)
//   G = 8  4096 x 32768: 40.3 -> 24.0 / 40.5 -> 25.7 | 40.6 -> 28.0 / 41.0 -> 29.5   (22.9)
// Not routed: 65 .. 128 rows as two passes of it (4096 x 22016 at 96 / 128 rows 39.0 -> 38.1 / 39.6 -> 44.4; 4096 x 12288 with a
// workspace 26.5 -> 28.7 / 29.0 -> 33.6): inside the spread or slower.
constexpr int kSharedXWideMinRows = 33;
constexpr int kSharedXWideMaxRows = 64;           // four row tiles
constexpr int kSharedXWideNever = kSharedXWideMaxRows + 1;
// first row count per strip width G from which it is routed, for three (33 .. 48) and four (49 .. 64) row tiles
constexpr int kSharedXWideMinRows3[kOneStripMaxGroups + 1] = {kSharedXWideNever, kSharedXWideNever, kSharedXWideNever, 33, 33, 33, 33, 33, 33};
constexpr int kSharedXWideMinRows4[kOneStripMaxGroups + 1] = {kSharedXWideNever, kSharedXWideNever, kSharedXWideNever, 49, 49, 49, 49, 49, 49};
inline bool sharedx_wide_wins(int64_t M, int64_t K, int64_t N) {
  const int64_t NG = (N + 15) / 16, G = (NG + 255) / 256;
  (void)K;
  if (M < kSharedXWideMinRows || M > kSharedXWideMaxRows || G > kOneStripMaxGroups) return false;
  return M <= 48 ? M >= kSharedXWideMinRows3[G] : M >= kSharedXWideMinRows4[G];
}

// ---- bf16 shared-activation GEMV, 1 .. 64 rows (awq_repacked_sharedx_bf16.hip; awq_capi.hip: repacked_dispatch)
// Routed per (row tiles, strip width G) where the forced kernel measured faster than the parent route (gemv_rpx_kernel in 16-row launches
// on strips of at most 4 column groups; the generic 128 x 256 tiles from 33 rows) by more than the spread of repeated runs (median
// 0.07 us, at most 0.7 us / 2.7 %).  profiles/kbench_sharedx_bf16_ab.txt, us old -> new, g = 128; every cell of the table was measured:
//   1 .. 16 rows (at 1 / 8 / 16): routed on G = 5  4096 x 20480: 19.0 -> 16.1 / 19.6 -> 17.0 / 20.7 -> 17.4
//                                       and G = 6  4096 x 22016: 19.0 -> 17.5 / 19.6 -> 18.1 / 20.8 -> 18.7
//     lost, not routed: G = 1 4096 x 4096 4.9 -> 6.4 / 5.6 -> 6.8 / 6.8 -> 7.2, 11008 x 4096 10.1 -> 13.8 / 11.5 -> 14.2 / 15.4 -> 15.4 (inside the
//     spread); G = 2 8192 x 7168 11.8 -> 13.3 / 12.0 -> 13.8 / 14.0 -> 15.1; G = 3 4096 x 12288 9.2 -> 10.7 / 9.8 -> 11.5 / 10.3 -> 12.1;
//     G = 4 4096 x 16384 11.7 -> 12.9 / 11.8 -> 13.5 / 12.5 -> 14.0; G = 7 4096 x 28672 20.1 -> 21.5 / 21.0 -> 22.3 / 22.1 -> 22.6, 8192 x 28672
//     36.5 -> 39.3 / 37.8 -> 40.1 / 39.6 -> 40.8; G = 8 4096 x 32768 21.6 -> 22.5 / 22.3 -> 23.1 / 23.1 -> 23.5
//   17 .. 32 rows (at 17 / 24 / 32): routed on every G
//     G = 1 4096 x 4096 11.2 -> 8.6 / 11.8 -> 9.1 / 13.3 -> 9.5, 11008 x 4096 25.0 -> 19.6 / 26.1 -> 20.4 / 30.2 -> 21.7; G = 2 8192 x 7168 24.9 -> 17.0 /
//     25.4 -> 17.7 / 27.3 -> 18.5; G = 3 4096 x 12288 18.7 -> 13.5 / 19.5 -> 14.1 / 19.7 -> 14.6; G = 4 4096 x 16384 22.8 -> 15.5 / 23.1 -> 16.1 / 23.6 -> 16.6;
//     G = 5 4096 x 20480 38.9 -> 19.5 / 39.6 -> 20.1 / 40.6 -> 20.8; G = 6 4096 x 22016 39.2 -> 20.4 / 39.9 -> 20.9 / 40.8 -> 21.4; G = 7 4096 x 28672
//     40.7 -> 24.5 / 41.4 -> 25.3 / 42.5 -> 26.1, 8192 x 28672 75.1 -> 44.1 / 75.9 -> 45.6 / 77.9 -> 46.6; G = 8 4096 x 32768 43.2 -> 25.4 / 43.9 -> 25.9 / 44.0 -> 26.7
//   33 .. 48 | 49 .. 64 rows (at 33 / 48 | 49 / 64; two launches of the kernel): routed on G = 3 .. 8, its whole domain
//     G = 3 4096 x 12288 84.9 -> 24.4 / 85.1 -> 25.4 | 85.1 -> 27.0 / 85.3 -> 28.3; G = 4 4096 x 16384 84.9 -> 28.3 / 85.0 -> 29.3 | 84.9 -> 30.7 / 85.3 -> 31.8;
//     G = 5 4096 x 20480 85.2 -> 35.2 / 85.3 -> 36.8 | 85.3 -> 38.9 / 85.3 -> 39.9; G = 6 4096 x 22016 85.1 -> 37.8 / 85.2 -> 38.9 | 85.2 -> 40.7 / 85.4 -> 41.5;
//     G = 7 4096 x 28672 85.3 -> 45.7 / 85.3 -> 46.6 | 85.3 -> 48.1 / 85.7 -> 50.1, 8192 x 28672 162.5 -> 82.9 / 162.8 -> 84.9 | 162.9 -> 88.5 / 163.2 -> 91.1;
//     G = 8 4096 x 32768 85.2 -> 47.0 / 85.5 -> 48.3 | 85.8 -> 49.7 / 85.9 -> 51.1
// The fp16 shared-activation kernels on the same shapes: 18.4 us (32 rows) and 23.2 (64 rows, one launch with four row tiles) on 4096 x 22016.
constexpr int kSharedXBf16MaxRows = 64;           // two launches of two row tiles
constexpr int kSharedXBf16Never = kSharedXBf16MaxRows + 1;
// first row count per (row tiles 1 .. 4, strip width G) from which it is routed, up to the last row of that tile count
constexpr int kSharedXBf16MinRows[4][kOneStripMaxGroups + 1] = {
    {kSharedXBf16Never, kSharedXBf16Never, kSharedXBf16Never, kSharedXBf16Never, kSharedXBf16Never, 1, 1, kSharedXBf16Never, kSharedXBf16Never},
    {kSharedXBf16Never, 17, 17, 17, 17, 17, 17, 17, 17},
    {kSharedXBf16Never, kSharedXBf16Never, kSharedXBf16Never, 33, 33, 33, 33, 33, 33},
    {kSharedXBf16Never, kSharedXBf16Never, kSharedXBf16Never, 49, 49, 49, 49, 49, 49}};
// A pure function of the shape: the same call always takes the same route.
inline bool sharedx_bf16_wins(int64_t M, int64_t K, int64_t N) {
  const int64_t NG = (N + 15) / 16, G = (NG + 255) / 256;
  (void)K;
  if (M < 1 || M > kSharedXBf16MaxRows || G > kOneStripMaxGroups) return false;
  return M >= kSharedXBf16MinRows[(M - 1) / 16][G];
}

// ---- bf16 straight-line GEMV, 1 .. 16 rows (awq_repacked_gemv_bf16.hip; awq_capi.hip: repacked_dispatch, consulted before sharedx_bf16_wins)
// Routed per (row bucket 1 / 2 .. 8 / 9 .. 16, strip width G) where both runs of the forced kernel (variant 7) were faster than both runs
// of the parent route (gemv_rpx_kernel; gemv_sharedx_bf16_kernel on G = 5, 6) and the gain is larger than the spread of identical
// repeated runs (median 0.1 us, at most 0.6).  profiles/kbench_gemv_bf16_ab.txt, us old -> new at 1 / 8 / 16 rows, g = 128, fp16's route
// on the same shape in brackets; "-": no instantiation (staging area past the LDS, or more than 32 units / staging chunks), the cell
// keeps its route.  Every measured cell won; a cell without a measurement is left unrouted (9 .. 16 rows on G = 6, 7, 8):
//   G = 1  4096 x 4096   4.95 -> 4.47 [4.09] / 5.58 -> 5.27 [5.00] / 6.82 -> 5.84 [6.92];  11008 x 4096  10.05 -> 7.73 [6.34] / - / -;
//          14336 x 4096 (one row, long form) 11.59 -> 9.41 [7.71]
//   G = 2  4096 x 8192   7.51 -> 6.04 [5.47] / 7.83 -> 6.92 [6.22] / 8.19 -> 7.91 [8.68];  8192 x 7168  11.76 -> 8.97 [7.72] / 12.06 -> 10.25 [10.64] / -;
//          28672 x 8192 (one row) - (34.3 [22.9]: 173 KiB of staging)
//   G = 3  4096 x 11008  8.90 -> 7.70 [6.20] / 9.37 -> 8.19 [7.26] / 10.04 -> 9.31 [8.99];  4096 x 12288  9.29 -> 8.00 [6.53] / 9.76 -> 8.52 [7.53] /
//          10.27 -> 9.66 [9.17]
//   G = 4  4096 x 16384  11.73 -> 9.44 [8.10] / 11.90 -> 10.75 [9.01] / 12.80 -> 11.54 [10.71]
//   G = 5  4096 x 20480  16.36 -> 11.96 [9.70] / 16.86 -> 12.32 [10.86] / 17.53 -> 13.74 [13.77]   (parent: the shared-activation kernel)
//   G = 6  4096 x 22016  17.61 -> 12.62 [10.72] / 18.14 -> 13.32 [11.48] / - (18.8: the shared-activation kernel stays)
//   G = 7  4096 x 28672  20.16 -> 15.10 [12.91] / 20.74 -> 15.85 [14.08] / -;  8192 x 28672  36.59 -> 27.15 [22.88] / - / -
//   G = 8  4096 x 32768  21.52 -> 17.27 [14.04] / 22.11 -> 18.10 [17.32] / -
// The 2 .. 8-row bucket was measured at 8 rows only and the 9 .. 16-row bucket at 16 only; G = 4 .. 8 rest on one matrix each.
// A routed cell whose shape has no instantiation (deep K at several rows) falls through to the routes below, as before.
constexpr int kGemvBf16MaxRows = 16;
// routed cells per (row bucket 1 / 2 .. 8 / 9 .. 16, strip width G)
constexpr bool kGemvBf16Routed[3][kOneStripMaxGroups + 1] = {
    {false, true, true, true, true, true, true, true, true},
    {false, true, true, true, true, true, true, true, true},
    {false, true, true, true, true, true, false, false, false}};
// A pure function of the shape: the same call always takes the same route.
inline bool gemv_bf16_wins(int64_t M, int64_t K, int64_t N) {
  const int64_t NG = (N + 15) / 16, G = (NG + 255) / 256;
  (void)K;
  if (M < 1 || M > kGemvBf16MaxRows || G > kOneStripMaxGroups) return false;
  return kGemvBf16Routed[M == 1 ? 0 : M <= 8 ? 1 : 2][G];
}

// ---- prefill tile model (awq_repacked_prefill.hip), in rounds of the 256 CUs
constexpr double kNarrowRound192 = 0.84;          // a round of 128 x 192 tiles / a round of 128 x 256 tiles (62 vs 73.5 us at K = 4096)
constexpr double kNarrowRound128 = 0.65;          // a round of 128 x 128 tiles (43.5 us for 172 tiles at M = 256, 4096 x 11008)
constexpr double kSecondLaunch = 0.02;

// ---- bf16 hand-pipelined tiles (awq_repacked_prefill_bf16.hip; awq_capi.hip: repacked_dispatch)
// Round model of its planned form, as above, from full rounds of 16 x 16 tiles at K = 4096 (profiles/kbench_tiles_bf16_ab.txt): 71.5 us
// for 256-wide tiles (fp16: 73.5), 59.1 for 192-wide, 47.9 for 128-wide (172 of them at 256 rows on 4096 x 11008: 44.4 against 64.0
// for the 86 wide ones).  The second launch was not measured on its own: the fp16 value.
constexpr double kTilesBf16Round192 = 0.83;
constexpr double kTilesBf16Round128 = 0.67;
constexpr double kTilesBf16SecondLaunch = 0.02;
// Routed from 33 rows: consulted after sharedx_bf16_wins, so at 33 .. 64 rows only where the two-launch bf16 GEMV is not routed
// (N <= 8192 or N > 32768).  The forced planned form (variant 4) against the parent route, us old -> new at 33 / 64 / 65 / 96 / 128 /
// 160 / 256 / 512 / 2048 / 4096 rows, g = 128, every cell measured twice, spread of identical runs at most 0.9 % (median 0.1 %):
//   4096 x 4096    84.3 -> 41.4 / 84.5 -> 41.5 / 84.5 -> 41.6 / 84.7 -> 41.7 / 84.9 -> 42.0 / 85.2 -> 42.0 / 85.1 -> 42.1 / 86.9 -> 43.0 / 95.7 -> 75.0 / 181.4 -> 141.5
//   4096 x 12288   (33 / 64 rows: the GEMV stays, 25.3 / 28.8 against 42.6 / 42.8) 85.4 -> 42.8 / 86.1 -> 43.1 / 87.2 -> 43.4 / 87.5 -> 43.9 / 87.5 -> 44.5 /
//                  89.4 -> 60.7 / 262.8 -> 202.1 / 519.1 -> 391.4
//   4096 x 22016   (33 / 64 rows: the GEMV stays, 38.6 / 42.5 against 43.0 / 43.3) 85.5 -> 43.4 / 86.2 -> 44.1 / 87.5 -> 44.5 / 88.8 -> 55.3 / 88.9 -> 57.4 /
//                  172.8 -> 109.3 / 518.2 -> 367.5 / 950.1 -> 701.9
//   11008 x 4096   214.6 -> 105.1 / 214.9 -> 105.2 / 214.9 -> 105.2 / 217.5 -> 105.3 / 221.4 -> 105.7 / 221.0 -> 105.1 / 221.2 -> 105.0 / 221.3 -> 105.3 /
//                  225.6 -> 172.1 / 444.3 -> 335.9
//   8192 x 28672   (33 / 64 rows: the GEMV stays although the tiles measured 84.0 -> 81.1 / 91.2 -> 82.1: one matrix of that strip width) 163.1 -> 82.2 /
//                  164.3 -> 82.9 / 165.7 -> 84.6 / 167.2 -> 121.1 / 167.6 -> 125.4 / 329.7 -> 235.4 / 1154.1 -> 876.5 / 2334.6 -> 1748.2
// The parent in every routed cell is gemm_rpx_tiled_kernel, the same decomposition compiler-scheduled, and no measured cell lost, so
// the rule is rows alone; shapes between and beyond the measured ones (other K, N > 32768) were not measured.  The fp16 routes on the
// same shapes: 72.1 / 137.0 us at 2048 / 4096 rows on 4096 x 4096, 679.6 at 4096 rows on 4096 x 22016 (bf16: 3 % behind); under-filled
// launches (one tile per CU or fewer: ~1.3 us per k-block) stay 2 .. 4 x behind fp16's split-K and GEMV-pass routes wherever the bf16
// split-K form below is not routed: without a workspace, and up to 64 rows.
constexpr int kTilesBf16MinRows = 33;
// A pure function of the shape: the same call always takes the same route.
inline bool tiles_bf16_wins(int64_t M, int64_t K, int64_t N) {
  (void)K; (void)N;
  return M >= kTilesBf16MinRows;
}

// ---- bf16 split-K tiles, 65 rows up, workspace given (awq_repacked_prefill_bf16.hip: pfb_split_plan; awq_capi.hip: repacked_dispatch,
// consulted before tiles_bf16_wins).  The slice rule shares kPfSplitMaxSlices / kPfSplitMinBlocks with fp16: S = min(256 / tiles, 8,
// k-blocks / 4, slices the workspace holds).  The forced planned form (variant 11) against the parent route (variant 4: one workgroup per
// tile, the whole K loop in it), us old -> new at 65 / 96 / 128 / 160 / 256 / 512 rows, g = 128, every cell measured twice (means; identical
// runs differ by 0.1 us in the median, at most 1.2 us / 2.0 %), fp16's route with its workspace in brackets, "-": fewer than two slices
// (more than 128 wide tiles, or the 32 MiB of scratch hold one slice): the variant refuses, the cell keeps its route
// (profiles/kbench_split_tiles_bf16_ab.txt):
//   4096 x 4096    41.6 -> 16.9 [16.5] / 41.8 -> 18.8 [18.9] / 41.9 -> 20.9 [20.5] / 42.0 -> 21.9 [21.0] / 42.2 -> 24.7 [23.9] / 42.9 -> 33.1 [39.2]
//   4096 x 12288   42.8 -> 26.0 [25.3] / 43.1 -> 27.5 [27.2] / 43.4 -> 29.7 [29.5] / 43.7 -> 41.9 [39.5] / 44.4 -> 43.6 [40.9] / 60.6 -> - [58.2]
//   4096 x 22016   43.6 -> 39.7 [38.9] / 43.9 -> 41.7 [39.8] / 44.8 -> 43.4 [40.2] / 55.0 -> - [51.4] / 56.8 -> - [54.3] / 109.0 -> - [103.7]
//   11008 x 4096   104.9 -> 24.7 [23.5] / 105.1 -> 25.8 [25.0] / 105.6 -> 26.8 [26.1] / 104.8 -> 34.2 [35.8] / 105.1 -> 38.4 [38.4] / 105.1 -> 60.2 [58.7]
//   8192 x 8192    79.6 -> 28.2 [28.0] / 79.8 -> 30.2 [29.7] / 80.0 -> 32.8 [31.6] / 79.5 -> 44.2 [43.5] / 79.9 -> 48.2 [47.7] / 85.3 -> 79.5 [78.0]
//   8192 x 28672   82.0 -> 70.5 [68.0] / 82.6 -> 73.4 [72.0] / 84.1 -> 76.6 [75.1] / 121.2 -> - [112.8] / 124.0 -> - [119.6] / 231.7 -> - [223.9]
// Routed: every cell in which both runs of the new form beat both runs of the parent by more than that spread — all that ran except
// 4096 x 12288 at 256 rows (96 wide tiles in two slices: 44.4 / 44.5 -> 43.5 / 43.7, 1.6 %, inside the largest spread; an earlier run
// of the same cell gave 44.2 / 44.4 -> 44.1 / 44.2): the partial traffic of 2 x 256 x 12288 floats cancels what half a K loop of 32
// k-blocks saves.  The smallest routed gains: 4096 x 22016 at 128 rows 2.3 % (2.5 % in the earlier run), 4096 x 12288 at 160 rows 3.6 %.
// As a rule over (wide tiles, depth, rows): at most 64 wide tiles at any measured depth; 65 .. 128 wide tiles on matrices of 64 k-blocks
// and more (8192 x 28672 up to 128 rows: 112 tiles; 8192 x 8192 at 512 rows: 128), on shallower ones up to 160 rows (4096 x 22016 up to
// 128 rows: 86 tiles; 4096 x 12288 at 160 rows: 96).  Matrices shallower than 32 k-blocks were not measured and keep their route.
// Tile width of the plan (variants 12 / 13, one run each, us 256-wide | 128-wide): the width with more workgroups wins; at equal
// counts (both fill the chip) 128-wide on the 32-k-block matrices (4096 x 4096 at 160 / 256 rows 26.1 | 21.9, 28.1 | 24.6: 64 narrow tiles)
// and 256-wide, with twice the slices, from 64 k-blocks (11008 x 4096 at 160 / 256 rows 34.1 | 37.9, 37.9 | 39.7; 8192 x 8192 at 65 / 96
// rows 28.3 | 29.3, 30.4 | 30.8: 64 narrow tiles) — narrow there only up to 32 tiles (11008 x 4096 at 65 rows 30.9 | 24.7).
constexpr int kPfSplitBf16MinRows = 65;           // up to 64 rows bf16 keeps its scratch-free GEMV and tile routes (the workspace query returns 0)
constexpr int kPfSplitBf16MinDepth = 32;          // routed on matrices at least this many k-blocks deep (nothing shallower was measured)
constexpr int kPfSplitBf16FewWideTiles = 64;      // ... when the 128 x 256 tiling gives at most this many tiles,
constexpr int kPfSplitBf16MaxWideTiles = 128;     // ... or at most this many (two slices; also the bound of the workspace query)
constexpr int kPfSplitBf16DeepBlocks = 64;        //     on matrices at least this many k-blocks deep,
constexpr int kPfSplitBf16ShallowMaxRows = 160;   //     on shallower ones up to this many rows
constexpr int kPfSplitBf16NarrowTilesMax = 64;    // 128 x 128 tiles while there are at most this many of them, 128 x 256 beyond;
constexpr int kPfSplitBf16NarrowTilesMaxDeep = 32;   // ... on matrices of kPfSplitBf16DeepBlocks k-blocks and more, this many
// A pure function of the shape: the same call (with a workspace) always takes the same route.
inline bool split_tiles_bf16_wins(int64_t M, int64_t K, int64_t N) {
  const int64_t wide_tiles = ((M + 127) / 128) * ((N + 255) / 256), KBT = K / 128;
  if (M < kPfSplitBf16MinRows || KBT < kPfSplitBf16MinDepth || wide_tiles > kPfSplitBf16MaxWideTiles) return false;
  return wide_tiles <= kPfSplitBf16FewWideTiles || KBT >= kPfSplitBf16DeepBlocks || M <= kPfSplitBf16ShallowMaxRows;
}

// ---- fp16 hand-pipelined tiles for group sizes 32 / 64 (awq_repacked_prefill_sg.hip; awq_capi.hip: repacked_dispatch)
// Round model of its planned form, as above, from full rounds of 16 x 16 tiles at K = 4096 (profiles/kbench_tiles_sg_ab.txt, two runs
// each): g = 64: 73.2 us for 256-wide tiles, 61.4 for 192-wide, 48.6 for 128-wide -> 0.84 / 0.66; g = 32: 74.8 / 60.9 / 48.3 ->
// 0.81 / 0.65.  Both ratios are measured and straddle fp16's 0.84 / 0.65, which are kept (the A/B below ran with them).  The second
// launch was not measured on its own: the fp16 value.  172 128-wide tiles at 256 rows on 4096 x 11008: 41.3 (g = 64) / 41.7 (g = 32)
// against 59.3 / 62.8 for the 86 wide ones.
constexpr double kTilesSgRound192 = 0.84;
constexpr double kTilesSgRound128 = 0.65;
constexpr double kTilesSgSecondLaunch = 0.02;
// Routed from 33 rows.  The forced planned form (variant 8) against the parent route (gemm_rpx_tiled_kernel: the same decomposition
// compiler-scheduled, 128 x 256 tiles only), us old -> new at 33 / 64 / 65 / 96 / 128 / 160 / 256 / 512 / 2048 / 4096 rows (means of the
// two runs of a cell; identical runs differ by at most 2.5 %, 0.12 % in the median):
//   4096 x 4096 g = 64  71.2 -> 38.6 / 71.7 -> 38.7 / 71.8 -> 38.7 / 71.9 -> 38.8 / 72.2 -> 39.0 / 72.3 -> 39.1 / 72.6 -> 39.1 / 73.2 -> 40.2 / 84.2 -> 73.7 / 157.6 -> 139.9
//   4096 x 4096 g = 32  71.6 -> 39.6 / 72.4 -> 39.7 / 72.4 -> 39.8 / 72.5 -> 39.9 / 72.7 -> 40.0 / 72.5 -> 39.5 / 72.7 -> 39.7 / 73.4 -> 40.3 / 84.3 -> 74.8 / 158.4 -> 141.1
//   4096 x 12288 g = 64  72.9 -> 39.3 / 78.2 -> 39.4 / 78.3 -> 39.5 / 78.9 -> 39.8 / 79.3 -> 40.1 / 74.6 -> 41.3 / 78.6 -> 42.6 / 81.4 -> 59.7 / 235.3 -> 201.5 / 459.0 -> 391.5
//   4096 x 12288 g = 32  76.5 -> 39.8 / 78.7 -> 39.9 / 78.7 -> 40.1 / 79.1 -> 40.2 / 79.6 -> 40.6 / 77.0 -> 41.4 / 78.7 -> 42.3 / 81.2 -> 59.7 / 237.5 -> 204.4 / 457.5 -> 398.2
//   4096 x 22016 g = 64  73.5 -> 40.1 / 79.0 -> 40.6 / 78.9 -> 40.2 / 79.6 -> 41.0 / 80.2 -> 41.7 / 76.0 -> 52.9 / 80.2 -> 55.7 / 155.6 -> 105.9 / 448.1 -> 368.6 / 824.6 -> 706.5
//   4096 x 22016 g = 32  77.1 -> 40.4 / 79.3 -> 40.9 / 79.2 -> 40.8 / 79.7 -> 41.4 / 80.3 -> 42.4 / 78.5 -> 54.0 / 80.6 -> 56.6 / 157.0 -> 107.9 / 450.0 -> 373.3 / 829.4 -> 710.1
//   11008 x 4096 g = 64  187.9 -> 95.9 / 201.4 -> 95.9 / 201.5 -> 95.9 / 202.3 -> 95.9 / 202.6 -> 96.1 / 187.9 -> 96.1 / 199.6 -> 96.5 / 199.7 -> 97.4 / 205.3 -> 170.2 / 391.4 -> 331.9
//   11008 x 4096 g = 32  194.9 -> 97.9 / 202.9 -> 97.8 / 202.9 -> 97.7 / 203.4 -> 97.8 / 203.6 -> 98.1 / 194.3 -> 97.4 / 200.0 -> 97.6 / 200.3 -> 98.3 / 205.8 -> 173.0 / 390.0 -> 334.2
//   8192 x 28672 g = 64  140.2 -> 75.4 / 150.5 -> 76.5 / 150.5 -> 76.7 / 151.5 -> 79.0 / 151.8 -> 82.5 / 143.5 -> 116.1 / 152.6 -> 125.3 / 296.9 -> 236.8 / 1030.7 -> 871.3 / 2049.5 -> 1729.7
//   8192 x 28672 g = 32  147.2 -> 76.7 / 151.5 -> 78.0 / 151.6 -> 77.6 / 151.9 -> 79.8 / 152.4 -> 82.7 / 149.2 -> 120.3 / 153.5 -> 126.6 / 298.5 -> 239.1 / 1034.5 -> 880.7 / 2052.6 -> 1758.8
// In every cell both runs of the new kernel beat both runs of the parent, by at least 10 % (4096 x 4096 at 4096 rows): no measured cell
// lost, so the rule is rows alone; shapes between and beyond the measured ones (other K, N > 32768) were not measured — their parent is
// the same generic kernel.  The fp16 g = 128 routes on the same shapes: 71.8 / 136.9 us at 2048 / 4096 rows on 4096 x 4096, 687.7 at 4096
// rows on 4096 x 22016 (g = 64 / 32: 3 % behind); under-filled launches (one tile per CU or fewer: ~1.2 us per k-block) stay up to
// 3 x behind g = 128's split-K and GEMV-pass routes, which the small groups lack.
constexpr int kTilesSgMinRows = 33;
// A pure function of the shape: the same call always takes the same route.
inline bool tiles_sg_wins(int64_t M, int64_t K, int64_t N, int64_t g) {
  (void)K; (void)N; (void)g;
  return M >= kTilesSgMinRows;
}

}  // namespace route
}  // namespace awq

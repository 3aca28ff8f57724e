// The tile GEMM kernels of csrc/gemm.hip: the ONE launch plan.  Host code only.  cogv_gemm and cogv_gemm_grouped ask gemm_plan /
// gemm_plan_persistent before every launch and launch what the plan says; cogv_gemm_plan answers from the same functions, so
// tests/test_gemm_plan.py pins kernel generation, grid, threads, dynamic LDS and every refusal without a GPU.
// The device's CU count, the reserved CUs, the raster group height and the COGV_GEMM_XP switch are the caller's to read (GemmEnv).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "cogview_hip.h"
#include "gemm_tile_order.h"

// tile, threads and dynamic LDS of each generation (index 1 .. 4).  Generations 3 and 4 are persistent: one workgroup per CU
// walks the launch's work list, which may hold several problems.
struct GemmGen { int tile_m, tile_n, threads, lds; };
constexpr GemmGen GEMM_GEN[5] = {{0, 0, 0, 0},
                                 {128, 128, 256, 65536},                          // register-staged, 128x128x64
                                 {256, 128, 256, 3 * (256 + 128) * 2 * 32},       // 3-stage ring of 256x128x32 tiles
                                 {256, 256, 512, 2 * 65536},                      // 8 waves ping-pong on a granule ring of 256x256x64
                                 {256, 256, 256, 2 * 65536 + 4 * 4096}};          // 4 waves on the same ring + the next item's first granules
constexpr int GEMM_BK = 64;                                                          // k-tile that split-K counts in (every generation)

enum { GEMM_TILE = 0, GEMM_SKINNY = 1 };
// The plan of one problem of a launch; the ints are cogv_gemm_plan's `out`, in this order.  items, grid_*, threads, lds and xp_* are
// the launch's (the same in every problem of a group); item_start is the problem's first item in the launch's work list.
// family GEMM_SKINNY (cogv_gemm, M <= 8): everything else is 0 and gemv_plan.h decides.
struct GemmPlan {
  int family, generation, tile_m, tile_n, tiles_m, tiles_n, splitk, ktiles_per_split, item_start, items, grid_x, grid_y, threads, lds,
      reduce_blocks, xp_ok, layout;
  uint32_t xp_magic_ig, xp_magic_gfull, xp_magic_gtail;
};
struct GemmEnv { int num_cus, reserved_cus, group_m, xp_enabled; };

// layout index, also the generation-4 unit's (bits 1..0 of COGV_W4_TU): 0 NT (forward), 1 NN (dgrad: B stored [K, N]),
// 2 TN (wgrad: both stored contraction-major), 3 A stored [K, M] only
constexpr int gemm_layout(bool trans_a, bool trans_b) { return trans_a ? (trans_b ? 2 : 3) : (trans_b ? 1 : 0); }

// split-K as the kernels run it: clamped to the k-tiles, then re-derived so that no split is empty
inline void gemm_split(int K, int requested, int& splitk, int& ktiles_per_split) {
  const int nk = (K + GEMM_BK - 1) / GEMM_BK;
  splitk = requested > 1 ? requested : 1;
  if (splitk > nk) splitk = nk;
  ktiles_per_split = (nk + splitk - 1) / splitk;
  splitk = (nk + ktiles_per_split - 1) / ktiles_per_split;
}

// generations 3 and 4 (the persistent kernels; every problem of a grouped launch) take the problem: whole k-tiles, at least one
// full tile each way, 32-bit DMA offsets into A and B, 16-byte rows of a contraction-major operand
inline bool gemm_persistent_takes(const cogv_gemm_desc& d) {
  const size_t a_span = (size_t)(d.trans_a ? d.K : d.M) * d.lda * 2, b_span = (size_t)(d.trans_b ? d.K : d.N) * d.ldb * 2;
  return d.M >= 256 && d.N >= 256 && d.K % GEMM_BK == 0 && a_span < (1ull << 32) && b_span < (1ull << 32) &&
         (!d.trans_a || (d.M & 7) == 0) && (!d.trans_b || (d.N & 7) == 0);
}

// auto dispatch between generation 2 (two workgroups per CU: 2 * cus slots a round) and generation 4 (cus slots) by how well the
// items fill whole rounds; generation 4 measured 1.1-1.4x at equal fill (16x16x32 MFMAs: less power per flop)
inline bool gemm_fill_prefers_persistent(int M, int N, int splitk, int cus) {
  const int i2 = ((M + 255) / 256) * ((N + 127) / 128) * splitk, i4 = ((M + 255) / 256) * ((N + 255) / 256) * splitk;
  const float e2 = (float)i2 / (float)(((i2 + 2 * cus - 1) / (2 * cus)) * 2 * cus);
  const float e4 = (float)i4 / (float)(((i4 + cus - 1) / cus) * cus);
  return e4 * 1.1f >= e2;
}

// workgroups of a persistent launch: one per CU the reserve leaves (at least 8: one per XCD), no more than items
inline int persistent_grid(int items, const GemmEnv& env) {
  return std::min(items, std::max(env.num_cus - env.reserved_cus, 8));
}

// The generation-4 kernel prefetches across item boundaries with the three divisions of the tile order as multiplications
// (w4_tile_fast).  The magic numbers of a geometry, and whether they reproduce w4_tile_slow for EVERY item of it (cached: a
// training step launches a handful of distinct geometries).
inline bool gemm_xp_magics(int tiles_m, int tiles_n, int group_m, uint32_t& mig, uint32_t& mgf, uint32_t& mgt) {
  struct Geo { int tm, tn, gm, ok; uint32_t mig, mgf, mgt; };
  static Geo cache[32];
  static int ncache = 0;
  Geo g{tiles_m, tiles_n, group_m, 1, 0, 0, 0};
  int i = 0;
  while (i < ncache && !(cache[i].tm == tiles_m && cache[i].tn == tiles_n && cache[i].gm == group_m)) ++i;
  if (i < ncache) g = cache[i];
  else {
    g.mig = w4_magic((uint32_t)(group_m * tiles_n)); g.mgf = w4_magic((uint32_t)group_m); g.mgt = w4_magic((uint32_t)(tiles_m % group_m));
    for (uint32_t b = 0; b < (uint32_t)(tiles_m * tiles_n) && g.ok; ++b) {
      uint32_t m1, n1, m2, n2;
      w4_tile_slow(b, (uint32_t)tiles_m, (uint32_t)tiles_n, (uint32_t)group_m, m1, n1);
      w4_tile_fast(b, (uint32_t)tiles_m, (uint32_t)tiles_n, (uint32_t)group_m, g.mig, g.mgf, g.mgt, m2, n2);
      if (m1 != m2 || n1 != n2) g.ok = 0;
    }
    if (ncache < 32) cache[ncache++] = g;
  }
  mig = g.mig; mgf = g.mgf; mgt = g.mgt;
  return g.ok != 0;
}

// one problem's share of a plan of `generation`
inline void gemm_plan_problem(const cogv_gemm_desc& d, int generation, GemmPlan& p) {
  const GemmGen& g = GEMM_GEN[generation];
  p = GemmPlan{};
  p.family = GEMM_TILE; p.generation = generation; p.tile_m = g.tile_m; p.tile_n = g.tile_n;
  p.tiles_m = (d.M + g.tile_m - 1) / g.tile_m; p.tiles_n = (d.N + g.tile_n - 1) / g.tile_n;
  gemm_split(d.K, d.splitk, p.splitk, p.ktiles_per_split);
  p.items = p.tiles_m * p.tiles_n * p.splitk;
  p.grid_x = p.tiles_m * p.tiles_n; p.grid_y = p.splitk;
  p.threads = g.threads; p.lds = g.lds;
  // the reduce pass: 256 threads, 8 columns each, grid-stride above 2048 blocks
  if (p.splitk > 1) p.reduce_blocks = (int)std::min<size_t>(((size_t)d.M * (d.N / 8) + 255) / 256, 2048);
  p.layout = gemm_layout(d.trans_a, d.trans_b);
}

// `count` problems gemm_persistent_takes, of one layout, in ONE launch of generation 3 or 4: the work list is the problems' items
// one after the other.  Exact prefetch (generation 4): one problem, no split-K, an even number (>= 4) of k-tiles, more items than
// CUs, and magic numbers that verify.
inline void gemm_plan_persistent(const cogv_gemm_desc* d, int count, int generation, const GemmEnv& env, GemmPlan* pl) {
  int items = 0;
  for (int i = 0; i < count; ++i) {
    gemm_plan_problem(d[i], generation, pl[i]);
    pl[i].item_start = items;
    items += pl[i].items;
  }
  GemmPlan& p0 = pl[0];
  const int nkt = d[0].K / GEMM_BK;
  if (generation == 4 && env.xp_enabled && count == 1 && p0.splitk == 1 && nkt >= 4 && (nkt & 1) == 0 && items > env.num_cus)
    p0.xp_ok = gemm_xp_magics(p0.tiles_m, p0.tiles_n, env.group_m, p0.xp_magic_ig, p0.xp_magic_gfull, p0.xp_magic_gtail);
  for (int i = 0; i < count; ++i) { pl[i].items = items; pl[i].grid_x = persistent_grid(items, env); pl[i].grid_y = 1; }
}

// cogv_gemm's launch of a descriptor build_gemm_args accepted and the skinny-M kernels did not take: kernel_variant and the shape
// -> generation, or false: the launch's refusal (3, unsupported).
//   1 asks for generation 1, which also takes what the LDS-ring kernels (2 .. 4) do not: K % 64, M or N < 64
//   3 asks for generation 2; 9 / 10 for generation 3 / 4, where the persistent kernels take the problem (else: as auto)
//   anything else is auto: generation 4 if it takes the problem and fills its rounds about as well as generation 2, else 2
//   COGV_EPI_COLSUM exists in generations 3 and 4 only: unsupported where they do not take the problem or another one is asked for
inline bool gemm_plan(const cogv_gemm_desc& d, const GemmEnv& env, GemmPlan& p) {
  const bool ring_ok = d.K % GEMM_BK == 0 && d.M >= 64 && d.N >= 64 && (!d.trans_a || (d.M & 7) == 0) && (!d.trans_b || (d.N & 7) == 0) &&
                       d.kernel_variant != 1;
  const bool colsum = (d.flags & COGV_EPI_COLSUM) != 0;
  if (!ring_ok) {
    if (colsum) return false;
    gemm_plan_problem(d, 1, p);
    return true;
  }
  const bool persistent = gemm_persistent_takes(d);
  int v = d.kernel_variant;
  if (v != 3 && v != 9 && v != 10) v = 0;
  if (colsum && (!persistent || v == 3)) return false;
  if (colsum && v != 9) v = 10;
  if ((v == 9 || v == 10) && !persistent) v = 0;
  if (v == 0) {
    int splitk, kps;
    gemm_split(d.K, d.splitk, splitk, kps);
    v = persistent && gemm_fill_prefers_persistent(d.M, d.N, splitk, env.num_cus) ? 10 : 3;
  }
  if (v == 3) gemm_plan_problem(d, 2, p);
  else gemm_plan_persistent(&d, 1, v == 9 ? 3 : 4, env, &p);
  return true;
}

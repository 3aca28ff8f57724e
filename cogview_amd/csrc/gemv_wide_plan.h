// Wide products of the decode step (1 .. 64 rows on 16-bit weights): the ONE class list and the ONE launch plan of
// csrc/gemv_wide.hip's kernel.  Host code only.  cogv_gemm_rows asks gw_plan() before its launch, cogv_gemm_rows_plan answers from
// the same function, and a unit of gemv_wide.hip turns the plan into its template instantiation by expanding the same list.
#pragma once
#include "weight_operand.h"      // the weight formats GV_W16 | GV_W8 | GV_W4

// The classes.  A product takes the FIRST row whose K range holds K: the class depends on K ALONE, so the association of a
// column's sum -- which contraction slots a wave adds up, and the order the waves' partial tiles are summed in -- does not depend
// on the row count, and a row's bits do not depend on the rows next to it.
//   X(name, K from, K to, NWK, LP, guarded)
//   NWK waves share a 16-column tile: wave kw takes the load PAIRS q = kw, kw + NWK, .. (a pair: contraction elements 64 q .. 64 q
//   + 63, one 128-byte line of each weight row), LP of them at most;  guarded: K below the class's maximum (pairs past K are loaded
//   from a clamped address and not multiplied).
// Exact classes for the widths of the model family (h = 1024: K = 1024 / 4096; h = 2560: K = 2560 / 10240), guarded ones for any
// other multiple of 512.
#define GW_CLASSES(X)                      \
  X(K1024,  1024,  1024,  4,  4,  false)   \
  X(K2560,  2560,  2560,  8,  5,  false)   \
  X(K4096,  4096,  4096,  16, 4,  false)   \
  X(K10240, 10240, 10240, 16, 10, false)   \
  X(G4,     512,   1024,  4,  4,  true)    \
  X(G8,     512,   2560,  8,  5,  true)    \
  X(G16,    512,   10240, 16, 10, true)

#define GW_ENUM_ROW(NAME, ...) GWC_##NAME,
enum GwClassId { GW_CLASSES(GW_ENUM_ROW) GWC_COUNT };
#undef GW_ENUM_ROW

struct GwClass { int k_from, k_to, nwk, lp, guard; };
#define GW_ROW(NAME, KF, KT, NWK, LP, G) {KF, KT, NWK, LP, G},
constexpr GwClass GW_CLASS_TABLE[GWC_COUNT] = {GW_CLASSES(GW_ROW)};
#undef GW_ROW

constexpr int GW_MAX_M = 64, GW_MIN_K = 512, GW_MAX_K = 10240;
// Column tiles per workgroup.  The x rows are read straight from L2 as MFMA fragments, RG * 16 rows per 16 weight rows: with one
// tile a workgroup of 4 row groups reads four times as many x bytes as weight bytes.  With two tiles a wave feeds one x fragment to
// both, and the ratio halves -- taken from 2 row groups on wherever that still leaves 128 workgroups (N >= 4096: the QKV, h -> 4h
// and logits products of the model family; their N = h products keep one tile and N / 16 workgroups).
constexpr int GW_CT2_MIN_N = 4096;
constexpr int gw_rg(int M) { return (M + 15) / 16; }
constexpr int gw_ct(int rg, int N, int ct2_min_n = GW_CT2_MIN_N) { return rg >= 2 && N >= ct2_min_n ? 2 : 1; }
// Load pairs a wave keeps in flight.  A pair is 2 * (RG + CT) loads of 16 bytes per lane = 8 (RG + CT) registers; a wave of a
// 16-wave workgroup has 128 registers, of an 8- or 4-wave one 256 (two workgroups of 4 waves per CU).  What is left after the
// RG * CT accumulators of 4 registers and 40 for addresses and the epilogue goes to the ring, up to all LP pairs (then every load
// of the wave is requested at the top, as in gemv.hip).
constexpr int gw_depth(int nwk, int rg, int ct, int lp) {
  const int d = ((nwk == 16 ? 128 : 256) - 4 * rg * ct - 40) / (8 * (rg + ct));
  return d < 1 ? 1 : d > lp ? lp : d;
}
// Accumulator tiles summed per round of the tail: every wave writes that many partial tiles (1 KB each) to LDS, the first R waves
// sum one tile each in wave order and finish it.  R <= NWK, at most 32 KB of partials; even wherever CT = 2 (a finishing wave
// keeps one column tile through all rounds).
constexpr int gw_round(int nwk, int tiles) {
  const int cap = nwk < 32 / nwk ? nwk : 32 / nwk;
  return tiles < cap ? tiles : cap;
}
constexpr int gw_lds(int nwk, int tiles) { return gw_round(nwk, tiles) * (nwk + 1) * 1024; }

// The plan of one launch: cls and (rg, ct) name the instantiation.  gw_plan(), below the quantized classes, makes it.
struct GwPlan { int rg, nwk, ct, lp, guard, depth, threads, grid, lds, cls; };

// ---------------------------------------------------------------------------------------------------------------------
// The same kernel on the quantized weight operands of gemv_operand.cuh (cogv_gemm_rows_w8: E4M3 bytes and a row scale,
// cogv_gemm_rows_w4: MXFP4 blocks).  A 16-byte load of a lane holds 16 (W8) or 32 (W4) contraction elements of its weight row, so a
// wave's UNIT -- what the 16-bit kernel calls a load pair -- is 128 contraction elements for both formats: two loads of 2 fragments
// (W8), one load of 4 fragments and its scale byte (W4).  Per unit and lane: 16 x registers per row group (4 fragments of 16 bytes),
// 8 (W8) or 5 (W4) weight registers per column tile.  Half or a quarter of the bytes per contraction element take half the waves
// per tile to keep the same weight bytes in flight per workgroup column; every class has at most 8 waves, so a wave has 256
// registers and no class spills (the table per instantiation class).
//   X(name, K from, K to, NWK, LP units per wave, guarded)     -- the class depends on K ALONE, as above
#define GWQ_CLASSES(X)                     \
  X(K1024,  1024,  1024,  4,  2,  false)   \
  X(K2560,  2560,  2560,  4,  5,  false)   \
  X(K4096,  4096,  4096,  8,  4,  false)   \
  X(K10240, 10240, 10240, 8,  10, false)   \
  X(G2,     512,   1024,  4,  2,  true)    \
  X(G5,     512,   2560,  4,  5,  true)    \
  X(G10,    512,   10240, 8,  10, true)

#define GWQ_ENUM_ROW(NAME, ...) GWQC_##NAME,
enum GwqClassId { GWQ_CLASSES(GWQ_ENUM_ROW) GWQC_COUNT };
#undef GWQ_ENUM_ROW
#define GW_ROW(NAME, KF, KT, NWK, LP, G) {KF, KT, NWK, LP, G},
constexpr GwClass GWQ_CLASS_TABLE[GWQC_COUNT] = {GWQ_CLASSES(GW_ROW)};
#undef GW_ROW

// Two column tiles from 2 row groups on where N reaches this bound: the 16-bit rule (GW_CT2_MIN_N) unless an A/B build says
// otherwise (tools/mb_gemm_rows_q.py; DESIGN 4.5.8 has the measurement that keeps it).
#ifndef GWQ_CT2_MIN_N
#define GWQ_CT2_MIN_N GW_CT2_MIN_N
#endif
constexpr int GWQ_UNIT = 128;                                         // contraction elements of a unit
// x bytes a workgroup requests from L2 per weight byte: 4 fragments of 16 bytes per row group against 2 (W8) or 1 (W4) loads of 16
// bytes per column tile = 2 RG / CT and 4 RG / CT, twice and four times the 16-bit kernel's RG / CT.  The column tiles follow the
// 16-bit rule (gw_ct: two from 2 row groups on where N >= 4096); four tiles or x staged in LDS were not built -- DESIGN 4.5.8 has
// the ratio per plan and what was and was not measured.
// Units a wave keeps in flight, from its 256 registers: the accumulators, 40 for addresses and the epilogue, 8 for the row scales
// of a finishing lane (W8), and 16 for a unit's conversion (8 floats and the packed fragment of one column tile at a time).
constexpr int gwq_depth(int fmt, int rg, int ct, int lp) {
  const int unit = 16 * rg + (fmt == GV_W4 ? 5 : 8) * ct;
  const int d = (256 - 4 * rg * ct - 40 - (fmt == GV_W8 ? 8 : 0) - 16) / unit;
  return d < 1 ? 1 : d > lp ? lp : d;
}
constexpr int gwq_depth_w8(int, int rg, int ct, int lp) { return gwq_depth(GV_W8, rg, ct, lp); }
constexpr int gwq_depth_w4(int, int rg, int ct, int lp) { return gwq_depth(GV_W4, rg, ct, lp); }

// ---------------------------------------------------------------------------------------------------------------------
// What a weight format (GV_W16 | GV_W8 | GV_W4, weight_operand.h) means for the plan: its class list, the N from which 2 row groups
// on take two column tiles, the pairs or units in flight, and the 16-byte weight loads of a lane per pair or unit and column tile.
struct GwFormat { const GwClass* classes; int count, ct2_min_n; int (*depth)(int nwk, int rg, int ct, int lp); int loads; };
constexpr GwFormat GW_FORMATS[3] = {
    {GW_CLASS_TABLE, GWC_COUNT, GW_CT2_MIN_N, gw_depth, 2},
    {GWQ_CLASS_TABLE, GWQC_COUNT, GWQ_CT2_MIN_N, gwq_depth_w8, 2},
    {GWQ_CLASS_TABLE, GWQC_COUNT, GWQ_CT2_MIN_N, gwq_depth_w4, 1},
};

// the plan of a product on weights of format fmt; cls indexes the format's class list.  false: the wide kernel does not take the
// product (unsupported)
inline bool gw_plan(int fmt, int M, int N, int K, GwPlan& pl) {
  if (M < 1 || M > GW_MAX_M || N < 8 || (N & 7) || K < GW_MIN_K || K > GW_MAX_K || (K & 511)) return false;
  const GwFormat& f = GW_FORMATS[fmt];
  for (int i = 0; i < f.count; ++i) {
    const GwClass& c = f.classes[i];
    if (K < c.k_from || K > c.k_to) continue;
    const int rg = gw_rg(M), ct = gw_ct(rg, N, f.ct2_min_n), cols = 16 * ct;
    pl = GwPlan{rg, c.nwk, ct, c.lp, c.guard, f.depth(c.nwk, rg, ct, c.lp), 64 * c.nwk, (N + cols - 1) / cols, gw_lds(c.nwk, rg * ct), i};
    return true;
  }
  return false;
}

// Skinny-M (M <= 8) products of the decode step: the ONE class list and the ONE launch plan of csrc/gemv.hip's kernels.
// Host code only.  gemm.hip asks gv_plan() before every launch of the three kinds (plain, attention-combine prologue, LayerNorm
// prologue) on either weight format, cogv_gemv_plan answers from the same function, and a unit of gemv.hip turns the plan's class
// into its template instantiation by expanding the same list (gv2_run there).
#pragma once
#include <cstdlib>

#include "weight_operand.h"                                      // the weight formats GV_W16 | GV_W8 | GV_W4

enum { GV_PLAIN = 1, GV_ATTN = 2, GV_LN = 4, GV_ALL = 7 };       // kind (bits: a class row names the kinds that take it)
enum { GV_FORM_V = 0, GV_FORM_M = 1 };                           // FormV: one row, vector ALU | FormM: 2 .. 8 rows, MFMA (either weight operand)

// The classes.  A product of MT rows (1 | 2, 4, 8: the row count rounded up) takes the FIRST row of its format whose form
// matches (V: MT = 1, M: MT > 1) and whose K range holds K; a kind in STOP ends the search there (first generation / unsupported),
// a kind not in KINDS reads on.
//   X(name, form, K from, K to, J | NWK, KCMAX | LMAX, guarded, KINDS, STOP, K2MTS, LNTW2, LNTW48)
//   J columns per wave (V: 4 waves) | NWK waves per 16-column tile (M);  KCMAX 512-chunks of K | LMAX loads per lane;  guarded: K
//   below the class's maximum;  K2MTS: the MTs at which the plain kind stages the x rows in two halves (gemv2_k2_kernel);
//   LNTW2 / LNTW48: 16-column tiles per workgroup of the LayerNorm kind at MT = 2 / at 4 and 8 (its prologue wants 4 or 8 waves);
//   the other kinds have one tile.
// Exact classes for the widths of the model family (h = 1024: K = 1024 / 4096; h = 2560: K = 2560 / 10240), guarded ones for any
// other multiple of 512.  The 8-bit rows keep the 16-bit rows' 16-20 KB in flight per wave with half the bytes per slot: twice the
// columns per wave (V), half the waves per tile (M).  The plain and the attention kind of a format share every M row they both
// take and differ in J only on V rows (a V column's arithmetic does not depend on the class; an M class's depends on NWK
// alone): the combine-prologue form and the two-launch form of the projection agree bit for bit.
#define GV_CLASSES_16(X)                                                                   \
  X(H_V1024,  V, 1024,  1024,  8,  2,  false, GV_ALL,              0,       0,     1, 1)   \
  X(H_V2560,  V, 2560,  2560,  4,  5,  false, GV_ALL,              0,       0,     1, 1)   \
  X(H_V4096,  V, 4096,  4096,  2,  8,  false, GV_PLAIN,            0,       0,     1, 1)   \
  X(H_V10240, V, 10240, 10240, 2,  20, false, GV_PLAIN,            0,       0,     1, 1)   \
  X(H_VG8,    V, 512,   4096,  2,  8,  true,  GV_LN,               0,       0,     1, 1)   \
  X(H_VG20,   V, 512,   10240, 2,  20, true,  GV_PLAIN | GV_ATTN,  0,       0,     1, 1)   \
  X(H_M1024,  M, 1024,  1024,  4,  8,  false, GV_ALL,              0,       0,     1, 2)   \
  X(H_M2560,  M, 2560,  2560,  4,  20, false, GV_ALL,              0,       0,     1, 2)   \
  X(H_M4096,  M, 4096,  4096,  8,  16, false, GV_PLAIN,            GV_ATTN, 0,     1, 1)   \
  X(H_M10240, M, 10240, 10240, 16, 20, false, GV_PLAIN,            GV_ATTN, 4 | 8, 1, 1)   \
  X(H_MG4,    M, 512,   2560,  4,  20, true,  GV_ALL,              0,       0,     1, 2)   \
  X(H_MG8,    M, 512,   5120,  8,  20, true,  GV_ALL,              0,       0,     1, 1)
#define GV_CLASSES_8(X)                                                                    \
  X(B_V1024,  V, 1024,  1024,  16, 2,  false, GV_ALL,              0,       0,     1, 1)   \
  X(B_V2560,  V, 2560,  2560,  8,  5,  false, GV_ALL,              0,       0,     1, 1)   \
  X(B_V4096,  V, 4096,  4096,  4,  8,  false, GV_PLAIN,            0,       0,     1, 1)   \
  X(B_V10240, V, 10240, 10240, 4,  20, false, GV_PLAIN,            0,       0,     1, 1)   \
  X(B_VG8,    V, 512,   4096,  4,  8,  true,  GV_LN,               0,       0,     1, 1)   \
  X(B_VG20,   V, 512,   10240, 4,  20, true,  GV_PLAIN | GV_ATTN,  0,       0,     1, 1)   \
  X(B_M1024,  M, 1024,  1024,  2,  8,  false, GV_ALL,              0,       0,     2, 4)   \
  X(B_M2560,  M, 2560,  2560,  2,  20, false, GV_ALL,              0,       0,     2, 4)   \
  X(B_M4096,  M, 4096,  4096,  4,  16, false, GV_PLAIN,            0,       8,     1, 1)   \
  X(B_M10240, M, 10240, 10240, 8,  20, false, GV_PLAIN,            0,       4 | 8, 1, 1)   \
  X(B_MG2,    M, 512,   2560,  2,  20, true,  GV_ALL,              0,       0,     2, 4)   \
  X(B_MG4,    M, 512,   5120,  4,  20, true,  GV_ALL,              0,       0,     2, 2)
// The 4-bit rows (MXFP4: a lane's 16-byte load is one block of 32 contraction elements, gemv.hip W4).  V: KCMAX still counts the
// 512-chunks of K (the x side's unit); a wave's slot covers 2048 elements of a column, so a column takes ceil(K / 2048) slots of
// 16 + 1 bytes per lane and J is sized for 16-20 slots: 16-20 KB requested per wave (at K = 1024 and 2560 the lanes past the
// column's end re-read its last block, so 8 and 10 KB of them are distinct -- twice the columns would need 160 registers of
// slots; above K = 1024 the LayerNorm kind takes half the columns, 8 slots: its prologue lives next to them in the 168 registers
// of three waves per SIMD).  M: a load is four fragments (KL = 128).  A tile of K = 2560 is 20 KB in all: one wave would hold it, but the
// LayerNorm kind's prologue wants 4 or 8 waves, i.e. 8 one-wave tiles per workgroup at 4 and 8 rows -- 60 workgroups for the 4B
// model's QKV product.  Measured in the captured 4B step: 2.38 / 3.08 / 4.36 ms at 2 / 4 / 8 rows with one wave per
// tile against 2.33 / 2.65 / 4.12 with two (10 KB per wave, W8's workgroup shapes), so the rows up to K = 5120 take two waves per
// tile and 2 or 4 tiles per LayerNorm workgroup; K = 10240 keeps 20 KB per wave on four.
#define GV_CLASSES_4(X)                                                                    \
  X(Q_V1024,  V, 1024,  1024,  16, 2,  false, GV_ALL,              0,       0,     1, 1)   \
  X(Q_V2560,  V, 2560,  2560,  8,  5,  false, GV_PLAIN | GV_ATTN,  0,       0,     1, 1)   \
  X(Q_VL2560, V, 2560,  2560,  4,  5,  false, GV_LN,               0,       0,     1, 1)   \
  X(Q_V4096,  V, 4096,  4096,  8,  8,  false, GV_PLAIN,            0,       0,     1, 1)   \
  X(Q_V10240, V, 10240, 10240, 4,  20, false, GV_PLAIN,            0,       0,     1, 1)   \
  X(Q_VG8,    V, 512,   4096,  2,  8,  true,  GV_LN,               0,       0,     1, 1)   \
  X(Q_VG20,   V, 512,   10240, 4,  20, true,  GV_PLAIN | GV_ATTN,  0,       0,     1, 1)   \
  X(Q_M1024,  M, 1024,  1024,  2,  4,  false, GV_ALL,              0,       0,     2, 4)   \
  X(Q_M2560,  M, 2560,  2560,  2,  10, false, GV_ALL,              0,       0,     2, 4)   \
  X(Q_M4096,  M, 4096,  4096,  2,  16, false, GV_PLAIN,            0,       8,     1, 1)   \
  X(Q_M10240, M, 10240, 10240, 4,  20, false, GV_PLAIN,            0,       4 | 8, 1, 1)   \
  X(Q_MG2,    M, 512,   5120,  2,  20, true,  GV_ALL,              0,       0,     2, 4)

#define GV_ENUM_ROW(NAME, ...) GVC_##NAME,
enum GvClassId { GV_CLASSES_16(GV_ENUM_ROW) GV_CLASSES_8(GV_ENUM_ROW) GV_CLASSES_4(GV_ENUM_ROW) GVC_COUNT };
#undef GV_ENUM_ROW

struct GvClass { int fmt, form, k_from, k_to, p0, p1, guard, kinds, stop, k2mts, lntw2, lntw48; };
#define GV_ROW_16(NAME, FORM, KF, KT, P0, P1, G, KINDS, STOP, K2MTS, TW2, TW48) {GV_W16, GV_FORM_##FORM, KF, KT, P0, P1, G, KINDS, STOP, K2MTS, TW2, TW48},
#define GV_ROW_8(NAME, FORM, KF, KT, P0, P1, G, KINDS, STOP, K2MTS, TW2, TW48) {GV_W8, GV_FORM_##FORM, KF, KT, P0, P1, G, KINDS, STOP, K2MTS, TW2, TW48},
#define GV_ROW_4(NAME, FORM, KF, KT, P0, P1, G, KINDS, STOP, K2MTS, TW2, TW48) {GV_W4, GV_FORM_##FORM, KF, KT, P0, P1, G, KINDS, STOP, K2MTS, TW2, TW48},
constexpr GvClass GV_CLASS_TABLE[GVC_COUNT] = {GV_CLASSES_16(GV_ROW_16) GV_CLASSES_8(GV_ROW_8) GV_CLASSES_4(GV_ROW_4)};
#undef GV_ROW_16
#undef GV_ROW_8
#undef GV_ROW_4

// What a class means for a launch; gemv.hip asserts these against its forms' own constants (NW, COLS, XPAD).
constexpr int gv_threads(int form, int p0, int tw) { return 64 * (form == GV_FORM_V ? 4 : p0 * tw); }
constexpr int gv_cols(int form, int p0, int tw) { return form == GV_FORM_V ? 4 * p0 : 16 * tw; }
constexpr int gv_xpad(int form) { return form == GV_FORM_V ? 0 : 8; }
// x rows in LDS (dynamic) + the kernels' static arrays stay inside the 64 KB a workgroup gets without an attribute.  Only the
// two-halves kernel goes above (8 rows of K = 10240: 82 KB + 17 KB static), by attribute.
constexpr int GV_MAX_SHMEM = 56 * 1024;
constexpr int GV_LN_MAX_K = 4096, GV_MAX_NSPLIT = 32;

// The plan of one launch.  generation 2: a kernel of gemv.hip (cls and the class fields say which); generation 1: the 16-bit
// fallback in gemm.hip (gemv_kernel, gemv_attn_kernel, gemv_ln_kernel: 8 columns per workgroup), class fields 0.
struct GvPlan { int generation, form, p0, p1, guard, mt, tw, k2, threads, grid, lds, cls; };
// what a unit of gemv.hip needs besides the plan: args = GemmArgs (GV_LN: GemvLnArgs)
struct GvCall { const void* args; const float* partials; int heads, nsplit, stream_f32; void* stream; };

// the first generation's launch: 8 columns per workgroup of 4 waves; the LayerNorm kind keeps its mt rows of x in LDS
inline GvPlan gv_plan_gen1(int kind, int mt, int N, int K) { return GvPlan{1, 0, 0, 0, 0, mt, 0, 0, 256, N / 8, kind == GV_LN ? mt * K * 2 : 0, -1}; }
inline int gv_mt(int M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8; }
// COGV_GEMV2=0 (read once per process) keeps the 16-bit products on the first generation (A/B runs)
inline bool gv_gen2_enabled() {
  static const bool on = [] { const char* e = getenv("COGV_GEMV2"); return !e || atoi(e) != 0; }();
  return on;
}

// false: the skinny-M kernels do not take the product at all (3, unsupported, from the entry points that have nothing else);
// gv_shape_taken is the part of that answer no format or generation changes.
// 16-bit weights always get a plan past the shape checks -- what the classes do not take is the first generation's; the 8-bit
// and the 4-bit format have no other kernel.  ldb: elements (bytes) between the weight's rows; nsplit: key splits the attention
// kind combines.
inline bool gv_shape_taken(int kind, int M, int N, int K) {
  return M >= 1 && M <= 8 && K >= 512 && (K & 511) == 0 && N >= 8 && (N & 7) == 0 && !(kind == GV_LN && K > GV_LN_MAX_K);
}
inline bool gv_plan(int kind, int fmt, int M, int N, int K, int ldb, int nsplit, GvPlan& pl) {
  if (!gv_shape_taken(kind, M, N, K)) return false;
  const int mt = gv_mt(M);
  const bool gen2 = fmt == GV_W16 ? gv_gen2_enabled() : ldb >= weight_row(fmt, K);
  if (gen2 && !(kind == GV_ATTN && nsplit > GV_MAX_NSPLIT))
    for (int i = 0; i < GVC_COUNT; ++i) {
      const GvClass& c = GV_CLASS_TABLE[i];
      if (c.fmt != fmt || c.form != (mt == 1 ? GV_FORM_V : GV_FORM_M) || K < c.k_from || K > c.k_to) continue;
      if (c.stop & kind) break;
      if (!(c.kinds & kind)) continue;
      const int tw = kind == GV_LN ? (mt == 2 ? c.lntw2 : c.lntw48) : 1, k2 = kind == GV_PLAIN && (c.k2mts & mt);
      const int lds = mt * ((k2 ? K / 2 : K) + gv_xpad(c.form)) * 2;
      if (!k2 && lds > GV_MAX_SHMEM) break;
      const int cols = gv_cols(c.form, c.p0, tw);
      pl = GvPlan{2, c.form, c.p0, c.p1, c.guard, mt, tw, k2, gv_threads(c.form, c.p0, tw), (N + cols - 1) / cols, lds, i};
      return true;
    }
  if (fmt != GV_W16) return false;
  pl = gv_plan_gen1(kind, mt, N, K);
  return true;
}

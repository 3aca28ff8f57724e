// The weight operand of the decode step's products (gemv.hip, gemv_wide.hip) as the host sees it: ONE format enum, ONE struct the
// entry points of gemm.hip and gemv_wide.hip turn their ABI operand into, and what differs between the formats as one row of data
// each.  Host code only.  A further format is a row here, a class list in gemv_plan.h / gemv_wide_plan.h and a unit in build.py.
#pragma once
#include <cstdint>

#include "cogview_hip.h"
#include "gemm_shared.cuh"

enum { GV_W16 = 0, GV_W8 = 1, GV_W4 = 2 };      // weight format: the dtype's 16 bits | E4M3 bytes + row scales | MXFP4 blocks

namespace {      // (GemmArgs has internal linkage: gemm_shared.cuh)

// q: [N][ldq] -- elements of the dtype (W16: d->B / d->ldb) or bytes; scale: [N] fp32 row scales (W8) | [N][lds] E8M0 block scales (W4)
struct WeightOperand { int fmt; const void* q; int ldq; const void* scale; int lds; };

//   k_per_ld: contraction elements per unit of ldq, so a row of K takes K / k_per_ld of them;  scale_align16: the scales are read
//   in 16-byte loads;  block_scales: scale has rows of its own, lds >= K / 32 bytes apart
struct WeightFormat { int k_per_ld; bool scale_align16, block_scales; };
constexpr WeightFormat WEIGHT_FORMATS[3] = {
    {1, false, false},      // GV_W16
    {1, true, false},       // GV_W8
    {2, false, true},       // GV_W4
};
constexpr int weight_row(int fmt, int K) { return K / WEIGHT_FORMATS[fmt].k_per_ld; }

// the ABI's operands (cogview_hip.h); NULL in, NULL out -- which the fronts read as "16-bit weights in d->B"
inline const WeightOperand* weight_operand(const cogv_w8_weight* w, WeightOperand& o) {
  if (!w) return nullptr;
  o = WeightOperand{GV_W8, w->q, w->ldq, w->scale, 0};
  return &o;
}
inline const WeightOperand* weight_operand(const cogv_w4_weight* w, WeightOperand& o) {
  if (!w) return nullptr;
  o = WeightOperand{GV_W4, w->q, w->ldq, w->scale, w->lds};
  return &o;
}
inline int weight_format(const WeightOperand* w) { return w ? w->fmt : GV_W16; }

// The two things an entry point calls a bad argument (1) in a quantized operand.  They are two functions because the skinny front
// (gemm.hip, gemv_front) asks the descriptor's shape between them and the wide front (gemv_wide.hip, gw_front) does not.
inline bool weight_operand_null(const WeightOperand& w) { return !w.q || !w.scale; }
inline bool weight_operand_misplaced(const WeightOperand& w, int K) {
  const WeightFormat& f = WEIGHT_FORMATS[w.fmt];
  return (w.ldq & 15) || ((uintptr_t)w.q & 15) || (f.scale_align16 && ((uintptr_t)w.scale & 15)) || (f.block_scales && w.lds < K / 32);
}

// the operand in the argument block: B / ldb, and the scales where the kernels of its format look for them
inline void weight_operand_put(const WeightOperand& w, GemmArgs& a) {
  a.B = w.q; a.ldb = w.ldq;
  if (w.fmt == GV_W8) a.wscale = reinterpret_cast<const float*>(w.scale);
  if (w.fmt == GV_W4) { a.bscale = reinterpret_cast<const uint8_t*>(w.scale); a.ldbs = w.lds; }
}

}  // namespace

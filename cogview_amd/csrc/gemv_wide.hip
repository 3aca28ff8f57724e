// Wide products of the decode step: 1 .. 64 rows on the 16-bit weights (cogv_gemm_rows) and on the quantized weight operands of
// gemv_operand.cuh (cogv_gemm_rows_w8: E4M3 bytes and a row scale; cogv_gemm_rows_w4: MXFP4 blocks) -- see THE WEIGHT OPERAND below.
//
//   C[M,N] = epilogue( A[M,K] * B[N,K]^T ),   1 <= M <= 64, trans_a = trans_b = 0, flags BIAS | GELU | ABSMAX
//
// A decode step is a weight stream whatever its row count: every launch reads B once, 13-52 MB at the widths of the 4B model,
// and the rows that share the stream are nearly free.  gemv.hip's FormM stops at 8 rows because its x rows live in LDS and its one
// accumulator tile has 16 result columns of which 8 are looked at; above it cogv_gemm falls to the tile kernels, which give a
// workgroup 128 columns: 20 workgroups for an N = 2560 product on a 256-CU part.  This kernel is FormM carried on:
// v_mfma_f32_16x16x32 with the WEIGHTS as the A operand straight from their 16-byte loads (lane l: column n0 + l % 16, contraction
// slots 8 (l / 16) ..), a workgroup owns whole columns, its NWK waves split the contraction in load pairs (one 128-byte line of
// each of the 16 weight rows) round robin, and the waves' partial tiles are summed through LDS in wave order.  What is new:
//
//   ROW GROUPS.  RG = ceil(M / 16) accumulators of 4 registers per column tile; one weight fragment feeds RG MFMAs.  Rows past M
//   are don't-care columns of the result: their x address is clamped to row M - 1 (nothing is read past A) and they are never
//   stored.
//
//   THE x OPERAND COMES FROM L2, not from LDS.  64 rows are 320 KB at K = 2560 and 1.3 MB at K = 10240.  A wave needs of x exactly
//   the contraction slots of its own load pairs, as fragments of the same shape as the weights' (lane l: row 16 rg + l % 16, slots
//   8 (l / 16) ..), so the waves of a workgroup read every x byte once between them whether or not LDS stands in between: staging
//   would add a copy and barriers and remove no L2 traffic.  What lowers the traffic is columns per workgroup: a wave that owns
//   the same load pairs of CT = 2 column tiles feeds one x fragment to both (gemv_wide_plan.h: from 2 row groups on, where the
//   grid stays large).
//
//   A RING OF LOAD PAIRS instead of every load at the top: 64 rows times 20 loads do not fit in a wave's registers.  A wave
//   requests DP pairs ahead (x fragments first, then the weights: the memory counter retires in order, and the L2-resident rows
//   must not wait behind an HBM miss they do not depend on), multiplies pair i when it lands and requests pair i + DP into its
//   registers.  DP = LP (all at the top, as in gemv.hip) wherever the registers allow: gemv_wide_plan.h, gw_depth.
//
// Every byte of B is requested by exactly one workgroup, once (a ragged last tile re-reads row N - 1 for its columns past N; a
// guarded class re-reads its last pair instead of branching around a load).  No floating-point atomics; the only atomic is the
// non-negative abs-max.  The association of a column's sum is fixed by K alone (the class), so the same call gives the same bits
// and a row's bits do not depend on the other rows of the call.  The epilogue is gemm_shared.cuh's epilogue8: every rounding point
// is the skinny case's.
//
//   THE WEIGHT OPERAND is a type parameter, as in gemv.hip's FormM (W16 | W8 | W4, gemv_operand.cuh).  A lane's 16-byte weight load
//   covers KL = 32 / 64 / 128 contraction elements of its weight row = FR = 1 / 2 / 4 MFMA fragments: lane l supplies elements
//   (KL / 4) (l >> 4) + 8 f .. + 7 of the load's block to fragment f, and the x fragments -- still 16-byte loads of the 16-bit x
//   from L2, one per fragment and row group -- take the same elements of their rows.  W8: the bytes convert to T exactly, and the
//   fp32 row scale (requested behind the first weights, clamped column) multiplies the finished column sum once, in front of
//   epilogue8.  W4: the E8M0 byte of a load is requested right behind it and folded into the conversion (v_cvt_scalef32_pk_*_fp4).
//   Columns past N re-read row N - 1, codes and scales alike.  The matrix core multiplies T by T: x is never quantized (the
//   block-scaled MFMA would do that, and is a different feature).  The quantized classes and their plan: gemv_wide_plan.h,
//   GWQ_CLASSES.  The 16-bit instantiations kept their instruction text (profiles/r22_gemv_wide_operand_parent_vs_head.log).
//
// Compiled as one unit per dtype and operand (-DCOGV_GEMV_WIDE_TU=0: bf16, 1: fp16; with -DCOGV_GEMV_WIDE_W8 / -DCOGV_GEMV_WIDE_W4
// the quantized operands; build.py) with the kernels; without the macro this file holds the entry points and nothing that runs on
// the device.
#include "gemv_operand.cuh"
#include "gemv_wide_plan.h"

#include <type_traits>

#ifdef COGV_GEMV_WIDE_TU

namespace {

// a zero the compiler cannot see through, in a vector register (gemv.hip, gv2_vzero: keeps a wave-uniform address on the vector
// memory path, so that the first weight load does not wait for the scalar counter)
__device__ __forceinline__ int gw_vzero() {
  int zero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
  return zero;
}

// W: what B holds (gemv_operand.cuh).  A wave's UNIT of the contraction is LU loads of W::KL elements: the load pair of the
// 16-bit operand (2 x 32), two loads of the 8-bit one (2 x 64), one block load of the 4-bit one (1 x 128); LP, DP count units.
template <typename W, int RG, int CT, int NWK, int LP, int DP, bool GUARD>
__global__ __launch_bounds__(NWK * 64) void gemv_wide_kernel(const GemmArgs p) {
  typedef typename W::T T;
  typedef typename W::Elem Elem;
  typedef typename HT<T>::v8 v8;
  constexpr int KL = W::KL, FR = W::FR, PK = W::PK, LU = PK == 2 ? 1 : 2, UE = LU * KL;
  constexpr int TILES = RG * CT, R = gw_round(NWK, TILES), ROUNDS = (TILES + R - 1) / R;
  static_assert(DP >= 1 && DP <= LP && (CT == 1 || R % CT == 0), "gemv_wide_plan.h");
  extern __shared__ __attribute__((aligned(16))) char gw_smem[];      // red [R][NWK][64] f32x4 | outp [R][16][16] float
  f32x4 (*red)[NWK][64] = reinterpret_cast<f32x4 (*)[NWK][64]>(gw_smem);
  float (*outp)[16][16] = reinterpret_cast<float (*)[16][16]>(gw_smem + R * NWK * 1024);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = GUARD ? p.K : LP * NWK * UE, npairs = K >> (UE == 64 ? 6 : 7);
  const int n0 = blockIdx.x * (16 * CT);
  // the bias of the 8 columns this lane finishes (lanes 0 .. 31 of the first R waves: wave w keeps column tile w % CT through all
  // rounds), requested ahead of everything; unconditional, with a stand-in address where there is none (gemv.hip, gv2_bias)
  const int nfin = n0 + (wave % CT) * 16 + (lane & 1) * 8;
  const T* bsrc = (p.flags & COGV_EPI_BIAS) ? reinterpret_cast<const T*>(p.bias) : reinterpret_cast<const T*>(p.B);
  const u32x4 bias_pre = gload16(bsrc + (nfin < p.N ? nfin : p.N - 8) + gw_vzero());
  // A operand = weights: lane l supplies column (tile) + (l & 15); B operand = x: lane l supplies row 16 rg + (l & 15); both the
  // contraction slots 8 (l >> 4) .. + 7 of a 32-deep step -- of fragment f of a load, elements (KL / 4) (l >> 4) + 8 f .. + 7 of its
  // KL-element block (FormM's mapping: the 16 bytes of a lane are consecutive elements of its weight row)
  const Elem* wrow[CT];
  const uint8_t* srow[CT];      // W4: the row's block scales, from this lane's block of a load on
  const T* xrow[RG];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int nt = n0 + ct * 16 + (lane & 15);
    wrow[ct] = reinterpret_cast<const Elem*>(p.B) + (size_t)(nt < p.N ? nt : p.N - 1) * p.ldb + (lane >> 4) * (KL / 4 / PK);
    if constexpr (PK == 2) srow[ct] = p.bscale + (size_t)(nt < p.N ? nt : p.N - 1) * p.ldbs + (lane >> 4);
  }
#pragma unroll
  for (int rg = 0; rg < RG; ++rg) {
    const int m = rg * 16 + (lane & 15);
    xrow[rg] = reinterpret_cast<const T*>(p.A) + (size_t)(m < p.M ? m : p.M - 1) * p.lda + (lane >> 4) * (KL / 4);
  }
  u32x4 xr[DP][LU][RG][FR], wr[DP][LU][CT];
  uint32_t ws[DP][LU][PK == 2 ? CT : 1];      // W4: the E8M0 byte of each load, requested right behind it
  // pair i of this wave into ring slot i % DP
  auto issue = [&](int i) {
    int q = wave + NWK * i;
    if (GUARD) q = q < npairs ? q : npairs - 1;
#pragma unroll
    for (int s = 0; s < LU; ++s) {
#pragma unroll
      for (int rg = 0; rg < RG; ++rg)
#pragma unroll
        for (int f = 0; f < FR; ++f) xr[i % DP][s][rg][f] = gload16(xrow[rg] + UE * q + KL * s + 8 * f);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        wr[i % DP][s][ct] = gload16(wrow[ct] + (UE / PK) * q + (KL / PK) * s);
        if constexpr (PK == 2) ws[i % DP][s][ct] = *(const COGV_GLOBAL uint8_t*)(srow[ct] + 4 * (LU * q + s));
      }
    }
  };
#pragma unroll
  for (int i = 0; i < DP; ++i) issue(i);
  // W8: the row scales of the 8 columns this lane finishes, behind the first weights and far ahead of the tail (clamped column)
  const typename W::Scale sc = W::scale(p, n0 + (wave % CT) * 16, lane & 1);
  f32x4 acc[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // (the scheduling barriers keep the requests where they are written: left alone, the compiler moves every load down to its
  // MFMAs to save registers, and a wave has one pair in flight)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < LP; ++i) {
    if (!GUARD || wave + NWK * i < npairs) {
#pragma unroll
      for (int s = 0; s < LU; ++s)
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          v8 a[CT];
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            if constexpr (PK == 2) a[ct] = W::frag(wr[i % DP][s][ct], ws[i % DP][s][ct], f);
            else a[ct] = W::frag(wr[i % DP][s][ct], f);
          }
#pragma unroll
          for (int rg = 0; rg < RG; ++rg)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
              acc[rg * CT + ct] = HT<T>::mfma16(a[ct], __builtin_bit_cast(v8, xr[i % DP][s][rg][f]), acc[rg * CT + ct]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (i + DP < LP) {
      issue(i + DP);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // D: lane l holds C[16 rg + (l & 15)][(tile) + 4 (l >> 4) + i], i = 0 .. 3.  The tail, R tiles per round: every wave leaves its
  // partial of the round's tiles in LDS; wave w < R sums tile r R + w over the waves in wave order, regroups it into 8 consecutive
  // columns per (row, half), and its lanes 0 .. 31 run the fused epilogue on one (row, half) each.
  uint32_t am = 0u;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int rn = TILES - r * R < R ? TILES - r * R : R;
#pragma unroll
    for (int tl = 0; tl < R; ++tl)
      if (tl < rn) red[tl][wave][lane] = acc[r * R + tl];
    __syncthreads();
    if (wave < rn) {
      f32x4 s = red[wave][0][lane];
#pragma unroll
      for (int w = 1; w < NWK; ++w) s += red[wave][w][lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) outp[wave][lane & 15][(lane >> 4) * 4 + i] = s[i];
    }
    __syncthreads();
    if (wave < rn && lane < 32) {
      const int t = r * R + wave;
      const int m = (t / CT) * 16 + (lane >> 1), n = n0 + (t % CT) * 16 + (lane & 1) * 8;
      if (m < p.M && n < p.N) {
        const typename W::Factors s8 = W::factors(sc);      // (W8: the row scale, once, in front of the shared epilogue)
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = W::mul(outp[wave][lane >> 1][(lane & 1) * 8 + i], s8, i);
        am = absmax_pk(am, epilogue8<T>(p, m, n, v, &bias_pre));
      }
    }
  }
  if ((p.flags & COGV_EPI_ABSMAX) && wave < R) {
    uint32_t wv = max(am & 0xffffu, am >> 16);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wv = max(wv, (uint32_t)__shfl_xor((int)wv, o, 64));
    if (lane == 0) atomic_max_nonneg(p.absmax, bits_to_f<T>((uint16_t)wv));
  }
}

using TT = std::conditional<COGV_GEMV_WIDE_TU != 0, f16_t, bf16_t>::type;

#define GW_CAT2(a, b) a##b
#define GW_CAT(a, b) GW_CAT2(a, b)

// the unit's operand, class list and entry point (build.py: -DCOGV_GEMV_WIDE_W8 / -DCOGV_GEMV_WIDE_W4 for the quantized units)
#if defined(COGV_GEMV_WIDE_W4)
using WT = W4<TT>;
#define GW_UNIT_CLASSES GWQ_CLASSES
#define GW_CLS(NAME) GWQC_##NAME
#define GW_RUN GW_CAT(cogv_gemv_wide_w4_run_, COGV_GEMV_WIDE_TU)
constexpr int gw_unit_depth(int, int rg, int ct, int lp) { return gwq_depth(GV_W4, rg, ct, lp); }
#elif defined(COGV_GEMV_WIDE_W8)
using WT = W8<TT>;
#define GW_UNIT_CLASSES GWQ_CLASSES
#define GW_CLS(NAME) GWQC_##NAME
#define GW_RUN GW_CAT(cogv_gemv_wide_w8_run_, COGV_GEMV_WIDE_TU)
constexpr int gw_unit_depth(int, int rg, int ct, int lp) { return gwq_depth(GV_W8, rg, ct, lp); }
#else
using WT = W16<TT>;
#define GW_UNIT_CLASSES GW_CLASSES
#define GW_CLS(NAME) GWC_##NAME
#define GW_RUN GW_CAT(cogv_gemv_wide_run_, COGV_GEMV_WIDE_TU)
constexpr int gw_unit_depth(int nwk, int rg, int ct, int lp) { return gw_depth(nwk, rg, ct, lp); }
#endif

template <int NWK, int LP, bool G, int RG, int CT>
int gw_launch(const GwPlan& pl, const GemmArgs& a, void* stream) {
  constexpr int DP = gw_unit_depth(NWK, RG, CT, LP);
  hipLaunchKernelGGL((gemv_wide_kernel<WT, RG, CT, NWK, LP, DP, G>), dim3(pl.grid), dim3(pl.threads), (size_t)pl.lds,
                     reinterpret_cast<hipStream_t>(stream), a);
  return COGV_OK;
}

// (one row group never takes two tiles: gemv_wide_plan.h, gw_ct)
#define GW_RUN_RG(NWK, LP, G, RG) (pl.ct == 2 ? gw_launch<NWK, LP, G, RG, 2>(pl, a, stream) : gw_launch<NWK, LP, G, RG, 1>(pl, a, stream))
#define GW_RUN_ROW(NAME, KF, KT, NWK, LP, G)                                            \
  case GW_CLS(NAME):                                                                    \
    return pl.rg == 1 ? gw_launch<NWK, LP, G, 1, 1>(pl, a, stream)                      \
         : pl.rg == 2 ? GW_RUN_RG(NWK, LP, G, 2) : pl.rg == 3 ? GW_RUN_RG(NWK, LP, G, 3) : GW_RUN_RG(NWK, LP, G, 4);

}  // namespace

// the unit's one entry point: the kernel of plan `plan`; args = GemmArgs
extern "C" __attribute__((visibility("hidden"))) int GW_RUN(const GwPlan* plan, const void* args, void* stream) {
  const GwPlan& pl = *plan;
  const GemmArgs& a = *reinterpret_cast<const GemmArgs*>(args);
  switch (pl.cls) {
    GW_UNIT_CLASSES(GW_RUN_ROW)
    default: return COGV_ERR_UNSUPPORTED;
  }
}

#else  // !COGV_GEMV_WIDE_TU: the entry points

extern "C" __attribute__((visibility("hidden"))) int cogv_gemv_wide_run_0(const GwPlan* plan, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv_wide_run_1(const GwPlan* plan, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv_wide_w8_run_0(const GwPlan* plan, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv_wide_w8_run_1(const GwPlan* plan, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv_wide_w4_run_0(const GwPlan* plan, const void* args, void* stream);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv_wide_w4_run_1(const GwPlan* plan, const void* args, void* stream);

namespace {

// Descriptor -> argument block and launch plan, or the call's error: bad arguments (1) as cogv_gemm reports them, then what this
// kernel does not take (3).  Nothing a pointer points to is read.
// w: the quantized operand that takes the place of d->B / d->ldb, or NULL: 16-bit weights there.
// The whole operand is judged BEFORE the descriptor -- NULL q or scale, alignment, ldq % 16, and with block scales K <= 0 and lds <
// K / 32 are bad arguments (1) whatever the shape says -- and an ldq shorter than a row of K is one too, with lda and ldc.  (The
// skinny front, gemm.hip's gemv_front, asks the shape between the operand's NULLs and its alignment, and leaves a short ldq to
// its plan: 3.)
int gw_front(const cogv_gemm_desc* d, const WeightOperand* w, GemmArgs& a, GwPlan& pl) {
  if (!d) return COGV_ERR_ARG;
  if (w && (weight_operand_null(*w) || (WEIGHT_FORMATS[w->fmt].block_scales && d->K <= 0) || weight_operand_misplaced(*w, d->K))) return COGV_ERR_ARG;
  const WeightOperand b = w ? *w : WeightOperand{GV_W16, d->B, d->ldb, nullptr, 0};
  if (d->dtype != COGV_F16 && d->dtype != COGV_BF16) return COGV_ERR_UNSUPPORTED;
  if (d->M <= 0 || d->N <= 0 || d->K <= 0) return COGV_ERR_ARG;
  if ((d->N & 7) || (d->ldc & 7) || (d->lda & 7) || (b.ldq & 7) || (d->K & 7)) return COGV_ERR_ARG;
  if (((uintptr_t)d->A | (uintptr_t)b.q | (uintptr_t)d->C) & 15) return COGV_ERR_ARG;
  if (!d->A || !b.q || !d->C) return COGV_ERR_ARG;
  if ((d->flags & COGV_EPI_BIAS) && (!d->bias || ((uintptr_t)d->bias & 15))) return COGV_ERR_ARG;
  if ((d->flags & COGV_EPI_ABSMAX) && !d->absmax) return COGV_ERR_ARG;
  if (d->trans_a || d->trans_b || (d->flags & ~(COGV_EPI_BIAS | COGV_EPI_GELU | COGV_EPI_ABSMAX)) || d->out_f32 || d->splitk > 1 ||
      d->kernel_variant != 0 || d->aux)
    return COGV_ERR_UNSUPPORTED;
  if (d->lda < d->K || b.ldq < weight_row(b.fmt, d->K) || d->ldc < d->N) return COGV_ERR_ARG;
  if (!gw_plan(b.fmt, d->M, d->N, d->K, pl)) return COGV_ERR_UNSUPPORTED;
  a = GemmArgs{};
  a.A = d->A; a.C = d->C;
  a.M = d->M; a.N = d->N; a.K = d->K;
  a.lda = d->lda; a.ldc = d->ldc;
  a.bias = d->bias; a.absmax = d->absmax;
  a.flags = d->flags;
  a.keep_scale = 1.0f;
  a.splitk = 1;
  weight_operand_put(b, a);
  return COGV_OK;
}

// the launch of a product, by the operand's format and the dtype
int gw_run(const cogv_gemm_desc* d, const WeightOperand* w, void* stream) {
  static int (*const RUN[3][2])(const GwPlan*, const void*, void*) = {{cogv_gemv_wide_run_0, cogv_gemv_wide_run_1},
                                                                      {cogv_gemv_wide_w8_run_0, cogv_gemv_wide_w8_run_1},
                                                                      {cogv_gemv_wide_w4_run_0, cogv_gemv_wide_w4_run_1}};
  GemmArgs a;
  GwPlan pl;
  const int rc = gw_front(d, w, a, pl);
  if (rc != COGV_OK) return rc;
  const int rr = RUN[weight_format(w)][d->dtype == COGV_F16](&pl, &a, stream);
  return rr != COGV_OK ? rr : cogv_check_launch();
}

// host-only: the plan that launch would use
int gw_query(const cogv_gemm_desc* d, const WeightOperand* w, int* out) {
  if (!out) return COGV_ERR_ARG;
  GemmArgs a;
  GwPlan pl;
  const int rc = gw_front(d, w, a, pl);
  if (rc != COGV_OK) return rc;
  const int loads = GW_FORMATS[weight_format(w)].loads;
  const int v[COGV_GEMM_ROWS_PLAN_INTS] = {pl.rg, pl.nwk, pl.ct, loads * pl.lp * pl.ct, pl.guard, 0, pl.threads, pl.grid, pl.lds, pl.depth};
  for (int i = 0; i < COGV_GEMM_ROWS_PLAN_INTS; ++i) out[i] = v[i];
  return COGV_OK;
}

}  // namespace

// (a _w8 / _w4 call without its operand is a bad argument; to gw_front a NULL operand means 16-bit weights)
extern "C" int cogv_gemm_rows(const cogv_gemm_desc* d, void* stream) { return gw_run(d, nullptr, stream); }
extern "C" int cogv_gemm_rows_w8(const cogv_gemm_desc* d, const cogv_w8_weight* w, void* stream) {
  WeightOperand o; return w ? gw_run(d, weight_operand(w, o), stream) : COGV_ERR_ARG;
}
extern "C" int cogv_gemm_rows_w4(const cogv_gemm_desc* d, const cogv_w4_weight* w, void* stream) {
  WeightOperand o; return w ? gw_run(d, weight_operand(w, o), stream) : COGV_ERR_ARG;
}
extern "C" int cogv_gemm_rows_plan(const cogv_gemm_desc* d, int out[COGV_GEMM_ROWS_PLAN_INTS]) { return gw_query(d, nullptr, out); }
extern "C" int cogv_gemm_rows_w8_plan(const cogv_gemm_desc* d, const cogv_w8_weight* w, int out[COGV_GEMM_ROWS_PLAN_INTS]) {
  WeightOperand o; return w ? gw_query(d, weight_operand(w, o), out) : COGV_ERR_ARG;
}
extern "C" int cogv_gemm_rows_w4_plan(const cogv_gemm_desc* d, const cogv_w4_weight* w, int out[COGV_GEMM_ROWS_PLAN_INTS]) {
  WeightOperand o; return w ? gw_query(d, weight_operand(w, o), out) : COGV_ERR_ARG;
}

#endif  // COGV_GEMV_WIDE_TU

// MFMA GEMM family for the CogView GPT hot path (gfx950).
//
//   C[M,N] = epilogue( A_op[M,K] * B_op[N,K]^T )         fp16/bf16 inputs, fp32 accumulate
//
// Replaces the cuBLAS calls reached through F.linear in the reference:
//   forward  Y = X W^T + b         mpu/layers.py:243 (ColumnParallelLinear), :319 (RowParallelLinear),
//                                  model/gpt2_modeling.py:117 (tied logits)          -> transA=0, transB=0
//   dgrad    dX = dY W             autograd of the above                            -> transA=0, transB=1
//   wgrad    dW = dY^T X           autograd of the above                            -> transA=1, transB=1
//
// "trans" means the operand is stored with the contraction index as the SLOW dimension (A stored [K][M], B stored
// [K][N]): dgrad's W and both weight-gradient operands.  No transposed copies exist in HBM.
//
// This file: the host side (argument checks, launches, split-K reduce, C entry points).  The kernels live in the headers
// included below, one per generation -- gemm_gen4.cuh is the one the train step runs; gemm_gen1 / 2 / 3.cuh are the fallbacks
// for shapes it does not take; gemm_lds.cuh holds the LDS images and fragment reads generations 2-4 share; gemv_gen1.cuh the
// first-generation skinny-M kernels (csrc/gemv.hip has the second).
// Dispatch: cogv_gemm checks the descriptor (build_gemm_args), gives M <= 8 (decode steps: a pure HBM stream of the weights)
// to the skinny-M kernels where gemv_plan.h takes the product, and launches every other product from ONE plan -- gemm_plan.h:
// kernel_variant and shape -> generation, tiles, grid, threads, dynamic LDS, reduce blocks, or the refusal; cogv_gemm_grouped
// plans its problems with the same functions and cogv_gemm_plan reports them (tests/test_gemm_plan.py).  launch_tiles turns a
// plan into one launch by (generation, dtype, layout) and one reduce pass per problem that splits K.
// The four tile kernels, newest first (kernel_variant 10, 9, 3, 1):
//   generation 4  gemm_w4_kernel     256x256x64 tiles, 4 waves of 128x128 (accumulators fill the AGPR file), software-
//                                    pipelined quarter-steps, LDS-DMA granule ring, persistent with per-XCD work queues,
//                                    up to 16 problems per launch.  Auto for M, N >= 256, K % 64 == 0, operands < 4 GiB,
//                                    unless generation 2 fills its rounds 1.1x better.  Its 2 x 4 instantiations compile as
//                                    separate translation units (-DCOGV_W4_TU=k, build.py).
//   generation 3  gemm_pp64_kernel   the same tile, ring and queues with 8 waves of 128x64 in a ping-pong schedule
//                                    (on request only; 5-15 % slower than generation 4: 1.5x the LDS fragment bytes).
//   generation 2  gemm_glds_kernel   256x128x32 tiles, 4 waves of 128x64, 3-stage LDS-DMA ring, 2 workgroups per CU.
//                                    For M or N in [64, 256) and operands >= 4 GiB.
//   generation 1  gemm_kernel        128x128x64 tiles, register-staged with register transposes.  For K % 64 != 0, M or
//                                    N < 64.
// All share the fused epilogue (epilogue8): bias, GeLU (+ stored pre-activation), dGeLU, dropout, += C, abs-max for
// Sandwich-LN, and (generations 3, 4) the bias-gradient column sums of the output.
#include "common.cuh"
#include "cogview_hip.h"
#include "gemm_shared.cuh"

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#ifndef COGV_EXP
#define COGV_EXP 0     // schedule experiments of tools/probes/{gemm_exp,w4_dev}.py (bit 0: no DMA, 1: no reads, 2: no MFMA, 3: DMA re-reads k-tiles 0..3, 4: clock probe, 6: no epilogue math/stores, 11: no epilogue at all, 12: no barriers, 13: no DMA waits)
#endif

#include "gemm_common.cuh"
#include "gemm_gen1.cuh"
#include "gemm_lds.cuh"
#include "gemm_gen2.cuh"
#include "gemm_gen3.cuh"
#include "gemm_gen4.cuh"
#include "gemv_gen1.cuh"
#include "gemv_plan.h"
#include "gemm_plan.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmArgs p) {
  __shared__ float red[16];
  const size_t nvec = (size_t)p.M * (p.N / 8);
  uint32_t amax_pk = 0u;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / (p.N / 8));
    const int n = (int)(i % (p.N / 8)) * 8;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < p.splitk; ++s) {
      const float* w = p.ws + ((size_t)s * p.M + m) * p.N + n;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(w);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(w + 4);
      v[0] += x0[0]; v[1] += x0[1]; v[2] += x0[2]; v[3] += x0[3];
      v[4] += x1[0]; v[5] += x1[1]; v[6] += x1[2]; v[7] += x1[3];
    }
    amax_pk = absmax_pk(amax_pk, epilogue8<T>(p, m, n, v));
  }
  if (p.flags & COGV_EPI_ABSMAX) {
    const float bm = absmax_pk_block<T>(amax_pk, reinterpret_cast<uint32_t*>(red));
    if (threadIdx.x == 0) atomic_max_nonneg(p.absmax, bm);
  }
}

int num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0; hipDeviceProp_t prop;
    (void)hipGetDevice(&dev);
    n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  return n;
}

// Work-queue counters of the persistent kernel: 64 zero-initialised slots of 16 ints per device (8 per-XCD item
// counters + the finished-workgroup count), used round robin (a launch re-arms its slot when it finishes; launches
// on one stream are ordered anyway).  The only device memory this library allocates itself: 4 KiB per GPU, on first use.
int* sched_slot() {
  constexpr int MAX_DEV = 16, SLOTS = 64;
  static int* pool[MAX_DEV] = {};
  static unsigned turn[MAX_DEV] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= MAX_DEV) return nullptr;
  if (!pool[dev]) {
    if (hipMalloc(reinterpret_cast<void**>(&pool[dev]), SLOTS * 16 * sizeof(int)) != hipSuccess) return nullptr;
    (void)hipMemset(pool[dev], 0, SLOTS * 16 * sizeof(int));
    (void)hipDeviceSynchronize();
  }
  return pool[dev] + 16 * (turn[dev]++ % SLOTS);
}

// one planned launch of KERNEL (its dynamic LDS raised on first use)
template <auto KERNEL, typename Args>
int launch_planned(const GemmPlan& pl, const Args& args, hipStream_t st) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds);
    attr_set = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(pl.grid_x, pl.grid_y), dim3(pl.threads), pl.lds, st, args);
  return COGV_OK;
}

#ifndef COGV_W4_TU
// CUs the persistent kernels leave free (cogv_gemm_reserve_cus): a collective that runs CONCURRENTLY with a GEMM needs somewhere
// to live -- a generation-3 / 4 workgroup owns its CU's whole register file, so a persistent launch over all CUs keeps RCCL's
// channel workgroups waiting until it ends.
int g_reserved_cus = 0;

// what the launch plan takes from the device and the environment; cus > 0: plan for that many CUs (cogv_gemm_plan)
GemmEnv gemm_env(int cus = 0) {
  // raster group height (experiments: COGV_GEMM_GROUP_M); 4 rows x 8 columns of tiles per XCD by default
  static const int gm = [] { const char* e = getenv("COGV_GEMM_GROUP_M"); const int v = e ? atoi(e) : 4; return v >= 1 && v <= 32 ? v : 4; }();
  const char* xp = getenv("COGV_GEMM_XP");                // read per launch: tests and A/B runs switch it inside one process
  return GemmEnv{cus > 0 ? cus : num_cus(), g_reserved_cus, gm, !xp || atoi(xp) != 0};
}

// The generation-4 kernel's eight instantiations (2 dtypes x 4 layouts) are compiled from this same file in eight
// separate translation units (-DCOGV_W4_TU=k, see build.py: they build in parallel); unit k = 4 * fp16 + layout index
// (gemm_layout) exports cogv_w4_launch_k.
#define W4_DECL(k) extern "C" __attribute__((visibility("hidden"))) int cogv_w4_launch_##k(const GemmPlan* pl, const void* ga, void* stream);
W4_DECL(0) W4_DECL(1) W4_DECL(2) W4_DECL(3) W4_DECL(4) W4_DECL(5) W4_DECL(6) W4_DECL(7)
#undef W4_DECL
const decltype(&cogv_w4_launch_0) W4_LAUNCH[8] = {cogv_w4_launch_0, cogv_w4_launch_1, cogv_w4_launch_2, cogv_w4_launch_3,
                                                  cogv_w4_launch_4, cogv_w4_launch_5, cogv_w4_launch_6, cogv_w4_launch_7};

// the plan's generation in dtype T and layout index L: TILE_LAUNCH[fp16][L]
template <typename T, int L>
int launch_generation(const GemmPlan& pl, const GroupArgs& ga, hipStream_t st) {
  constexpr bool AT = L >= 2, BT = L == 1 || L == 2;
  static_assert(gemm_layout(AT, BT) == L, "gemm_plan.h");
  switch (pl.generation) {
    case 1: return launch_planned<&gemm_kernel<T, AT, BT>>(pl, ga.g[0], st);
    case 2: return launch_planned<&gemm_glds_kernel<T, AT, BT, 2, 2, 4, 2, 32>>(pl, ga.g[0], st);      // 4 waves of 128x64
    case 3: return launch_planned<&gemm_pp64_kernel<T, AT, BT>>(pl, ga, st);
    default: return W4_LAUNCH[(std::is_same<T, f16_t>::value ? 4 : 0) + L](&pl, &ga, st);
  }
}
typedef int (*tile_launch_fn)(const GemmPlan&, const GroupArgs&, hipStream_t);
#define LAYOUTS(T) {launch_generation<T, 0>, launch_generation<T, 1>, launch_generation<T, 2>, launch_generation<T, 3>}
const tile_launch_fn TILE_LAUNCH[2][4] = {LAYOUTS(bf16_t), LAYOUTS(f16_t)};
#undef LAYOUTS

// The launch of pl[0 .. count): the plan goes into the argument block(s) build_gemm_args filled, one kernel launch by (generation,
// dtype, layout), and one reduce pass per problem that splits K.
int launch_tiles(int dtype, const GemmPlan* pl, int count, const GemmEnv& env, GroupArgs& ga, hipStream_t st) {
  ga.count = count; ga.group_m = env.group_m;
  ga.xp_ok = pl[0].xp_ok; ga.xp_magic_ig = pl[0].xp_magic_ig; ga.xp_magic_gfull = pl[0].xp_magic_gfull; ga.xp_magic_gtail = pl[0].xp_magic_gtail;
  for (int i = 0; i < count; ++i) { ga.g[i].tiles_m = pl[i].tiles_m; ga.g[i].tiles_n = pl[i].tiles_n; ga.item_start[i] = pl[i].item_start; }
  for (int i = count; i <= MAX_GROUP; ++i) ga.item_start[i] = pl[0].items;
  if (pl[0].generation >= 3 && !(ga.sched = sched_slot())) return COGV_ERR_LAUNCH;
  const int rc = TILE_LAUNCH[dtype == COGV_F16][pl[0].layout](pl[0], ga, st);
  if (rc != COGV_OK) return rc;
  const auto reduce = dtype == COGV_F16 ? splitk_reduce_kernel<f16_t> : splitk_reduce_kernel<bf16_t>;
  for (int i = 0; i < count; ++i)
    if (pl[i].reduce_blocks) hipLaunchKernelGGL(reduce, dim3(pl[i].reduce_blocks), dim3(256), 0, st, ga.g[i]);
  return cogv_check_launch();
}

// Skinny-M products (M <= 8: the decode step).  gv_plan (gemv_plan.h) decides every launch: a second-generation kernel of
// gemv.hip -- one unit per weight format and dtype (0 bf16, 1 fp16), each with one entry point that takes the plan -- or, for
// 16-bit weights outside its classes and under COGV_GEMV2=0, a first-generation kernel (gemv_gen1.cuh).
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv2_run_0(int kind, const GvPlan* plan, const GvCall* call);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv2_run_1(int kind, const GvPlan* plan, const GvCall* call);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv2_w8_run_0(int kind, const GvPlan* plan, const GvCall* call);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv2_w8_run_1(int kind, const GvPlan* plan, const GvCall* call);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv2_w4_run_0(int kind, const GvPlan* plan, const GvCall* call);
extern "C" __attribute__((visibility("hidden"))) int cogv_gemv2_w4_run_1(int kind, const GvPlan* plan, const GvCall* call);

template <typename T>
void gemv1_launch(int kind, const GvPlan& pl, const GvCall& c) {
  const dim3 grid(pl.grid), block(pl.threads);
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  if (kind == GV_LN) {
    const GemvLnArgs& a = *reinterpret_cast<const GemvLnArgs*>(c.args);       // rows [M, mt) are written as zeros-normalised junk nobody reads
#define GEMV_LN_LAUNCH(MT_)                                                                                              \
  do {                                                                                                                   \
    static bool attr = false;                                                                                            \
    if (!attr) {                                                                                                         \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_ln_kernel<T, MT_, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536); \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_ln_kernel<T, MT_, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);  \
      attr = true;                                                                                                       \
    }                                                                                                                    \
    if (c.stream_f32) hipLaunchKernelGGL((gemv_ln_kernel<T, MT_, true>), grid, block, pl.lds, st, a);                     \
    else hipLaunchKernelGGL((gemv_ln_kernel<T, MT_, false>), grid, block, pl.lds, st, a);                                 \
  } while (0)
    if (pl.mt == 1) GEMV_LN_LAUNCH(1); else if (pl.mt == 2) GEMV_LN_LAUNCH(2); else if (pl.mt == 4) GEMV_LN_LAUNCH(4); else GEMV_LN_LAUNCH(8);
#undef GEMV_LN_LAUNCH
    return;
  }
  const GemmArgs& a = *reinterpret_cast<const GemmArgs*>(c.args);
  if (kind == GV_ATTN) hipLaunchKernelGGL((gemv_attn_kernel<T>), grid, block, 0, st, a, c.partials, c.heads, c.nsplit);
  else hipLaunchKernelGGL((gemv_kernel<T>), grid, block, 0, st, a);
}

// the launch of a planned product.  (A second-generation launcher answers COGV_ERR_UNSUPPORTED only when the runtime refuses the
// two-halves kernel its LDS: the first generation takes the product then, where there is one.)
int gemv_launch(int kind, int fmt, int dtype, GvPlan pl, const GvCall& c) {
  static int (*const RUN[3][2])(int, const GvPlan*, const GvCall*) = {{cogv_gemv2_run_0, cogv_gemv2_run_1}, {cogv_gemv2_w8_run_0, cogv_gemv2_w8_run_1},
                                                                      {cogv_gemv2_w4_run_0, cogv_gemv2_w4_run_1}};
  if (pl.generation == 2) {
    const int rc = RUN[fmt][dtype == COGV_F16](kind, &pl, &c);
    if (rc != COGV_ERR_UNSUPPORTED || fmt != GV_W16) return rc != COGV_OK ? rc : cogv_check_launch();
    const GemmArgs& a = *reinterpret_cast<const GemmArgs*>(c.args);          // (GemvLnArgs begins with its GemmArgs)
    pl = gv_plan_gen1(kind, pl.mt, a.N, a.K);
  }
  if (dtype == COGV_F16) gemv1_launch<f16_t>(kind, pl, c);
  else gemv1_launch<bf16_t>(kind, pl, c);
  return cogv_check_launch();
}

// what the 16-bit skinny-M kernels of either generation do not take of a descriptor build_gemm_args accepted
bool gemv16_refuses(int kind, const cogv_gemm_desc* d) {
  if (d->trans_a || d->trans_b) return true;
  if (kind == GV_PLAIN) return (d->flags & COGV_EPI_COLSUM) || d->kernel_variant != 0;      // takes every other fused epilogue
  const int refused = COGV_EPI_COLSUM | COGV_EPI_ACCUM | COGV_EPI_DGELU | COGV_EPI_MULAUX | COGV_EPI_DROPOUT | (kind == GV_ATTN ? COGV_EPI_GELU : 0);
  return (d->flags & refused) || d->out_f32 || d->splitk > 1;
}

}  // namespace

extern "C" size_t cogv_gemm_workspace_bytes(const cogv_gemm_desc* d) {
  if (!d || d->splitk <= 1) return 0;
  return (size_t)d->splitk * (size_t)d->M * (size_t)d->N * sizeof(float);
}

// Heuristic used by the host side: split the contraction when the output has too few tiles to fill 256 CUs
// (weight-gradient GEMMs of the 336M config: 64..256 tiles, contraction = b*1088 tokens).
extern "C" int cogv_gemm_colsum_rows(int M) { return 2 * ((M + 255) / 256); }

extern "C" int cogv_gemm_pick_splitk(int M, int N, int K) {
  // 256x256 tiles on one persistent workgroup per CU.  Pick the split that fills whole rounds best; every split
  // costs an fp32 slab write + read (8 M N bytes at ~4 TB/s) against 2 M N K flops at ~1.1 PFLOP/s: 1100 / K each.
  return cogv_gemm_pick_splitk_tiles(((M + 255) / 256) * ((N + 255) / 256), K);
}

// the same for `tiles` 256x256 output tiles in total (a grouped launch): one split count for all problems
extern "C" int cogv_gemm_pick_splitk_tiles(int tiles, int K) {
  const int nk = (K + BK - 1) / BK;
  const int slots = 256;
  if (tiles >= 4 * slots || nk < 16) return 1;
  const float cost = 1100.f / (float)K;
  int best = 1; float best_score = -1.f;
  for (int s = 1; s <= 16 && nk / s >= 8; ++s) {
    const int items = tiles * s;
    const int rounds = (items + slots - 1) / slots;
    const float eff = (float)items / (float)(rounds * slots);
    const float score = eff / (1.f + (s > 1 ? cost * s : 0.f));
    if (score > best_score) { best_score = score; best = s; }
  }
  return best;
}

static int build_gemm_args(const cogv_gemm_desc* d, GemmArgs& a) {
  if (!d) return COGV_ERR_ARG;
  if (d->dtype != COGV_F16 && d->dtype != COGV_BF16) return COGV_ERR_UNSUPPORTED;
  if (d->M <= 0 || d->N <= 0 || d->K <= 0) return COGV_ERR_ARG;
  if ((d->N & 7) || (d->ldc & 7)) return COGV_ERR_ARG;
  if ((d->lda & 7) || (d->ldb & 7)) return COGV_ERR_ARG;
  if (!d->trans_a && (d->K & 7)) return COGV_ERR_ARG;   // K-contiguous operands are read in 16-byte chunks
  if (!d->trans_b && (d->K & 7)) return COGV_ERR_ARG;
  if (d->trans_a && (d->M & 7)) return COGV_ERR_ARG;
  if (((uintptr_t)d->A | (uintptr_t)d->B | (uintptr_t)d->C) & 15) return COGV_ERR_ARG;
  if ((d->flags & COGV_EPI_BIAS) && (!d->bias || ((uintptr_t)d->bias & 15))) return COGV_ERR_ARG;
  if ((d->flags & (COGV_EPI_DGELU | COGV_EPI_MULAUX)) && !d->aux) return COGV_ERR_ARG;
  if ((d->flags & COGV_EPI_DGELU) && (d->flags & COGV_EPI_MULAUX)) return COGV_ERR_ARG;      // one aux operand
  if ((d->flags & COGV_EPI_GELU_DAUX) && !(d->flags & COGV_EPI_GELU)) return COGV_ERR_ARG;
  if ((d->flags & (COGV_EPI_DGELU | COGV_EPI_GELU | COGV_EPI_MULAUX)) && d->aux && ((d->ldaux & 7) || ((uintptr_t)d->aux & 15)))
    return COGV_ERR_ARG;
  if ((d->flags & COGV_EPI_ABSMAX) && !d->absmax) return COGV_ERR_ARG;
  if ((d->flags & COGV_EPI_DROPOUT) && !(d->dropout_p >= 0.f && d->dropout_p < 1.f)) return COGV_ERR_ARG;
  if (d->dropout_row0 < 0) return COGV_ERR_ARG;

  a.A = d->A; a.B = d->B; a.C = d->C;
  a.M = d->M; a.N = d->N; a.K = d->K;
  a.lda = d->lda; a.ldb = d->ldb; a.ldc = d->ldc;
  a.bias = d->bias; a.aux = d->aux; a.ldaux = d->ldaux; a.absmax = d->absmax;
  a.flags = d->flags; a.out_f32 = d->out_f32;
  a.seed = d->seed; a.stream_id = d->stream_id;
  a.drop_c0 = ((uint64_t)d->dropout_row0 * (uint64_t)d->N) >> 3;       // N % 8 == 0 (checked above)
  a.thr16 = (d->flags & COGV_EPI_DROPOUT) ? (uint32_t)(d->dropout_p * 65536.0f + 0.5f) : 0u;
  a.keep_scale = 65536.0f / (65536.0f - (float)a.thr16);
  gemm_split(d->K, d->splitk, a.splitk, a.ktiles_per_split);
  a.colsum_ws = d->colsum_partial;
  if ((d->flags & COGV_EPI_COLSUM) && (!d->colsum_partial || ((uintptr_t)d->colsum_partial & 15) || d->splitk > 1 || d->out_f32)) return COGV_ERR_ARG;
  a.ws = reinterpret_cast<float*>(d->workspace);
  if (a.splitk > 1) {
    if (!a.ws || d->workspace_bytes < (size_t)a.splitk * a.M * a.N * sizeof(float)) return COGV_ERR_ARG;
    if ((uintptr_t)a.ws & 15) return COGV_ERR_ARG;
  }
  return COGV_OK;
}

extern "C" int cogv_gemm_reserve_cus(int n) {
  const int prev = g_reserved_cus;
  if (n >= 0) g_reserved_cus = n;
  return prev;
}

// what cogv_gemm decides before it launches: the argument block, then the skinny-M plan (M <= 8, decode steps: the HBM-streaming
// matrix-vector kernels) or the tile plan, or the call's error
static int gemm_front(const cogv_gemm_desc* d, const GemmEnv& env, GemmArgs& a, GvPlan& gv, GemmPlan& pl) {
  const int rc = build_gemm_args(d, a);
  if (rc != COGV_OK) return rc;
  if (!gemv16_refuses(GV_PLAIN, d) && gv_plan(GV_PLAIN, GV_W16, a.M, a.N, a.K, a.ldb, 0, gv)) {
    pl = GemmPlan{GEMM_SKINNY};
    return COGV_OK;
  }
  return gemm_plan(*d, env, pl) ? COGV_OK : COGV_ERR_UNSUPPORTED;
}

extern "C" int cogv_gemm(const cogv_gemm_desc* d, void* stream) {
  GroupArgs ga;
  GvPlan gv;
  GemmPlan pl;
  const GemmEnv env = gemm_env();
  const int rc = gemm_front(d, env, ga.g[0], gv, pl);
  if (rc != COGV_OK) return rc;
  if (pl.family == GEMM_SKINNY) {
    ga.g[0].splitk = 1;
    return gemv_launch(GV_PLAIN, GV_W16, d->dtype, gv, GvCall{&ga.g[0], nullptr, 0, 0, 0, stream});
  }
  return launch_tiles(d->dtype, &pl, 1, env, ga, reinterpret_cast<hipStream_t>(stream));
}

// ---- the skinny-M products with a prologue, and all three on a quantized weight operand (gemv.hip, FormV / FormM on W8 / W4: it
//      travels in the argument block as B / ldb and its scales, weight_operand.h; no first-generation kernel stands behind those)

// the descriptor with the quantized operand in B's place -> argument block; `allowed`: the epilogue flags the product takes
static int build_q_args(const cogv_gemm_desc* d, const WeightOperand& w, int allowed, bool has_a, GemmArgs& a) {
  if (!d || weight_operand_null(w)) return COGV_ERR_ARG;
  if (d->M > GEMV_MAX_M || (d->N & 7) || (d->K & 511) || d->trans_a || d->trans_b || (d->flags & ~allowed) || d->out_f32 || d->splitk > 1)
    return COGV_ERR_UNSUPPORTED;
  if (weight_operand_misplaced(w, d->K)) return COGV_ERR_ARG;
  cogv_gemm_desc dd = *d;
  dd.B = w.q; dd.ldb = w.ldq;
  if (!has_a) { dd.A = dd.B; dd.lda = dd.K; }          // (no A operand: keep build_gemm_args' pointer checks happy)
  const int rc = build_gemm_args(&dd, a);
  if (rc == COGV_OK) weight_operand_put(w, a);
  return rc;
}

static int gemv_ln_args(const cogv_ln_prologue* ln, GemvLnArgs& a) {
  if (!ln->z || !ln->gamma || !ln->beta) return COGV_ERR_ARG;
  if (ln->gamma_post && (!ln->beta_post || !ln->residual)) return COGV_ERR_ARG;
  if (((uintptr_t)ln->z | (uintptr_t)ln->gamma | (uintptr_t)ln->beta | (uintptr_t)ln->gamma_post | (uintptr_t)ln->beta_post |
       (uintptr_t)ln->residual | (uintptr_t)ln->t_out) & 15) return COGV_ERR_ARG;
  a.z = ln->z; a.z_absmax = ln->z_absmax; a.gamma_p = ln->gamma_post; a.beta_p = ln->beta_post; a.res = ln->residual;
  a.t_out = ln->t_out; a.gamma = ln->gamma; a.beta = ln->beta; a.eps = ln->eps;
  return COGV_OK;
}

// Descriptor of a product of `kind` (w: its quantized weight, or NULL: 16-bit weights in d->B) -> argument block and launch plan,
// or the entry point's error: the front of cogv_gemv_ln, cogv_gemv_attn, the three _w8 and the three _w4 calls and the two plan
// queries (cogv_gemm's is gemm_front).
// The order of the checks on a quantized operand, which callers rely on (tests/test_weight_operand_cpu.py has it as a table): a
// NULL descriptor, operand, q or scale (1); M, N, K % 512, the layout, the flags, out_f32, splitk (3); the operand's alignment,
// ldq % 16 and the block scales' lds (1); build_gemm_args (1 | 3); aux on the plain and the LayerNorm kind (3); gv_shape_taken (3);
// the prologue (1: a bad prologue is reported before a class's refusal); the plan (3) -- which is where an ldq shorter than a row of
// K ends up, since gv_plan refuses it.  The wide front (gemv_wide.hip, gw_front) judges the whole operand BEFORE the descriptor
// and answers 1 for a short ldq.
static int gemv_front(int kind, const cogv_gemm_desc* d, const WeightOperand* w, int nsplit, GemmArgs& a, GvPlan& pl,
                      const cogv_ln_prologue* ln = nullptr, GemvLnArgs* la = nullptr) {
  int rc;
  if (w) {
    rc = build_q_args(d, *w, COGV_EPI_BIAS | COGV_EPI_ABSMAX | (kind == GV_ATTN ? 0 : COGV_EPI_GELU), kind == GV_PLAIN, a);
    if (rc == COGV_OK && kind != GV_ATTN && d->aux) rc = COGV_ERR_UNSUPPORTED;
  }
  else if (!d) rc = COGV_ERR_ARG;
  else {
    cogv_gemm_desc dd = *d;
    if (kind == GV_ATTN) { dd.A = dd.B; dd.lda = dd.K; }        // (as above)
    rc = build_gemm_args(&dd, a);
    if (rc == COGV_OK && gemv16_refuses(kind, d)) rc = COGV_ERR_UNSUPPORTED;
  }
  if (rc != COGV_OK) return rc;
  a.splitk = 1;
  if (!gv_shape_taken(kind, a.M, a.N, a.K)) return COGV_ERR_UNSUPPORTED;
  if (ln && (rc = gemv_ln_args(ln, *la)) != COGV_OK) return rc;
  return gv_plan(kind, weight_format(w), a.M, a.N, a.K, a.ldb, nsplit, pl) ? COGV_OK : COGV_ERR_UNSUPPORTED;
}

// The entry points below turn their ABI operand into a WeightOperand (weight_operand: NULL stays NULL).  A _w8 / _w4 call without
// its operand is a bad argument; cogv_gemv_plan without one is the 16-bit query.

// y = epilogue(LN_pre([res + LN_post(z)]) . B^T): the decode step's GEMV with its LayerNorms as prologue
static int gemv_ln(const cogv_gemm_desc* d, const cogv_ln_prologue* ln, const WeightOperand* w, void* stream) {
  if (!ln) return COGV_ERR_ARG;
  GemvLnArgs a;
  GvPlan pl;
  const int rc = gemv_front(GV_LN, d, w, 0, a.g, pl, ln, &a);
  if (rc != COGV_OK) return rc;
  return gemv_launch(GV_LN, weight_format(w), d->dtype, pl, GvCall{&a, nullptr, 0, 0, ln->stream_f32 != 0, stream});
}
extern "C" int cogv_gemv_ln(const cogv_gemm_desc* d, const cogv_ln_prologue* ln, void* stream) { return gemv_ln(d, ln, nullptr, stream); }
extern "C" int cogv_gemv_ln_w8(const cogv_gemm_desc* d, const cogv_ln_prologue* ln, const cogv_w8_weight* w, void* stream) {
  WeightOperand o; return w ? gemv_ln(d, ln, weight_operand(w, o), stream) : COGV_ERR_ARG;
}
extern "C" int cogv_gemv_ln_w4(const cogv_gemm_desc* d, const cogv_ln_prologue* ln, const cogv_w4_weight* w, void* stream) {
  WeightOperand o; return w ? gemv_ln(d, ln, weight_operand(w, o), stream) : COGV_ERR_ARG;
}

// y = epilogue(att . B^T), att = the combination of cogv_attention_decode's split partials (skip_combine form)
static int gemv_attn(const cogv_gemm_desc* d, const WeightOperand* w, const void* partials, int heads, int capacity, void* stream) {
  if (!partials || heads <= 0 || capacity <= 0 || capacity > 4096 || ((uintptr_t)partials & 15)) return COGV_ERR_ARG;
  const int nsplit = (capacity + 127) / 128;
  GemmArgs a;
  GvPlan pl;
  const int rc = gemv_front(GV_ATTN, d, w, nsplit, a, pl);
  if (rc != COGV_OK) return rc;
  if (a.K != heads * 64) return COGV_ERR_UNSUPPORTED;
  return gemv_launch(GV_ATTN, weight_format(w), d->dtype, pl, GvCall{&a, reinterpret_cast<const float*>(partials), heads, nsplit, 0, stream});
}
extern "C" int cogv_gemv_attn(const cogv_gemm_desc* d, const void* partials, int heads, int capacity, void* stream) {
  return gemv_attn(d, nullptr, partials, heads, capacity, stream);
}
extern "C" int cogv_gemv_attn_w8(const cogv_gemm_desc* d, const cogv_w8_weight* w, const void* partials, int heads, int capacity, void* stream) {
  WeightOperand o; return w ? gemv_attn(d, weight_operand(w, o), partials, heads, capacity, stream) : COGV_ERR_ARG;
}
extern "C" int cogv_gemv_attn_w4(const cogv_gemm_desc* d, const cogv_w4_weight* w, const void* partials, int heads, int capacity, void* stream) {
  WeightOperand o; return w ? gemv_attn(d, weight_operand(w, o), partials, heads, capacity, stream) : COGV_ERR_ARG;
}

// cogv_gemm's skinny case on a quantized weight
static int gemm_q(const cogv_gemm_desc* d, const WeightOperand* w, void* stream) {
  if (!w) return COGV_ERR_ARG;
  GemmArgs a;
  GvPlan pl;
  const int rc = gemv_front(GV_PLAIN, d, w, 0, a, pl);
  return rc != COGV_OK ? rc : gemv_launch(GV_PLAIN, w->fmt, d->dtype, pl, GvCall{&a, nullptr, 0, 0, 0, stream});
}
extern "C" int cogv_gemm_w8(const cogv_gemm_desc* d, const cogv_w8_weight* w, void* stream) { WeightOperand o; return gemm_q(d, weight_operand(w, o), stream); }
extern "C" int cogv_gemm_w4(const cogv_gemm_desc* d, const cogv_w4_weight* w, void* stream) { WeightOperand o; return gemm_q(d, weight_operand(w, o), stream); }

// host-only: the plan the entry points above (and cogv_gemm's skinny case) would launch with
static int gemv_plan_query(int kind, const cogv_gemm_desc* d, const WeightOperand* w, int nsplit, int* out) {
  if (!out || kind < COGV_GEMV_PLAIN || kind > COGV_GEMV_LN || (kind == COGV_GEMV_ATTN && nsplit < 1)) return COGV_ERR_ARG;
  GemmArgs a;
  GvPlan pl;
  const int rc = gemv_front(1 << kind, d, w, nsplit, a, pl);
  if (rc != COGV_OK) return rc;
  const int v[COGV_GEMV_PLAN_INTS] = {pl.generation, pl.form, pl.p0, pl.p1, pl.guard, pl.mt, pl.tw, pl.k2, pl.threads, pl.grid, pl.lds};
  for (int i = 0; i < COGV_GEMV_PLAN_INTS; ++i) out[i] = v[i];
  return COGV_OK;
}
extern "C" int cogv_gemv_plan(int kind, const cogv_gemm_desc* d, const cogv_w8_weight* w, int nsplit, int out[COGV_GEMV_PLAN_INTS]) {
  WeightOperand o; return gemv_plan_query(kind, d, weight_operand(w, o), nsplit, out);
}
extern "C" int cogv_gemv_w4_plan(int kind, const cogv_gemm_desc* d, const cogv_w4_weight* w, int nsplit, int out[COGV_GEMV_PLAN_INTS]) {
  WeightOperand o; return w ? gemv_plan_query(kind, d, weight_operand(w, o), nsplit, out) : COGV_ERR_ARG;
}

// Several GEMMs of the same dtype and layout in one persistent launch of the generation-4 kernel (see GroupArgs).
// Every problem must satisfy that kernel's requirements (gemm_persistent_takes); otherwise COGV_ERR_UNSUPPORTED and the caller
// issues them one by one.
static int grouped_front(const cogv_gemm_desc* descs, int count, const GemmEnv& env, GroupArgs& ga, GemmPlan* pl) {
  if (!descs || count < 1 || count > MAX_GROUP) return COGV_ERR_ARG;
  for (int i = 0; i < count; ++i) {
    const cogv_gemm_desc* d = descs + i;
    const int rc = build_gemm_args(d, ga.g[i]);
    if (rc != COGV_OK) return rc;
    if (d->dtype != descs[0].dtype || d->trans_a != descs[0].trans_a || d->trans_b != descs[0].trans_b) return COGV_ERR_ARG;
    if (!gemm_persistent_takes(*d)) return COGV_ERR_UNSUPPORTED;
  }
  gemm_plan_persistent(descs, count, 4, env, pl);
  return COGV_OK;
}

extern "C" int cogv_gemm_grouped(const cogv_gemm_desc* descs, int count, void* stream) {
  GroupArgs ga;
  GemmPlan pl[MAX_GROUP];
  const GemmEnv env = gemm_env();
  const int rc = grouped_front(descs, count, env, ga, pl);
  return rc != COGV_OK ? rc : launch_tiles(descs[0].dtype, pl, count, env, ga, reinterpret_cast<hipStream_t>(stream));
}

// host-only: the plan cogv_gemm (count 0) or cogv_gemm_grouped (count >= 1) would launch with, or the call's error
extern "C" int cogv_gemm_plan(const cogv_gemm_desc* descs, int count, int num_cus, int* out) {
  static_assert(offsetof(GemmPlan, xp_magic_ig) == COGV_GEMM_PLAN_INTS * sizeof(int), "cogview_hip.h");
  if (!out || count < 0 || num_cus < 0) return COGV_ERR_ARG;
  GroupArgs ga;
  GvPlan gv;
  GemmPlan pl[MAX_GROUP];
  const GemmEnv env = gemm_env(num_cus);
  const int rc = count ? grouped_front(descs, count, env, ga, pl) : gemm_front(descs, env, ga.g[0], gv, pl[0]);
  if (rc != COGV_OK) return rc;
  for (int i = 0; i < (count ? count : 1); ++i) memcpy(out + i * COGV_GEMM_PLAN_INTS, &pl[i], COGV_GEMM_PLAN_INTS * sizeof(int));
  return COGV_OK;
}
#else   // COGV_W4_TU: one instantiation of the generation-4 kernel and its launcher
}  // namespace

#define W4_CAT2(a, b) a##b
#define W4_CAT(a, b) W4_CAT2(a, b)
extern "C" __attribute__((visibility("hidden"))) int W4_CAT(cogv_w4_launch_, COGV_W4_TU)(const GemmPlan* pl, const void* ga, void* stream) {
  using T = std::conditional<(COGV_W4_TU & 4) != 0, f16_t, bf16_t>::type;
  constexpr int L = COGV_W4_TU & 3;                      // layout index (gemm_layout)
  return launch_planned<&gemm_w4_kernel<T, (L >= 2), (L == 1 || L == 2)>>(*pl, *reinterpret_cast<const GroupArgs*>(ga), reinterpret_cast<hipStream_t>(stream));
}
#endif

// Candidate scoring on the device: the log-probability of one target id per row of logits, under a softmax restricted to an
// allowed id range, and its sum over groups of rows.  Replaces the host tail of the reference's post-selection score
// (generation/sampling.py:214-230: logits.float(), -inf over the image codes, log_softmax, gather, sum over the text).
//
// One workgroup of 1024 threads per row, two streaming passes over [allow_lo, allow_hi) (max, then sum of exp(x - max)); the
// row is never held in registers, so any vocab >= 1 works.  Thread t visits its ids in a fixed order:
//   vector path (row base and row stride 16-byte aligned): the 16-byte chunks that lie wholly inside the range, chunk
//                t, t + 1024, ... of them (ascending); AFTER them thread t < (ids of the two ragged ends) takes the t-th end id;
//   scalar path: ids allow_lo + t, + 1024, ... (ascending)
// Per-thread partial sums in that order, then wave butterflies and a fixed loop over the 16 wave totals (block_sum): the same
// input gives the same bits.  The two paths assign ids to threads differently, so they agree to rounding, not bit for bit.
// scores[g] is formed by ONE thread of a second small launch over the stored logp, in ascending row order (so scores needs
// logp).  No floating-point atomics.
#include "common.cuh"
#include "cogview_hip.h"

namespace {

constexpr int SB = 1024;                 // threads per workgroup (16 waves)

template <typename T> struct Chunk;      // one 16-byte load
template <> struct Chunk<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float* f) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = v[j];
  }
};
template <> struct Chunk<f16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const f16_t* p, float* f) { unpack8<f16_t>(*reinterpret_cast<const u32x4*>(p), f); }
};
template <> struct Chunk<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float* f) { unpack8<bf16_t>(*reinterpret_cast<const u32x4*>(p), f); }
};

// f(x) for every id of [lo, hi) this thread owns, in a fixed order (whole chunks ascending, then one ragged-end id)
template <typename T, bool VEC, typename F>
__device__ __forceinline__ void for_owned(const T* src, int lo, int hi, int t, F f) {
  if constexpr (VEC) {
    constexpr int N = Chunk<T>::N;
    const int vlo = min((lo + N - 1) / N * N, hi);       // [lo, vlo) ragged head, [vlo, vhi) whole chunks, [vhi, hi) ragged tail
    const int vhi = max(hi / N * N, vlo);
    for (int i = vlo + t * N; i < vhi; i += SB * N) {
      float x[N];
      Chunk<T>::load(src + i, x);
#pragma unroll
      for (int j = 0; j < N; ++j) f(x[j]);
    }
    const int nhead = vlo - lo;                          // < N each: fewer end ids than threads
    if (t < nhead) f((float)src[lo + t]);
    else if (t < nhead + (hi - vhi)) f((float)src[vhi + (t - nhead)]);
  } else {
    for (int i = lo + t; i < hi; i += SB) f((float)src[i]);
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(SB) void score_kernel(cogv_score_desc d) {
  __shared__ float red[SB / 64];
  const int row = blockIdx.x, t = threadIdx.x;
  const T* src = reinterpret_cast<const T*>(d.logits) + (size_t)row * (size_t)d.row_stride;
  const int lo = d.allow_lo, hi = d.allow_hi;
  float m = -INFINITY;
  for_owned<T, VEC>(src, lo, hi, t, [&](float x) { m = fmaxf(m, x); });
  m = block_max(m, red);
  float s = 0.f;
  for_owned<T, VEC>(src, lo, hi, t, [&](float x) { s += expf(x - m); });
  s = block_sum(s, red);
  if (t == 0) {
    const int64_t id = d.target[row];
    d.logp[row] = (id >= lo && id < hi) ? (float)src[id] - m - logf(s) : -INFINITY;
  }
}

__global__ void score_group_kernel(const float* logp, float* scores, int groups, int group) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= groups) return;
  const float* p = logp + (size_t)g * (size_t)group;
  float s = 0.f;
  for (int j = 0; j < group; ++j) s += p[j];
  scores[g] = s;
}

template <typename T>
void launch_rows(const cogv_score_desc& d, bool vec, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((score_kernel<T, true>), dim3(d.rows), dim3(SB), 0, s, d);
  else hipLaunchKernelGGL((score_kernel<T, false>), dim3(d.rows), dim3(SB), 0, s, d);
}

}  // namespace

extern "C" int cogv_score_targets(const cogv_score_desc* d, void* stream) {
  if (!d || !d->logits || !d->target || d->rows <= 0 || d->group <= 0 || d->vocab <= 0) return COGV_ERR_ARG;
  if (d->rows % d->group != 0) return COGV_ERR_ARG;
  if (d->allow_lo < 0 || d->allow_hi > d->vocab || d->allow_lo >= d->allow_hi) return COGV_ERR_ARG;
  if (d->row_stride < d->vocab) return COGV_ERR_ARG;
  if (d->scores && !d->logp) return COGV_ERR_ARG;        // the group sums are formed from the stored per-row values
  if (d->dtype != COGV_F16 && d->dtype != COGV_BF16 && d->dtype != COGV_F32) return COGV_ERR_ARG;
  if (d->rows > 65535) return COGV_ERR_UNSUPPORTED;
  if (!d->logp) return COGV_OK;                          // nothing asked for
  hipStream_t s = (hipStream_t)stream;
  const size_t esz = d->dtype == COGV_F32 ? 4 : 2;
  const bool vec = (uintptr_t)d->logits % 16 == 0 && ((size_t)d->row_stride * esz) % 16 == 0;
  switch (d->dtype) {
    case COGV_F16: launch_rows<f16_t>(*d, vec, s); break;
    case COGV_BF16: launch_rows<bf16_t>(*d, vec, s); break;
    default: launch_rows<float>(*d, vec, s); break;
  }
  if (d->scores) {
    const int groups = d->rows / d->group;
    hipLaunchKernelGGL(score_group_kernel, dim3((groups + 255) / 256), dim3(256), 0, s, d->logp, d->scores, groups, d->group);
  }
  return cogv_check_launch();
}

// Token sampling on the device: temperature, allowed-id range, top-k, top-p, softmax and one inverse-CDF draw per row,
// plus the decode graph's between-step bookkeeping (generation/decoder.py SamplingDecoder).  Replaces the host sampling of
// the reference's generation/sampling.py:24-50 (top_k_logits) and :168-186 (softmax, multinomial, gather, log, cat).
//
// One workgroup of 1024 threads per row.  Thread t owns the CONTIGUOUS ids [t * PER, (t + 1) * PER) (PER = 64, vocab <=
// 65536), held in registers as the order-preserving uint32 image of x = float(logit) / temperature (key(a) < key(b) iff
// a < b for non-NaN floats); ids outside [allow_lo, allow_hi) hold the key of -inf.  Contiguous ownership makes the draw an
// index-order scan: a per-thread running sum, then one block scan over the 1024 thread totals.
//   top-k  the k-th largest key by a 4-pass radix select (8-bit digits, 256-bin LDS histograms of integer counts); every
//          key >= it is kept, so ties at the threshold all survive (torch.topk(...)[-1] + `logits < kth` semantics).
//   top-p  the masses e = exp(x - max) of the top-k survivors replace the keys (exp is monotone: their bit patterns order the
//          ids as the logits do); the smallest pattern kappa with  mass(e > kappa) <= top_p * Z  by bisection (block sums
//          in a fixed order, <= 30 steps); e >= kappa is kept: the descending prefix whose mass first exceeds top_p, the
//          first id always included.
//   draw   u = 24 bits of the counter-based generator keyed (seed, *offset), counter = row (common.cuh); the first kept id
//          whose inclusive prefix mass exceeds u * Z wins.  Every sum has a fixed order: same (seed, offset) -> same ids.
//   given  decode mode with a table of given ids (magnify's windows, generation/sampling.py DeviceFiller): where
//          given[*pos_index + 1] >= 0 that id is fed instead of drawn -- the logits are not read, logp = 0, scores and the
//          probabilities untouched; the bookkeeping and the counter are those of a draw.  With given_stride > 0 every row
//          reads its own table, given[row * given_stride + *pos_index + 1] (DeviceBatchFiller: several images on one decode
//          graph), and rows that are fed and rows that draw share a launch.
#include "common.cuh"
#include "cogview_hip.h"

namespace {

constexpr int SB = 1024;                 // threads per workgroup (16 waves)
constexpr int PER = 64;                  // ids per thread
constexpr uint32_t KEY_NEG_INF = 0x007fffffu;   // key(-inf)

__device__ __forceinline__ uint32_t f2key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <typename T> __device__ __forceinline__ float load_logit(const T* p, int j) { return (float)p[j]; }

// exclusive prefix sum over the threads in index order (fixed order); *total receives the grand total
__device__ __forceinline__ float block_exclusive_scan(float v, float* red, float* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  __syncthreads();
  if (lane == 63) red[w] = incl;
  __syncthreads();
  float before = 0.f, all = 0.f;
#pragma unroll
  for (int i = 0; i < SB / 64; ++i) {
    if (i < w) before += red[i];
    all += red[i];
  }
  *total = all;
  return before + (incl - v);
}

struct SampleSmem {
  uint32_t hist[256];
  uint32_t red_u[SB / 64];
  float red_f[SB / 64];
  uint32_t sel;        // chosen digit of the radix pass
  uint32_t need;       // rank still to find inside the chosen bin
  int win;             // drawn id: the first whose inclusive prefix mass exceeds u * Z
  int last;            // the last kept id
};

// the per-row results of one position (one thread): the id, its log-probability (added to the score when `score`), and in
// decode mode the next step's token, position, visible slot and output column
__device__ __forceinline__ void publish(const cogv_sample_desc& d, int row, int64_t id, float lp, bool score) {
  if (d.ids) d.ids[row] = id;
  if (d.logp) d.logp[row] = lp;
  if (score && d.scores) d.scores[row] += lp;
  if (d.pos_index) {
    const int64_t p1 = *d.pos_index + 1;                 // sequence position the id will occupy
    if (d.tok) d.tok[row] = id;
    if (d.pos) d.pos[row] += 1;
    if (d.table && p1 < d.capacity) d.table[(size_t)row * (size_t)d.capacity + p1] = (int32_t)p1;
    const int64_t c = p1 - d.out_base;
    if (d.out_tokens && c >= 0 && c < d.out_len) d.out_tokens[(size_t)row * (size_t)d.out_len + c] = id;
  }
}

// filter + draw of one row (every thread of the workgroup).  Returns true on the thread that holds the drawn id, with the id
// and its log-probability in *id_out / *lp_out
template <typename T>
__device__ __forceinline__ bool sample_row(const cogv_sample_desc& d, SampleSmem& sm, int row, int t, const T* src, int64_t off,
                                           int64_t* id_out, float* lp_out) {
  const int vocab = d.vocab;
  const int64_t i0 = (int64_t)t * PER;

  // ---- load: x = float(logit) / temperature (a true division, as the host's `logits /= temperature`).  One base address
  // per thread and immediate offsets: per-element 64-bit addresses would not fit next to the 64 keys.
  const T* p = src + i0;
  const int nv = min(max(vocab - (int)i0, 0), PER);                  // ids of this thread inside the vocabulary
  const int jlo = max(d.allow_lo - (int)i0, 0), jhi = min(d.allow_hi - (int)i0, nv);
  uint32_t key[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    key[j] = KEY_NEG_INF;
    if (j >= jlo && j < jhi) key[j] = f2key(load_logit<T>(p, j) / d.temperature);
  }

  // ---- top-k: k-th largest key by radix select, most significant digit first
  uint32_t kth = KEY_NEG_INF;
  if (d.top_k > 0) {
    uint32_t prefix = 0, need = (uint32_t)d.top_k;
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t hmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
      for (int b = t; b < 256; b += SB) sm.hist[b] = 0;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < PER; ++j)
        if (j < nv && (key[j] & hmask) == prefix) atomicAdd(&sm.hist[(key[j] >> shift) & 255u], 1u);
      __syncthreads();
      if (t < 64) {                         // wave 0: lane l owns bins 255-4l .. 252-4l (descending)
        uint32_t c[4], s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c[q] = sm.hist[255 - 4 * t - q]; s += c[q]; }
        uint32_t incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
          if (t >= o) incl += y;
        }
        uint32_t above = incl - s;          // count in the bins above this lane's four
        if (above < need && incl >= need) { // exactly one lane holds the bin where the rank falls
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (above < need && above + c[q] >= need) { sm.sel = 255 - 4 * t - q; sm.need = need - above; }
            above += c[q];
          }
        }
      }
      __syncthreads();
      prefix |= sm.sel << shift;
      need = sm.need;
      __syncthreads();
    }
    kth = prefix;
  }

  // ---- softmax statistics over the top-k survivors
  uint32_t kmax = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) if (key[j] >= kth && key[j] > KEY_NEG_INF) kmax = max(kmax, key[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
  __syncthreads();
  if ((t & 63) == 0) sm.red_u[t >> 6] = kmax;
  __syncthreads();
  kmax = sm.red_u[0];
#pragma unroll
  for (int i = 1; i < SB / 64; ++i) kmax = max(kmax, sm.red_u[i]);
  const float m = key2f(kmax);
  const bool any = kmax > KEY_NEG_INF;
  __syncthreads();

  // ---- unnormalised masses e = exp(x - max) of the top-k survivors, in place of the keys (exp is monotone, so the bit
  // patterns of e order the ids as their logits do; ties stay ties)
  float e[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const uint32_t k = key[j];
    e[j] = (k >= kth && k > KEY_NEG_INF) ? expf(key2f(k) - m) : 0.f;
  }

  // ---- top-p: smallest mass pattern kappa with  mass(e > kappa) <= top_p * Z;  e >= kappa is kept
  if (d.top_p > 0.f && any) {
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) z += e[j];
    const float bound = d.top_p * block_sum(z, sm.red_f);
    // invariant: mass(> hi) <= bound (hi = pattern of 1.0 = the max's mass: nothing above), mass(> lo) > bound or lo = 0
    uint32_t lo = 0, hi = __float_as_uint(1.0f);
#pragma unroll 1
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j) s += __float_as_uint(e[j]) > mid ? e[j] : 0.f;
      s = block_sum(s, sm.red_f);
      if (s <= bound) hi = mid; else lo = mid;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) e[j] = __float_as_uint(e[j]) >= hi ? e[j] : 0.f;
  }

  // ---- kept mass in index order; the draw
  float run = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) run += e[j];
  float zall;
  const float before = block_exclusive_scan(run, sm.red_f, &zall);
  if (t == 0) { sm.win = 0x7fffffff; sm.last = -1; }
  __syncthreads();
  const uint32_t rk = rng_key(d.seed, (uint64_t)off);
  const float u = (float)(Philox::gen_k(rk, (uint64_t)row)[0] >> 8) * (1.0f / 16777216.0f);
  const float target = u * zall;
  {
    float acc = before;
    int first = 0x7fffffff, last = -1;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (e[j] > 0.f) {
        acc += e[j];
        if (acc > target && first == 0x7fffffff) first = (int)(i0 + j);
        last = (int)(i0 + j);
      }
    }
    if (first != 0x7fffffff) atomicMin(&sm.win, first);
    if (last >= 0) atomicMax(&sm.last, last);
    __syncthreads();
  }
  // rounding can leave u * Z at the total: then the last kept id; nothing finite in range: the first allowed id
  const int id = sm.win != 0x7fffffff ? sm.win : (sm.last >= 0 ? sm.last : d.allow_lo);

  if (d.probs) {
    float* pr = d.probs + (size_t)row * (size_t)vocab + i0;
    const float rz = 1.0f / zall;
#pragma unroll
    for (int j = 0; j < PER; ++j) if (j < nv) pr[j] = any ? e[j] * rz : 0.f;
  }
  // the winner's thread hands the per-row results back
  if (i0 <= id && id < i0 + PER) {
    float ew = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) if (i0 + j == id) ew = e[j];
    *id_out = id;
    *lp_out = any ? logf(ew / zall) : -INFINITY;
    return true;
  }
  return false;
}

template <typename T>
__global__ __launch_bounds__(SB) void sample_kernel(cogv_sample_desc d) {
  __shared__ SampleSmem sm;
  const int row = blockIdx.x, t = threadIdx.x;
  const T* src = reinterpret_cast<const T*>(d.logits) + (size_t)row * (size_t)d.row_stride;
  const int64_t off = d.offset ? *d.offset : 0;
  // a given id for the position this launch fills (decode mode only, checked by the host), from the shared table
  // (given_stride 0) or from this row's own: the same address for every thread of the workgroup -- a workgroup is one row --
  // so the branch below is uniform across it and is taken before any barrier, while other rows of the launch may take the
  // other side.  A given id is published by thread 0 with logp 0 and no score; one publish site for both paths keeps the
  // register allocation of the draw
  int64_t fed = -1;
  if (d.given) {
    const int64_t p1 = *d.pos_index + 1;
    if (p1 >= 0 && p1 < d.capacity) fed = d.given[(int64_t)row * d.given_stride + p1];
  }
  int64_t id = fed;
  float lp = 0.f;
  bool mine = t == 0;
  if (fed < 0) mine = sample_row<T>(d, sm, row, t, src, off, &id, &lp);
  if (mine) publish(d, row, id, lp, fed < 0);
  // the last workgroup to finish advances the shared scalars (every other one has read them by then) and resets the counter
  if (d.counter && (d.pos_index || d.offset)) {
    __shared__ bool last;
    __threadfence();
    __syncthreads();
    if (t == 0) last = atomicAdd(d.counter, 1u) == (uint32_t)gridDim.x - 1;
    __syncthreads();
    if (last && t == 0) {
      __threadfence();
      if (d.pos_index) *d.pos_index += 1;
      if (d.offset) *d.offset += 1;
      *d.counter = 0;
    }
  }
}

}  // namespace

extern "C" int cogv_sample_logits(const cogv_sample_desc* d, void* stream) {
  if (!d || !d->logits || d->rows <= 0 || d->vocab <= 0 || d->vocab > SB * PER || d->row_stride < 0) return COGV_ERR_ARG;
  if (!(d->temperature > 0.f) || d->top_k < 0 || !(d->top_p >= 0.f)) return COGV_ERR_ARG;
  if (d->allow_lo < 0 || d->allow_hi > d->vocab || d->allow_lo >= d->allow_hi) return COGV_ERR_ARG;
  if (d->top_k > d->allow_hi - d->allow_lo) return COGV_ERR_ARG;
  if (d->row_stride != 0 && d->row_stride < d->vocab) return COGV_ERR_ARG;
  if (d->pos_index && (!d->counter || (d->table && d->capacity <= 0) || (d->out_tokens && d->out_len <= 0))) return COGV_ERR_ARG;
  if (d->given && (!d->pos_index || d->capacity <= 0)) return COGV_ERR_ARG;
  if (d->given && (d->given_stride < 0 || (d->given_stride > 0 && d->given_stride < d->capacity))) return COGV_ERR_ARG;
  if (d->rows > 65535) return COGV_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  switch (d->dtype) {
    case COGV_F16: hipLaunchKernelGGL(sample_kernel<f16_t>, dim3(d->rows), dim3(SB), 0, s, *d); break;
    case COGV_BF16: hipLaunchKernelGGL(sample_kernel<bf16_t>, dim3(d->rows), dim3(SB), 0, s, *d); break;
    case COGV_F32: hipLaunchKernelGGL(sample_kernel<float>, dim3(d->rows), dim3(SB), 0, s, *d); break;
    default: return COGV_ERR_ARG;
  }
  return cogv_check_launch();
}

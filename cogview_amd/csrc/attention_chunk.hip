// Decode step of m tokens per cache row (cogv_attention_decode_chunk; generation/decoder.py chunk=C).
// generation/sampling.py:139-148 makes one model call per token, also for a token that is already known: a run of known ids
// costs one replay of the captured step each.  Here rows r = b * m + j, j = 0 ... m - 1, are the tokens of slots *pos + j of cache
// row b; row (b, j) attends slots [first_b, *pos + j], the slots [*pos, *pos + j] being the chunk's own rows.  This unit is
// separate from attention.hip: its kernels compile what they always did; the combine launch is attention.hip's, reached through
// cogv_attn_decode_combine_launch, and the partials are those of attn_decode_kernel indexed by row r.
#include "common.cuh"
#include "cogview_hip.h"

// attention.hip: the combine launch of a decode step (partials in split order -> out)
extern "C" __attribute__((visibility("hidden"))) int cogv_attn_decode_combine_launch(int dtype, const void* ws, void* out, long long out_bs,
                                                                                     int B, int H, int nsplit, void* stream);

namespace {

constexpr int HD = 64;
constexpr int MAX_M = 8;

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// attn_decode_kernel (attention.hip) for m queries per cache row: the same grid (capacity / 128, H, B), 8 lanes per key, 4 passes
// of 32 keys, the same partial (max, sum, 64 outputs) per (row, head, split).  A workgroup requests its 128 keys and values ONCE,
// before *pos is read; the m rows' q | k | v of this head (3 * m 16-byte words per 8-lane group) go through LDS.  Once *pos is
// known, the registers that hold slots [*pos, *pos + m) take the chunk's own keys / values (and these are stored into the cache):
// they now hold the cache as it will be after the step.  Then, per query j, EXACTLY the arithmetic of attn_decode_kernel at position
// *pos + j -- same lane mapping, same fused multiply-adds, same reduction order; a slot that query j does not attend takes row j's
// own key / value bits and a score of -inf, as there -- so every partial is bit-identical to the one-token call's, and a query's
// numbers do not involve the other queries.  Two barriers per query, as in the one-token kernel (red_m alternates).
struct ChunkArgs {
  const void* qkv; void* cache; const long long* pos; float* ws;
  long long qkv_rs, cache_bs; int cache_rs;
  int B, H, cap, nsplit, m; float scale_l2e;
  const int* first;
};
template <typename T, bool RAGGED = false>
__global__ __launch_bounds__(256) void attn_decode_chunk_kernel(const ChunkArgs p) {
  __shared__ float red_o[32][64];
  __shared__ float red_m[2][4], red_l[32];
  __shared__ __attribute__((aligned(16))) u32x4 snew[3][MAX_M][8];          // q | k | v, row j, 16-byte word of the head
  const int t = threadIdx.x, dch = t & 7, kg = t >> 3, lane = t & 63, wave = t >> 6;
  const int split = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int hp = p.H * HD;
  // the chunk's rows first: the wait for them then leaves the cache rows in flight
  u32x4 staged = {0u, 0u, 0u, 0u};
  const int sj = t / 24, ssect = (t % 24) >> 3, sd = t & 7;        // (t % 24) & 7 == t & 7: 24 is a multiple of 8
  if (t < p.m * 24)
    staged = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(p.qkv) + ((long long)b * p.m + sj) * p.qkv_rs + ssect * hp + head * HD + sd * 8);
  T* crow = reinterpret_cast<T*>(p.cache) + b * p.cache_bs + head * HD + dch * 8;
  u32x4 v8[4], kc8[4];
  int first_b = 0;
  if (RAGGED) first_b = p.first[b];          // requested with the cache rows, ahead of *pos
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const long long key = (long long)split * 128 + ps * 32 + kg;
    // requested whatever *pos says, as in attn_decode_kernel (a key past the capacity re-reads the last row)
    const long long krow = key < p.cap ? key : p.cap - 1;
#if !defined(COGV_DECODE_NT) || COGV_DECODE_NT
    kc8[ps] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(crow + krow * p.cache_rs));
    v8[ps] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(crow + krow * p.cache_rs + hp));
#else
    kc8[ps] = *reinterpret_cast<const u32x4*>(crow + krow * p.cache_rs);
    v8[ps] = *reinterpret_cast<const u32x4*>(crow + krow * p.cache_rs + hp);
#endif
  }
  if (t < p.m * 24) snew[ssect][sj][sd] = staged;
  const long long pos = *p.pos;
  __syncthreads();
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const long long key = (long long)split * 128 + ps * 32 + kg;
    const long long off = key - pos;
    const bool own = off >= 0 && off < p.m && key < p.cap;          // a slot of the chunk: row `off` of this cache row
    const int i = own ? (int)off : 0;
    const u32x4 kn = snew[1][i][dch], vn = snew[2][i][dch];
    // (bit masks, not a select: the compiler turns a select of a loaded value into a branch and sinks the load into it)
    const uint32_t mk = own ? 0xffffffffu : 0u;
    kc8[ps] = (kc8[ps] & ~mk) | (kn & mk);
    v8[ps] = (v8[ps] & ~mk) | (vn & mk);
    if (own) {                               // stored for the steps to come (by the lane that loaded these 16 bytes)
      *reinterpret_cast<u32x4*>(crow + key * p.cache_rs) = kn;
      *reinterpret_cast<u32x4*>(crow + key * p.cache_rs + hp) = vn;
    }
  }
  for (int j = 0; j < p.m; ++j) {
    float q8[8];
    unpack8<T>(snew[0][j][dch], q8);
    const u32x4 knew = snew[1][j][dch], vnew = snew[2][j][dch];
    const long long posj = pos + j;
    // first[b] < 0 counts as 0; first[b] > the row's own slot leaves that slot
    const long long first = RAGGED ? (first_b < 0 ? 0 : (first_b > posj ? posj : (long long)first_b)) : 0;
    float sc[4]; u32x4 vj[4];
    float m_loc = -INFINITY;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const long long key = (long long)split * 128 + ps * 32 + kg;
      const bool valid = (!RAGGED || key >= first) && key <= posj && key < p.cap;
      const uint32_t mk = valid ? 0xffffffffu : 0u;
      const u32x4 k8 = (kc8[ps] & mk) | (knew & ~mk);
      vj[ps] = (v8[ps] & mk) | (vnew & ~mk);
      float kf[8]; unpack8<T>(k8, kf);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(q8[e], kf[e], d);
      d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);     // the key's 8 lanes
      sc[ps] = valid ? d * p.scale_l2e : -INFINITY;
      m_loc = fmaxf(m_loc, sc[ps]);
    }
    m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 8, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 16, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 32, 64));
    float* rm = red_m[j & 1];
    if (lane == 0) rm[wave] = m_loc;
    __syncthreads();
    const float m = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
    float o8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, l = 0.f;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const float pr = (sc[ps] == -INFINITY) ? 0.f : fast_exp2(sc[ps] - m);
      float vf[8]; unpack8<T>(vj[ps], vf);
      l += pr;
#pragma unroll
      for (int e = 0; e < 8; ++e) o8[e] = fmaf(pr, vf[e], o8[e]);
    }
    // (the readers of the previous query's red_o / red_l are wave 0's lanes, which passed the barrier above after reading)
#pragma unroll
    for (int e = 0; e < 8; ++e) red_o[kg][dch * 8 + e] = o8[e];
    if (dch == 0) red_l[kg] = l;
    __syncthreads();
    float* part = p.ws + ((((size_t)b * p.m + j) * p.H + head) * p.nsplit + split) * 66;
    if (t < 64) {
      float o = 0.f;
#pragma unroll 8
      for (int g = 0; g < 32; ++g) o += red_o[g][t];
      part[2 + t] = o;
      if (t == 0) {
        float ls = 0.f;
        for (int g = 0; g < 32; ++g) ls += red_l[g];
        part[0] = m; part[1] = ls;
      }
    }
  }
}

}  // namespace

extern "C" int cogv_attention_decode_chunk(const cogv_attn_decode_chunk_desc* d, void* stream) {
  if (!d || (d->dtype != COGV_F16 && d->dtype != COGV_BF16) || d->head_dim != HD) return COGV_ERR_UNSUPPORTED;
  if (d->m < 1 || d->m > MAX_M) return COGV_ERR_ARG;
  // (B * m rows go to the workspace query and the combine launch as an int)
  if (d->B <= 0 || d->H <= 0 || d->capacity <= 0 || d->capacity > 4096 || (long long)d->B * d->m > (1 << 20)) return COGV_ERR_ARG;
  if (!d->qkv || !d->cache || (!d->out && !d->skip_combine) || !d->pos || !d->workspace) return COGV_ERR_ARG;
  if (((uintptr_t)d->qkv & 15) || ((uintptr_t)d->cache & 15) || ((d->qkv_rs | d->cache_bs | d->cache_rs) & 7)) return COGV_ERR_ARG;
  if (d->workspace_bytes < cogv_attention_decode_workspace_bytes(d->B * d->m, d->H, d->capacity) || ((uintptr_t)d->workspace & 15)) return COGV_ERR_ARG;
  if ((uintptr_t)d->first & 3) return COGV_ERR_ARG;
  ChunkArgs a;
  a.qkv = d->qkv; a.cache = d->cache; a.pos = d->pos; a.first = d->first;
  a.ws = reinterpret_cast<float*>(d->workspace);
  a.qkv_rs = d->qkv_rs; a.cache_bs = d->cache_bs; a.cache_rs = d->cache_rs;
  a.B = d->B; a.H = d->H; a.cap = d->capacity; a.nsplit = (d->capacity + 127) / 128; a.m = d->m;
  a.scale_l2e = d->scale * 1.4426950408889634f;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(a.nsplit, a.H, a.B);
  if (d->dtype == COGV_F16) {
    if (a.first) hipLaunchKernelGGL((attn_decode_chunk_kernel<f16_t, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_decode_chunk_kernel<f16_t>), grid, dim3(256), 0, st, a);
  } else {
    if (a.first) hipLaunchKernelGGL((attn_decode_chunk_kernel<bf16_t, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_decode_chunk_kernel<bf16_t>), grid, dim3(256), 0, st, a);
  }
  // skip_combine: the consumer (cogv_gemv_attn / cogv_gemv_attn_w8 with B * m rows) recombines the partials itself
  if (!d->skip_combine) return cogv_attn_decode_combine_launch(d->dtype, d->workspace, d->out, d->out_rs, a.B * a.m, a.H, a.nsplit, stream);
  return cogv_check_launch();
}

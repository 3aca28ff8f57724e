// Attention of a decode step: ONE query token per batch row (cogv_attention_decode), m <= 8 tokens per row
// (cogv_attention_decode_chunk), one token on an 8-bit cache (cogv_kv_quantize_e4m3, cogv_attention_decode_kv8) or m <= 8 tokens
// on it (cogv_attention_decode_chunk_kv8) against a fixed-capacity key/value cache (generation/sampling.py:139-148, one model
// call per generated token; generation/decoder.py).
// The 128-query tile kernels of attention.hip spend a whole workgroup per (batch, head) on one row (40 workgroups on 256 CUs,
// 34 us per layer at 1152 slots); the kernels here split the KEYS: grid (capacity / 128, H, B), a partial (max, sum, output)
// per split; a second small launch combines the partials in split order (deterministic).  The new token's key / value come
// straight from the QKV GEMM's output row and are written into the cache slot *pos by the split that owns it: the cat +
// index_copy_ launches of the generic cache append disappear.  Valid slots are [0, *pos] (device data: no launch parameter
// depends on the length).
// WHAT THE KERNELS SHARE is what compiles to the same instructions in each of them as when it was written out there (DESIGN.md
// 4.5): the pieces below, each called from a kernel's OWN loops.  A piece that holds a whole loop over the four passes (the
// request of a split, the P.V sum) or the whole per-query body changes the kernels' code -- they then no longer share the keys
// and comparisons of a pass between their loops -- and so does passing `own` to clamp_first by value: leave the signatures.
#include "e4m3_stream.cuh"
#include "cogview_hip.h"

namespace {

constexpr int HD = 64;                   // head dim
constexpr int SPLIT_KEYS = 128;          // keys per workgroup
constexpr int PARTIAL = 2 + HD;          // floats a split leaves per (row, head): max, sum, 64 outputs
constexpr int MAX_M = 8;                 // tokens per cache row of a chunk step

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ float* partial_of(float* ws, size_t row, int H, int head, int nsplit, int split) {
  return ws + ((row * H + head) * nsplit + split) * PARTIAL;
}

// first[b] < 0 counts as 0; first[b] > the row's own slot leaves that slot
__device__ __forceinline__ long long clamp_first(int first_b, const long long& own) {
  return first_b < 0 ? 0 : (first_b > own ? own : (long long)first_b);
}

// A slot's key and value of the 16-bit cache, 8 lanes per key (16 bytes of the 128-byte row each: coalesced); a kernel requests
// its split's 128 slots in four passes of 32.  The rows are requested whatever *pos says (slots past it hold stale or no data
// and are replaced by the caller; a key past the capacity re-reads the last row): the position is a device scalar, and loads
// that waited for it would start one memory latency late -- the launch is a chain of latencies, not of bytes.  Streamed once per
// step: ld_stream.
template <typename T>
__device__ __forceinline__ void request_slot(const T* crow, long long key, int cap, int cache_rs, int hp, u32x4& k, u32x4& v) {
  const long long krow = key < cap ? key : cap - 1;
  k = ld_stream<u32x4>(crow + krow * cache_rs);
  v = ld_stream<u32x4>(crow + krow * cache_rs + hp);
}

// One key against the query: the cached bits where mk is set, `other` elsewhere (bit masks, not a select: the compiler turns a
// select of a loaded value into a branch and sinks the load into it); the 8-term dot product, summed over the key's 8 lanes.
template <typename T>
__device__ __forceinline__ float masked_dot(const u32x4& cached, const u32x4& other, uint32_t mk, const float (&q8)[8]) {
  const u32x4 k8 = (cached & mk) | (other & ~mk);
  float kf[8]; unpack8<T>(k8, kf);
  float d = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) d = fmaf(q8[e], kf[e], d);
  d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
  return d;
}

// P.V of one key: o8 += 2^(sc - m) * v, l += 2^(sc - m); a score of -inf weighs 0 whatever m is.
template <typename T>
__device__ __forceinline__ void pv_add(float sc, const u32x4& v, float m, float (&o8)[8], float& l) {
  const float pr = (sc == -INFINITY) ? 0.f : fast_exp2(sc - m);
  float vf[8]; unpack8<T>(v, vf);
  l += pr;
#pragma unroll
  for (int e = 0; e < 8; ++e) o8[e] = fmaf(pr, vf[e], o8[e]);
}

// Reduction tail of the 16-bit kernels: the 32 key groups' outputs and sums -> the split's partial, in a fixed order.
__device__ __forceinline__ void reduce_to_partial(float (&red_o)[32][64], float (&red_l)[32], const float (&o8)[8], float l, float m,
                                                  float* part, int t, int kg, int dch) {
#pragma unroll
  for (int e = 0; e < 8; ++e) red_o[kg][dch * 8 + e] = o8[e];
  if (dch == 0) red_l[kg] = l;
  __syncthreads();
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

// ---------------------------------------------------------------------------------------------------- one token, 16-bit cache
// RAGGED (cogv_attn_decode_desc.first != NULL; a second instantiation): row b attends slots [first[b], *pos] -- rows of one
// launch hold right-aligned contexts of different lengths, slots below first[b] are padding.  A padding slot is treated like a
// slot past *pos: it takes the new token's bits through the masks below and a score of -inf, so whatever it holds never enters
// a product; a split that lies wholly in the padding leaves the partial (-inf, 0, 0...) a split past *pos leaves, which both
// combines weight with 0.
struct DecodeArgs {
  const void* qkv; void* cache; void* out; const long long* pos; float* ws; int* tickets;          // tickets: unused, kept for the layout
  long long qkv_bs, cache_bs, out_bs; int cache_rs;
  int B, H, cap, nsplit; float scale_l2e;
  const int* first;
};
template <typename T, bool RAGGED = false>
__global__ __launch_bounds__(256) void attn_decode_kernel(const DecodeArgs p) {
  __shared__ float red_o[32][64];
  __shared__ float red_m[4], red_l[32];
  const int t = threadIdx.x, dch = t & 7, kg = t >> 3, lane = t & 63, wave = t >> 6;
  const int split = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int hp = p.H * HD;
  const T* qrow = reinterpret_cast<const T*>(p.qkv) + b * p.qkv_bs + head * HD + dch * 8;
  float q8[8];
  unpack8<T>(*reinterpret_cast<const u32x4*>(qrow), q8);
  const u32x4 knew = *reinterpret_cast<const u32x4*>(qrow + hp), vnew = *reinterpret_cast<const u32x4*>(qrow + 2 * hp);
  T* crow = reinterpret_cast<T*>(p.cache) + b * p.cache_bs + head * HD + dch * 8;
  float sc[4]; u32x4 v8[4], kc8[4];
  float m_loc = -INFINITY;
  int first_b = 0;
  if (RAGGED) first_b = p.first[b];          // requested with the cache rows, ahead of *pos
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) request_slot(crow, (long long)split * SPLIT_KEYS + ps * 32 + kg, p.cap, p.cache_rs, hp, kc8[ps], v8[ps]);
  const long long pos = *p.pos;
  const long long first = RAGGED ? clamp_first(first_b, pos) : 0;
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const long long key = (long long)split * SPLIT_KEYS + ps * 32 + kg;
    const bool valid = (!RAGGED || key >= first) && key <= pos && key < p.cap;
    const bool cached = valid && key != pos;
    // (bit masks, not a select: the compiler turns a select of a loaded value into a branch and sinks the load into it)
    const uint32_t mk = cached ? 0xffffffffu : 0u;
    v8[ps] = (v8[ps] & mk) | (vnew & ~mk);
    if (valid && !cached) {                  // the new token's own slot: store it for the steps to come
      *reinterpret_cast<u32x4*>(crow + key * p.cache_rs) = knew;
      *reinterpret_cast<u32x4*>(crow + key * p.cache_rs + hp) = vnew;
    }
    const float d = masked_dot<T>(kc8[ps], knew, mk, q8);
    sc[ps] = valid ? d * p.scale_l2e : -INFINITY;
    m_loc = fmaxf(m_loc, sc[ps]);
  }
  m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 8, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 16, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 32, 64));
  if (lane == 0) red_m[wave] = m_loc;
  __syncthreads();
  const float m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
  float o8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, l = 0.f;
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) pv_add<T>(sc[ps], v8[ps], m, o8, l);
  reduce_to_partial(red_o, red_l, o8, l, m, partial_of(p.ws, b, p.H, head, p.nsplit, split), t, kg, dch);
}
// second launch of a decode step: combine the splits' partial (max, sum, output) in split order.  (A device-scope
// release fence + arrival ticket inside the first kernel costs an L2 write-back per workgroup on this part -- measured
// 50 us per layer; the kernel boundary publishes the partials for free.)
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_combine_kernel(const DecodeArgs p) {
  __shared__ float wgt[64];
  const int t = threadIdx.x, head = blockIdx.x, b = blockIdx.y;
  const float* base = partial_of(p.ws, b, p.H, head, p.nsplit, 0);
  // lane i holds split i's (max, sum): one independent load each instead of a chain of dependent ones (nsplit <= 32)
  const float mi = t < p.nsplit ? base[t * PARTIAL] : -INFINITY;
  const float li = t < p.nsplit ? base[t * PARTIAL + 1] : 0.f;
  // the partial outputs of up to 16 splits are requested together with the statistics (clamped index: unconditional), so the
  // launch pays one memory round trip instead of two
  float ov[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) ov[i] = base[(i < p.nsplit ? i : p.nsplit - 1) * PARTIAL + 2 + t];
  float M = mi;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
  const float w = (mi == -INFINITY) ? 0.f : fast_exp2(mi - M);
  float L = li * w;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) L += __shfl_xor(L, o, 64);
  wgt[t] = w;
  __syncthreads();
  float O = 0.f;
  if (p.nsplit <= 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) O = i < p.nsplit ? fmaf(ov[i], wgt[i], O) : O;         // same order as the loop below
  } else {
#pragma unroll 8
    for (int i = 0; i < p.nsplit; ++i) O = fmaf(base[i * PARTIAL + 2 + t], wgt[i], O);
  }
  reinterpret_cast<T*>(p.out)[b * p.out_bs + head * HD + t] = HT<T>::from_f(O / L);
}

// ---------------------------------------------------------------------------------------------------- m tokens, 16-bit cache
// generation/sampling.py:139-148 makes one model call per token, also for a token that is already known: a run of known ids
// costs one replay of the captured step each.  Here rows r = b * m + j, j = 0 ... m - 1, are the tokens of slots *pos + j of
// cache row b; row (b, j) attends slots [first_b, *pos + j], the slots [*pos, *pos + j] being the chunk's own rows.  Differs
// from attn_decode_kernel in this: the m rows' q | k | v of this head (3 * m 16-byte words per 8-lane group) go through LDS;
// once *pos is known, the registers that hold slots [*pos, *pos + m) take the chunk's own keys / values (and these are stored
// into the cache): they now hold the cache as it will be after the step.  Then, per query j, the one-token kernel's arithmetic
// at position *pos + j (a slot that query j does not attend takes row j's own key / value bits and a score of -inf), so every
// partial, indexed by row r, is bit-identical to the one-token call's.  Two barriers per query (red_m alternates).
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
  for (int ps = 0; ps < 4; ++ps) request_slot(crow, (long long)split * SPLIT_KEYS + ps * 32 + kg, p.cap, p.cache_rs, hp, kc8[ps], v8[ps]);
  if (t < p.m * 24) snew[ssect][sj][sd] = staged;
  const long long pos = *p.pos;
  __syncthreads();
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const long long key = (long long)split * SPLIT_KEYS + ps * 32 + kg;
    const long long off = key - pos;
    const bool own = off >= 0 && off < p.m && key < p.cap;          // a slot of the chunk: row `off` of this cache row
    const int i = own ? (int)off : 0;
    const u32x4 kn = snew[1][i][dch], vn = snew[2][i][dch];
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
    const long long first = RAGGED ? clamp_first(first_b, posj) : 0;
    float sc[4]; u32x4 vj[4];
    float m_loc = -INFINITY;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const long long key = (long long)split * SPLIT_KEYS + ps * 32 + kg;
      const bool valid = (!RAGGED || key >= first) && key <= posj && key < p.cap;
      const uint32_t mk = valid ? 0xffffffffu : 0u;
      vj[ps] = (v8[ps] & mk) | (vnew & ~mk);
      const float d = masked_dot<T>(kc8[ps], knew, mk, q8);
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
    for (int ps = 0; ps < 4; ++ps) pv_add<T>(sc[ps], vj[ps], m, o8, l);
    // (the readers of the previous query's red_o / red_l are wave 0's lanes, which passed the barrier above after reading)
    reduce_to_partial(red_o, red_l, o8, l, m, partial_of(p.ws, (size_t)b * p.m + j, p.H, head, p.nsplit, split), t, kg, dch);
  }
}

// ---------------------------------------------------------------------------------------------------- 8-bit cache
// The decode attention requests every slot of the fixed-capacity cache on every step, so a step streams the whole cache: here
// the cache holds OCP E4M3 bytes ("e4m3fn": no infinities, largest value 448) with one fp32 scale per (slot, head, K | V) -- the
// rule of e4m3_stream.cuh with the 64 elements of one head of one slot as the group.  Head-major layout, so that the 128 keys of
// one split are one contiguous 8-KB block:
//     q     uint8 [B][2][H][capacity][64]      plane 0: keys, plane 1: values
//     scale fp32  [B][2][H][capacity]
// 136 bytes per (slot, head) for its key and value instead of 256.

// The 16 elements one lane holds of a head's 64 (two 16-byte words of the 16-bit type), the head spread over 4 adjacent lanes:
// scale of the head and this lane's 16 E4M3 bytes.  Same operations, in the same order per element, as quantize_rows_e4m3_kernel.
template <typename T>
__device__ __forceinline__ u32x4 quantize_head16(const u32x4& a, const u32x4& b, float& scale) {
  uint32_t m = absmax_pk8(absmax_pk8(0u, a), b);
  m = max(m & 0xffffu, m >> 16);
  m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
  m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
  const float amax = bits_to_f<T>((uint16_t)m);
  const float s = e4m3_scale(amax);
  scale = s;
  float f[16];
  unpack8<T>(a, f);
  unpack8<T>(b, f + 8);
#pragma unroll
  for (int i = 0; i < 16; ++i) f[i] = f[i] / s;
  u32x4 q;
#pragma unroll
  for (int w = 0; w < 4; ++w) q[w] = pack4_e4m3(f[4 * w], f[4 * w + 1], f[4 * w + 2], f[4 * w + 3]);
  return q;
}

// Cache quantizer: the 16-bit K | V rows a prefill leaves, kv [B][n][2 * H * 64] -> slots [slot0, slot0 + n) of q / scale.  Four
// lanes own one (row, head, K | V): 64 of them per workgroup (a 256-thread workgroup per 64 elements is what the weight quantizer
// on a [rows, 64] view would spend).  The maximum crosses the 4 lanes by shuffles: no LDS, no atomics.  Once per layer per prefill.
struct KvQuantArgs {
  const void* kv; void* q; float* scale;
  long long kv_bs, kv_rs, q_bs, scale_bs;
  int B, n, H, cap, slot0;
};
template <typename T>
__global__ __launch_bounds__(256) void kv_quantize_e4m3_kernel(const KvQuantArgs p) {
  const int part = threadIdx.x & 3;
  const long long g = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);          // ((b * n + r) * 2 + plane) * H + head
  const long long total = (long long)p.B * p.n * 2 * p.H;
  const bool live = g < total;
  const long long gg = live ? g : total - 1;              // (the idle groups of the last workgroup redo the last one and store nothing)
  const int head = (int)(gg % p.H);
  const int plane = (int)((gg / p.H) & 1);
  const long long br = gg / (2 * p.H);
  const int r = (int)(br % p.n), b = (int)(br / p.n);
  const T* src = reinterpret_cast<const T*>(p.kv) + b * p.kv_bs + r * p.kv_rs + (size_t)(plane * p.H + head) * HD + part * 16;
  const u32x4 x0 = *reinterpret_cast<const u32x4*>(src), x1 = *reinterpret_cast<const u32x4*>(src + 8);
  float s;
  const u32x4 q = quantize_head16<T>(x0, x1, s);
  if (!live) return;
  const size_t row = ((size_t)plane * p.H + head) * p.cap + p.slot0 + r;
  *reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(p.q) + b * p.q_bs + row * HD + part * 16) = q;
  if (part == 0) p.scale[b * p.scale_bs + row] = s;
}

// One token on the 8-bit cache.  Differs from attn_decode_kernel in this: FOUR lanes per key, 16 bytes each (a 64-byte row; a
// wave's request is one contiguous 1-KB piece of the split's 8-KB block), two passes of 64 keys: 2 key + 2 value 16-byte loads
// and 4 scale loads per lane, all issued before *pos is read.  The new token's key / value are QUANTIZED FIRST (its 64 elements
// live in 4 lanes: the maximum crosses them by two shuffles), stored into slot *pos as bytes + scale, and the step's own
// attention uses the dequantized values -- a token's key has one value in every step that reads it.  Bytes become fp32 exactly
// (v_cvt_pk_f32_fp8); the scale multiplies the 64-term dot product (keys) and the probability (values): all arithmetic fp32.
// A padding slot (RAGGED) takes the new token's bytes AND scales.  The reduction goes over 64 key groups in two levels.
struct DecodeKv8Args {
  const void* qkv; uint8_t* q; float* scale; const long long* pos; float* ws;
  long long qkv_bs, q_bs, scale_bs;
  int B, H, cap, nsplit; float scale_l2e;
  const int* first;
};
constexpr int RED_LD = 68;        // floats per row of the output reduction (16-byte rows, off the 64-float bank period)
template <typename T, bool RAGGED = false>
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const DecodeKv8Args p) {
  __shared__ __attribute__((aligned(16))) float red_o[64 * RED_LD];
  __shared__ float red_p[4][64];
  __shared__ float red_m[4], red_l[64];
  const int t = threadIdx.x, part = t & 3, kg = t >> 2, lane = t & 63, wave = t >> 6;
  const int split = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int hp = p.H * HD;
  const T* qrow = reinterpret_cast<const T*>(p.qkv) + b * p.qkv_bs + head * HD + part * 16;
  const u32x4 q0 = *reinterpret_cast<const u32x4*>(qrow), q1 = *reinterpret_cast<const u32x4*>(qrow + 8);
  const u32x4 k0 = *reinterpret_cast<const u32x4*>(qrow + hp), k1 = *reinterpret_cast<const u32x4*>(qrow + hp + 8);
  const u32x4 v0 = *reinterpret_cast<const u32x4*>(qrow + 2 * hp), v1 = *reinterpret_cast<const u32x4*>(qrow + 2 * hp + 8);
  // planes of this (batch row, head): keys at kq / ks, values one plane (H * cap rows) further
  const size_t prow = (size_t)head * p.cap, plane = (size_t)p.H * p.cap;
  uint8_t* kq = p.q + b * p.q_bs + prow * HD + part * 16;
  float* ks = p.scale + b * p.scale_bs + prow;
  u32x4 kc[2], vc[2]; uint32_t ksc[2], vsc[2];
  int first_b = 0;
  if (RAGGED) first_b = p.first[b];          // requested with the cache rows, ahead of *pos
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int key = split * SPLIT_KEYS + ps * 64 + kg;
    const int krow = key < p.cap ? key : p.cap - 1;          // requested whatever *pos says, as in request_split
    kc[ps] = ld_stream<u32x4>(kq + (size_t)krow * HD);
    vc[ps] = ld_stream<u32x4>(kq + (plane + krow) * HD);
    ksc[ps] = ld_stream<uint32_t>(ks + krow);
    vsc[ps] = ld_stream<uint32_t>(ks + plane + krow);
  }
  // (the scheduler otherwise sinks the 16-byte loads below the quantization, behind the wait for the qkv row)
  __builtin_amdgcn_sched_barrier(0);
  // the new token, quantized while the loads fly (every 4-lane group computes the same bytes: no broadcast needed)
  float kns, vns;
  const u32x4 knew = quantize_head16<T>(k0, k1, kns), vnew = quantize_head16<T>(v0, v1, vns);
  float qf[16];
  unpack8<T>(q0, qf); unpack8<T>(q1, qf + 8);
  const long long pos = *p.pos;
  const long long first = RAGGED ? clamp_first(first_b, pos) : 0;
  float sc[2], m_loc = -INFINITY;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int key = split * SPLIT_KEYS + ps * 64 + kg;
    const bool valid = (!RAGGED || key >= first) && key <= pos && key < p.cap;
    const bool cached = valid && key != pos;
    // every slot that is not a cached one takes the new token's bytes and scales (bit masks, as in attn_decode_kernel):
    // whatever the cache holds there never enters a product
    const uint32_t mk = cached ? 0xffffffffu : 0u;
    const u32x4 k16 = (kc[ps] & mk) | (knew & ~mk);
    vc[ps] = (vc[ps] & mk) | (vnew & ~mk);
    const float kscale = __uint_as_float((ksc[ps] & mk) | (__float_as_uint(kns) & ~mk));
    vsc[ps] = (vsc[ps] & mk) | (__float_as_uint(vns) & ~mk);
    if (valid && !cached) {                  // the new token's own slot: store it for the steps to come
      *reinterpret_cast<u32x4*>(kq + (size_t)key * HD) = knew;
      *reinterpret_cast<u32x4*>(kq + (plane + key) * HD) = vnew;
      if (part == 0) { ks[key] = kns; ks[plane + key] = vns; }
    }
    float kf[16]; unpack16_e4m3(k16, kf);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) d = fmaf(qf[e], kf[e], d);
    d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64);                  // the key's 4 lanes
    sc[ps] = valid ? d * kscale * p.scale_l2e : -INFINITY;
    m_loc = fmaxf(m_loc, sc[ps]);
  }
  m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 4, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 8, 64));
  m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 16, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 32, 64));
  if (lane == 0) red_m[wave] = m_loc;
  __syncthreads();
  const float m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
  float o[16], l = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const float pr = (sc[ps] == -INFINITY) ? 0.f : fast_exp2(sc[ps] - m);
    const float w = pr * __uint_as_float(vsc[ps]);
    float vf[16]; unpack16_e4m3(vc[ps], vf);
    l += pr;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = fmaf(w, vf[e], o[e]);
  }
#pragma unroll
  for (int w4 = 0; w4 < 4; ++w4)
    *reinterpret_cast<f32x4*>(&red_o[kg * RED_LD + part * 16 + w4 * 4]) = f32x4{o[4 * w4], o[4 * w4 + 1], o[4 * w4 + 2], o[4 * w4 + 3]};
  if (part == 0) red_l[kg] = l;
  __syncthreads();
  {                                          // 64 key groups -> 4 quarter sums per column, then one: fixed order
    const int c = t & 63, qr = t >> 6;
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) s += red_o[(qr * 16 + g) * RED_LD + c];
    red_p[qr][c] = s;
  }
  __syncthreads();
  float* part_out = partial_of(p.ws, b, p.H, head, p.nsplit, split);
  if (t < 64) {
    part_out[2 + t] = (red_p[0][t] + red_p[1][t]) + (red_p[2][t] + red_p[3][t]);
    if (t == 0) {
      float ls = 0.f;
      for (int g = 0; g < 64; ++g) ls += red_l[g];
      part_out[0] = m; part_out[1] = ls;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- m tokens, 8-bit cache
// The chunk step (attn_decode_chunk_kernel) on the 8-bit cache: lanes, loads and reduction are attn_decode_kv8_kernel's, the
// chunk's rows go through LDS as in attn_decode_chunk_kernel.  The chunk's m keys and m values are QUANTIZED FIRST, as m one-token
// steps would quantize them: the 2 * m 4-lane groups of wave 0 do one quantize_head16 each (16 divisions per lane; every group
// redoing all 2 * m of them would cost up to 256) and publish bytes and scales through LDS; wave 1 stages the m queries.  Once *pos is
// known, the registers that hold slots [*pos, *pos + m) take the chunk's bytes and scales (and store them): they hold the cache
// as it will be after the step.  Then, per query j, the one-token kernel's arithmetic at position *pos + j: a slot that query j
// does not attend takes row j's own bytes AND scales through the masks (0 * NaN of a stale value scale would reach the output)
// and a score of -inf.  Partials, indexed by row r = b * m + j, outputs and cache are bit-identical to m one-token calls'.  Three
// barriers per query, as in the one-token kernel.  (Its own loops and reduction, written out: see the header of this file.)
struct ChunkKv8Args {
  const void* qkv; uint8_t* q; float* scale; const long long* pos; float* ws;
  long long qkv_rs, q_bs, scale_bs;
  int B, H, cap, nsplit, m; float scale_l2e;
  const int* first;
};
template <typename T, bool RAGGED = false>
__global__ __launch_bounds__(256) void attn_decode_chunk_kv8_kernel(const ChunkKv8Args p) {
  __shared__ __attribute__((aligned(16))) float red_o[64 * RED_LD];
  __shared__ float red_p[4][64];
  __shared__ float red_m[4], red_l[64];
  __shared__ __attribute__((aligned(16))) u32x4 sq[MAX_M][8];               // queries: row j, 16-byte word of the head (16-bit)
  __shared__ __attribute__((aligned(16))) u32x4 skv[2][MAX_M][4];           // K | V of row j as E4M3 bytes
  __shared__ float sscale[2][MAX_M];                                        // and their scales
  const int t = threadIdx.x, part = t & 3, kg = t >> 2, lane = t & 63, wave = t >> 6;
  const int split = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int hp = p.H * HD;
  // the chunk's rows first: the wait for them then leaves the cache rows in flight.  Wave 0: group kg = 2 * j + (K | V) holds one
  // head of 64 elements, 16 per lane; wave 1: lane = 8 * j + word of query j.  (Groups / lanes past the chunk redo its last row
  // and publish nothing: the shuffles of the quantization run with every lane of the wave.)
  const T* rows = reinterpret_cast<const T*>(p.qkv) + (long long)b * p.m * p.qkv_rs + head * HD;
  u32x4 st0 = {0u, 0u, 0u, 0u}, st1 = {0u, 0u, 0u, 0u};
  const int g2 = kg < 2 * p.m ? kg : 2 * p.m - 1;                           // wave 0: kg = 0 ... 15
  const int qj = (lane >> 3) < p.m ? (lane >> 3) : p.m - 1;
  if (wave == 0) {
    const T* src = rows + (long long)(g2 >> 1) * p.qkv_rs + (1 + (g2 & 1)) * hp + part * 16;
    st0 = *reinterpret_cast<const u32x4*>(src); st1 = *reinterpret_cast<const u32x4*>(src + 8);
  } else if (wave == 1) {
    st0 = *reinterpret_cast<const u32x4*>(rows + (long long)qj * p.qkv_rs + (lane & 7) * 8);
  }
  // planes of this (batch row, head): keys at kq / ks, values one plane (H * cap rows) further
  const size_t prow = (size_t)head * p.cap, plane = (size_t)p.H * p.cap;
  uint8_t* kq = p.q + b * p.q_bs + prow * HD + part * 16;
  float* ks = p.scale + b * p.scale_bs + prow;
  u32x4 kc[2], vc[2]; uint32_t ksc[2], vsc[2];
  int first_b = 0;
  if (RAGGED) first_b = p.first[b];          // requested with the cache rows, ahead of *pos
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int key = split * SPLIT_KEYS + ps * 64 + kg;
    const int krow = key < p.cap ? key : p.cap - 1;          // requested whatever *pos says
    kc[ps] = ld_stream<u32x4>(kq + (size_t)krow * HD);
    vc[ps] = ld_stream<u32x4>(kq + (plane + krow) * HD);
    ksc[ps] = ld_stream<uint32_t>(ks + krow);
    vsc[ps] = ld_stream<uint32_t>(ks + plane + krow);
  }
  // (the scheduler otherwise sinks the 16-byte loads below the quantization, behind the wait for the qkv rows)
  __builtin_amdgcn_sched_barrier(0);
  if (wave == 0) {                           // the chunk's keys and values, quantized while the loads fly
    float s;
    const u32x4 q16 = quantize_head16<T>(st0, st1, s);
    if (kg < 2 * p.m) {
      skv[kg & 1][kg >> 1][part] = q16;
      if (part == 0) sscale[kg & 1][kg >> 1] = s;
    }
  } else if (wave == 1) {
    if ((lane >> 3) < p.m) sq[lane >> 3][lane & 7] = st0;
  }
  const long long pos = *p.pos;
  __syncthreads();
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int key = split * SPLIT_KEYS + ps * 64 + kg;
    const long long off = key - pos;
    const bool own = off >= 0 && off < p.m && key < p.cap;          // a slot of the chunk: row `off` of this cache row
    const int i = own ? (int)off : 0;
    const u32x4 kn = skv[0][i][part], vn = skv[1][i][part];
    const uint32_t kns = __float_as_uint(sscale[0][i]), vns = __float_as_uint(sscale[1][i]);
    const uint32_t mk = own ? 0xffffffffu : 0u;
    kc[ps] = (kc[ps] & ~mk) | (kn & mk);
    vc[ps] = (vc[ps] & ~mk) | (vn & mk);
    ksc[ps] = (ksc[ps] & ~mk) | (kns & mk);
    vsc[ps] = (vsc[ps] & ~mk) | (vns & mk);
    if (own) {                               // stored for the steps to come (by the lanes that loaded this slot)
      *reinterpret_cast<u32x4*>(kq + (size_t)key * HD) = kn;
      *reinterpret_cast<u32x4*>(kq + (plane + key) * HD) = vn;
      if (part == 0) { ks[key] = __uint_as_float(kns); ks[plane + key] = __uint_as_float(vns); }
    }
  }
  for (int j = 0; j < p.m; ++j) {
    float qf[16];
    unpack8<T>(sq[j][2 * part], qf); unpack8<T>(sq[j][2 * part + 1], qf + 8);
    const u32x4 knew = skv[0][j][part], vnew = skv[1][j][part];
    const uint32_t kns = __float_as_uint(sscale[0][j]), vns = __float_as_uint(sscale[1][j]);
    const long long posj = pos + j;
    const long long first = RAGGED ? clamp_first(first_b, posj) : 0;
    float sc[2], m_loc = -INFINITY;
    u32x4 vj[2]; uint32_t vsj[2];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int key = split * SPLIT_KEYS + ps * 64 + kg;
      const bool valid = (!RAGGED || key >= first) && key <= posj && key < p.cap;
      // a slot that query j does not attend takes row j's own bytes and scales: whatever the cache holds there never enters a product
      const uint32_t mk = valid ? 0xffffffffu : 0u;
      const u32x4 k16 = (kc[ps] & mk) | (knew & ~mk);
      vj[ps] = (vc[ps] & mk) | (vnew & ~mk);
      const float kscale = __uint_as_float((ksc[ps] & mk) | (kns & ~mk));
      vsj[ps] = (vsc[ps] & mk) | (vns & ~mk);
      float kf[16]; unpack16_e4m3(k16, kf);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) d = fmaf(qf[e], kf[e], d);
      d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64);                  // the key's 4 lanes
      sc[ps] = valid ? d * kscale * p.scale_l2e : -INFINITY;
      m_loc = fmaxf(m_loc, sc[ps]);
    }
    m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 4, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 8, 64));
    m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 16, 64)); m_loc = fmaxf(m_loc, __shfl_xor(m_loc, 32, 64));
    // (red_m, red_l, red_o and red_p of the previous query were last read before, or by the threads that write them after, its third barrier)
    if (lane == 0) red_m[wave] = m_loc;
    __syncthreads();
    const float m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    float o[16], l = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const float pr = (sc[ps] == -INFINITY) ? 0.f : fast_exp2(sc[ps] - m);
      const float w = pr * __uint_as_float(vsj[ps]);
      float vf[16]; unpack16_e4m3(vj[ps], vf);
      l += pr;
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e] = fmaf(w, vf[e], o[e]);
    }
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4)
      *reinterpret_cast<f32x4*>(&red_o[kg * RED_LD + part * 16 + w4 * 4]) = f32x4{o[4 * w4], o[4 * w4 + 1], o[4 * w4 + 2], o[4 * w4 + 3]};
    if (part == 0) red_l[kg] = l;
    __syncthreads();
    {                                          // 64 key groups -> 4 quarter sums per column, then one: fixed order
      const int c = t & 63, qr = t >> 6;
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) s += red_o[(qr * 16 + g) * RED_LD + c];
      red_p[qr][c] = s;
    }
    __syncthreads();
    float* part_out = partial_of(p.ws, (size_t)b * p.m + j, p.H, head, p.nsplit, split);
    if (t < 64) {
      part_out[2 + t] = (red_p[0][t] + red_p[1][t]) + (red_p[2][t] + red_p[3][t]);
      if (t == 0) {
        float ls = 0.f;
        for (int g = 0; g < 64; ++g) ls += red_l[g];
        part_out[0] = m; part_out[1] = ls;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- host
// What the entry points share of their descriptors.  rows = B * m: the rows of the workspace and of the combine launch.
struct DecodeCall {
  int dtype, B, rows, H, capacity, head_dim;
  const void* qkv; long long qkv_stride; const long long* pos;
  void* out; long long out_stride;
  void* workspace; size_t workspace_bytes; int skip_combine;
  const int* first;
};

inline int nsplit_of(int capacity) { return (capacity + SPLIT_KEYS - 1) / SPLIT_KEYS; }
inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// The shared fields.  head_dim_rc: what a head_dim other than 64 returns (it differs between the entry points: cogview_hip.h).
// dtype and head_dim last: a descriptor refused as unsupported has passed every other check of the entry point.
int decode_check(const DecodeCall& c, int head_dim_rc) {
  if (c.B <= 0 || c.H <= 0 || c.capacity <= 0 || c.capacity > 4096) return COGV_ERR_ARG;
  if (!c.qkv || (!c.out && !c.skip_combine) || !c.pos || !c.workspace) return COGV_ERR_ARG;
  if (misaligned(c.qkv, 16) || (c.qkv_stride & 7) || misaligned(c.workspace, 16) || misaligned(c.first, 4)) return COGV_ERR_ARG;
  if (c.workspace_bytes < cogv_attention_decode_workspace_bytes(c.rows, c.H, c.capacity)) return COGV_ERR_ARG;
  if (c.head_dim != HD) return head_dim_rc;
  if (c.dtype != COGV_F16 && c.dtype != COGV_BF16) return COGV_ERR_UNSUPPORTED;
  return COGV_OK;
}

// The kernel of an argument struct: each kernel has its own.
template <typename T, bool R> constexpr auto decode_kernel(const DecodeArgs&) { return &attn_decode_kernel<T, R>; }
template <typename T, bool R> constexpr auto decode_kernel(const ChunkArgs&) { return &attn_decode_chunk_kernel<T, R>; }
template <typename T, bool R> constexpr auto decode_kernel(const DecodeKv8Args&) { return &attn_decode_kv8_kernel<T, R>; }
template <typename T, bool R> constexpr auto decode_kernel(const ChunkKv8Args&) { return &attn_decode_chunk_kv8_kernel<T, R>; }

// The end of a call: the combine launch (partials in split order -> out) -- or none: skip_combine, the consumer (cogv_gemv_attn /
// cogv_gemv_attn_w8: the attention-output projection of a decode step) recombines the partials itself.
int decode_finish(const DecodeCall& c, hipStream_t st) {
  if (!c.skip_combine) {
    DecodeArgs k = {};
    k.out = c.out; k.ws = reinterpret_cast<float*>(c.workspace);
    k.out_bs = c.out_stride; k.B = c.rows; k.H = c.H; k.nsplit = nsplit_of(c.capacity);
    if (c.dtype == COGV_F16) hipLaunchKernelGGL((attn_decode_combine_kernel<f16_t>), dim3(c.H, c.rows), dim3(64), 0, st, k);
    else hipLaunchKernelGGL((attn_decode_combine_kernel<bf16_t>), dim3(c.H, c.rows), dim3(64), 0, st, k);
  }
  return cogv_check_launch();
}

// Launches KERNEL<T, RAGGED> by (dtype, first != NULL), then finishes the call.
template <typename Args>
int decode_run(const DecodeCall& c, const Args& a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(nsplit_of(c.capacity), c.H, c.B);
  if (c.dtype == COGV_F16) {
    if (c.first) hipLaunchKernelGGL((decode_kernel<f16_t, true>(a)), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((decode_kernel<f16_t, false>(a)), grid, dim3(256), 0, st, a);
  } else {
    if (c.first) hipLaunchKernelGGL((decode_kernel<bf16_t, true>(a)), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((decode_kernel<bf16_t, false>(a)), grid, dim3(256), 0, st, a);
  }
  return decode_finish(c, st);
}

}  // namespace

extern "C" size_t cogv_attention_decode_workspace_bytes(int B, int H, int capacity) {
  if (B <= 0 || H <= 0 || capacity <= 0) return 0;
  return (size_t)B * H * nsplit_of(capacity) * PARTIAL * sizeof(float);
}

extern "C" int cogv_attention_decode(const cogv_attn_decode_desc* d, void* stream) {
  if (!d) return COGV_ERR_UNSUPPORTED;
  const DecodeCall c = {d->dtype, d->B, d->B, d->H, d->capacity, d->head_dim, d->qkv, d->qkv_bs, d->pos, d->out, d->out_bs,
                        d->workspace, d->workspace_bytes, d->skip_combine, d->first};
  if (!d->cache || misaligned(d->cache, 16) || ((d->cache_bs | d->cache_rs) & 7)) return COGV_ERR_ARG;
  if (const int rc = decode_check(c, COGV_ERR_ARG)) return rc;
  DecodeArgs a;
  a.qkv = d->qkv; a.cache = d->cache; a.out = d->out; a.pos = d->pos; a.first = d->first;
  a.tickets = nullptr;
  a.ws = reinterpret_cast<float*>(d->workspace);
  a.qkv_bs = d->qkv_bs; a.cache_bs = d->cache_bs; a.out_bs = d->out_bs; a.cache_rs = d->cache_rs;
  a.B = d->B; a.H = d->H; a.cap = d->capacity; a.nsplit = nsplit_of(d->capacity);
  a.scale_l2e = d->scale * 1.4426950408889634f;
  return decode_run(c, a, stream);
}

extern "C" int cogv_attention_decode_chunk(const cogv_attn_decode_chunk_desc* d, void* stream) {
  if (!d) return COGV_ERR_UNSUPPORTED;
  // (B * m rows go to the workspace query and the combine launch as an int)
  if (d->m < 1 || d->m > MAX_M || (long long)d->B * d->m > (1 << 20)) return COGV_ERR_ARG;
  const DecodeCall c = {d->dtype, d->B, d->B * d->m, d->H, d->capacity, d->head_dim, d->qkv, d->qkv_rs, d->pos, d->out, d->out_rs,
                        d->workspace, d->workspace_bytes, d->skip_combine, d->first};
  if (!d->cache || misaligned(d->cache, 16) || ((d->cache_bs | d->cache_rs) & 7)) return COGV_ERR_ARG;
  if (const int rc = decode_check(c, COGV_ERR_UNSUPPORTED)) return rc;
  ChunkArgs a;
  a.qkv = d->qkv; a.cache = d->cache; a.pos = d->pos; a.first = d->first;
  a.ws = reinterpret_cast<float*>(d->workspace);
  a.qkv_rs = d->qkv_rs; a.cache_bs = d->cache_bs; a.cache_rs = d->cache_rs;
  a.B = d->B; a.H = d->H; a.cap = d->capacity; a.nsplit = nsplit_of(d->capacity); a.m = d->m;
  a.scale_l2e = d->scale * 1.4426950408889634f;
  return decode_run(c, a, stream);
}

extern "C" int cogv_kv_quantize_e4m3(int dtype, const void* kv, long long kv_bs, long long kv_rs, int B, int n, int H, void* q,
                                     long long q_bs, float* scale, long long scale_bs, int capacity, int slot0, void* stream) {
  if (!kv || !q || !scale || B <= 0 || n <= 0 || H <= 0 || capacity <= 0 || slot0 < 0 || (long long)slot0 + n > capacity) return COGV_ERR_ARG;
  if (((uintptr_t)kv & 15) || ((uintptr_t)q & 15) || ((uintptr_t)scale & 3) || ((kv_bs | kv_rs) & 7) || (q_bs & 15)) return COGV_ERR_ARG;
  if (kv_rs < 2LL * H * HD || q_bs < 2LL * H * capacity * HD || scale_bs < 2LL * H * capacity) return COGV_ERR_ARG;
  if (dtype != COGV_F16 && dtype != COGV_BF16) return COGV_ERR_UNSUPPORTED;
  KvQuantArgs a;
  a.kv = kv; a.q = q; a.scale = scale;
  a.kv_bs = kv_bs; a.kv_rs = kv_rs; a.q_bs = q_bs; a.scale_bs = scale_bs;
  a.B = B; a.n = n; a.H = H; a.cap = capacity; a.slot0 = slot0;
  const long long groups = (long long)B * n * 2 * H;
  if (groups > (1LL << 30)) return COGV_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)((groups + 63) / 64));
  if (dtype == COGV_F16) hipLaunchKernelGGL((kv_quantize_e4m3_kernel<f16_t>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((kv_quantize_e4m3_kernel<bf16_t>), grid, dim3(256), 0, st, a);
  return cogv_check_launch();
}

extern "C" int cogv_attention_decode_kv8(const cogv_attn_decode_kv8_desc* d, void* stream) {
  if (!d) return COGV_ERR_ARG;
  const DecodeCall c = {d->dtype, d->B, d->B, d->H, d->capacity, d->head_dim, d->qkv, d->qkv_bs, d->pos, d->out, d->out_bs,
                        d->workspace, d->workspace_bytes, d->skip_combine, d->first};
  if (!d->kv_q || !d->kv_scale || misaligned(d->kv_q, 16) || misaligned(d->kv_scale, 4) || (d->kv_q_bs & 15)) return COGV_ERR_ARG;
  if (d->kv_q_bs < 2LL * d->H * d->capacity * HD || d->kv_scale_bs < 2LL * d->H * d->capacity) return COGV_ERR_ARG;
  if (const int rc = decode_check(c, COGV_ERR_ARG)) return rc;
  DecodeKv8Args a;
  a.qkv = d->qkv; a.q = reinterpret_cast<uint8_t*>(d->kv_q); a.scale = d->kv_scale; a.pos = d->pos; a.first = d->first;
  a.ws = reinterpret_cast<float*>(d->workspace);
  a.qkv_bs = d->qkv_bs; a.q_bs = d->kv_q_bs; a.scale_bs = d->kv_scale_bs;
  a.B = d->B; a.H = d->H; a.cap = d->capacity; a.nsplit = nsplit_of(d->capacity);
  a.scale_l2e = d->scale * 1.4426950408889634f;
  return decode_run(c, a, stream);
}

extern "C" int cogv_attention_decode_chunk_kv8(const cogv_attn_decode_chunk_kv8_desc* d, void* stream) {
  if (!d) return COGV_ERR_UNSUPPORTED;
  // (B * m rows go to the workspace query and the combine launch as an int)
  if (d->m < 1 || d->m > MAX_M || (long long)d->B * d->m > (1 << 20)) return COGV_ERR_ARG;
  const DecodeCall c = {d->dtype, d->B, d->B * d->m, d->H, d->capacity, d->head_dim, d->qkv, d->qkv_rs, d->pos, d->out, d->out_rs,
                        d->workspace, d->workspace_bytes, d->skip_combine, d->first};
  if (!d->kv_q || !d->kv_scale || misaligned(d->kv_q, 16) || misaligned(d->kv_scale, 4) || (d->kv_q_bs & 15)) return COGV_ERR_ARG;
  if (d->kv_q_bs < 2LL * d->H * d->capacity * HD || d->kv_scale_bs < 2LL * d->H * d->capacity) return COGV_ERR_ARG;
  if (const int rc = decode_check(c, COGV_ERR_UNSUPPORTED)) return rc;
  ChunkKv8Args a;
  a.qkv = d->qkv; a.q = reinterpret_cast<uint8_t*>(d->kv_q); a.scale = d->kv_scale; a.pos = d->pos; a.first = d->first;
  a.ws = reinterpret_cast<float*>(d->workspace);
  a.qkv_rs = d->qkv_rs; a.q_bs = d->kv_q_bs; a.scale_bs = d->kv_scale_bs;
  a.B = d->B; a.H = d->H; a.cap = d->capacity; a.nsplit = nsplit_of(d->capacity); a.m = d->m;
  a.scale_l2e = d->scale * 1.4426950408889634f;
  return decode_run(c, a, stream);
}

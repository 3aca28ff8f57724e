// Decode step on an 8-bit key/value cache (cogv_kv_quantize_e4m3, cogv_attention_decode_kv8; generation/decoder.py kv="e4m3").
// The decode attention of attention.hip requests every slot of the fixed-capacity cache on every step, so a step streams the
// whole cache: here the cache holds OCP E4M3 bytes ("e4m3fn": no infinities, largest value 448) with one fp32 scale per
// (slot, head, K | V) -- the rule of e4m3_stream.cuh with the 64 elements of one head of one slot as the group.
// Head-major layout, so that the 128 keys of one split are one contiguous 8-KB block:
//     q     uint8 [B][2][H][capacity][64]      plane 0: keys, plane 1: values
//     scale fp32  [B][2][H][capacity]
// 136 bytes per (slot, head) for its key and value instead of 256.  This unit is separate from attention.hip: the 16-bit kernels compile what
// they always did; the second launch (combine) is attention.hip's, reached through cogv_attn_decode_combine_launch.
#include "e4m3_stream.cuh"
#include "cogview_hip.h"

// attention.hip: the combine launch of a decode step (partials in split order -> out)
extern "C" __attribute__((visibility("hidden"))) int cogv_attn_decode_combine_launch(int dtype, const void* ws, void* out, long long out_bs,
                                                                                     int B, int H, int nsplit, void* stream);

namespace {

constexpr int HD = 64;

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

// ---------------------------------------------------------------------------------------------------- cache quantizer
// The 16-bit K | V rows a prefill leaves, kv [B][n][2 * H * 64] -> slots [slot0, slot0 + n) of q / scale.  Four lanes own one
// (row, head, K | V): 64 of them per workgroup (a 256-thread workgroup per 64 elements is what the weight quantizer on a
// [rows, 64] view would spend).  The maximum crosses the 4 lanes by shuffles: no LDS, no atomics.  Once per layer per prefill.
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

// ---------------------------------------------------------------------------------------------------- decode attention
// attn_decode_kernel (attention.hip) on the 8-bit cache: grid (capacity / 128, H, B), 128 keys per split, the same partial
// (max, sum, 64 outputs) per split -- so the combine launch and the combine prologue of the attention-output GEMV are shared.
// FOUR lanes per key, 16 bytes each (a 64-byte row; a wave's request is one contiguous 1-KB piece of the split's 8-KB block),
// two passes of 64 keys: 2 key + 2 value 16-byte loads and 4 scale loads per lane, all issued before *pos is read.
// The new token's key / value are QUANTIZED FIRST (its 64 elements live in 4 lanes: the maximum crosses them by two shuffles),
// stored into slot *pos as bytes + scale, and the step's own attention uses the dequantized values -- a token's key has one value
// in every step that reads it.  Bytes become fp32 exactly (v_cvt_pk_f32_fp8); the scale multiplies the 64-term dot product (keys)
// and the probability (values): all arithmetic fp32.
// RAGGED (cogv_attn_decode_kv8_desc.first != NULL; a second instantiation): row b attends slots [first[b], *pos], as in
// attn_decode_kernel -- a padding slot takes the new token's bytes and scales through the masks below and a score of -inf.
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
    const int key = split * 128 + ps * 64 + kg;
    // requested whatever *pos says (slots past it hold stale or no data and are replaced below; a key past the capacity re-reads
    // the last row): loads that waited for the position would start one memory latency late
    const int krow = key < p.cap ? key : p.cap - 1;
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
  // first[b] < 0 counts as 0; first[b] > *pos leaves the new token's own slot
  const long long first = RAGGED ? (first_b < 0 ? 0 : (first_b > pos ? pos : (long long)first_b)) : 0;
  float sc[2], m_loc = -INFINITY;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    const int key = split * 128 + ps * 64 + kg;
    const bool valid = (!RAGGED || key >= first) && key <= pos && key < p.cap;
    const bool cached = valid && key != pos;
    // (bit masks, not a select: the compiler turns a select of a loaded value into a branch and sinks the load into it).  Every
    // slot that is not a cached one takes the new token's bytes and scales: whatever the cache holds there never enters a product
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
    const float pr = (sc[ps] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(sc[ps] - m);
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
  float* part_out = p.ws + (((size_t)b * p.H + head) * p.nsplit + split) * 66;
  if (t < 64) {
    part_out[2 + t] = (red_p[0][t] + red_p[1][t]) + (red_p[2][t] + red_p[3][t]);
    if (t == 0) {
      float ls = 0.f;
      for (int g = 0; g < 64; ++g) ls += red_l[g];
      part_out[0] = m; part_out[1] = ls;
    }
  }
}

}  // namespace

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
  if (d->B <= 0 || d->H <= 0 || d->capacity <= 0 || d->capacity > 4096 || d->head_dim != HD) return COGV_ERR_ARG;
  if (!d->qkv || !d->kv_q || !d->kv_scale || (!d->out && !d->skip_combine) || !d->pos || !d->workspace) return COGV_ERR_ARG;
  if (((uintptr_t)d->qkv & 15) || ((uintptr_t)d->kv_q & 15) || ((uintptr_t)d->kv_scale & 3) || (d->qkv_bs & 7) || (d->kv_q_bs & 15)) return COGV_ERR_ARG;
  if (d->kv_q_bs < 2LL * d->H * d->capacity * HD || d->kv_scale_bs < 2LL * d->H * d->capacity) return COGV_ERR_ARG;
  if (d->workspace_bytes < cogv_attention_decode_workspace_bytes(d->B, d->H, d->capacity) || ((uintptr_t)d->workspace & 15)) return COGV_ERR_ARG;
  if ((uintptr_t)d->first & 3) return COGV_ERR_ARG;
  if (d->dtype != COGV_F16 && d->dtype != COGV_BF16) return COGV_ERR_UNSUPPORTED;
  DecodeKv8Args a;
  a.qkv = d->qkv; a.q = reinterpret_cast<uint8_t*>(d->kv_q); a.scale = d->kv_scale; a.pos = d->pos; a.first = d->first;
  a.ws = reinterpret_cast<float*>(d->workspace);
  a.qkv_bs = d->qkv_bs; a.q_bs = d->kv_q_bs; a.scale_bs = d->kv_scale_bs;
  a.B = d->B; a.H = d->H; a.cap = d->capacity; a.nsplit = (d->capacity + 127) / 128;
  a.scale_l2e = d->scale * 1.4426950408889634f;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid(a.nsplit, a.H, a.B);
  if (d->dtype == COGV_F16) {
    if (a.first) hipLaunchKernelGGL((attn_decode_kv8_kernel<f16_t, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_decode_kv8_kernel<f16_t>), grid, dim3(256), 0, st, a);
  } else {
    if (a.first) hipLaunchKernelGGL((attn_decode_kv8_kernel<bf16_t, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((attn_decode_kv8_kernel<bf16_t>), grid, dim3(256), 0, st, a);
  }
  // skip_combine: the consumer (cogv_gemv_attn / cogv_gemv_attn_w8) recombines the partials itself
  if (!d->skip_combine) return cogv_attn_decode_combine_launch(d->dtype, d->workspace, d->out, d->out_bs, a.B, a.H, a.nsplit, stream);
  return cogv_check_launch();
}

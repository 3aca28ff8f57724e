// The 8-bit format of the decode step (weights: quantize.hip, gemv.hip; key/value cache: attention_decode.hip) and the load its
// streams are read with.  One place for both: the producers and the consumers below agree to the bit because they call these.
//
// THE E4M3 RULE.  A group of elements (a weight row; the 64 elements of one head of one cache slot) becomes OCP E4M3 bytes
// ("e4m3fn": no infinities, largest value 448) and one fp32 scale:
//     scale = max |x| / 448                    (fp32 division; 1.0 for an all-zero group)
//     q     = rne_e4m3( float(x) / scale )     (a true fp32 division, not a reciprocal multiply: a CPU reproduces the bytes with
//                                               the same two operations)
// |x| / scale exceeds 448 by fp32 rounding error at most, which still rounds to 448: no value leaves the representable range.
// Byte order: element i of a group is byte i (v_cvt_pk_fp8_f32 fills the low half of a word from two floats, then the high half).
// Back to fp32 the bytes are exact (v_cvt_pk_f32_fp8: two bytes of the selected half per instruction).
#pragma once
#include "common.cuh"

#define COGV_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ float e4m3_scale(float amax) { return amax == 0.f ? 1.0f : amax / 448.0f; }

// four floats -> one word of four E4M3 bytes
__device__ __forceinline__ uint32_t pack4_e4m3(float a, float b, float c, float d) {
  int x = 0;
  x = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, x, false);
  x = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, x, true);
  return (uint32_t)x;
}

// 8 E4M3 bytes -> 8 floats
__device__ __forceinline__ void unpack8_e4m3(uint32_t lo, uint32_t hi, float* f) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1]; f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}
__device__ __forceinline__ void unpack16_e4m3(const u32x4& q, float* f) {
  unpack8_e4m3(q[0], q[1], f);
  unpack8_e4m3(q[2], q[3], f + 8);
}

// STREAMED-ONCE DATA (the weight rows and the cache rows of a decode step: every byte is read by ONE workgroup, once per token):
// the non-temporal policy (global_load_dwordx4 ... nt) keeps the stream from displacing the step's small reused vectors in the
// caches.  Measured in the captured 4B decode step (profiles/r05_decode_nt_ab.log): one row (gemv.hip's FormV, a wave streams
// whole weight rows) 2.78 -> 2.69 ms per token; 2 / 4 rows (FormM: the 16 lanes of a 16 x 16 fragment read 16 different rows,
// 16 bytes each per step) 3.06 -> 3.50 and 3.74 -> 4.23 ms -- so FormV and the decode attention's cache rows take it, FormM
// keeps the default policy.  COGV_DECODE_NT=0 builds default-policy loads everywhere.
#ifndef COGV_DECODE_NT
#define COGV_DECODE_NT 1
#endif
template <typename V>
__device__ __forceinline__ V ld_stream(const void* q) {
#if COGV_DECODE_NT
  return __builtin_nontemporal_load((const COGV_GLOBAL V*)q);
#else
  return *(const COGV_GLOBAL V*)q;
#endif
}

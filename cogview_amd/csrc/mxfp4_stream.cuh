// The 4-bit format of the decode step's weight stream (producer: quantize.hip; consumer: gemv.hip's W4 operand): OCP MXFP4.  One
// place for both, in the role e4m3_stream.cuh has for the 8-bit format.
//
// THE MXFP4 RULE.  32 consecutive elements of a weight row (a block) become 16 bytes of E2M1 codes and one E8M0 scale byte:
//     amax = max |x| over the block
//     e    = clamp(floor(log2(amax)) - 2, -126, 127),  s = e + 127      (all-zero block: s = 127; s is never 0 and never 255)
//     code = E2M1 nearest to float(x) / 2^e, ties to the even code, magnitudes above 6 saturate to 6
// A nibble is the sign (bit 3) and a 3-bit code of the magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}; element 2i of a block is the low
// nibble of byte i, element 2i + 1 the high one.  (uint32)s << 23 is the scale 2^(s - 127) as an fp32 bit pattern.
// The producer takes the rule on BIT PATTERNS (integer compares, no division, no rounding mode, no denormal mode): a CPU reproduces
// it with the same integer operations (tests/w4_cases.py).  With |x| = M * 2^(E - 150) (E the biased fp32 exponent, M the
// significand with its hidden bit; E = 1 without one for a subnormal), 4 |x| / 2^e = M / 2^r, r = s + 21 - E, and the seven code
// boundaries 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 are the integers 1, 3, 5, 7, 10, 14, 20 there; a tie goes to the even code, i.e.
// the boundaries below codes 1, 3, 5, 7 belong to the code below them (>) and the others to the code above (>=).
// The consumers convert two codes per instruction with the block scale folded in (v_cvt_scalef32_pk_{f32,f16,bf16}_fp4): code *
// 2^e is exact in fp32 and bf16, and in fp16 wherever it is a multiple of 2^-24 below 65520.
#pragma once
#include "common.cuh"

// the scale byte of a block from the bit pattern of its abs-max (sign bit clear)
__device__ __forceinline__ uint32_t mxfp4_scale_byte(uint32_t amax_bits) {
  const int ea = (int)(amax_bits >> 23);
  return amax_bits == 0u ? 127u : (uint32_t)(ea - 2 > 1 ? ea - 2 : 1);
}

// one element (fp32 bit pattern) -> its nibble under the block's scale byte s
__device__ __forceinline__ uint32_t mxfp4_code(uint32_t bits, uint32_t s) {
  const uint32_t mag = bits & 0x7fffffffu;
  const int E = (int)(mag >> 23);
  const uint32_t M = E ? ((mag & 0x7fffffu) | 0x800000u) : mag;
  int r = (int)s + 21 - (E ? E : 1);
  r = r < 0 ? 0 : (r > 26 ? 26 : r);            // r >= 19 by the choice of s; from 25 on every M < 2^24 is below the first boundary
  const uint32_t c = (uint32_t)(M > (1u << r)) + (uint32_t)(M >= (3u << r)) + (uint32_t)(M > (5u << r)) + (uint32_t)(M >= (7u << r)) +
                     (uint32_t)(M > (10u << r)) + (uint32_t)(M >= (14u << r)) + (uint32_t)(M > (20u << r));
  return ((bits >> 28) & 8u) | c;
}

// 8 consecutive elements -> one word of 8 nibbles (element i in bits 4i .. 4i + 3)
__device__ __forceinline__ uint32_t pack8_mxfp4(const float* f, uint32_t s) {
  uint32_t w = 0u;
#pragma unroll
  for (int i = 0; i < 8; ++i) w |= mxfp4_code(__float_as_uint(f[i]), s) << (4 * i);
  return w;
}

// the block scale as the fp32 the conversions take
__device__ __forceinline__ float mxfp4_scale_f32(uint32_t s) { return __uint_as_float(s << 23); }

// one word of 8 nibbles -> 8 elements of the storage type (an MFMA fragment's 16 bytes), scale folded in
template <typename T> __device__ __forceinline__ u32x4 unpack8_mxfp4_to(uint32_t w, float scale);
template <> __device__ __forceinline__ u32x4 unpack8_mxfp4_to<f16_t>(uint32_t w, float scale) {
  return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 0)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 1)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 2)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, 3))};
}
template <> __device__ __forceinline__ u32x4 unpack8_mxfp4_to<bf16_t>(uint32_t w, float scale) {
  return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3))};
}

// one word of 8 nibbles -> 8 floats, scale folded in
__device__ __forceinline__ void unpack8_mxfp4(uint32_t w, float scale, float* f) {
  const f32x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 0), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 1);
  const f32x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 2), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 3);
  f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1]; f[4] = c[0]; f[5] = c[1]; f[6] = d[0]; f[7] = d[1];
}

// The weight quantizers of the decode step's weight stream: E4M3 rows (below) and MXFP4 blocks (at the end of the file).
// Row-wise 8-bit weight quantizer of the decode step's weight stream (cogv_quantize_rows_e4m3; consumed by the 8-bit operand of
// gemv.hip).  W[N][K] in the 16-bit storage type -> q[N][K] as OCP E4M3 bytes and one fp32 scale per row: the rule of
// e4m3_stream.cuh with a row as the group.
// One workgroup per row, two passes over it (the second is served by L2); the row maximum is taken on the bit patterns and
// reduced through LDS in a fixed order -- no atomics.  Runs once per weight matrix when a decoder is built: not a hot path.
#include "e4m3_stream.cuh"
#include "mxfp4_stream.cuh"
#include "cogview_hip.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void quantize_rows_e4m3_kernel(const T* __restrict__ w, int ldw, int K, uint8_t* __restrict__ q, int ldq,
                                                                 float* __restrict__ scale) {
  __shared__ uint32_t redm[16];
  const int n = blockIdx.x, nvec = K >> 3;
  const T* row = w + (size_t)n * ldw;
  uint32_t m = 0u;
  for (int v = threadIdx.x; v < nvec; v += 256) m = absmax_pk8(m, *reinterpret_cast<const u32x4*>(row + v * 8));
  const float amax = absmax_pk_block<T>(m, redm);
  const float s = e4m3_scale(amax);
  if (threadIdx.x == 0) scale[n] = s;
  uint8_t* qrow = q + (size_t)n * ldq;
  for (int v = threadIdx.x; v < nvec; v += 256) {
    float f[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(row + v * 8), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = f[i] / s;
    *reinterpret_cast<u32x2*>(qrow + v * 8) = u32x2{pack4_e4m3(f[0], f[1], f[2], f[3]), pack4_e4m3(f[4], f[5], f[6], f[7])};
  }
}

// The 4-bit quantizer (cogv_quantize_rows_mxfp4; consumed by the 4-bit operand of gemv.hip): the rule of mxfp4_stream.cuh.  One
// workgroup per row; a lane owns 8 elements, four neighbouring lanes one block of 32: its abs-max is taken on the bit patterns
// across the four lanes (no atomics), every lane writes its word of 8 codes and the first of the four the scale byte.
template <typename T>
__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(const T* __restrict__ w, int ldw, int K, uint8_t* __restrict__ q, int ldq,
                                                                  uint8_t* __restrict__ scale, int lds) {
  const int n = blockIdx.x, nvec = K >> 3;                  // K % 32 == 0: the four lanes of a block are in or out together
  const T* row = w + (size_t)n * ldw;
  for (int v = threadIdx.x; v < nvec; v += 256) {
    float f[8];
    unpack8<T>(*reinterpret_cast<const u32x4*>(row + v * 8), f);
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = max(m, __float_as_uint(f[i]) & 0x7fffffffu);
    m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
    m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
    const uint32_t s = mxfp4_scale_byte(m);
    *reinterpret_cast<uint32_t*>(q + (size_t)n * ldq + v * 4) = pack8_mxfp4(f, s);
    if ((v & 3) == 0) scale[(size_t)n * lds + (v >> 2)] = (uint8_t)s;
  }
}

}  // namespace

extern "C" int cogv_quantize_rows_mxfp4(int dtype, const void* w, int ldw, int N, int K, void* q, int ldq, void* scale, int lds, void* stream) {
  if (!w || !q || !scale || N <= 0 || K <= 0) return COGV_ERR_ARG;
  if ((K & 31) || (ldw & 7) || (ldq & 3) || ldw < K || ldq < K / 2 || lds < K / 32 || ((uintptr_t)w & 15) || ((uintptr_t)q & 3)) return COGV_ERR_ARG;
  if (dtype != COGV_F16 && dtype != COGV_BF16) return COGV_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == COGV_F16)
    hipLaunchKernelGGL((quantize_rows_mxfp4_kernel<f16_t>), dim3(N), dim3(256), 0, st, reinterpret_cast<const f16_t*>(w), ldw, K,
                       reinterpret_cast<uint8_t*>(q), ldq, reinterpret_cast<uint8_t*>(scale), lds);
  else
    hipLaunchKernelGGL((quantize_rows_mxfp4_kernel<bf16_t>), dim3(N), dim3(256), 0, st, reinterpret_cast<const bf16_t*>(w), ldw, K,
                       reinterpret_cast<uint8_t*>(q), ldq, reinterpret_cast<uint8_t*>(scale), lds);
  return cogv_check_launch();
}

extern "C" int cogv_quantize_rows_e4m3(int dtype, const void* w, int ldw, int N, int K, void* q, int ldq, float* scale, void* stream) {
  if (!w || !q || !scale || N <= 0 || K <= 0) return COGV_ERR_ARG;
  if ((K & 7) || (ldw & 7) || (ldq & 7) || ldw < K || ldq < K || ((uintptr_t)w & 15) || ((uintptr_t)q & 7) || ((uintptr_t)scale & 3)) return COGV_ERR_ARG;
  if (dtype != COGV_F16 && dtype != COGV_BF16) return COGV_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == COGV_F16)
    hipLaunchKernelGGL((quantize_rows_e4m3_kernel<f16_t>), dim3(N), dim3(256), 0, st, reinterpret_cast<const f16_t*>(w), ldw, K,
                       reinterpret_cast<uint8_t*>(q), ldq, scale);
  else
    hipLaunchKernelGGL((quantize_rows_e4m3_kernel<bf16_t>), dim3(N), dim3(256), 0, st, reinterpret_cast<const bf16_t*>(w), ldw, K,
                       reinterpret_cast<uint8_t*>(q), ldq, scale);
  return cogv_check_launch();
}

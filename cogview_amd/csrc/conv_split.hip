// Split-bf16 form of the tokenizer's implicit-GEMM convolution (COGV_CONV_BF16X3, see cogv_conv_desc in cogview_hip.h): the
// layers of conv.hip -- same tap arithmetic (conv_taps.cuh), same NHWC fp32 activations, same packed weights
// [parity][Cout][tap][Cin], same descriptor checks and grid (conv_args.cuh), and the very same tile walk, activation staging
// and epilogue (conv_tile.cuh, one copy for both kernels) -- on v_mfma_f32_32x32x16_bf16 instead of the exact-fp32
// v_mfma_f32_32x32x2_f32.
//
// Arithmetic.  Every fp32 operand x is the exact sum of three bf16 limbs, x = x0 + x1 + x2, made by truncation: x0 = the top
// 16 bits of x, x1 = the top 16 bits of (x - x0), x2 = the top 16 bits of (x - x0 - x1).  Each subtraction is exact and the
// three limbs carry 8 significand bits each = the 24 of an fp32 value; nothing is rounded up, so nothing overflows near
// FLT_MAX.  A product x*y is replaced by the six limb products x_i*y_j with i + j <= 2 (each exact in fp32); what is dropped
// (x1y2, x2y1, x2y2) is below 2^-21 |x*y| in the worst case and about 2^-25 |x*y| rms.
//   Per MFMA k-step the products are issued smallest first, (2,0) (1,1) (0,2) (1,0) (0,1) (0,0) -- a fixed order, so two runs
// give the same bits -- into TWO accumulator sets: the five small products into `lo`, x0*y0 into `hi`, added once in front
// of the epilogue.  Every accumulation rounds to the accumulator's own magnitude: in one set the five small products of a
// k-step would each cost the sum a full fp32 rounding (6 roundings per 16 k, which at K = 8192 is most of a 1e-6 budget);
// apart, `hi` rounds once per 16 k and the roundings of `lo` are 2^-7 smaller.
//   Weights are split once (cogv_conv_split_weights, when they are packed) into three bf16 planes and go from global memory
// to LDS as they are; activations are split when their fp32 registers are parked in LDS (after relu_in and the zero-fill
// of taps outside the image, rows past M and channels past the tensor).
//
// Tile 128 pixels x 128 channels x 32 k, 4 waves, 2x2 MFMA 32x32 per wave, as conv.hip.  LDS: an operand tile is three limb
// planes of 128 rows x 64 B (32 bf16, k contiguous), 24 KiB; A + B = one 48-KiB stage, filled between two barriers from
// registers that were loaded before the tile's MFMAs.  With the epilogue's 64-KiB C tile that is two workgroups per CU, and
// the second one's MFMAs run under the first one's split and LDS traffic: measured 1.3-1.4x the exact kernel end to end,
// against 1.12x for the double-buffered 96-KiB form (one workgroup per CU, one wave per SIMD, nothing to overlap).  A lane's
// 8 k-values of one limb are one ds_read_b128; the 16-byte chunk index is XORed with (row >> 2) & 3, which spreads each of
// the four 16-lane groups a ds_read_b128 is served in over all 64 banks (rows are 16 banks apart, 4 rows wrap around).
// C/D lane map of 32x32x16_bf16 = that of 32x32x2_f32, so both kernels store their accumulators into the C tile the same
// way and share one epilogue (conv_epilogue, conv_tile.cuh).
#include "common.cuh"
#include "cogview_hip.h"
#include "conv_tile.cuh"

namespace {

constexpr int PLANE = BM * BK * 2;       // bytes of one limb plane of an operand tile (128 rows x 32 bf16)
constexpr int OPER = 3 * PLANE;          // one operand tile: three planes
constexpr int SMEM = BM * BN * 4;        // one stage (48 KiB) during the k-loop; the epilogue's C tile needs 64 KiB

struct SplitArgs {
  ConvArgs c;
  const uint16_t* wl;        // limb planes of c.w: plane p at wl + p * plane
  long long plane;           // elements per plane = nz * Cout * K
};

__device__ __forceinline__ int swz(int row) { return (row >> 2) & 3; }

// Operand staging: thread t -> (tile row t/8 + 32 q for q = 0..3, 4 consecutive k = piece t%8 of the 32-k slice).  The
// activation side (RowCtx, make_a_ctx, load_a) is conv_tile.cuh's, with loads the compiler tracks; the weight side reads limb planes.
// Every load is unconditional, from a clamped (always valid) address; what lies outside is zeroed when it is parked in LDS.
struct WRowCtx {
  long long wrow[4];         // element index of row q's first weight inside a plane
  uint32_t valid;            // bit q: the row exists (n < Cout)
};
__device__ __forceinline__ WRowCtx make_b_ctx(const ConvArgs& p, int z, int n0) {
  WRowCtx c; c.valid = 0u;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + (t >> 3) + 32 * q;
    const bool ok = n < p.Cout;
    c.wrow[q] = (long long)z * p.w_parity_stride + (long long)(ok ? n : 0) * p.K;
    c.valid |= ok ? (1u << q) : 0u;
  }
  return c;
}
// B tile: 128 weight rows x 32 k, three planes of bf16; piece = 4 k = 8 bytes (K % 4 == 0 keeps every piece inside its row
// and 8-byte aligned).  A piece past the row's K columns loads the row start instead and is zeroed when parked.
__device__ __forceinline__ uint32_t load_b(const SplitArgs& s, const WRowCtx& c, int k0, u32x2 (&r)[4][3]) {
  const int kc = k0 + (threadIdx.x & 7) * 4;
  const bool kok = kc < s.c.K;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int l = 0; l < 3; ++l)
      r[q][l] = *reinterpret_cast<const u32x2*>(s.wl + l * s.plane + c.wrow[q] + (kok ? kc : 0));
  return kok ? c.valid : 0u;
}
__device__ __forceinline__ int piece_addr(int row, int t) {       // byte offset inside a plane of thread t's 8-byte piece of `row`
  return row * 64 + (((((t & 7) >> 1) ^ swz(row)) << 4) | ((t & 1) << 3));
}
// the truncating three-limb split of x: h[l] holds limb l in its top 16 bits (the low bits are whatever remained)
__device__ __forceinline__ void split3(float x, uint32_t (&h)[3]) {
  h[0] = __float_as_uint(x);
  const float r1 = x - __uint_as_float(h[0] & 0xffff0000u);
  h[1] = __float_as_uint(r1);
  const float r2 = r1 - __uint_as_float(h[1] & 0xffff0000u);
  h[2] = __float_as_uint(r2);
}
__device__ __forceinline__ void store_a(char* lds, const f32x4 (&r)[4], uint32_t keep, bool relu) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = (t >> 3) + 32 * q;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 v = ((keep >> q) & 1u) ? r[q] : zero;
    if (relu) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
    }
    uint32_t h[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3(v[i], h[i]);
    const int a = piece_addr(row, t);
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      u32x2 w;
      w[0] = (h[0][l] >> 16) | (h[1][l] & 0xffff0000u);
      w[1] = (h[2][l] >> 16) | (h[3][l] & 0xffff0000u);
      *reinterpret_cast<u32x2*>(lds + l * PLANE + a) = w;
    }
  }
}
__device__ __forceinline__ void store_b(char* lds, const u32x2 (&r)[4][3], uint32_t keep) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = (t >> 3) + 32 * q;
    const int a = piece_addr(row, t);
    const bool k = (keep >> q) & 1u;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
      const u32x2 zero = {0u, 0u};
      *reinterpret_cast<u32x2*>(lds + l * PLANE + a) = k ? r[q][l] : zero;
    }
  }
}
// lane (row fr, half fg) of MFMA k-step s reads the 8 k-values 8 * (2 s + fg) .. + 7 of its row: A and B use the same
// relabelling of k, which is all a contraction needs
__device__ __forceinline__ bf16x8 frag(const char* plane, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(plane + row * 64 + ((chunk ^ swz(row)) << 4));
}

// one k-tile (32 k = two MFMA k-steps) for a wave's 64x64 sub-tile: per k-step the five small limb products into `lo`, then
// x0*y0 into `hi`.  Consecutive MFMAs write different accumulators (4 independent chains).
__device__ __forceinline__ void mma_tile(const char* la, const char* lb, int wm, int wn, int fr, int fg, f32x16 (&hi)[2][2],
                                         f32x16 (&lo)[2][2]) {
  bf16x8 fa[2][2][3], fb[2][2][3];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        fa[s][i][l] = frag(la + l * PLANE, wm + 32 * i + fr, 2 * s + fg);
        fb[s][i][l] = frag(lb + l * PLANE, wn + 32 * i + fr, 2 * s + fg);
      }
  constexpr int PA[6] = {2, 1, 0, 1, 0, 0}, PB[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int pr = 0; pr < 6; ++pr)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
        {
          f32x16& acc = pr == 5 ? hi[i][j] : lo[i][j];
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s][i][PA[pr]], fb[s][j][PB[pr]], acc, 0, 0, 0);
        }
}

template <bool UT>      // UT: Cin % 32 == 0 (every k-tile lies inside one tap)
__global__ __launch_bounds__(NT, 2) void conv_split_kernel(const SplitArgs s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ConvArgs& p = s.c;
  const ConvTile tile = conv_tile(p);               // conv_tile.cuh: the XCD-aware walk of the one-dimensional grid
  if (!tile.live) return;
  const int z = tile.z(), m0 = tile.m0(), n0 = tile.n0(z), wm = tile.wm(), wn = tile.wn(), fr = tile.fr(), fg = tile.fg();

  f32x16 acc[2][2], lo[2][2];             // acc: the x0*y0 sums (`hi`), lo: the five small products
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = lo[i][j][e] = 0.f;

  const int nk = (p.K + BK - 1) / BK;
  const RowCtx actx = make_a_ctx(p, m0);
  const WRowCtx bctx = make_b_ctx(p, z, n0);
  const bool relu_in = p.relu_in != 0;
  // one k-tile in flight in registers: the loads of tile kt+1 are issued before the MFMAs of tile kt and parked in the
  // (single) LDS stage after them, between two barriers -- the CU's second workgroup runs its MFMAs meanwhile; the tile
  // index is clamped, so the last iteration parks a copy nobody reads
  f32x4 ra[4]; u32x2 rb[4][3];
  uint32_t ka = load_a<UT, false>(p, actx, z, 0, ra), kb = load_b(s, bctx, 0, rb);
  store_a(smem, ra, ka, relu_in); store_b(smem + OPER, rb, kb);
  __syncthreads();
#pragma unroll 1
  for (int kt = 0; kt < nk; ++kt) {
    const int k1 = min(kt + 1, nk - 1) * BK;
    ka = load_a<UT, false>(p, actx, z, k1, ra); kb = load_b(s, bctx, k1, rb);
    mma_tile(smem, smem + OPER, wm, wn, fr, fg, acc, lo);
    __syncthreads();
    store_a(smem, ra, ka, relu_in); store_b(smem + OPER, rb, kb);
    __syncthreads();
  }
  // the two accumulator sets are joined on their way into the C tile; from there on the epilogue is conv_tile.cuh's
  float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        ct[(wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fg) * BN + wn + 32 * j + fr] = acc[i][j][e] + lo[i][j][e];
  conv_epilogue(p, ct, z, m0, n0);
}

// w[n] -> three planes of bf16 bits (see cogv_conv_split_weights)
__global__ __launch_bounds__(256) void split_weights_kernel(const float* w, uint16_t* limbs, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t h[3];
    split3(w[i], h);
#pragma unroll
    for (int l = 0; l < 3; ++l) limbs[(size_t)l * n + i] = (uint16_t)(h[l] >> 16);
  }
}

}  // namespace

// the COGV_CONV_BF16X3 launch of cogv_conv2d_nhwc_f32 (conv.hip calls it with a descriptor it has checked)
int cogv_conv_split_launch(const cogv_conv_desc* d, void* stream) {
  SplitArgs s;
  long long blocks = 0;
  const int rc = conv_fill_args(d, s.c, blocks);
  if (rc != COGV_OK) return rc;
  if (d->precision != COGV_CONV_BF16X3) return COGV_ERR_ARG;
  s.wl = reinterpret_cast<const uint16_t*>(d->w_limbs);
  s.plane = (long long)s.c.nz * s.c.w_parity_stride;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_split_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_split_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
    attr = true;
  }
  if (s.c.Cin % BK == 0) hipLaunchKernelGGL(conv_split_kernel<true>, dim3((unsigned)blocks), dim3(NT), SMEM, reinterpret_cast<hipStream_t>(stream), s);
  else hipLaunchKernelGGL(conv_split_kernel<false>, dim3((unsigned)blocks), dim3(NT), SMEM, reinterpret_cast<hipStream_t>(stream), s);
  return cogv_check_launch();
}

extern "C" int cogv_conv_split_weights(const float* w, void* limbs, size_t n, void* stream) {
  if (!w || !limbs || n == 0 || (n & 3) || ((uintptr_t)limbs & 15) || ((uintptr_t)w & 3)) return COGV_ERR_ARG;
  size_t blocks = (n + 255) / 256; if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(split_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w,
                     reinterpret_cast<uint16_t*>(limbs), n);
  return cogv_check_launch();
}

// VQ-VAE tokenizer kernels (reference vqvae/vqvae_zc.py, production config vqvae/api.py:12-20:
// channel 512, embed_dim 256, n_embed 8192, stride 6 -> three 4x4 stride-2 convs + 1x1, quantise,
// three 4x4 stride-2 transposed convs + 1x1).  gfx950, fp32 end to end.
//
// Why fp32: the reference runs the tokenizer in fp32 and the token id is an argmin over fp32 distances; the
// north star asks for ids that match the CPU path.  CDNA4 has an exact-fp32 MFMA (v_mfma_f32_32x32x2_f32,
// 157 TFLOP/s peak = 16x below bf16 MFMA, bit-for-bit an fmaf chain), so the convolutions stay on the matrix
// cores without giving up fp32 products/accumulation.  Only the summation ORDER differs from the CPU path.
//
// One implicit-GEMM kernel covers every layer through a tap table:
//     out[b, y*om+oy, x*om+ox, co] = act( bias[co] + sum_t sum_ci in[b, y*im+dy[t], x*im+dx[t], ci] * W[co][t][ci] )
//   4x4 stride-2 pad-1 conv   : im=2, om=1, 16 taps (dy,dx) = (ky-1, kx-1)
//   1x1 conv                  : im=1, om=1, 1 tap
//   4x4 stride-2 pad-1 convT  : 4 output parities (blockIdx.z), each a 2x2-tap conv at input resolution
//                               (sub-pixel decomposition), im=1, om=2
// Activations are NHWC fp32 (channels contiguous = the contraction index contiguous), weights are repacked
// once on the host side to [parity][Cout][tap][Cin].  Tile 128 pixels x 128 channels x 32 (k), 4 waves,
// 2x2 MFMA 32x32 per wave, LDS rows of 128 B with the same XOR swizzle as the 16-bit GEMM.
// The k-slot relabelling trick (attention.hip) lets one ds_read_b128 feed four MFMA k-steps.
#include "common.cuh"
#include "cogview_hip.h"
#include "conv_tile.cuh"

#include <cstdlib>
#include <type_traits>

namespace {

// BM / BN / BK / NT, ConvArgs and conv_fill_args (descriptor -> arguments, every refusal): conv_args.cuh
// tap_offset(kind, z, tap, dy, dx): conv_taps.cuh (shared with the weight gradient, conv_bwd.hip)
// ld4 / ld4_async, ConvTile / conv_tile, RowCtx / make_a_ctx / load_a and conv_epilogue: conv_tile.cuh (shared with conv_split.hip)

__device__ __forceinline__ int swz(int row) { return ((row >> 1) & 7) ^ ((row >> 4) & 7); }

// all asynchronous loads retired; the operands tie BOTH register sets to the wait, so that the compiler cannot reuse
// a register an in-flight load still targets (found by build.py's asm_load_hazards: the epilogue's address arithmetic
// had been scheduled into those registers in front of a bare s_waitcnt)
__device__ __forceinline__ void drain_loads(f32x4 (&a)[4], f32x4 (&b)[4], f32x4 (&c)[4], f32x4 (&d)[4]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                 "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3])
               : : "memory");
}
template <int N>
__device__ __forceinline__ void wait_loads(f32x4 (&a)[4], f32x4 (&b)[4]) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
               : "n"(N) : "memory");
}

// a RowCtx over the rows of a row-major [N][ldw] matrix (the weights; x and E^T in the nearest-code search): base = row
// start, valid = n < N, no pixel coordinates
__device__ __forceinline__ RowCtx make_b_ctx(const float* w, int ldw, int n0, int N) {
  RowCtx c; c.valid = 0u;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + (t >> 3) + 32 * q;
    const bool ok = n < N;
    c.base[q] = w + (size_t)(ok ? n : 0) * ldw;          // row start; the lane's 16-byte chunk is added by load_b
    c.y0[q] = c.x0[q] = 0;
    c.valid |= ok ? (1u << q) : 0u;
  }
  return c;
}
// B tile: 128 rows x 32 k from a row-major [N][ldw] matrix (weights W[z][co][K]; x / E^T in the nearest-code search)
__device__ __forceinline__ uint32_t load_b(const RowCtx& c, int k0, int K, f32x4 (&r)[4]) {
  // a chunk past the row's K columns (K < 32 or K % 32 != 0) loads the ROW START instead (zeroed when parked): the
  // round-2 form added the chunk offset even then and read up to 112 bytes past the end of the matrix from its last row
  // -- a memory fault whenever that matrix ended a mapped segment (found in round 3: the 64 x 16 codebook of the small
  // golden model aborted the whole GPU suite in one particular allocation order)
  const int kc = k0 + (threadIdx.x & 7) * 4;
  const bool kok = kc < K;
#pragma unroll
  for (int q = 0; q < 4; ++q) ld4_async(r[q], c.base[q] + (kok ? kc : 0));
  return kok ? c.valid : 0u;
}
__device__ __forceinline__ void store_tile(char* lds, const f32x4 (&r)[4], uint32_t keep, bool relu = false) {
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
    *reinterpret_cast<f32x4*>(lds + row * 128 + (((t & 7) ^ swz(row)) << 4)) = v;
  }
}
__device__ __forceinline__ f32x4 frag(const char* lds, int row, int chunk) {
  return *reinterpret_cast<const f32x4*>(lds + row * 128 + ((chunk ^ swz(row)) << 4));
}

// one k-tile (32 floats) of MFMAs for a wave's 64x64 sub-tile.  The fragments of k-block kb+1 are read into a second
// register set BEFORE the 16 MFMAs of k-block kb (the compiler's own order reused one set and exposed the LDS latency
// four times per k-tile); the scheduling barriers pin that order.
__device__ __forceinline__ void mma_tile(const char* la, const char* lb, int wm, int wn, int fr, int fg,
                                         f32x16 (&acc)[2][2]) {
  f32x4 fa[2][2], fb[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) { fa[0][i] = frag(la, wm + 32 * i + fr, fg); fb[0][i] = frag(lb, wn + 32 * i + fr, fg); }
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {          // 8 k per step: lanes g=0 take slots 0..3, g=1 slots 4..7
    const int c = kb & 1;
    if (kb + 1 < 4) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[c ^ 1][i] = frag(la, wm + 32 * i + fr, 2 * (kb + 1) + fg);
        fb[c ^ 1][i] = frag(lb, wn + 32 * i + fr, 2 * (kb + 1) + fg);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i][s], fb[c][j][s], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool UT, int EXP = 0>      // UT: Cin % 32 == 0 (every k-tile lies inside one tap); EXP: timing probes (wrong results)
__global__ __launch_bounds__(NT, 2) void conv_kernel(const ConvArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];     // 2 stages x (A 16K + B 16K) = 64 KiB
  const ConvTile tile = conv_tile(p);               // conv_tile.cuh: the XCD-aware walk of the one-dimensional grid
  if (!tile.live) return;
  const int z = tile.z(), m0 = tile.m0(), n0 = tile.n0(z), wm = tile.wm(), wn = tile.wn(), fr = tile.fr(), fg = tile.fg();
  const float* W = p.w + (size_t)z * p.w_parity_stride;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nk = (p.K + BK - 1) / BK;
  const RowCtx ctx = make_a_ctx(p, m0), bctx = make_b_ctx(W, p.K, n0, p.Cout);
  // two k-tiles in flight in registers: the loads of kt+2 are issued before the MFMAs of kt, the loads of kt+1
  // (issued one iteration earlier) are parked in LDS after them -- two MFMA phases between issue and use
  // The loop body is branch-free around the asynchronous loads: every iteration issues eight loads (the tile index is
  // clamped, so the last two iterations re-read the last tile from L2) and every iteration parks a tile in LDS (the
  // last one parks a copy nobody reads).  With the waits inside `if (more tiles)` branches the compiler copied the
  // in-flight destination registers at the joins BEFORE the s_waitcnt of one branch -- stale data for nk == 1.
  f32x4 ra[2][4], rb[2][4];
  uint32_t ka[2], kb[2];
  ka[0] = load_a<UT, true>(p, ctx, z, 0, ra[0]); kb[0] = load_b(bctx, 0, p.K, rb[0]);
  ka[1] = load_a<UT, true>(p, ctx, z, min(1, nk - 1) * BK, ra[1]); kb[1] = load_b(bctx, min(1, nk - 1) * BK, p.K, rb[1]);
  wait_loads<8>(ra[0], rb[0]);
  const bool relu_in = p.relu_in != 0;
  store_tile(smem, ra[0], ka[0], relu_in); store_tile(smem + 16384, rb[0], kb[0]);
  __syncthreads();
  // one iteration: loads of tile kt+2 -> set `l`; MFMAs on LDS buffer `bo`; tile kt+1 (set `s`) -> the other buffer
  auto step = [&](int kt, auto lc, auto sc, int bo) {
    constexpr int l = decltype(lc)::value, sset = decltype(sc)::value;
    if (!(EXP & 1)) {
      const int k2 = min(kt + 2, nk - 1) * BK;
      ka[l] = load_a<UT, true>(p, ctx, z, k2, ra[l]); kb[l] = load_b(bctx, k2, p.K, rb[l]);
    }
    __builtin_amdgcn_sched_barrier(0);     // nothing that needs tile kt+1's registers may move above the MFMAs
    mma_tile(smem + bo, smem + bo + 16384, wm, wn, fr, fg, acc);
    __builtin_amdgcn_sched_barrier(0);
    if (!(EXP & 2)) {
      if (EXP & 1) wait_loads<0>(ra[sset], rb[sset]); else wait_loads<8>(ra[sset], rb[sset]);    // tile kt+2 stays in flight
      store_tile(smem + (bo ^ 32768), ra[sset], ka[sset], relu_in); store_tile(smem + (bo ^ 32768) + 16384, rb[sset], kb[sset]);
    }
    if (!(EXP & 4)) __syncthreads();
  };
#pragma unroll 1
  for (int kt = 0; kt < nk; kt += 2) {
    step(kt, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, 0);
    if (kt + 1 < nk) step(kt + 1, std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, 32768);
  }
  drain_loads(ra[0], rb[0], ra[1], rb[1]);               // the clamped loads of the last iteration
  float* ct = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        ct[(wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fg) * BN + wn + 32 * j + fr] = acc[i][j][e];
  conv_epilogue(p, ct, z, m0, n0);
}

// ---------------------------------------------------------------------------------------------------
// Quantize.forward_ (eval branch, vqvae/vqvae_zc.py:41-54): dist = |x|^2 - 2 x E + |E|^2, id = argmax(-dist)
// (first maximum on ties).  GEMM x[M,256] . Et[8192,256]^T with a running (min, index) epilogue: the
// 33.5 MB/image distance map of the reference is never written.  One workgroup = 128 rows x ALL codes.
struct VqArgs { const float* x; const float* et; const float* e2; long long* ids; int M, D, NE; };

__global__ __launch_bounds__(NT) void vq_argmin_kernel(const VqArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float x2s[BM];
  __shared__ float best_v[2][BM];
  __shared__ int best_i[2][BM];
  const int m0 = blockIdx.x * BM;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int fr = lane & 31, fg = lane >> 5;
  // |x|^2 per row (2 threads per row, fp32)
  {
    const int row = threadIdx.x >> 1, half = threadIdx.x & 1;
    float s = 0.f;
    if (m0 + row < p.M)
      for (int k = half * (p.D / 2); k < (half + 1) * (p.D / 2); k += 4) {
        const f32x4 v = ld4(p.x + (size_t)(m0 + row) * p.D + k);
        s += v[0] * v[0]; s += v[1] * v[1]; s += v[2] * v[2]; s += v[3] * v[3];
      }
    s += __shfl_xor(s, 1, 64);
    if (half == 0) x2s[row] = s;
  }
  __syncthreads();
  float bv[2][16]; int bi[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) { bv[i][e] = INFINITY; bi[i][e] = 0; }

  const int nk = (p.D + BK - 1) / BK;
  const RowCtx xctx = make_b_ctx(p.x, p.D, m0, p.M);
  for (int n0 = 0; n0 < p.NE; n0 += BN) {
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    f32x4 ra[4], rb[4];
    const RowCtx ectx = make_b_ctx(p.et, p.D, n0, p.NE);
    uint32_t ka = load_b(xctx, 0, p.D, ra), kb = load_b(ectx, 0, p.D, rb);
    __syncthreads();
    wait_loads<0>(ra, rb);
    store_tile(smem, ra, ka); store_tile(smem + 16384, rb, kb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      { const int k1 = min(kt + 1, nk - 1) * BK; ka = load_b(xctx, k1, p.D, ra); kb = load_b(ectx, k1, p.D, rb); }   // branch-free, see conv_kernel
      mma_tile(smem + cur * 32768, smem + cur * 32768 + 16384, wm, wn, fr, fg, acc);
      wait_loads<0>(ra, rb);
      store_tile(smem + (cur ^ 1) * 32768, ra, ka); store_tile(smem + (cur ^ 1) * 32768 + 16384, rb, kb);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + 32 * j + fr;
      const float c2 = col < p.NE ? p.e2[col] : INFINITY;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fg;
          const float d = (x2s[row] - 2.0f * acc[i][j][e]) + c2;      // same expression order as the reference
          if (d < bv[i][e]) { bv[i][e] = d; bi[i][e] = col; }          // columns visited in increasing order
        }
    }
  }
  // reduce over the 32 lanes that hold different columns of the same row (ties -> smaller index)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float v = bv[i][e]; int ix = bi[i][e];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(ix, o, 64);
        if (ov < v || (ov == v && oi < ix)) { v = ov; ix = oi; }
      }
      if (fr == 0) {
        const int row = wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fg;
        best_v[wave & 1][row] = v; best_i[wave & 1][row] = ix;
      }
    }
  __syncthreads();
  if (threadIdx.x < BM && m0 + threadIdx.x < p.M) {
    const int r = threadIdx.x;
    const float v0 = best_v[0][r], v1 = best_v[1][r];
    const int i0 = best_i[0][r], i1 = best_i[1][r];
    p.ids[m0 + r] = (v1 < v0 || (v1 == v0 && i1 < i0)) ? i1 : i0;
  }
}

// ---------------------------------------------------------------------------------------------------
// layout helpers
// NCHW (c = 3) -> NHWC4 (4th channel zero) : input of encoder conv 1
__global__ void nchw3_to_nhwc4_kernel(const float* in, float* out, int B, int H, int W) {
  const size_t n = (size_t)B * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / ((size_t)H * W), px = i % ((size_t)H * W);
    f32x4 v;
    v[0] = in[(b * 3 + 0) * H * W + px]; v[1] = in[(b * 3 + 1) * H * W + px]; v[2] = in[(b * 3 + 2) * H * W + px]; v[3] = 0.f;
    *reinterpret_cast<f32x4*>(out + i * 4) = v;
  }
}
// embed_code (vqvae/vqvae_zc.py:95-96): out[pixel][:] = Et[id][:]   (NHWC == the reference's pre-permute layout)
__global__ void embed_code_kernel(const long long* ids, const float* et, float* out, size_t npix, int D, int NE) {
  const int dv = D / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix * dv; i += (size_t)gridDim.x * blockDim.x) {
    const size_t px = i / dv; const int c = (int)(i % dv) * 4;
    long long id = ids[px]; id = id < 0 ? 0 : (id >= NE ? NE - 1 : id);
    *reinterpret_cast<f32x4*>(out + px * D + c) = ld4(et + (size_t)id * D + c);
  }
}
// final 1x1 conv 512 -> 3 (vqvae/vqvae_zc.py:190) on NHWC input, output NCHW, optional de-normalisation
// out = (w . x + b) * scale[c] + shift[c]  (vqvae/api.py:43).  One wave per pixel group; HBM-bound.
__global__ __launch_bounds__(256) void conv1x1_to3_kernel(const float* in, const float* w, const float* bias,
                                                         float* out, size_t npix, int HW, int Cin,
                                                         float s0, float s1, float s2, float t0, float t1, float t2) {
  const int lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t px = wave; px < npix; px += nw) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int c = lane * 4; c < Cin; c += 256) {
      const f32x4 x = ld4(in + px * Cin + c);
      const f32x4 w0 = ld4(w + c), w1 = ld4(w + Cin + c), w2 = ld4(w + 2 * Cin + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) { a0 += x[i] * w0[i]; a1 += x[i] * w1[i]; a2 += x[i] * w2[i]; }
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (lane == 0) {
      const size_t b = px / HW, r = px % HW;
      out[(b * 3 + 0) * HW + r] = (a0 + bias[0]) * s0 + t0;
      out[(b * 3 + 1) * HW + r] = (a1 + bias[1]) * s1 + t1;
      out[(b * 3 + 2) * HW + r] = (a2 + bias[2]) * s2 + t2;
    }
  }
}

// out[b][c][pix] = (sum over channel tiles of the fused-projection partial sums + bias[c]) * scale[c] + shift[c]
__global__ __launch_bounds__(256) void rgb_finalize_kernel(const float* part, int ntiles, const float* bias, float* out, size_t npix,
                                                           int HW, float s0, float s1, float s2, float t0, float t1, float t2) {
  for (size_t px = (size_t)blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += (size_t)gridDim.x * blockDim.x) {
    f32x4 a = ld4(part + px * 4);
    for (int t = 1; t < ntiles; ++t) a += ld4(part + ((size_t)t * npix + px) * 4);
    const size_t b = px / HW, r = px % HW;
    out[(b * 3 + 0) * HW + r] = (a[0] + bias[0]) * s0 + t0;
    out[(b * 3 + 1) * HW + r] = (a[1] + bias[1]) * s1 + t1;
    out[(b * 3 + 2) * HW + r] = (a[2] + bias[2]) * s2 + t2;
  }
}

}  // namespace

int cogv_conv_split_launch(const cogv_conv_desc* d, void* stream);   // conv_split.hip: the COGV_CONV_BF16X3 form of a checked descriptor

extern "C" int cogv_conv2d_nhwc_f32(const cogv_conv_desc* d, void* stream) {
  ConvArgs a;
  long long blocks = 0;
  const int rc = conv_fill_args(d, a, blocks);
  if (rc != COGV_OK) return rc;
  if (d->precision == COGV_CONV_BF16X3) return cogv_conv_split_launch(d, stream);     // conv_split.hip
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    attr = true;
  }
  static const int probe = [] { const char* e = getenv("COGV_CONV_EXP"); return e ? atoi(e) : 0; }();
  if (probe && a.Cin % BK == 0) {
    void (*k)(const ConvArgs) = probe == 1 ? conv_kernel<true, 1> : probe == 2 ? conv_kernel<true, 2> : probe == 3 ? conv_kernel<true, 3>
                              : probe == 4 ? conv_kernel<true, 4> : probe == 6 ? conv_kernel<true, 6> : conv_kernel<true, 7>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(NT), 65536, reinterpret_cast<hipStream_t>(stream), a);
    return cogv_check_launch();
  }
  if (a.Cin % BK == 0) hipLaunchKernelGGL(conv_kernel<true>, dim3((unsigned)blocks), dim3(NT), 65536, reinterpret_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(conv_kernel<false>, dim3((unsigned)blocks), dim3(NT), 65536, reinterpret_cast<hipStream_t>(stream), a);
  return cogv_check_launch();
}

extern "C" int cogv_rgb_finalize_f32(const float* partial, int ntiles, const float* bias, float* out, int B, int H, int W,
                                     const float* scale3_host, const float* shift3_host, void* stream) {
  if (!partial || !bias || !out || ntiles <= 0 || B <= 0 || H <= 0 || W <= 0 || ((uintptr_t)partial & 15)) return COGV_ERR_ARG;
  const float s[3] = {scale3_host ? scale3_host[0] : 1.f, scale3_host ? scale3_host[1] : 1.f, scale3_host ? scale3_host[2] : 1.f};
  const float t[3] = {shift3_host ? shift3_host[0] : 0.f, shift3_host ? shift3_host[1] : 0.f, shift3_host ? shift3_host[2] : 0.f};
  const size_t npix = (size_t)B * H * W;
  size_t blocks = (npix + 255) / 256; if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(rgb_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), partial, ntiles,
                     bias, out, npix, H * W, s[0], s[1], s[2], t[0], t[1], t[2]);
  return cogv_check_launch();
}

extern "C" int cogv_vq_argmin_f32(const float* x, const float* embed_t, const float* embed_sq, int64_t* ids, int M,
                                  int D, int n_embed, void* stream) {
  if (!x || !embed_t || !embed_sq || !ids || M <= 0 || D <= 0 || (D & 7) || n_embed <= 0) return COGV_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)embed_t) & 15) return COGV_ERR_ARG;
  VqArgs a{x, embed_t, embed_sq, reinterpret_cast<long long*>(ids), M, D, n_embed};
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vq_argmin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 65536); attr = true; }
  hipLaunchKernelGGL(vq_argmin_kernel, dim3((M + BM - 1) / BM), dim3(NT), 65536, reinterpret_cast<hipStream_t>(stream), a);
  return cogv_check_launch();
}

extern "C" int cogv_nchw3_to_nhwc4_f32(const float* in, float* out, int B, int H, int W, void* stream) {
  if (!in || !out || B <= 0 || H <= 0 || W <= 0 || ((uintptr_t)out & 15)) return COGV_ERR_ARG;
  const size_t n = (size_t)B * H * W;
  int g = (int)((n + 255) / 256); if (g > 4096) g = 4096;
  hipLaunchKernelGGL(nchw3_to_nhwc4_kernel, dim3(g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in, out, B, H, W);
  return cogv_check_launch();
}

extern "C" int cogv_embed_code_f32(const int64_t* ids, const float* embed_t, float* out, int64_t npix, int D,
                                   int n_embed, void* stream) {
  if (!ids || !embed_t || !out || npix <= 0 || (D & 3) || (((uintptr_t)embed_t | (uintptr_t)out) & 15)) return COGV_ERR_ARG;
  const size_t n = (size_t)npix * (D / 4);
  int g = (int)((n + 255) / 256); if (g > 4096) g = 4096;
  hipLaunchKernelGGL(embed_code_kernel, dim3(g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(ids), embed_t, out, (size_t)npix, D, n_embed);
  return cogv_check_launch();
}

extern "C" int cogv_conv1x1_to_rgb_f32(const float* in, const float* w, const float* bias, float* out, int B, int H,
                                       int W, int Cin, const float* scale3_host, const float* shift3_host,
                                       void* stream) {
  if (!in || !w || !bias || !out || B <= 0 || (Cin & 3) || (((uintptr_t)in | (uintptr_t)w) & 15)) return COGV_ERR_ARG;
  const float s[3] = {scale3_host ? scale3_host[0] : 1.f, scale3_host ? scale3_host[1] : 1.f, scale3_host ? scale3_host[2] : 1.f};
  const float t[3] = {shift3_host ? shift3_host[0] : 0.f, shift3_host ? shift3_host[1] : 0.f, shift3_host ? shift3_host[2] : 0.f};
  const size_t npix = (size_t)B * H * W;
  size_t blocks = (npix + 3) / 4; if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(conv1x1_to3_kernel, dim3((int)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), in, w,
                     bias, out, npix, H * W, Cin, s[0], s[1], s[2], t[0], t[1], t[2]);
  return cogv_check_launch();
}

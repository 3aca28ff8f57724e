// Device pieces shared by the two forward forms of the implicit-GEMM convolution, conv_kernel (conv.hip, exact fp32) and
// conv_split_kernel (conv_split.hip, split bf16): the workgroup's tile, the staging of the activation operand and the
// epilogue.  The k-loops, the MFMA tiles and the parking of operands in LDS are each kernel's own.  ld4 / st4 also
// serve the training kernels (conv_bwd.hip).
#pragma once
#include "common.cuh"
#include "cogview_hip.h"
#include "conv_args.cuh"
#include "conv_taps.cuh"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
// Asynchronous 16-byte load: issued through inline asm so that the COMPILER does not track it -- its own vmcnt
// bookkeeping turned "tile kt+1 is needed, tile kt+2 may stay in flight" into vmcnt(0) (it drained both register sets
// before every park in LDS, and half of the older set before issuing the newer one).  The consumer must call
// wait_loads<N>() on the destination registers before the first use (loads return in order: N = number of younger loads
// that may remain outstanding).  Must not be spilled around (cogview_amd/csrc/build.py scan_asm_hazards: no scratch access
// and no read of a destination register while the load is in flight).
__device__ __forceinline__ void ld4_async(f32x4& dst, const float* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(dst) : "v"(p) : "memory");
}

// Workgroup -> (pixel tile, channel tile, parity): the grid is one-dimensional and XCD-aware.  Hardware hands
// consecutive workgroup ids to the 8 XCDs round-robin, each XCD has its own 4-MiB L2, and 64 workgroups run on an XCD at
// a time (2 per CU).  An XCD therefore takes a contiguous chunk of pixel tiles and walks it with (channel tile, parity)
// varying fastest: the 64 concurrent workgroups are 64 / (channel tiles x parities) neighbouring pixel tiles times ALL
// their channel tiles / parities, so every activation line is fetched into that L2 once and hit by the other
// workgroups, and the weight slices are shared by the pixel tiles in flight.  (With a plain 3-D grid the workgroups
// that read the same activations sat on different XCDs or ran far apart in time: 50 % L2 hit rate, the input tensor
// streamed from HBM once per channel tile and parity -- 16 times for the last transposed convolution.)
struct ConvTile {
  int mt, yz, ntiles;        // pixel tile; (parity, channel tile) as one index; channel tiles
  bool live;                 // false: the grid's padding past the last pixel tile (the kernel returns at once)
  // The coordinates are derived where the kernel asks for them, after it has tested `live`: as fields filled in
  // conv_tile() the second division ran in front of that branch in every workgroup (0.3 % of the decoder's time in the
  // exact kernel); filled under an early return or `if (live)` they changed every kernel's register counts.  n0 takes
  // the z the kernel already has, so that there is one division as before.
  __device__ __forceinline__ int z() const { return yz / ntiles; }                       // parity
  __device__ __forceinline__ int m0() const { return mt * BM; }                          // first pixel
  __device__ __forceinline__ int n0(int z) const { return (yz - z * ntiles) * BN; }      // first channel, given z()
  // the wave's 64x64 sub-tile, the lane's MFMA row and k-half
  __device__ __forceinline__ int wm() const { const int wave = threadIdx.x >> 6; return (wave >> 1) * 64; }
  __device__ __forceinline__ int wn() const { const int wave = threadIdx.x >> 6; return (wave & 1) * 64; }
  __device__ __forceinline__ int fr() const { const int lane = threadIdx.x & 63; return lane & 31; }
  __device__ __forceinline__ int fg() const { const int lane = threadIdx.x & 63; return lane >> 5; }
};
__device__ __forceinline__ ConvTile conv_tile(const ConvArgs& p) {
  ConvTile t;
  const int mtiles = (p.M + BM - 1) / BM;
  t.ntiles = (p.Cout + BN - 1) / BN;
  const int per = t.ntiles * p.nz, chunk = (mtiles + 7) >> 3;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  t.mt = xcd * chunk + local / per; t.yz = local % per;
  t.live = t.mt < mtiles;
  return t;
}

// Activation staging.  thread t -> (tile row t/8 + 32 q for q = 0..3, 16-byte chunk t%8 of the 128-byte k-slice).
// Every load of a k-tile is UNCONDITIONAL, from a clamped (always valid) address, and the rows / taps that fall outside
// the image are zeroed when the registers are parked in LDS: a `v = 0; if (inside) v = load` form makes the compiler
// wait for each load before issuing the next one (the select needs the loaded value), which serialises eight memory
// latencies per k-tile -- measured: MFMA pipe 57 % busy with the waves waiting on vmcnt.
struct RowCtx {            // per thread, fixed for the whole tile: its four pixels (conv.hip's make_b_ctx: four matrix rows)
  const float* base[4];    // &in[b][0][0][0] of row q's image
  int y0[4], x0[4];        // y * in_mul, x * in_mul
  uint32_t valid;          // bit q: the row exists (m < M)
};
__device__ __forceinline__ RowCtx make_a_ctx(const ConvArgs& p, int m0) {
  RowCtx c; c.valid = 0u;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = m0 + (t >> 3) + 32 * q;
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    const int b = mm / (p.GH * p.GW);
    const int rem = mm - b * (p.GH * p.GW);
    const int y = rem / p.GW, x = rem - y * p.GW;
    c.base[q] = p.in + (size_t)b * p.IH * p.IW * p.Cin;
    c.y0[q] = y * p.in_mul; c.x0[q] = x * p.in_mul;
    c.valid |= ok ? (1u << q) : 0u;
  }
  return c;
}
// A tile: 128 pixels x 32 k; chunk = 4 consecutive k = 4 channels of one tap.  Returns the 4-bit keep mask.
// Offsets inside one image are 32-bit (IH * IW * Cin < 2^31, checked by the launcher); the products use the
// full-rate 24-bit multiplier (iy, ix < 2^15 and IW * Cin, Cin < 2^24, checked by the launcher).
// ASYNC: ld4_async (the caller waits with wait_loads) instead of a load the compiler tracks.
template <bool UNIFORM_TAP, bool ASYNC>
__device__ __forceinline__ uint32_t load_a(const ConvArgs& p, const RowCtx& c, int z, int k0, f32x4 (&r)[4]) {
  const int t = threadIdx.x;
  int dy, dx, ci; bool kok;
  if (UNIFORM_TAP) {           // Cin % 32 == 0: the whole k-tile lies inside one tap -> scalar arithmetic
    const int tap = __builtin_amdgcn_readfirstlane(k0 / p.Cin);
    kok = true;                                        // K % 32 == 0 as well
    tap_offset(p.kind, z, tap, dy, dx);
    ci = k0 - tap * p.Cin + (t & 7) * 4;
  } else {
    const int k = k0 + (t & 7) * 4;
    kok = k < p.K;
    const int tap = kok ? k / p.Cin : 0;
    ci = kok ? k - tap * p.Cin : 0;
    tap_offset(p.kind, z, tap, dy, dx);
  }
  const int row_pitch = p.IW * p.Cin;
  uint32_t keep = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int iy = c.y0[q] + dy, ix = c.x0[q] + dx;
    const bool ok = kok && ((c.valid >> q) & 1u) && (unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW;
    const int off = ok ? __mul24(iy, row_pitch) + __mul24(ix, p.Cin) + ci : 0;
    if (ASYNC) ld4_async(r[q], c.base[q] + off); else r[q] = ld4(c.base[q] + off);
    keep |= ok ? (1u << q) : 0u;
  }
  return keep;
}

// Epilogue of tile (z, m0, n0): every wave has stored its accumulators into the C tile `ct` ([BM][BN] floats in LDS, the
// C/D lane map of the 32x32 MFMAs is the same in both kernels); a thread then takes 8 consecutive channels of a pixel per
// pass: bias, ReLU, then either the residual and the store, or the fused RGB partial sums.
__device__ __forceinline__ void conv_epilogue(const ConvArgs& p, const float* ct, int z, int m0, int n0) {
  __syncthreads();
  const int cchunk = (threadIdx.x & 15) * 8;
#pragma unroll 1
  for (int pass = 0; pass < 8; ++pass) {
    const int row = pass * 16 + (threadIdx.x >> 4);
    const int m = m0 + row, n = n0 + cchunk;
    float rgb[3] = {0.f, 0.f, 0.f};
    size_t pix = 0;
    if (m < p.M && n < p.Cout) {
      f32x4 x0 = ld4(ct + row * BN + cchunk), x1 = ld4(ct + row * BN + cchunk + 4);
      if (p.bias) { const f32x4 b0 = ld4(p.bias + n), b1 = ld4(p.bias + n + 4); x0 += b0; x1 += b1; }
      if (p.relu_out) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { x0[i] = fmaxf(x0[i], 0.f); x1[i] = fmaxf(x1[i], 0.f); }
      }
      const int b = m / (p.GH * p.GW);
      const int rem = m - b * (p.GH * p.GW);
      const int y = rem / p.GW, x = rem - y * p.GW;
      const int oy = y * p.out_mul + (z >> 1), ox = x * p.out_mul + (z & 1);   // z = 0 unless transposed
      if (!p.rgb_part) {
        const size_t oidx = (((size_t)b * p.OH + oy) * p.OW + ox) * p.Cout + n;
        if (p.residual) {      // residual block: out = conv(...) + [relu](input)  (vqvae/vqvae_zc.py:110-114, see cogview_hip.h)
          f32x4 r0 = ld4(p.residual + oidx), r1 = ld4(p.residual + oidx + 4);
          if (p.relu_res) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { r0[i] = fmaxf(r0[i], 0.f); r1[i] = fmaxf(r1[i], 0.f); }
          }
          x0 += r0; x1 += r1;
        }
        st4(p.out + oidx, x0);
        st4(p.out + oidx + 4, x1);
      } else {
        // fused final 1x1 convolution (vqvae/vqvae_zc.py:190): this tile's 128 channels of the three output sums; the
        // 134-MB-per-image activation of the last transposed convolution is never written
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const f32x4 w0 = ld4(p.rgb_w + (size_t)c * p.Cout + n), w1 = ld4(p.rgb_w + (size_t)c * p.Cout + n + 4);
          float r = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) { r = fmaf(x0[i], w0[i], r); r = fmaf(x1[i], w1[i], r); }
          rgb[c] = r;
        }
        pix = ((size_t)b * p.OH + oy) * p.OW + ox;
      }
    }
    if (p.rgb_part) {        // the 16 lanes of a row hold its 16 channel groups: fold them, lane 0 of the group stores
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float r = rgb[c];
        r += __shfl_xor(r, 1, 64); r += __shfl_xor(r, 2, 64); r += __shfl_xor(r, 4, 64); r += __shfl_xor(r, 8, 64);
        rgb[c] = r;
      }
      if ((threadIdx.x & 15) == 0 && m < p.M)
        st4(p.rgb_part + ((size_t)(n0 / BN) * ((size_t)p.B * p.OH * p.OW) + pix) * 4, f32x4{rgb[0], rgb[1], rgb[2], 0.f});
    }
  }
}

}  // namespace

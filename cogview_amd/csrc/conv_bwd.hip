// VQ-VAE tokenizer TRAINING kernels (reference vqvae/vqvae_zc.py: the autograd of the conv stacks :116-214 and the training
// branch of Quantize.forward_ :67-86).  gfx950, fp32 end to end on the exact-fp32 MFMA, like conv.hip.
//
// The data gradient of every layer is a forward kernel with repacked weights (host side).  What is new here:
//   * the weight gradient                      dW[z][co][t][ci] = sum_m dY[out(m, z)][co] * X[in(m, t, z)][ci]
//   * the ReLU mask with the bias gradient     dX = dY * (A > 0),  db[c] = sum_m dX[m][c]
//   * the codebook statistics and EMA update   count[j], sum[j][:] over the pixels of code j, then vqvae_zc.py:74-83
//   * the straight-through / commitment gradient of the quantiser's input
// No floating-point atomics: every sum has a fixed order, the same inputs give the same bits run after run.
#include "common.cuh"
#include "cogview_hip.h"
#include "conv_tile.cuh"      // ld4 / st4; NT, conv_geometry (conv_args.cuh); tap_offset (conv_taps.cuh)

namespace {

// ---------------------------------------------------------------------------------------------------
// Weight gradient.  As a GEMM: rows = output channels co, columns = k = tap * Cin + ci (the forward kernel's contraction
// index: the packed layout [co][tap][ci] IS [co][k]), contraction over the pixels m of the forward iteration grid.  Both
// operands arrive NHWC, so an LDS row is a pixel and the 32 lanes of an MFMA operand read 32 consecutive channels of one
// row -- no transposition.  A column chunk of 4 consecutive k lies inside one tap (Cin % 4 == 0), and a thread stages the
// same chunk of every pixel, so its tap offset is fixed for the whole kernel.
// Tile: TCO co x 128 k, 32 pixels per contraction step, 4 waves.  TCO = 128: waves of 64 x 64 (2 x 2 MFMA 32x32x2).
// TCO = 32 (the plan's choice for Cout <= 32 under topologies == 1: a ResBlock's 3x3 has 32 output channels, and a 128-wide
// tile would spend three quarters of its MFMAs on zero rows): waves of 32 x 32, side by side over k.  Both widths add an
// element's pixels in the same order.  Workgroup -> (pixel split s, parity z, co tile, k tile); split s writes slab s,
// wgrad_reduce_kernel adds the slabs in order.
constexpr int TC = 128;      // k (= tap * Cin + ci) columns per tile; output channels per tile in the wide form
constexpr int TCN = 32;      // output channels per tile in the narrow form
constexpr int KP = 32;       // pixels per contraction step

struct WgradArgs {
  const float* x; const float* dy; float* out;     // out: dW itself (one split) or the slabs
  int B, IH, IW, Cin;
  int GH, GW;               // iteration grid of the forward kernel (pixels per image = GH * GW)
  int OH, OW, Cout;
  int in_mul, out_mul, kind, nz;
  int K;                    // ntaps * Cin
  int M;                    // B * GH * GW
  int span;                 // pixels per split, a multiple of KP
  int cot, kt;              // tiles over Cout and over K
  long long slab;           // floats of one slab = nz * Cout * K
};

template <int TCO, bool RELU_X>
__global__ __launch_bounds__(NT) void wgrad_kernel(const WgradArgs p) {
  constexpr int WM = TCO == TC ? 64 : 32;          // output channels per wave
  constexpr int WN = TC / (4 / (TCO / WM));        // k columns per wave: 64 (2 x 2 waves) or 32 (1 x 4 waves)
  constexpr int MI = WM / 32, NJ = WN / 32;
  constexpr int ACH = TCO / 4;                     // 16-byte chunks of a dy row
  constexpr int AROWS = NT / ACH, AQ = KP / AROWS; // pixel rows per staging pass and passes per step, dy operand
  static_assert(TCO == TC || AQ == 1, "the narrow form stages one chunk of dy per thread and step");
  __shared__ __attribute__((aligned(16))) float la[KP * TCO];    // [pixel][co]
  __shared__ __attribute__((aligned(16))) float lb[KP * TC];     // [pixel][k]
  int r = blockIdx.x;
  const int kti = r % p.kt; r /= p.kt;
  const int ct = r % p.cot; r /= p.cot;
  const int z = r % p.nz;
  const int s = r / p.nz;
  const int co0 = ct * TCO, k0 = kti * TC;
  const int m_begin = s * p.span, m_end = min(p.M, m_begin + p.span);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = TCO == TC ? (wave >> 1) * 64 : 0, wn = TCO == TC ? (wave & 1) * 64 : wave * 32;
  const int fr = lane & 31, fg = lane >> 5;

  // staging: x operand: thread t -> 16-byte chunk t % 32 of the 128 columns, pixel rows t / 32 + 8 q; dy operand: chunk
  // t % ACH of the TCO channels, pixel rows t / ACH + AROWS q (the same rows as x in the wide form)
  const int chunk = threadIdx.x & 31, prow = threadIdx.x >> 5;
  const int achunk = TCO == TC ? chunk : threadIdx.x % ACH, arow = TCO == TC ? prow : threadIdx.x / ACH;
  const bool a_ok = co0 + achunk * 4 < p.Cout;
  const int k = k0 + chunk * 4;
  const bool b_ok = k < p.K;
  const int tap = b_ok ? k / p.Cin : 0;
  const int ci = b_ok ? k - tap * p.Cin : 0;
  int dy, dx;
  tap_offset(p.kind, z, tap, dy, dx);
  const int gpix = p.GH * p.GW;

  f32x16 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  f32x4 ra[AQ], rb[4];
  // a pixel past the split's range, a channel chunk past the tensor and a tap outside the image contribute zero; nothing is
  // loaded from an address that is not inside its tensor
  auto load = [&](int m0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + prow + 8 * q;
      f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (m < m_end) {
        const int b = m / gpix;
        const int rem = m - b * gpix;
        const int y = rem / p.GW, x = rem - y * p.GW;
        if (TCO == TC && a_ok) {           // the wide form stages dy from the pixel rows it stages x from
          const int oy = y * p.out_mul + (z >> 1), ox = x * p.out_mul + (z & 1);     // z = 0 unless transposed
          va = ld4(p.dy + (((size_t)b * p.OH + oy) * p.OW + ox) * p.Cout + co0 + chunk * 4);
        }
        const int iy = y * p.in_mul + dy, ix = x * p.in_mul + dx;
        if (b_ok && (unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW)
          vb = ld4(p.x + (((size_t)b * p.IH + iy) * p.IW + ix) * p.Cin + ci);
      }
      if (TCO == TC) ra[q] = va;
      rb[q] = vb;
    }
    if (TCO != TC) {                       // the narrow form: one chunk of dy per thread, pixel row t / ACH
      const int m = m0 + arow;
      f32x4 va = {0.f, 0.f, 0.f, 0.f};
      if (m < m_end && a_ok) {
        const int b = m / gpix;
        const int rem = m - b * gpix;
        const int y = rem / p.GW, x = rem - y * p.GW;
        const int oy = y * p.out_mul + (z >> 1), ox = x * p.out_mul + (z & 1);
        va = ld4(p.dy + (((size_t)b * p.OH + oy) * p.OW + ox) * p.Cout + co0 + achunk * 4);
      }
      ra[0] = va;
    }
  };
  load(m_begin);
#pragma unroll 1
  for (int m0 = m_begin; m0 < m_end; m0 += KP) {
    __syncthreads();                       // the previous step's fragment reads are done
#pragma unroll
    for (int q = 0; q < AQ; ++q) st4(la + (arow + AROWS * q) * TCO + achunk * 4, ra[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 vb = rb[q];
      if (RELU_X) {                        // on the staged registers, after the loads have landed: -0.0, +0.0 and negatives -> +0.0
#pragma unroll
        for (int i = 0; i < 4; ++i) vb[i] = vb[i] > 0.f ? vb[i] : 0.f;
      }
      st4(lb + (prow + 8 * q) * TC + chunk * 4, vb);
    }
    __syncthreads();
    if (m0 + KP < m_end) load(m0 + KP);    // the next step's loads fly under this step's MFMAs
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {  // one MFMA contracts two pixels: lanes 0..31 pixel 2 kk, lanes 32..63 pixel 2 kk + 1
      const int prw = 2 * kk + fg;
      float fa[MI], fb[NJ];
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = la[prw * TCO + wm + 32 * i + fr];
#pragma unroll
      for (int j = 0; j < NJ; ++j) fb[j] = lb[prw * TC + wn + 32 * j + fr];
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }
  float* out = p.out + (size_t)s * p.slab + (size_t)z * p.Cout * p.K;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int kc = k0 + wn + 32 * j + fr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = co0 + wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fg;
        if (co < p.Cout && kc < p.K) out[(size_t)co * p.K + kc] = acc[i][j][e];
      }
    }
}

// out[i] = slab 0 [i] + slab 1 [i] + ... in slab order (n4 = floats / 4)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* slabs, float* out, size_t n4, int splits) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 a = ld4(slabs + i * 4);
    for (int s = 1; s < splits; ++s) a += ld4(slabs + ((size_t)s * n4 + i) * 4);
    st4(out + i * 4, a);
  }
}

struct WgradPlan { WgradArgs a; int splits; long long blocks; bool narrow, relu_x; };     // narrow, relu_x: the kernel instance

// host only: geometry, argument checks and the split of the pixel range
int wgrad_plan(const cogv_conv_wgrad_desc* d, WgradPlan& pl) {
  if (!d) return COGV_ERR_ARG;
  if (d->B <= 0 || d->IH <= 0 || d->IW <= 0 || d->Cin <= 0 || d->Cout <= 0 || (d->Cin & 3) || (d->Cout & 7) || d->splits < 0) return COGV_ERR_ARG;
  if ((unsigned)d->relu_x > 1u || (unsigned)d->topologies > 1u) return COGV_ERR_ARG;
  WgradArgs& a = pl.a;
  a.x = (const float*)d->x; a.dy = (const float*)d->dy; a.out = (float*)d->dw;
  a.B = d->B; a.IH = d->IH; a.IW = d->IW; a.Cin = d->Cin; a.Cout = d->Cout; a.kind = d->kind;
  ConvGeom g;
  const int rc = conv_geometry(d->kind, d->B, d->IH, d->IW, d->Cin, g);
  if (rc != COGV_OK) return rc;
  if (d->kind == COGV_CONV_3X3_S1 && !d->topologies) return COGV_ERR_UNSUPPORTED;     // 3x3 (ResBlock, stride-4 / stride-2 encoders): opt-in
  if (g.M >= (1ll << 31) - KP || (long long)g.ntaps * a.Cin >= (1 << 24)) return COGV_ERR_ARG;
  a.GH = g.GH; a.GW = g.GW; a.OH = g.OH; a.OW = g.OW; a.in_mul = g.in_mul; a.out_mul = g.out_mul; a.nz = g.nz;
  a.M = (int)g.M; a.K = g.K;
  pl.relu_x = d->relu_x != 0;
  pl.narrow = d->topologies == 1 && a.Cout <= TCN;
  const int tco = pl.narrow ? TCN : TC;
  a.cot = (a.Cout + tco - 1) / tco; a.kt = (a.K + TC - 1) / TC;
  a.slab = (long long)a.nz * a.Cout * a.K;
  // when (tiles x parities) does not fill the chip -- the first and the last layer, small batches -- the pixel range is
  // split: aim at four workgroups per CU, at least 256 pixels per split, at most 256 slabs
  const long long base = (long long)a.nz * a.cot * a.kt;
  long long want = d->splits > 0 ? d->splits : (1024 + base - 1) / base;
  if (d->splits == 0) { if (want > a.M / 256) want = a.M / 256; if (want > 256) want = 256; }
  if (want < 1) want = 1;
  if (want > a.M) want = a.M;
  long long span = (a.M + want - 1) / want;
  span = (span + KP - 1) / KP * KP;
  a.span = (int)span;
  pl.splits = (int)((a.M + span - 1) / span);    // every split owns at least one pixel
  pl.blocks = base * pl.splits;
  if (pl.blocks > 0x7fffffffll) return COGV_ERR_ARG;
  return COGV_OK;
}

// ---------------------------------------------------------------------------------------------------
// ReLU mask and bias gradient, fused: dx = act > 0 ? dy : 0 (act: the saved post-ReLU activation; NULL: no mask),
// partial[wg][c] = sum of dx over the workgroup's rows, then db[c] = sum over workgroups in order.
// thread t -> (row t / cv within a pass, 16-byte column chunk t % cv), cv = C / 4 chunks (at most 256 per column block:
// blockIdx.y walks wider tensors), so a pass reads rpp = 256 / cv whole rows, contiguous in memory.
constexpr int RB_MAX_WG = 512;

__global__ __launch_bounds__(256) void relu_bias_bwd_kernel(const float* dy, const float* act, float* dx, float* partial,
                                                            long long M, int C, long long rows_per_wg) {
  __shared__ f32x4 red[256];
  const int cv_all = C >> 2, cb = blockIdx.y * 256;
  const int cv = min(cv_all - cb, 256), rpp = 256 / cv;
  const int rl = threadIdx.x / cv, cc = threadIdx.x - rl * cv;
  const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = min(M, r0 + rows_per_wg);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (rl < rpp) {
    for (long long row = r0 + rl; row < r1; row += rpp) {
      const size_t idx = (size_t)row * C + (size_t)(cb + cc) * 4;
      f32x4 v = ld4(dy + idx);
      if (act) {
        const f32x4 a = ld4(act + idx);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = a[i] > 0.f ? v[i] : 0.f;      // -0.0 and +0.0 both mask
      }
      if (dx) st4(dx + idx, v);
      acc += v;
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (rl == 0) {
    for (int q = 1; q < rpp; ++q) acc += red[q * cv + cc];
    st4(partial + (size_t)blockIdx.x * C + (size_t)(cb + cc) * 4, acc);
  }
}
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* partial, float* db, int nwg, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float s = partial[c];
  for (int w = 1; w < nwg; ++w) s += partial[(size_t)w * C + c];
  db[c] = s;
}
inline int relu_bias_wgs(long long M) {
  long long n = (M + 63) / 64;
  return (int)(n < 1 ? 1 : (n > RB_MAX_WG ? RB_MAX_WG : n));
}

// ---------------------------------------------------------------------------------------------------
// Codebook statistics (vqvae/vqvae_zc.py:68-69: embed_onehot.sum(0) and flatten^T @ embed_onehot) without the dense one-hot
// product: an inverted index -- per code, its pixels in ascending order -- then a per-code sum of the indexed rows.
//   1 hist    pixels are cut into at most 64 ranges; hist[range][code] += 1 (integer atomics: exact, order-free)
//   2 scan    per code: hist -> exclusive prefix over the ranges (each range's first slot in the code's list) and count;
//             over the codes: list starts, and the starts of the codes' sum chunks (a list is summed SUM_CHUNK entries at a time)
//   3 fill    one wave per range walks its pixels in order, 64 at a time; lanes with the same code are ranked by lane
//             (ballot), the running per-code fill of the range lives in LDS -> every list is ascending, whatever the timing
//   4 sum     one workgroup per (code, chunk) adds its rows in list order -> partial row
//   5 finish  sum[code] = its partial rows in chunk order; a code without pixels gets zeros
constexpr int SUM_CHUNK = 256;
constexpr int MAX_RANGES = 64;
constexpr int STATS_MAX_CODES = 32768;        // the fill kernel keeps one LDS counter per code (128 KiB of the CU's 160)

__global__ __launch_bounds__(256) void vq_hist_kernel(const long long* ids, int* hist, int M, int NE, int range) {
  const int m0 = blockIdx.x * range, m1 = min(M, m0 + range);
  for (int m = m0 + threadIdx.x; m < m1; m += blockDim.x) {
    const long long id = ids[m];
    if (id >= 0 && id < NE) atomicAdd(hist + (size_t)blockIdx.x * NE + id, 1);
  }
}
__global__ __launch_bounds__(1024) void vq_scan_kernel(int* hist, int* count, int* start, int* cstart, int NE, int nranges) {
  __shared__ int sa[1024], sb[1024];
  const int t = threadIdx.x;
  for (int j = t; j < NE; j += 1024) {
    int run = 0;
    for (int c = 0; c < nranges; ++c) { const int v = hist[(size_t)c * NE + j]; hist[(size_t)c * NE + j] = run; run += v; }
    count[j] = run;
  }
  __syncthreads();
  const int seg = (NE + 1023) / 1024, j0 = min(NE, t * seg), j1 = min(NE, j0 + seg);
  int a = 0, b = 0;
  for (int j = j0; j < j1; ++j) { const int n = count[j]; a += n; b += (n + SUM_CHUNK - 1) / SUM_CHUNK; }
  sa[t] = a; sb[t] = b;
  __syncthreads();
  if (t == 0) {
    int ra = 0, rb = 0;
    for (int i = 0; i < 1024; ++i) { const int va = sa[i], vb = sb[i]; sa[i] = ra; sb[i] = rb; ra += va; rb += vb; }
    start[NE] = ra; cstart[NE] = rb;
  }
  __syncthreads();
  a = sa[t]; b = sb[t];
  for (int j = j0; j < j1; ++j) { const int n = count[j]; start[j] = a; cstart[j] = b; a += n; b += (n + SUM_CHUNK - 1) / SUM_CHUNK; }
}
__global__ __launch_bounds__(64) void vq_fill_kernel(const long long* ids, const int* hist, const int* start, int* list,
                                                     int M, int NE, int range) {
  extern __shared__ int run[];                 // [NE]: entries of each code this range has written so far
  const int lane = threadIdx.x;
  for (int j = lane; j < NE; j += 64) run[j] = 0;
  __syncthreads();
  const int m0 = blockIdx.x * range, m1 = min(M, m0 + range);
  const int* base = hist + (size_t)blockIdx.x * NE;
  for (int g = m0; g < m1; g += 64) {
    const int m = g + lane;
    long long id64 = m < m1 ? ids[m] : -1;
    const bool valid = id64 >= 0 && id64 < NE;
    const int id = valid ? (int)id64 : -1;
    int rank = 0, cnt = 0;
    bool leader = false;
    unsigned long long todo = __ballot(valid);
    while (todo) {                             // wave-uniform: one round per distinct code among the 64 pixels
      const int src = __ffsll((long long)todo) - 1;
      const int lid = __shfl(id, src, 64);
      const unsigned long long same = __ballot(valid && id == lid);
      if (valid && id == lid) {
        rank = __popcll(same & ((1ull << lane) - 1ull));
        cnt = __popcll(same);
        leader = lane == src;
      }
      todo &= ~same;
    }
    const int before = valid ? run[id] : 0;
    __syncthreads();                           // (one wave) every lane has read the counter before a leader moves it
    if (leader) run[id] = before + cnt;
    __syncthreads();
    if (valid) list[start[id] + base[id] + before + rank] = m;
  }
}
__global__ __launch_bounds__(256) void vq_sum_kernel(const float* x, const int* list, const int* start, const int* cstart,
                                                     float* part, int D, int NE) {
  __shared__ f32x4 red[256];
  const int b = blockIdx.x;
  if (b >= cstart[NE]) return;
  int lo = 0, hi = NE;                         // the code j with cstart[j] <= b < cstart[j + 1]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (cstart[mid] <= b) lo = mid; else hi = mid; }
  const int j = lo;
  const int e0 = start[j] + (b - cstart[j]) * SUM_CHUNK, e1 = min(start[j + 1], e0 + SUM_CHUNK);
  const int cv = D >> 2, rpp = 256 / cv;
  const int rl = threadIdx.x / cv, cc = threadIdx.x - rl * cv;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (rl < rpp)
    for (int e = e0 + rl; e < e1; e += rpp) acc += ld4(x + (size_t)list[e] * D + cc * 4);
  red[threadIdx.x] = acc;
  __syncthreads();
  if (rl == 0) {
    for (int q = 1; q < rpp; ++q) acc += red[q * cv + cc];
    st4(part + (size_t)b * D + cc * 4, acc);
  }
}
__global__ __launch_bounds__(256) void vq_sum_finish_kernel(const float* part, const int* cstart, float* sum, int D, int NE) {
  const int cv = D >> 2;
  const size_t n = (size_t)NE * cv;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i / cv), cc = (int)(i - (size_t)j * cv);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int c = cstart[j]; c < cstart[j + 1]; ++c) a += ld4(part + (size_t)c * D + cc * 4);
    st4(sum + (size_t)j * D + cc * 4, a);
  }
}

struct StatsLayout { int nranges, range, max_chunks; size_t hist, start, cstart, list, part, total; };
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
StatsLayout stats_layout(int M, int D, int NE) {
  StatsLayout l;
  long long range = ((long long)M + MAX_RANGES - 1) / MAX_RANGES;
  if (range < 1024) range = 1024;
  range = (range + 63) / 64 * 64;
  l.range = (int)range;
  l.nranges = (int)((M + range - 1) / range);
  l.max_chunks = (M < NE ? M : NE) + M / SUM_CHUNK + 1;     // sum over codes of ceil(count / SUM_CHUNK) never exceeds this
  l.hist = 0;
  l.start = l.hist + up16((size_t)l.nranges * NE * 4);
  l.cstart = l.start + up16((size_t)(NE + 1) * 4);
  l.list = l.cstart + up16((size_t)(NE + 1) * 4);
  l.part = l.list + up16((size_t)M * 4);
  l.total = l.part + up16((size_t)l.max_chunks * D * 4);
  return l;
}

// the EMA update (vqvae/vqvae_zc.py:74-83).  cluster sizes and their total n: one workgroup, fixed order.
__global__ __launch_bounds__(1024) void vq_ema_cluster_kernel(const int* count, float* cluster_size, float* n_out, float decay,
                                                              float one_minus_decay, int NE) {
  __shared__ float red[1024];
  float s = 0.f;
  for (int j = threadIdx.x; j < NE; j += 1024) {
    const float c = cluster_size[j] * decay + one_minus_decay * (float)count[j];
    cluster_size[j] = c;
    s += c;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_out[0] = red[0];
}
// embed_avg and embed are [D][n_embed] as in the reference; sum is [n_embed][D]
__global__ __launch_bounds__(256) void vq_ema_embed_kernel(const float* sum, const float* cluster_size, const float* n_ptr,
                                                           float* embed_avg, float* embed, float decay, float one_minus_decay,
                                                           float eps, int D, int NE) {
  const float n = n_ptr[0];
  const float denom = n + (float)NE * eps;
  const size_t total = (size_t)D * NE;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i / NE), j = (int)(i - (size_t)d * NE);
    const float avg = embed_avg[i] * decay + one_minus_decay * sum[(size_t)j * D + d];
    embed_avg[i] = avg;
    const float cl = (cluster_size[j] + eps) / denom * n;
    embed[i] = avg / cl;
  }
}

// g_x = g_q + g_diff * 2 (x - q) / numel   (vqvae_zc.py:85-86: diff = (q.detach() - x)^2 .mean(), out = x + (q - x).detach())
__global__ __launch_bounds__(256) void vq_ste_bwd_kernel(const float* g_q, const float* g_diff, const float* x, const float* q,
                                                         float* g_x, size_t n4, float two_over_numel) {
  const float s = g_diff ? g_diff[0] * two_over_numel : 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 d = ld4(x + i * 4) - ld4(q + i * 4);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (g_q) g = ld4(g_q + i * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) g[c] = fmaf(s, d[c], g[c]);
    st4(g_x + i * 4, g);
  }
}

inline int grid_for(size_t n, int cap) { size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > (size_t)cap ? cap : g)); }

}  // namespace

extern "C" int cogv_conv_wgrad_plan(const cogv_conv_wgrad_desc* d, int* plan) {
  WgradPlan pl;
  const int rc = wgrad_plan(d, pl);
  if (rc != COGV_OK) return rc;
  if (plan) { plan[0] = pl.splits; plan[1] = pl.a.span; plan[2] = (int)pl.blocks; plan[3] = pl.a.cot; plan[4] = pl.a.kt; plan[5] = pl.a.nz; }
  return COGV_OK;
}

extern "C" size_t cogv_conv_wgrad_workspace_bytes(const cogv_conv_wgrad_desc* d) {
  WgradPlan pl;
  if (wgrad_plan(d, pl) != COGV_OK || pl.splits <= 1) return 0;
  return (size_t)pl.splits * (size_t)pl.a.slab * 4;
}

extern "C" int cogv_conv_wgrad_nhwc_f32(const cogv_conv_wgrad_desc* d, void* stream) {
  WgradPlan pl;
  const int rc = wgrad_plan(d, pl);
  if (rc != COGV_OK) return rc;
  if (!d->x || !d->dy || !d->dw) return COGV_ERR_ARG;
  if (((uintptr_t)d->x | (uintptr_t)d->dy | (uintptr_t)d->dw | (uintptr_t)d->workspace) & 15) return COGV_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (pl.splits > 1) {
    if (!d->workspace || d->workspace_bytes < (size_t)pl.splits * (size_t)pl.a.slab * 4) return COGV_ERR_ARG;
    pl.a.out = (float*)d->workspace;
  }
  const dim3 grid((unsigned)pl.blocks), block(NT);
  if (pl.narrow && pl.relu_x) hipLaunchKernelGGL((wgrad_kernel<TCN, true>), grid, block, 0, st, pl.a);
  else if (pl.narrow) hipLaunchKernelGGL((wgrad_kernel<TCN, false>), grid, block, 0, st, pl.a);
  else if (pl.relu_x) hipLaunchKernelGGL((wgrad_kernel<TC, true>), grid, block, 0, st, pl.a);
  else hipLaunchKernelGGL((wgrad_kernel<TC, false>), grid, block, 0, st, pl.a);
  int e = cogv_check_launch();
  if (e != COGV_OK || pl.splits == 1) return e;
  const size_t n4 = (size_t)pl.a.slab / 4;           // Cin % 4 == 0
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_for(n4, 4096)), dim3(256), 0, st, (const float*)d->workspace, (float*)d->dw, n4, pl.splits);
  return cogv_check_launch();
}

extern "C" size_t cogv_relu_bias_bwd_workspace_bytes(int64_t M, int C) {
  if (M <= 0 || C <= 0) return 0;
  return (size_t)relu_bias_wgs(M) * (size_t)C * 4;
}

extern "C" int cogv_relu_bias_bwd_f32(const float* dy, const float* act, float* dx, float* db, float* workspace,
                                      size_t workspace_bytes, int64_t M, int C, void* stream) {
  if (!dy || !db || !workspace || M <= 0 || C <= 0 || (C & 3)) return COGV_ERR_ARG;
  if (((uintptr_t)dy | (uintptr_t)act | (uintptr_t)dx | (uintptr_t)workspace) & 15) return COGV_ERR_ARG;
  if (workspace_bytes < cogv_relu_bias_bwd_workspace_bytes(M, C)) return COGV_ERR_ARG;
  const int nwg = relu_bias_wgs(M);
  const long long rows = (M + nwg - 1) / nwg;
  const int cblocks = ((C >> 2) + 255) / 256;
  if (cblocks > 65535) return COGV_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(relu_bias_bwd_kernel, dim3(nwg, cblocks), dim3(256), 0, st, dy, act, dx, workspace, (long long)M, C, rows);
  int e = cogv_check_launch();
  if (e != COGV_OK) return e;
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const float*)workspace, db, nwg, C);
  return cogv_check_launch();
}

extern "C" size_t cogv_vq_code_stats_workspace_bytes(int M, int D, int n_embed) {
  if (M <= 0 || D <= 0 || n_embed <= 0) return 0;
  return stats_layout(M, D, n_embed).total;
}

extern "C" int cogv_vq_code_stats_f32(const int64_t* ids, const float* x, int* count, float* sum, void* workspace,
                                      size_t workspace_bytes, int M, int D, int n_embed, void* stream) {
  if (!ids || !x || !count || !sum || !workspace || M <= 0 || D <= 0 || n_embed <= 0 || (D & 3)) return COGV_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)sum | (uintptr_t)workspace) & 15) return COGV_ERR_ARG;
  if (D > 1024 || n_embed > STATS_MAX_CODES) return COGV_ERR_UNSUPPORTED;
  const StatsLayout l = stats_layout(M, D, n_embed);
  if (workspace_bytes < l.total) return COGV_ERR_ARG;
  char* ws = (char*)workspace;
  int* hist = (int*)(ws + l.hist); int* start = (int*)(ws + l.start); int* cstart = (int*)(ws + l.cstart);
  int* list = (int*)(ws + l.list); float* part = (float*)(ws + l.part);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long long* ids64 = reinterpret_cast<const long long*>(ids);
  if (hipMemsetAsync(hist, 0, (size_t)l.nranges * n_embed * 4, st) != hipSuccess) return COGV_ERR_LAUNCH;
  hipLaunchKernelGGL(vq_hist_kernel, dim3(l.nranges), dim3(256), 0, st, ids64, hist, M, n_embed, l.range);
  hipLaunchKernelGGL(vq_scan_kernel, dim3(1), dim3(1024), 0, st, hist, count, start, cstart, n_embed, l.nranges);
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vq_fill_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, STATS_MAX_CODES * 4); attr = true; }
  hipLaunchKernelGGL(vq_fill_kernel, dim3(l.nranges), dim3(64), (size_t)n_embed * 4, st, ids64, (const int*)hist, (const int*)start, list, M, n_embed, l.range);
  hipLaunchKernelGGL(vq_sum_kernel, dim3(l.max_chunks), dim3(256), 0, st, x, (const int*)list, (const int*)start, (const int*)cstart, part, D, n_embed);
  hipLaunchKernelGGL(vq_sum_finish_kernel, dim3(grid_for((size_t)n_embed * (D >> 2), 4096)), dim3(256), 0, st, (const float*)part, (const int*)cstart, sum, D, n_embed);
  return cogv_check_launch();
}

extern "C" int cogv_vq_ema_update_f32(const int* count, const float* sum, float* cluster_size, float* embed_avg, float* embed,
                                      float* n_out, double decay, double eps, int D, int n_embed, void* stream) {
  if (!count || !sum || !cluster_size || !embed_avg || !embed || !n_out || D <= 0 || n_embed <= 0) return COGV_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float dec = (float)decay, omd = (float)(1.0 - decay), e = (float)eps;      // alpha = 1 - self.decay is formed in double
  hipLaunchKernelGGL(vq_ema_cluster_kernel, dim3(1), dim3(1024), 0, st, count, cluster_size, n_out, dec, omd, n_embed);
  hipLaunchKernelGGL(vq_ema_embed_kernel, dim3(grid_for((size_t)D * n_embed, 4096)), dim3(256), 0, st, sum, (const float*)cluster_size,
                     (const float*)n_out, embed_avg, embed, dec, omd, e, D, n_embed);
  return cogv_check_launch();
}

extern "C" int cogv_vq_ste_bwd_f32(const float* g_q, const float* g_diff, const float* x, const float* q, float* g_x, int64_t n,
                                   void* stream) {
  if (!x || !q || !g_x || n <= 0 || (n & 3)) return COGV_ERR_ARG;
  if (((uintptr_t)g_q | (uintptr_t)x | (uintptr_t)q | (uintptr_t)g_x) & 15) return COGV_ERR_ARG;
  const size_t n4 = (size_t)n / 4;
  hipLaunchKernelGGL(vq_ste_bwd_kernel, dim3(grid_for(n4, 4096)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g_q, g_diff, x, q,
                     g_x, n4, (float)(2.0 / (double)n));
  return cogv_check_launch();
}

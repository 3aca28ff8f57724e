// Tokenizer ingest (gfx950): raw uint8 HWC images -> the encoder's NHWC4 fp32 input, and the crops / overview of a
// super-resolution training row.  DESIGN.md 4.6.1 gives the arithmetic; the uint8 stage is Pillow's
// Image.resize(BILINEAR) (what transforms.Resize does to a PIL image) followed by transforms.CenterCrop, bit for bit.
#include <algorithm>
#include <cmath>
#include "common.cuh"
#include "cogview_hip.h"

namespace {

constexpr int PREP_MAX_TAPS = 65;      // most source pixels one output pixel may read on one axis
constexpr int PREP_BAND = 8;           // output rows per workgroup
constexpr int PREP_SEGW = 128;         // output columns per workgroup == threads per workgroup
constexpr int PREP_LDS = 65536;        // LDS budget of a workgroup: the staged source row + the horizontal pass of a band
constexpr int PREP_PREC = 22;          // fixed-point bits of a coefficient
constexpr int PREP_MAX_SIDE = 1 << 24; // longest source or resized side accepted (byte offsets in a row stay in an int)

// Pillow's bilinear coefficients of one axis (precompute_coeffs + normalize_coeffs_8bpc for the triangle filter):
// xmin / count per output index and, when k != NULL, the integer weights k[xx * max_taps + x] (zero beyond count).
// Returns the largest count.  Plain doubles, no contraction: a fused multiply-add changes the last bit of a weight.
int resample_axis(int in, int out, int* xmin_o, int* count_o, int* k_o, int max_taps) {
#pragma clang fp contract(off)
  int maxc = 0;
  if (in == out) {                     // an axis that keeps its size is copied, not resampled
    for (int xx = 0; xx < out; ++xx) {
      if (xmin_o) xmin_o[xx] = xx;
      if (count_o) count_o[xx] = 1;
      if (k_o) {
        for (int x = 0; x < max_taps; ++x) k_o[(size_t)xx * max_taps + x] = 0;
        k_o[(size_t)xx * max_taps] = 1 << PREP_PREC;
      }
    }
    return 1;
  }
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int x0 = (int)(center - support + 0.5);
    if (x0 < 0) x0 = 0;
    int x1 = (int)(center + support + 0.5);
    if (x1 > in) x1 = in;
    const int c = x1 - x0;
    if (c > maxc) maxc = c;
    if (xmin_o) xmin_o[xx] = x0;
    if (count_o) count_o[xx] = c;
    if (!k_o || c > max_taps) continue;
    double ww = 0.0;                   // summed left to right
    for (int x = 0; x < c; ++x) {
      double w = 1.0 - fabs(((double)(x + x0) - center + 0.5) / fs);
      if (w < 0.0) w = 0.0;
      ww += w;
    }
    int* k = k_o + (size_t)xx * max_taps;
    for (int x = 0; x < max_taps; ++x) k[x] = 0;
    for (int x = 0; x < c; ++x) {
      double w = 1.0 - fabs(((double)(x + x0) - center + 0.5) / fs);
      if (w < 0.0) w = 0.0;
      if (ww != 0.0) w /= ww;
      k[x] = (int)(w * (double)(1 << PREP_PREC) + 0.5);
    }
  }
  return maxc;
}

struct PrepGeo { int nh, nw, top, left, taps_h, taps_v; double scale_h, scale_v; };

// transforms.Resize(S) + CenterCrop(S) of an H x W image: resized size, crop offsets, taps per axis
int prep_geometry(int H, int W, int S, PrepGeo& g) {
  if (S <= 0 || (S & 7) || S > 32768 || H <= 0 || W <= 0) return COGV_ERR_ARG;
  if (H > PREP_MAX_SIDE || W > PREP_MAX_SIDE) return COGV_ERR_UNSUPPORTED;
  const int sht = W <= H ? W : H, lng = W <= H ? H : W;
  const double nl = (double)((int64_t)S * lng) / (double)sht;          // int(S * long / short)
  if (!(nl < (double)PREP_MAX_SIDE)) return COGV_ERR_UNSUPPORTED;
  const int nlong = (int)nl;
  g.nw = W <= H ? S : nlong;
  g.nh = W <= H ? nlong : S;
  auto half_even = [](int d) { const int q = d >> 1; return (d & 1) ? q + (q & 1) : q; };   // round(d / 2.0)
  g.top = half_even(g.nh - S);
  g.left = half_even(g.nw - S);
  g.taps_h = resample_axis(W, g.nw, nullptr, nullptr, nullptr, 0);
  g.taps_v = resample_axis(H, g.nh, nullptr, nullptr, nullptr, 0);
  g.scale_h = (double)W / (double)g.nw;
  g.scale_v = (double)H / (double)g.nh;
  if (g.taps_h > PREP_MAX_TAPS || g.taps_v > PREP_MAX_TAPS) return COGV_ERR_UNSUPPORTED;
  return COGV_OK;
}

// LDS of a workgroup for one image: bytes of the staged source row segment, rows of the horizontal pass kept at once
void prep_lds_need(const PrepGeo& g, int S, int& stage_bytes, int& hrows) {
  const int segw = S < PREP_SEGW ? S : PREP_SEGW;
  // the windows of segw neighbouring outputs start within (segw - 1) * scale + 1 pixels of each other
  const int64_t span = (int64_t)((segw - 1) * g.scale_h) + g.taps_h + 2;
  stage_bytes = (int)((span * 3 + 8 + 15) & ~(int64_t)15);
  hrows = (int)((PREP_BAND - 1) * g.scale_v) + g.taps_v + 2;
}

struct PrepArgs {
  const unsigned char* pack; const int* table; const int* coeffs; const float* lut; float* out;
  int S, hrows, stage_bytes;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t clip8(int acc) { return (uint32_t)clampi(acc >> PREP_PREC, 0, 255); }

// One workgroup per (band of 8 output rows, segment of 128 output columns, image); thread = output column.
// The band is worked off in runs of output rows whose source rows fit the LDS tile together: each source row of the
// run is staged as whole aligned dwords, resampled horizontally into hbuf (uint8 x 4 per pixel, rounded as Pillow rounds
// between its passes), then the vertical pass, the value table and the 16-byte stores run from hbuf.
// Every index read from the tables is clamped into the image, so a wrong table gives wrong pixels, never a wild read.
__global__ __launch_bounds__(PREP_SEGW) void image_prep_kernel(const PrepArgs p) {
  extern __shared__ __align__(16) unsigned char prep_smem[];
  uint32_t* stage = reinterpret_cast<uint32_t*>(prep_smem);
  uint32_t* hbuf = reinterpret_cast<uint32_t*>(prep_smem + p.stage_bytes);
  const int S = p.S, img = blockIdx.z, x0 = blockIdx.y * PREP_SEGW, r0 = blockIdx.x * PREP_BAND;
  const int hstride = S < PREP_SEGW ? S : PREP_SEGW;
  const int segw = min(PREP_SEGW, S - x0);
  const int* rec = p.table + (size_t)img * 8;
  const size_t off = (size_t)(uint32_t)rec[0] | ((size_t)(uint32_t)rec[1] << 32);
  const int H = rec[2], W = rec[3];
  const int* hx = p.coeffs + rec[4];               // xmin[S], count[S], k[tap][S] of the crop's columns
  const int* vx = p.coeffs + rec[5];               // the same of the crop's rows
  const int htaps = min(rec[6], W), vtaps = min(min(rec[7], H), p.hrows);
  const int col = threadIdx.x, x = x0 + col;
  const bool act = col < segw;

  // source columns of this segment (the windows move right with the output index)
  const int xl = x0 + segw - 1;
  const int lcnt = clampi(hx[S + xl], 0, htaps);
  const int c0 = clampi(hx[x0], 0, W - 1);
  const int c1 = max(clampi(hx[xl], 0, W - lcnt) + lcnt, c0);
  int hcnt = 0, hmin = c0;
  if (act) {
    hcnt = clampi(hx[S + x], 0, htaps);
    hmin = clampi(hx[x], 0, W - hcnt);
    if (hmin < c0 || hmin + hcnt > c1 || (c1 - c0) * 3 + 8 > p.stage_bytes) hcnt = 0;
  }
  const int* hk = hx + 2 * S + x;
  const size_t row_bytes = (size_t)W * 3;

  for (int r = r0; r < r0 + PREP_BAND;) {
    // the run [r, r + n): source rows [ymin, yend), at most hrows of them
    const int cnt0 = clampi(vx[S + r], 0, vtaps);
    const int ymin = clampi(vx[r], 0, H - cnt0);
    int yend = ymin + cnt0, n = 1;
    while (r + n < r0 + PREP_BAND) {
      const int cn = clampi(vx[S + r + n], 0, vtaps);
      const int yn = clampi(vx[r + n], 0, H - cn);
      if (yn < ymin || yn + cn - ymin > p.hrows) break;
      yend = max(yend, yn + cn);
      ++n;
    }
    for (int y = ymin; y < yend; ++y) {
      const size_t start = off + (size_t)y * row_bytes + (size_t)c0 * 3, end = off + (size_t)y * row_bytes + (size_t)c1 * 3;
      const size_t a0 = start & ~(size_t)3;
      const int shift = (int)(start - a0);
      const int nd = min((int)((end - a0 + 3) >> 2), p.stage_bytes >> 2);
      const uint32_t* src = reinterpret_cast<const uint32_t*>(p.pack + a0);
      for (int i = threadIdx.x; i < nd; i += PREP_SEGW) stage[i] = src[i];
      __syncthreads();
      if (act) {
        const unsigned char* sb = reinterpret_cast<const unsigned char*>(stage) + shift + (hmin - c0) * 3;
        int s0 = 1 << (PREP_PREC - 1), s1 = s0, s2 = s0;
        for (int t = 0; t < hcnt; ++t) {
          const int k = hk[(size_t)t * S];
          s0 += (int)sb[3 * t] * k; s1 += (int)sb[3 * t + 1] * k; s2 += (int)sb[3 * t + 2] * k;
        }
        hbuf[(y - ymin) * hstride + col] = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16);
      }
      __syncthreads();
    }
    if (act) {
      for (int rr = r; rr < r + n; ++rr) {
        const int vc = clampi(vx[S + rr], 0, vtaps);
        const int vm = clampi(vx[rr], 0, H - vc) - ymin;
        const int* vk = vx + 2 * S + rr;
        int s0 = 1 << (PREP_PREC - 1), s1 = s0, s2 = s0;
        for (int t = 0; t < vc; ++t) {
          const int k = vk[(size_t)t * S];
          const uint32_t h = hbuf[(vm + t) * hstride + col];
          s0 += (int)(h & 255u) * k; s1 += (int)((h >> 8) & 255u) * k; s2 += (int)((h >> 16) & 255u) * k;
        }
        f32x4 o;
        o[0] = p.lut[clip8(s0)]; o[1] = p.lut[256 + clip8(s1)]; o[2] = p.lut[512 + clip8(s2)]; o[3] = 0.f;
        *reinterpret_cast<f32x4*>(p.out + (((size_t)img * S + rr) * S + x) * 4) = o;
      }
    }
    __syncthreads();                   // hbuf is rewritten by the next run
    r += n;
  }
}

// patches [b * k][T][T][4] (pure copies) and overview [b][T][T][4] (2 x 2 means) of x [b][S][S][4], T = S / 2
__global__ void sr_patches_kernel(const float* x, const int* positions, float* patches, float* overview, int b, int S, int k) {
  const int T = S >> 1, q = S >> 2;
  const size_t tt = (size_t)T * T, npatch = (size_t)b * k * tt, total = npatch + (size_t)b * tt;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    if (i < npatch) {
      const size_t n = i / tt, px = i % tt;
      const int im = (int)(n / k), j = (int)(n % k), row = (int)(px / T), c = (int)(px % T);
      const int pos = min(max(positions[j], 0), 8);
      const int ph = (pos / 3) * q, pw = (pos % 3) * q;
      *reinterpret_cast<f32x4*>(patches + i * 4) = *reinterpret_cast<const f32x4*>(x + (((size_t)im * S + ph + row) * S + pw + c) * 4);
    } else {
      const size_t o = i - npatch, im = o / tt, px = o % tt;
      const int row = (int)(px / T), c = (int)(px % T);
      const float* s = x + ((im * S + 2 * row) * S + 2 * c) * 4;
      const f32x4 a = *reinterpret_cast<const f32x4*>(s), bb = *reinterpret_cast<const f32x4*>(s + 4);
      const f32x4 cc = *reinterpret_cast<const f32x4*>(s + (size_t)S * 4), d = *reinterpret_cast<const f32x4*>(s + (size_t)S * 4 + 4);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = 0.5f * (0.5f * a[e] + 0.5f * bb[e]) + 0.5f * (0.5f * cc[e] + 0.5f * d[e]);
      *reinterpret_cast<f32x4*>(overview + o * 4) = v;
    }
  }
}

}  // namespace

extern "C" int cogv_resample_coeffs(int in, int out, int* xmin, int* count, int* k, int max_taps) {
  if (in <= 0 || out <= 0 || out > PREP_MAX_SIDE || max_taps <= 0 || !xmin || !count || !k) return COGV_ERR_ARG;
  if (resample_axis(in, out, nullptr, nullptr, nullptr, 0) > max_taps) return COGV_ERR_UNSUPPORTED;
  resample_axis(in, out, xmin, count, k, max_taps);
  return COGV_OK;
}

extern "C" int cogv_image_prep_plan(int H, int W, int S, int* plan) {
  if (!plan) return COGV_ERR_ARG;
  PrepGeo g;
  const int rc = prep_geometry(H, W, S, g);
  if (rc != COGV_OK) return rc;
  int stage, hrows;
  prep_lds_need(g, S, stage, hrows);
  const int segw = S < PREP_SEGW ? S : PREP_SEGW;
  hrows = std::min(hrows, (PREP_LDS - stage) / (segw * 4));
  if (stage > PREP_LDS / 2 || hrows < g.taps_v) return COGV_ERR_UNSUPPORTED;
  const int v[COGV_IMAGE_PREP_PLAN_INTS] = {g.nh, g.nw, g.top, g.left, g.taps_h, g.taps_v, PREP_BAND, PREP_SEGW, hrows, stage + hrows * segw * 4};
  for (int i = 0; i < COGV_IMAGE_PREP_PLAN_INTS; ++i) plan[i] = v[i];
  return COGV_OK;
}

extern "C" int cogv_image_prep_u8(const uint8_t* pack, size_t pack_bytes, const int* table, const int* table_host,
                                  const int* coeffs, size_t coeffs_ints, int B, int S, const float* lut, float* out,
                                  void* stream) {
  if (!pack || !table || !table_host || !coeffs || !lut || !out) return COGV_ERR_ARG;
  if (B <= 0 || B > 65535 || S <= 0 || (S & 7) || S > 32768 || (pack_bytes & 3)) return COGV_ERR_ARG;
  if ((((uintptr_t)pack | (uintptr_t)out) & 15) || (((uintptr_t)table | (uintptr_t)coeffs | (uintptr_t)lut) & 3)) return COGV_ERR_ARG;
  const int segw = S < PREP_SEGW ? S : PREP_SEGW;
  int stage = 16, hrows = 1, taps_v = 1;
  for (int i = 0; i < B; ++i) {
    const int* r = table_host + (size_t)i * 8;
    const uint64_t off = (uint64_t)(uint32_t)r[0] | ((uint64_t)(uint32_t)r[1] << 32);
    PrepGeo g;
    const int rc = prep_geometry(r[2], r[3], S, g);
    if (rc != COGV_OK) return rc;
    const uint64_t bytes = (uint64_t)r[2] * (uint64_t)r[3] * 3;
    if (off > pack_bytes || bytes > pack_bytes - off) return COGV_ERR_ARG;
    if (r[6] != g.taps_h || r[7] != g.taps_v || r[4] < 0 || r[5] < 0) return COGV_ERR_ARG;
    if ((uint64_t)r[4] + (uint64_t)(2 + g.taps_h) * S > coeffs_ints || (uint64_t)r[5] + (uint64_t)(2 + g.taps_v) * S > coeffs_ints) return COGV_ERR_ARG;
    int st, hr;
    prep_lds_need(g, S, st, hr);
    stage = std::max(stage, st); hrows = std::max(hrows, hr); taps_v = std::max(taps_v, g.taps_v);
  }
  hrows = std::min(hrows, (PREP_LDS - stage) / (segw * 4));
  if (stage > PREP_LDS / 2 || hrows < taps_v) return COGV_ERR_UNSUPPORTED;
  PrepArgs a{pack, table, coeffs, lut, out, S, hrows, stage};
  static bool attr = false;
  if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&image_prep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, PREP_LDS); attr = true; }
  const dim3 grid((unsigned)(S / PREP_BAND), (unsigned)((S + PREP_SEGW - 1) / PREP_SEGW), (unsigned)B);
  hipLaunchKernelGGL(image_prep_kernel, grid, dim3(PREP_SEGW), (size_t)(stage + hrows * segw * 4), reinterpret_cast<hipStream_t>(stream), a);
  return cogv_check_launch();
}

extern "C" int cogv_sr_patches_nhwc4_f32(const float* x, const int* positions, float* patches, float* overview, int b, int S,
                                         int k, void* stream) {
  if (!x || !positions || !patches || !overview || b <= 0 || k <= 0 || S <= 0 || (S & 15)) return COGV_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)patches | (uintptr_t)overview) & 15) || ((uintptr_t)positions & 3)) return COGV_ERR_ARG;
  const size_t n = (size_t)b * (k + 1) * (S / 2) * (S / 2);
  int g = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  hipLaunchKernelGGL(sr_patches_kernel, dim3(g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, positions, patches, overview, b, S, k);
  return cogv_check_launch();
}

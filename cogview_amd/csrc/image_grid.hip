// Image egress (gfx950): the decoder's fp32 NCHW images -> the uint8 HWC bytes of torchvision.utils.make_grid followed by
// save_image's conversion, byte for byte as torch computes them on the CPU.  DESIGN.md 4.6.2 gives the arithmetic.
#include <algorithm>
#include <cmath>
#include "common.cuh"
#include "cogview_hip.h"

namespace {

constexpr int GRID_THREADS = 256;
constexpr int GRID_TILE_PX = 4096;             // output pixels of a workgroup: 12288 bytes of LDS, 768 16-byte stores
constexpr int GRID_MAX_SIDE = 1 << 15;         // largest H, W or padding accepted
constexpr int64_t GRID_MAX_GW = 1 << 28;       // largest grid side in pixels (rows, 3 * GW and the items of a tile stay in an int)
constexpr int RANGE_MAX_CHUNKS = 64;           // workgroups per image of the range kernel

struct GridGeo { int xmaps, ymaps, pad; int64_t GH, GW, out_bytes, range_bytes; };

// make_grid's geometry; a single image is returned as it is, without padding
int grid_geometry(int B, int H, int W, int nrow, int padding, int scale_each, GridGeo& g) {
  if (B <= 0 || B > 65535 || nrow <= 0 || padding < 0 || H <= 0 || W <= 0) return COGV_ERR_ARG;
  if (H > GRID_MAX_SIDE || W > GRID_MAX_SIDE || padding > GRID_MAX_SIDE) return COGV_ERR_UNSUPPORTED;
  g.xmaps = B == 1 ? 1 : (nrow < B ? nrow : B);
  g.ymaps = (B + g.xmaps - 1) / g.xmaps;
  g.pad = B == 1 ? 0 : padding;
  g.GH = (int64_t)(H + g.pad) * g.ymaps + g.pad;
  g.GW = (int64_t)(W + g.pad) * g.xmaps + g.pad;
  if (g.GW > GRID_MAX_GW || g.GH > GRID_MAX_GW || (g.GH * g.GW + GRID_TILE_PX - 1) / GRID_TILE_PX > 0x7fffffff) return COGV_ERR_UNSUPPORTED;
  g.out_bytes = g.GH * g.GW * 3;
  g.range_bytes = 8 * (int64_t)(scale_each ? B : 1);
  return COGV_OK;
}

// the source table [K][8] = {pointer low, pointer high, n, h, w, factor, first image, 0} against B images of H x W
int grid_sources(const int* t, int K, int B, int H, int W) {
  if (!t || K <= 0 || K > B) return COGV_ERR_ARG;
  int64_t first = 0;
  for (int k = 0; k < K; ++k) {
    const int* r = t + (size_t)k * 8;
    const uint64_t ptr = (uint64_t)(uint32_t)r[0] | ((uint64_t)(uint32_t)r[1] << 32);
    if (!ptr || (ptr & 15) || r[2] <= 0 || r[3] <= 0 || r[4] <= 0 || r[6] != first) return COGV_ERR_ARG;
    const int f = r[5];
    if ((f != 1 && f != 2 && f != 4 && f != 8) || (int64_t)r[3] * f != H || (int64_t)r[4] * f != W) return COGV_ERR_UNSUPPORTED;
    first += r[2];
  }
  return first == B ? COGV_OK : COGV_ERR_ARG;
}

// save_image's conversion of one value: mul(255), add_(0.5), clamp_(0, 255), to(uint8) -- two roundings, never one fused
// multiply-add (contraction is on by default for device code)
__host__ __device__ inline uint32_t grid_byte(float y) {
#pragma clang fp contract(off)
  float t = y * 255.0f;
  t = t + 0.5f;
  t = fminf(fmaxf(t, 0.0f), 255.0f);
  return (uint32_t)(int)t;
}

// max(high - low, 1e-5) as torchvision takes it: in Python floats (doubles), rounded once when div_ reads the scalar
__host__ __device__ inline float grid_divisor(double low, double high) { return (float)fmax(high - low, 1e-5); }

// an order-preserving integer image of a float: a < b as floats <=> key(a) < key(b) as unsigned (-0 sorts below +0)
__device__ __forceinline__ uint32_t range_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float range_val(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// a source pointer comes out of the table as an integer: say that it is global memory, or every load of it is a flat load
typedef __attribute__((address_space(1))) const float gfloat;
typedef __attribute__((address_space(1))) const f32x4 gf32x4;
struct SrcRec { gfloat* p; int n, h, w, f, first; };

// the record of the source batch that holds image `img`: the last one whose first image is <= img
__device__ __forceinline__ SrcRec grid_source(const int* table, int K, int img) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid * 8 + 6] <= img) lo = mid; else hi = mid - 1;
  }
  const int* r = table + lo * 8;
  SrcRec s;
  s.p = (gfloat*)((size_t)(uint32_t)r[0] | ((size_t)(uint32_t)r[1] << 32));
  s.n = r[2]; s.h = r[3]; s.w = r[4]; s.f = r[5]; s.first = r[6];
  return s;
}

// range[slot] = {~key(minimum), key(maximum)} of image blockIdx.y (slot: the image, or 0 for one range over all of them);
// the slots are zero when the kernel starts and only grow (integer atomicMax), so the result is exact whatever the order.
// An image's floats start at any multiple of 4 bytes from its batch's 16-byte aligned base: 16-byte loads between the
// first and the last 16-byte boundary inside it, single loads for the up to 3 floats in front and behind.
__global__ __launch_bounds__(GRID_THREADS) void image_range_kernel(const int* table, int K, int per_image, uint32_t* range) {
  __shared__ float red[2][GRID_THREADS / 64];
  const int img = blockIdx.y, tid = threadIdx.x;
  const SrcRec s = grid_source(table, K, img);
  const size_t count = (size_t)3 * s.h * s.w;
  const size_t e0 = (size_t)min(max(img - s.first, 0), s.n - 1) * count, e1 = e0 + count;
  const size_t a = min((e0 + 3) & ~(size_t)3, e1), z = max(e1 & ~(size_t)3, a);
  float lo = INFINITY, hi = -INFINITY;
  gf32x4* pv = (gf32x4*)s.p;
  for (size_t v = (a >> 2) + (size_t)blockIdx.x * GRID_THREADS + tid; v < (z >> 2); v += (size_t)gridDim.x * GRID_THREADS) {
    const f32x4 x = pv[v];
    lo = fminf(fminf(lo, x[0]), fminf(x[1], fminf(x[2], x[3])));
    hi = fmaxf(fmaxf(hi, x[0]), fmaxf(x[1], fmaxf(x[2], x[3])));
  }
  if (blockIdx.x == 0) {
    if (e0 + tid < a) { const float x = s.p[e0 + tid]; lo = fminf(lo, x); hi = fmaxf(hi, x); }
    if (z + tid < e1) { const float x = s.p[z + tid]; lo = fminf(lo, x); hi = fmaxf(hi, x); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
  if ((tid & 63) == 0) { red[0][tid >> 6] = lo; red[1][tid >> 6] = hi; }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < GRID_THREADS / 64; ++i) { lo = fminf(lo, red[0][i]); hi = fmaxf(hi, red[1][i]); }
    uint32_t* slot = range + 2 * (size_t)(per_image ? img : 0);
    atomicMax(slot, ~range_key(lo));
    atomicMax(slot + 1, range_key(hi));
  }
}

struct GridArgs {
  const int* table; const uint32_t* range; uint8_t* out;
  size_t npx;                                  // GH * GW
  int K, B, H, W, xmaps, pad, GW, mode;
  float low, high, d;                          // COGV_GRID_NORM_FIXED
  uint32_t pad_word;                           // the padding byte four times
};

// One workgroup per run of GRID_TILE_PX output pixels in row-major order: HWC rows follow each other in memory, so a run of
// rows is a run of bytes, and cutting it every 12288 bytes instead of at row ends puts every row end INSIDE a run -- each
// workgroup's bytes start on a 16-byte boundary and all but the last store of the grid are whole 16-byte stores.
// The run is assembled in LDS: filled with the padding byte, then one item per (output row, grid column, 4 source pixels)
// loads the three planes (16 bytes each where the source width is a multiple of 4), converts and writes each pixel's 3
// bytes `factor` times; the 16-byte stores run from LDS.  Every byte of out is written exactly once.
__global__ __launch_bounds__(GRID_THREADS) void image_grid_kernel(const GridArgs p) {
  __shared__ __align__(16) uint32_t tile[GRID_TILE_PX * 3 / 4];
  unsigned char* tb = reinterpret_cast<unsigned char*>(tile);
  const int tid = threadIdx.x;
  const size_t q0 = (size_t)blockIdx.x * GRID_TILE_PX;
  const int npx = (int)min((size_t)GRID_TILE_PX, p.npx - q0);
  for (int i = tid; i < GRID_TILE_PX * 3 / 4; i += GRID_THREADS) tile[i] = p.pad_word;
  __syncthreads();

  const int y0 = (int)(q0 / (size_t)p.GW), y1 = (int)((q0 + npx - 1) / (size_t)p.GW);
  const int QW = (p.W + 3) >> 2, per_row = p.xmaps * QW, cellh = p.H + p.pad, cellw = p.W + p.pad;
  const int nitems = (y1 - y0 + 1) * per_row;
  for (int it = tid; it < nitems; it += GRID_THREADS) {
    const int rr = it / per_row, rem = it - rr * per_row, cx = rem / QW, sj = (rem - cx * QW) * 4;
    const int y = y0 + rr, yy = y - p.pad;
    if (yy < 0) continue;
    const int cy = yy / cellh, i = yy - cy * cellh;
    const long long k = (long long)cy * p.xmaps + cx;
    if (i >= p.H || k >= p.B) continue;        // a padding row, or a cell without an image
    const SrcRec s = grid_source(p.table, p.K, (int)k);
    const int si = i / s.f;
    if (sj >= s.w || si >= s.h) continue;
    const size_t plane = (size_t)s.h * s.w;
    gfloat* src = s.p + (size_t)min(max((int)k - s.first, 0), s.n - 1) * 3 * plane + (size_t)si * s.w + sj;
    float v[3][4];
    if ((s.w & 3) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 x = *(gf32x4*)(src + c * plane);
        v[c][0] = x[0]; v[c][1] = x[1]; v[c][2] = x[2]; v[c][3] = x[3];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c][e] = sj + e < s.w ? src[c * plane + e] : 0.0f;
    }
    if (p.mode != COGV_GRID_NORM_NONE) {
      float low = p.low, high = p.high, d = p.d;
      if (p.mode != COGV_GRID_NORM_FIXED) {
        const uint32_t* slot = p.range + 2 * (size_t)(p.mode == COGV_GRID_NORM_RANGE_EACH ? k : 0);
        low = range_val(~slot[0]);
        high = range_val(slot[1]);
        d = grid_divisor((double)low, (double)high);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)            // clamp_, sub_, div_: a true division, as torch's CPU kernel divides
          v[c][e] = __fdiv_rn(__fsub_rn(fminf(fmaxf(v[c][e], low), high), low), d);
    }
    // the pixels' place in the run: the first and the last row of a run are partial
    const long long base = (long long)y * p.GW + p.pad + (long long)cx * cellw + (long long)sj * s.f - (long long)q0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (sj + e >= s.w) break;
      const unsigned char b0 = (unsigned char)grid_byte(v[0][e]), b1 = (unsigned char)grid_byte(v[1][e]), b2 = (unsigned char)grid_byte(v[2][e]);
      for (int rep = 0; rep < s.f; ++rep) {
        const long long o = base + e * s.f + rep;
        if (o >= 0 && o < npx) { tb[3 * o] = b0; tb[3 * o + 1] = b1; tb[3 * o + 2] = b2; }
      }
    }
  }
  __syncthreads();

  const int nbytes = npx * 3;
  unsigned char* dst = p.out + q0 * 3;
  for (int off = tid * 16; off < nbytes; off += GRID_THREADS * 16) {
    if (off + 16 <= nbytes) *reinterpret_cast<u32x4*>(dst + off) = *reinterpret_cast<const u32x4*>(tb + off);
    else for (int j = off; j < nbytes; ++j) dst[j] = tb[j];   // the last bytes of the grid
  }
}

}  // namespace

extern "C" int cogv_image_grid_plan(const int* table_host, int K, int B, int H, int W, int nrow, int padding, int scale_each,
                                    int64_t* plan) {
  if (!plan) return COGV_ERR_ARG;
  GridGeo g;
  int rc = grid_geometry(B, H, W, nrow, padding, scale_each, g);
  if (rc == COGV_OK && table_host) rc = grid_sources(table_host, K, B, H, W);
  if (rc != COGV_OK) return rc;
  const int64_t v[COGV_IMAGE_GRID_PLAN_INTS] = {g.xmaps, g.ymaps, g.GH, g.GW, g.out_bytes, g.range_bytes};
  for (int i = 0; i < COGV_IMAGE_GRID_PLAN_INTS; ++i) plan[i] = v[i];
  return COGV_OK;
}

extern "C" int cogv_image_range_f32(const int* table, const int* table_host, int K, int B, int H, int W, int scale_each,
                                    void* range, size_t range_bytes, void* stream) {
  if (!table || !table_host || !range || (((uintptr_t)table | (uintptr_t)range) & 3)) return COGV_ERR_ARG;
  GridGeo g;
  int rc = grid_geometry(B, H, W, 1, 0, scale_each, g);
  if (rc == COGV_OK) rc = grid_sources(table_host, K, B, H, W);
  if (rc != COGV_OK) return rc;
  if (range_bytes < (size_t)g.range_bytes) return COGV_ERR_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(range, 0, (size_t)g.range_bytes, st) != hipSuccess) return COGV_ERR_LAUNCH;
  int64_t nvec = 1;                            // 16-byte loads of the largest image
  for (int k = 0; k < K; ++k) nvec = std::max(nvec, (int64_t)3 * table_host[k * 8 + 3] * table_host[k * 8 + 4] / 4);
  const int chunks = (int)std::min<int64_t>(RANGE_MAX_CHUNKS, (nvec + GRID_THREADS * 8 - 1) / (GRID_THREADS * 8));
  hipLaunchKernelGGL(image_range_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(GRID_THREADS), 0, st, table, K, scale_each ? 1 : 0,
                     reinterpret_cast<uint32_t*>(range));
  return cogv_check_launch();
}

extern "C" int cogv_image_grid_u8(const int* table, const int* table_host, int K, int B, int H, int W, int nrow, int padding,
                                  double pad_value, int norm, const void* range, double low, double high, uint8_t* out,
                                  size_t out_bytes, void* stream) {
  if (!table || !table_host || !out || ((uintptr_t)table & 3) || ((uintptr_t)out & 15)) return COGV_ERR_ARG;
  if (norm < COGV_GRID_NORM_NONE || norm > COGV_GRID_NORM_RANGE_EACH) return COGV_ERR_ARG;
  if (norm == COGV_GRID_NORM_FIXED && !(low <= high)) return COGV_ERR_ARG;
  if (norm >= COGV_GRID_NORM_RANGE && (!range || ((uintptr_t)range & 3))) return COGV_ERR_ARG;
  GridGeo g;
  int rc = grid_geometry(B, H, W, nrow, padding, norm == COGV_GRID_NORM_RANGE_EACH, g);
  if (rc == COGV_OK) rc = grid_sources(table_host, K, B, H, W);
  if (rc != COGV_OK) return rc;
  if (out_bytes < (size_t)g.out_bytes) return COGV_ERR_ARG;
  GridArgs a;
  a.table = table; a.range = reinterpret_cast<const uint32_t*>(range); a.out = out;
  a.npx = (size_t)(g.GH * g.GW);
  a.K = K; a.B = B; a.H = H; a.W = W; a.xmaps = g.xmaps; a.pad = g.pad; a.GW = (int)g.GW; a.mode = norm;
  a.low = (float)low; a.high = (float)high; a.d = grid_divisor(low, high);
  a.pad_word = grid_byte((float)pad_value) * 0x01010101u;
  const unsigned tiles = (unsigned)((a.npx + GRID_TILE_PX - 1) / GRID_TILE_PX);
  hipLaunchKernelGGL(image_grid_kernel, dim3(tiles), dim3(GRID_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  return cogv_check_launch();
}

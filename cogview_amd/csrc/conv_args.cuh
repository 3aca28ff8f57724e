// Kernel arguments of the implicit-GEMM convolution and the host-side check that fills them from a cogv_conv_desc:
// shared by the exact-fp32 kernel (conv.hip) and the split-bf16 kernel (conv_split.hip), so that both refuse and
// accept exactly the same descriptors and walk the same geometry; and the geometry of a layer kind itself (conv_geometry),
// which the weight gradient (conv_bwd.hip) plans from as well.
#pragma once
#include "common.cuh"
#include "cogview_hip.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 32;   // tile: 128 pixels x 128 channels x 32 k
constexpr int NT = 256;

struct ConvArgs {
  const float* in; const float* w; const float* bias; float* out;
  int B, IH, IW, Cin;
  int GH, GW;               // iteration grid (pixels per image = GH*GW)
  int OH, OW, Cout;
  int in_mul, out_mul;
  int ntaps;
  int kind;                 // COGV_CONV_*: tap offsets are arithmetic (tap_offset), no table in memory
  const float* rgb_w;       // optional fused 1x1 -> 3 projection of the (bias + ReLU) output: weights [3][Cout] ...
  float* rgb_part;          // ... partial sums [Cout / 128][B * OH * OW][4] instead of the output tensor
  long long w_parity_stride;
  int relu_out;
  int relu_in;              // ReLU applied to the INPUT activations while they are parked in LDS (pre-activation residual blocks)
  const float* residual;    // optional: out += (relu_res ? max(residual, 0) : residual), same NHWC shape as out, after bias / ReLU
  int relu_res;
  int nz;                   // parities (4 for the transposed convolution, else 1)
  int K;                    // ntaps * Cin
  int M;                    // B * GH * GW
};

// Geometry of a layer kind, host only: the one place that knows it, for the forward kernels (conv_fill_args) and the weight
// gradient (wgrad_plan, conv_bwd.hip).  M is 64-bit: each caller refuses what its kernel's int arithmetic cannot hold.
struct ConvGeom {
  int GH, GW;               // iteration grid (pixels per image = GH*GW)
  int OH, OW;
  int in_mul, out_mul, ntaps;
  int nz;                   // parities (4 for the transposed convolution, else 1)
  int K;                    // ntaps * Cin
  long long M;              // B * GH * GW
};
inline int conv_geometry(int kind, int B, int IH, int IW, int Cin, ConvGeom& g) {
  g.nz = 1;
  if (kind == COGV_CONV_4X4_S2) {
    if ((IH & 1) || (IW & 1)) return COGV_ERR_ARG;
    g.GH = g.OH = IH / 2; g.GW = g.OW = IW / 2; g.in_mul = 2; g.out_mul = 1; g.ntaps = 16;
  } else if (kind == COGV_CONV_1X1) {
    g.GH = g.OH = IH; g.GW = g.OW = IW; g.in_mul = 1; g.out_mul = 1; g.ntaps = 1;
  } else if (kind == COGV_CONV_3X3_S1) {
    g.GH = g.OH = IH; g.GW = g.OW = IW; g.in_mul = 1; g.out_mul = 1; g.ntaps = 9;
  } else if (kind == COGV_CONVT_4X4_S2) {
    // out[2y+py] gets taps ky with ky = (py+1) mod 2 (+2):  py=0: ky=1 (iy=y), ky=3 (iy=y-1);  py=1: ky=0 (iy=y+1), ky=2 (iy=y)
    // weights are packed [py*2+px][co][ty*2+tx][ci] with (ty -> ky) = py==0 ? {1,3} : {0,2}, same for x  => dy = py - ty
    g.GH = IH; g.GW = IW; g.OH = 2 * IH; g.OW = 2 * IW; g.in_mul = 1; g.out_mul = 2; g.ntaps = 4;
    g.nz = 4;
  } else return COGV_ERR_UNSUPPORTED;
  g.K = (int)((long long)g.ntaps * Cin);     // the callers bound Cin (forward: IW * Cin < 2^23; weight gradient: K < 2^24)
  g.M = (long long)B * g.GH * g.GW;
  return COGV_OK;
}

// descriptor -> arguments and the one-dimensional grid size; every refusal of cogv_conv2d_nhwc_f32 happens here, before any launch
inline int conv_fill_args(const cogv_conv_desc* d, ConvArgs& a, long long& blocks) {
  if (!d || !d->in || !d->w || (!d->out && !d->rgb_partial)) return COGV_ERR_ARG;
  if (d->precision != COGV_CONV_FP32 && d->precision != COGV_CONV_BF16X3) return COGV_ERR_ARG;
  if (d->precision == COGV_CONV_BF16X3 && (!d->w_limbs || ((uintptr_t)d->w_limbs & 15))) return COGV_ERR_ARG;
  if (d->rgb_partial && (!d->rgb_w || !d->relu || (d->Cout % 128) || (((uintptr_t)d->rgb_w | (uintptr_t)d->rgb_partial) & 15))) return COGV_ERR_ARG;
  if (d->Cin <= 0 || (d->Cin & 3) || (d->Cout & 7) || d->B <= 0) return COGV_ERR_ARG;
  if (((uintptr_t)d->in | (uintptr_t)d->w | (uintptr_t)d->out | (uintptr_t)d->bias) & 15) return COGV_ERR_ARG;
  a.in = (const float*)d->in; a.w = (const float*)d->w; a.bias = (const float*)d->bias; a.out = (float*)d->out;
  a.B = d->B; a.IH = d->IH; a.IW = d->IW; a.Cin = d->Cin; a.Cout = d->Cout; a.relu_out = d->relu;
  a.relu_in = d->relu_in; a.residual = (const float*)d->residual; a.relu_res = d->relu_residual;
  if (a.residual && (d->rgb_partial || ((uintptr_t)a.residual & 15))) return COGV_ERR_ARG;
  a.rgb_w = (const float*)d->rgb_w; a.rgb_part = (float*)d->rgb_partial;
  a.kind = d->kind;
  ConvGeom g;
  const int rc = conv_geometry(d->kind, d->B, d->IH, d->IW, d->Cin, g);
  if (rc != COGV_OK) return rc;
  if (g.M > 0x7fffffffll - BM) return COGV_ERR_ARG;       // the kernels form M + BM - 1 and m0 + row in int
  a.GH = g.GH; a.GW = g.GW; a.OH = g.OH; a.OW = g.OW; a.in_mul = g.in_mul; a.out_mul = g.out_mul; a.ntaps = g.ntaps;
  a.nz = g.nz; a.K = g.K; a.M = (int)g.M;
  a.w_parity_stride = (long long)a.Cout * a.K;
  if ((long long)a.IH * a.IW * a.Cin >= (1ll << 31) || (long long)a.IW * a.Cin >= (1 << 23) || a.IH >= 32768 || a.IW >= 32768) return COGV_ERR_ARG;
  const int mtiles = (a.M + BM - 1) / BM, ntiles = (a.Cout + BN - 1) / BN;
  blocks = 8ll * ((mtiles + 7) / 8) * ntiles * a.nz;
  if (blocks > 0x7fffffffll) return COGV_ERR_ARG;
  return COGV_OK;
}

}  // namespace

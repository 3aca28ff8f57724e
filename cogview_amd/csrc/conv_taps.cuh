// Tap arithmetic shared by the forward convolution (conv.hip) and its weight gradient (conv_bwd.hip).
#pragma once
#include "cogview_hip.h"

// input offset (dy, dx) of tap `tap` for output parity z (see the header comment of conv.hip and cogv_conv2d_nhwc_f32):
//   4x4 s2 p1 conv : tap = ky*4 + kx           -> (ky - 1, kx - 1)
//   1x1            : (0, 0)
//   4x4 s2 p1 convT: tap = ty*2 + tx, z = py*2+px -> (py - ty, px - tx)   [py = 0: rows y, y-1;  py = 1: rows y+1, y]
// Pure integer arithmetic on wave-uniform values: a byte table in the kernel arguments costs a vector memory load and a
// full memory latency in front of every k-tile's operand loads (scalar loads have no byte form on gfx950).
__device__ __forceinline__ void tap_offset(int kind, int z, int tap, int& dy, int& dx) {
  if (kind == COGV_CONV_4X4_S2) { dy = (tap >> 2) - 1; dx = (tap & 3) - 1; }
  else if (kind == COGV_CONVT_4X4_S2) { dy = (z >> 1) - (tap >> 1); dx = (z & 1) - (tap & 1); }
  else if (kind == COGV_CONV_3X3_S1) { const int ky = (tap * 11) >> 5; dy = ky - 1; dx = tap - 3 * ky - 1; }   // tap / 3 for tap < 9
  else { dy = 0; dx = 0; }
}

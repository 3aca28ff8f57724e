// Shared by every GEMM generation: tile constants, the grouped-launch argument block, the XCD-aware tile order
// (gemm_tile_order.h: the host-only launch plan reads it too).
// Part of the GEMM family of csrc/gemm.hip (included there, in this order: common, gen1, lds, gen2, gen3, gen4, gemv_gen1);
// not a stand-alone header.
#pragma once
#include "gemm_tile_order.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int NTHREADS = 256;

// Every generation's kernel declares its dynamic LDS as a block-scope `extern __shared__ char smem[]`, and inside one namespace
// those declarations name ONE variable.  Generations 2-4 need it 1024-byte aligned (their swizzled images; generation 3 has a
// static int in front of it), generation 1 asks for 16, and the compiler gives the variable the alignment of the declaration it
// emits first -- which follows the order in which the host code mentions the kernels.  Declared here, before all of them, every
// later declaration inherits the 1024.
extern __shared__ __attribute__((aligned(1024))) char smem[];

// Up to MAX_GROUP independent problems of one layout in ONE persistent launch.  The four weight gradients of a
// transformer layer are 300 + 100 + 400 + 400 tiles of 256x256 = 4.7 rounds of 256 CUs (each one alone leaves its
// last round half empty or needs split-K slabs); four layers' worth is 18.75 rounds, so the partial last round
// costs 1.3 % instead of 6 %.
constexpr int MAX_GROUP = 16;
struct GroupArgs {
  GemmArgs g[MAX_GROUP];
  int item_start[MAX_GROUP + 1];     // prefix sums of tiles_m * tiles_n * splitk
  int count;
  int* sched;                        // [0..7] per-XCD item counters, [8] finished workgroups: 0 at launch, re-armed by the last workgroup
  int group_m;                       // generation 4: tile rows per raster group (the 32 CUs of an XCD work on group_m x 32/group_m tiles)
  // generation 4, cross-item prefetch (round 4): one problem, no split-K, an even number (>= 4) of k-tiles, and the three
  // divisions of the tile order replaced by multiplications (w4_tile_fast) that the host verified against w4_tile_slow for
  // every item of this geometry.  xp_ok = 0: every item boundary takes the set-up + prologue path.
  int xp_ok;
  uint32_t xp_magic_ig, xp_magic_gfull, xp_magic_gtail;
};

__device__ __forceinline__ int swz(int row) { return ((row >> 1) & 7) ^ ((row >> 4) & 7); }

}  // namespace

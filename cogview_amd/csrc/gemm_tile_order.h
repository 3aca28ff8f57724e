// Tile order of the generation-3 / 4 GEMM kernels: item (position in the launch's work list) -> tile row / column.  Shared by the
// kernels (gemm_gen3.cuh, gemm_gen4.cuh) and the host-only launch plan (gemm_plan.h), so it compiles as plain C++ too.
// Workgroup ids are dealt to the 8 XCDs round robin; inside an XCD the tiles run in raster groups of group_m tile rows x all tile
// columns, row fastest (the 32 CUs of an XCD work on group_m x 32 / group_m neighbouring tiles: shared operand panels in one L2).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define COGV_HD __host__ __device__
#else
#define COGV_HD
#endif

namespace {

COGV_HD inline void w4_tile_slow(uint32_t bid, uint32_t tiles_m, uint32_t tiles_n, uint32_t group_m, uint32_t& tm, uint32_t& tn) {
  const uint32_t nwg = tiles_m * tiles_n, q = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const uint32_t wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (bid >> 3);
  const uint32_t in_group = group_m * tiles_n, group_id = wgid / in_group, first_m = group_id * group_m;
  const uint32_t gsz = tiles_m - first_m < group_m ? tiles_m - first_m : group_m;
  tm = first_m + (wgid % in_group) % gsz;
  tn = (wgid % in_group) / gsz;
}
// x / d as the high word of x * ceil(2^32 / d): exact while x * d < 2^32 (d = 1: magic 0, handled by the caller)
inline uint32_t w4_magic(uint32_t d) { return d <= 1 ? 0u : (uint32_t)((0x100000000ull + d - 1) / d); }
COGV_HD inline uint32_t w4_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((unsigned long long)a * b) >> 32); }
COGV_HD inline void w4_tile_fast(uint32_t bid, uint32_t tiles_m, uint32_t tiles_n, uint32_t group_m, uint32_t magic_ig,
                                 uint32_t magic_gfull, uint32_t magic_gtail, uint32_t& tm, uint32_t& tn) {
  const uint32_t nwg = tiles_m * tiles_n, q = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const uint32_t wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (bid >> 3);
  const uint32_t in_group = group_m * tiles_n;
  const uint32_t group_id = in_group == 1 ? wgid : w4_mulhi(wgid, magic_ig);
  const uint32_t rem = wgid - group_id * in_group, first_m = group_id * group_m;
  const bool tail = tiles_m - first_m < group_m;
  const uint32_t gsz = tail ? tiles_m - first_m : group_m, mg = tail ? magic_gtail : magic_gfull;
  tn = gsz == 1 ? rem : w4_mulhi(rem, mg);
  tm = first_m + rem - tn * gsz;
}

}  // namespace

// Shared pieces of the large-tile MFMA GEMMs (qmm_mfma_large.hip: 16x16x32 MFMA; the 32x32x16 experiment of r2 is kept as scripts/probes/qmm_mfma_large32.hip).
#pragma once
#include "qh_mfma.h"

namespace qh {
namespace lt {

constexpr int BK = 64;
constexpr int STAGES = 3;

typedef __attribute__((address_space(3))) void* lds_ptr_t;

using namespace w8;  // qh_mfma.h: W_I8 .. W_F8E4M3FNUZ, W_DENSE, convert_pair

__device__ __forceinline__ int swz_a(int row) {
  const int q = (row + 4) & 15;
  return ((((q >> 3) ^ 1) << 2) | ((q >> 1) & 3));
}
__device__ __forceinline__ int swz_w(int row) { return (-(row >> 2)) & 3; }

struct Args {
  const void* x;
  const uint8_t* w;
  const void* scale;
  const void* bias;
  void* y;
  int M, N, K;
  int group_m;  // tile raster: groups of group_m tile rows, column-major inside a group (see tile_coords)
  // split-K (S > 1): workgroup b computes K-range b % S of tile b / S; fp32 partial sums go to `partials` and the last
  // workgroup of a tile to arrive adds them in split order (the split-K tail of qh_mfma.h)
  int S;
  int* counters;    // [tiles], zero on entry, zero on exit
  float* partials;  // [tiles * S][NJ * MI][threads] float4
};

// XCD-aware tile order.  Consecutive workgroup ids land on different XCDs (id % 8), so first give every XCD a contiguous
// band of tile indices; inside the index space walk groups of `group_m` tile rows column by column, so that a band of
// B = tiles/8 consecutive indices is a (group_m x B/group_m) rectangle: its activation panels (group_m) and weight panels
// (B/group_m) are what that XCD's L2 has to fetch.  group_m ~ sqrt(B * bytes_per_weight_row / bytes_per_activation_row)
// minimises the fetched bytes (cfg4, 128-tiles: 294 MB of fabric traffic per launch with row-major order).
__device__ __forceinline__ void tile_coords(int bid, int tiles_m, int tiles_n, int group_m, int& tm, int& tn) {
  const int nwg = tiles_m * tiles_n;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  const int per_group = group_m * tiles_n;
  const int g = t / per_group, in_g = t - g * per_group;
  const int rows = tiles_m - g * group_m < group_m ? tiles_m - g * group_m : group_m;
  tn = in_g / rows;
  tm = g * group_m + (in_g - tn * rows);
}

}  // namespace lt
}  // namespace qh

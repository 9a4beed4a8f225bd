// Shared pieces of the large-tile MFMA GEMMs: qmm_mfma_large.hip (16-bit activations x 8-bit weights), qmm_native8.hip (quantized activations,
// dense 16-bit) and qbits_mfma_large.hip (int4 prefill); the 32x32x16 experiment of r2 is kept as scripts/probes/qmm_mfma_large32.hip.
// One copy of: the kernel arguments, the XCD-aware tile raster and its host rule, the prologue-parked scale / bias table, the three-stage
// ring driver and the LDS swizzles.  (The LDS-transposed epilogue stays per unit - qmm_mfma_large.hip inline, n8::epilogue - see there.)
#pragma once
#include <type_traits>

#include "qh_mfma.h"

namespace qh {
namespace lt {

constexpr int BK = 64;
constexpr int STAGES = 3;

using qh::lds_ptr_t;
typedef __attribute__((ext_vector_type(4))) int i32x4;

using namespace w8;  // qh_mfma.h: W_I8 .. W_F8E4M3FNUZ, W_DENSE, convert_pair

__device__ __forceinline__ int swz_a(int row) {
  const int q = (row + 4) & 15;
  return ((((q >> 3) ^ 1) << 2) | ((q >> 1) & 3));
}
__device__ __forceinline__ int swz_w(int row) { return (-(row >> 2)) & 3; }  // 64-byte rows, lanes read chunk lane >> 4

struct Args {
  const void* x;      // [M, K]
  const uint8_t* w;   // [N, K]
  const void* scale;  // [N] output dtype, or null (= 1)
  const void* bias;   // [N] or null
  void* y;            // [M, N]
  int M, N, K;
  int group_m;  // tile raster: groups of group_m tile rows, column-major inside a group (see grouped_tile; 1 = row-major)
  // split-K (S > 1): S workgroups per tile, each multiplies one K-range; fp32 / int32 partial sums travel through `partials` and an arrival counter
  // per tile elects who adds them in split order (qmm_mfma_large.hip: the split-K tail of qh_mfma.h; qmm_native8.hip: its own sliced tail)
  int S;
  int* counters;    // [tiles], zero on entry, zero on exit
  float* partials;  // [tiles * S][fragments][threads] 16-byte accumulator quads
};

// XCD-aware tile order.  Consecutive workgroup ids land on different XCDs (id % 8), so first give every XCD (its own 4 MiB L2, 32 CUs) a
// contiguous band of tile indices (xcd_band); inside the index space walk groups of `gm` tile rows column by column (grouped_tile), so that a
// band of B = tiles/8 consecutive indices is a (gm x B/gm) rectangle: its activation panels (gm) and weight panels (B/gm) are what that XCD's
// L2 has to fetch - all of an XCD's workgroups walk K in step, so every operand line is fetched once per distinct tile row / column of the band.
// gm ~ sqrt(B * bytes_per_weight_row / bytes_per_activation_row) minimises the fetched bytes (cfg4, 128-tiles: 294 MB of fabric traffic per
// launch with row-major order; r5, quantized activations: L2 misses -27 %, (512,8192,8192) int8 / fp8 46.1 / 46.5 -> 42.8 / 43.4 us).
__device__ __forceinline__ int xcd_band(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
__device__ __forceinline__ void grouped_tile(int t, int tiles_m, int tiles_n, int gm, int& tm, int& tn) {
  const int per_group = gm * tiles_n;
  const int g = t / per_group, in_g = t - g * per_group;
  const int rows = tiles_m - g * gm < gm ? tiles_m - g * gm : gm;
  tn = in_g / rows;
  tm = g * gm + (in_g - tn * rows);
}
__device__ __forceinline__ void tile_coords(int bid, int tiles_m, int tiles_n, int group_m, int& tm, int& tn) {
  grouped_tile(xcd_band(bid, tiles_m * tiles_n), tiles_m, tiles_n, group_m, tm, tn);
}
// host: per-XCD band of B tiles as a (g x B/g) rectangle: fetched bytes per k ~ g * BM * 2 (16-bit activations) + (B / g) * weight_row_bytes
// -> g = sqrt(B * weight_row_bytes / (2 * BM))
inline int raster_group_m(int tiles, int tiles_m, int BM, int weight_row_bytes) {
  const int band = (tiles + 7) / 8;
  int g = 1;
  while ((g + 1) * (g + 1) * 2 * BM <= band * weight_row_bytes) ++g;
  const int forced = env_int("QUANTO_HIP_GROUP_M", 0);  // experiments
  if (forced > 0) g = forced;
  return g < tiles_m ? g : tiles_m;
}

// ---- r6: per-feature scale / bias of the tile, parked in LDS behind the operand ring by the prologue ------------------------------------
// The epilogue used to fetch them from global memory after the K loop: a round trip in front of the first output byte of every tile, and all
// tiles of these grids end together.  One load per thread (threads >= 2 * BN), issued in FRONT of the prologue's DMA - the oldest entry of the
// in-order vector-memory queue, so the prologue's counted wait covers it - and stored behind the ring before the prologue's barrier.  As asm:
// a load hipcc can see makes it drain the DMA queue (vmcnt(0)) at the store.  (cfg2 -1.4 us, cfg4 -1.1 us.)
template <int ODT, int BN>
struct FeatureTable {
  using T = typename Elem<ODT>::T;
  static constexpr int BYTES = 2 * BN * (int)sizeof(T);  // [scale x BN | bias x BN]
  uint32_t v;
  bool have;
  __device__ __forceinline__ void fetch(const void* scale, const void* bias, int N, int n0, int tid) {
    v = 0;
    have = tid < BN ? scale != nullptr : bias != nullptr;
    if (tid < 2 * BN && have) {
      int n = n0 + (tid < BN ? tid : tid - BN);
      n = n < N ? n : N - 1;
      const T* src = reinterpret_cast<const T*>(tid < BN ? scale : bias) + n;
      if constexpr (sizeof(T) == 2)
        asm volatile("global_load_ushort %0, %1, off" : "=v"(v) : "v"(src) : "memory");
      else
        asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(src) : "memory");
    }
  }
  // after the prologue's vmcnt wait, before its barrier
  __device__ __forceinline__ void park(uint8_t* tab, int tid) {
    asm volatile("" : "+v"(v));
    if (tid < 2 * BN) {
      if constexpr (sizeof(T) == 2) {
        const uint16_t one = ODT == QUANTO_HIP_BF16 ? 0x3F80 : 0x3C00;
        reinterpret_cast<uint16_t*>(tab)[tid] = have ? (uint16_t)v : (tid < BN ? one : (uint16_t)0);
      } else {
        reinterpret_cast<uint32_t*>(tab)[tid] = have ? v : (tid < BN ? 0x3F800000u : 0u);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
};

// Driver of a three-stage ring (tile kt lives in stage kt % 3, tile kt + 2 is fetched during tile kt), NK >= 2:
// TILE(stage tag, kt, dma, barrier) - integral_constants in the steady state, run-time flags in the tail.
// A macro: as a __forceinline__ function taking the generic lambda, hipcc laid out the K loops of both users differently.
#define QH_RING3_FOR_EACH_TILE(NK, TILE)                                                                       \
  do {                                                                                                         \
    using yes = std::integral_constant<bool, true>;                                                            \
    using S0 = std::integral_constant<int, 0>;                                                                 \
    using S1 = std::integral_constant<int, 1>;                                                                 \
    using S2 = std::integral_constant<int, 2>;                                                                 \
    static_assert(qh::lt::STAGES == 3, "unrolled over three stages");                                          \
    int kt = 0;                                                                                                \
    for (; kt + 4 < (NK); kt += 3) { /* three tiles that all still have a tile kt + 2 to fetch */              \
      TILE(S0{}, kt, yes{}, yes{});                                                                            \
      TILE(S1{}, kt + 1, yes{}, yes{});                                                                        \
      TILE(S2{}, kt + 2, yes{}, yes{});                                                                        \
    }                                                                                                          \
    /* tail: 2..4 tiles, kt % 3 == 0; the last two have nothing left to prefetch, the last one no barrier */   \
    const int rem = (NK) - kt;                                                                                 \
    TILE(S0{}, kt, rem > 2, true);                                                                             \
    TILE(S1{}, kt + 1, rem > 3, rem > 2);                                                                      \
    if (rem > 2) TILE(S2{}, kt + 2, false, rem > 3);                                                           \
    if (rem > 3) TILE(S0{}, kt + 3, false, false);                                                             \
  } while (0)

}  // namespace lt
}  // namespace qh

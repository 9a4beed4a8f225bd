// The K split of the convolution kernels (qconv_mfma.hip, qconv_a8.hip): how many splits, the scratch they take, and the separate kernel's
// sum of the partial tiles.
#pragma once
#include <type_traits>

#include "qh_common.h"

namespace qh {

// K split of the convolutions (qconv_mfma.hip, qconv_a8.hip; BK k per K-tile, BM x BN output tiles).  The tile kernel is bound by its gather
// per K-tile (~1.9 us per workgroup and K-tile whatever M is), so what matters is how many workgroups run at once: split until the grid reaches
// ~2 workgroups per CU, keeping at least 4 K-tiles per split (r5, after the gather and the epilogue got cheaper: profiles/r05_qconv2d_split_sweep.jsonl
// - 3 per split over-split 26-49-tile grids by 10-14 %).  1 = no split (and no workspace).
template <int BK, int BM, int BN>
static int conv_pick_split(int64_t M, int64_t N, int64_t K) {
  const int forced = env_int("QUANTO_HIP_CONV_SPLIT", 0);  // experiments
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN), nk = (K + BK - 1) / BK;
  if (forced > 0) return (int)(forced <= nk ? forced : nk);
  // measured (profiles/r04_qconv2d_forced_split.jsonl): at 196 tiles a split of 2 costs more in partial sums than the second workgroup per CU
  // brings while K is short (9 K-tiles 23.9 -> 31.9 us, 18 K-tiles 43.0 -> 44.7) and pays from ~32 K-tiles on (192 tiles x 45: 81.6 -> 72.9,
  // 256 tiles x 49: 86.8 -> 84.3)
  if (tiles > 128) return tiles <= 256 && nk >= 32 ? 2 : 1;
  int s = 1;
  while (tiles * (s + 1) <= 512 && nk / (s + 1) >= 4 && s < 64) ++s;
  return s;
}
// S partial tiles of 4-byte accumulators (fp32, int32 for int8 x int8); no counters: a second kernel adds them
template <int BM, int BN>
static size_t conv_split_workspace(int64_t M, int64_t N, int S) { return S <= 1 ? 0 : (size_t)S * ((M + BM - 1) / BM) * ((N + BN - 1) / BN) * (BM * BN * 4); }

// Split-K reduce (one wave per (output tile, wave slot of the tile kernel), launched as a separate kernel after the tile kernel): ACC, an
// AV[4][2] of the lane's eight fragments of slot WAVE, = the S partial tiles ([S][tiles][8 slots][8 fragments][64 lanes] of AV: float4, or
// int4 for int8 x int8) added in split order, four splits' loads in flight together.  A macro for the reason given at QH_SPLITK_SUM in
// qh_mfma.h: as a function, hipcc optimized the loop before inlining it and the reduce kernels came out with other registers (132 -> 110 VGPRs).
// fp32 partials are added per component, int32 ones as vectors: the two forms the kernels were tuned with.
#define QH_CONV_SPLIT_SUM(AV, PARTIALS, S, LANE, WAVE, ACC)                                                                                 \
  {                                                                                                                                       \
    _Pragma("unroll") for (int qh_i = 0; qh_i < 4; ++qh_i) _Pragma("unroll") for (int qh_j = 0; qh_j < 2; ++qh_j)(ACC)[qh_i][qh_j] =      \
        AV{0, 0, 0, 0};                                                                                                                   \
    const AV* const qh_base =                                                                                                             \
        reinterpret_cast<const AV*>(PARTIALS) + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (8 * 8 * 64) + ((WAVE) * 8) * 64 + (LANE); \
    const size_t qh_split_stride = (size_t)gridDim.y * gridDim.x * (8 * 8 * 64);                                                          \
    for (int qh_sp0 = 0; qh_sp0 < (S); qh_sp0 += 4) {                                                                                     \
      AV qh_v[4][8];                                                                                                                      \
      _Pragma("unroll") for (int qh_u = 0; qh_u < 4; ++qh_u) {                                                                            \
        const int qh_sp = qh_sp0 + qh_u < (S) ? qh_sp0 + qh_u : (S) - 1;                                                                  \
        _Pragma("unroll") for (int qh_f = 0; qh_f < 8; ++qh_f) qh_v[qh_u][qh_f] = qh_base[qh_sp * qh_split_stride + qh_f * 64];           \
      }                                                                                                                                   \
      _Pragma("unroll") for (int qh_u = 0; qh_u < 4; ++qh_u) if (qh_sp0 + qh_u < (S)) {                                                   \
        _Pragma("unroll") for (int qh_f = 0; qh_f < 8; ++qh_f) {                                                                          \
          if constexpr (std::is_same<AV, f32x4>::value) {                                                                                 \
            _Pragma("unroll") for (int qh_r = 0; qh_r < 4; ++qh_r)(ACC)[qh_f >> 1][qh_f & 1][qh_r] += qh_v[qh_u][qh_f][qh_r];             \
          } else {                                                                                                                        \
            (ACC)[qh_f >> 1][qh_f & 1] += qh_v[qh_u][qh_f];                                                                               \
          }                                                                                                                               \
        }                                                                                                                                 \
      }                                                                                                                                   \
    }                                                                                                                                     \
  }

}  // namespace qh

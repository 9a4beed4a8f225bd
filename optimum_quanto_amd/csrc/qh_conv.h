// What the implicit-GEMM convolutions (qconv_mfma.hip, qconv_a8.hip) share.  Host: the geometry of a call (ConvGeom), the one rule for what the
// kernels can index, the geometry part of a kernel's arguments, the K split (how many splits, their scratch, the plan against a caller's workspace).
// Device: the tap-table gather - LDS tile layout, k -> (offset, tap) table, the validity test of a tap, the NCHW epilogue - and the split's partial
// tiles (parking store, the separate kernel's sum).  Parameterised by what differs between the units: element bytes ES (2 / 1), BK (64 / 128 at the
// same 128-byte LDS row), WIDE, PAIR and the accumulator vector type.
#pragma once
#include <type_traits>

#include "qh_kernels.h"

namespace qh {

// ---- host: geometry ----------------------------------------------------------------------------------------------------------------------------
// (ConvGeom, one conv2d call: qh_kernels.h)
constexpr int kConvBM = 128;  // pixels per output tile, every implicit-GEMM kernel

// What the implicit-GEMM kernels index: one validity bit per tap (two 64-bit mask words, one bit kept free), k and m below 2^24 (magic-number and
// fp32-reciprocal divisions), byte offsets into x (two bytes per element at most) and element offsets into y / w in 31 bits, pixel tiles in grid.y
// (the K split is at most 64: grid.z)
static bool conv_geometry_ok(const ConvGeom& g) {
  return g.B >= 1 && g.OH >= 1 && g.OW >= 1 && g.K() >= 1 && g.K() < (1ll << 24) && g.KH * g.KW <= 127 && g.B * g.cin * g.H * g.W < (1ll << 30) &&
         g.B * g.OC * g.OH * g.OW < (1ll << 31) && g.OC * g.K() < (1ll << 31) && (g.M() + kConvBM - 1) / kConvBM <= 65535;
}

// ceil(2^32 / d) for conv_div_small; 0 when the divisor is 1
static uint32_t div_magic(int d) { return d <= 1 ? 0u : (uint32_t)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d); }

// the geometry part of a kernel's Args (conv::Args, conv8::Args: the same members by name), magic numbers included
template <typename A>
static void conv_set_geometry(A& a, const ConvGeom& g) {
  a.M = (int)g.M(), a.N = (int)g.OC, a.K = (int)g.K();
  a.cin = (int)g.cin, a.H = (int)g.H, a.W = (int)g.W, a.KH = (int)g.KH, a.KW = (int)g.KW, a.OH = (int)g.OH, a.OW = (int)g.OW;
  a.sh = g.sh, a.sw = g.sw, a.ph = g.ph, a.pw = g.pw, a.dh = g.dh, a.dw = g.dw;
  a.khw_magic = div_magic((int)(g.KH * g.KW)), a.kw_magic = div_magic((int)g.KW);
}

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
// the split a call runs with: conv_pick_split's, or 1 when the caller's workspace cannot hold its partial tiles
template <int BK, int BM, int BN>
static int conv_plan_split(int64_t M, int64_t N, int64_t K, const void* workspace, size_t workspace_bytes) {
  const int S = conv_pick_split<BK, BM, BN>(M, N, K);
  return S > 1 && !ws_holds(workspace, workspace_bytes, conv_split_workspace<BM, BN>(M, N, S)) ? 1 : S;
}

// ---- device: the tap-table gather ----------------------------------------------------------------------------------------------------------------
// byte-aligned 4-, 8- and 16-byte loads (K = cin KH KW need not be a multiple of anything: an RGB stem has K = 27 or 147): hipcc lowers them to
// global_load_dword / x2 / x4, which the gfx950 memory pipeline serves at any alignment (unaligned access mode, the HSA default)
struct __attribute__((packed, aligned(1))) U4u { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(1))) U2u { uint32_t x, y; };
struct __attribute__((packed, aligned(1))) U1u { uint32_t x; };

// n / d and its remainder for a small run-time d: q = mulhi(n, ceil(2^32 / d)), exact for n < 2^24 and d <= 127 (n (M d - 2^32) < 2^24 * 127 < 2^32);
// the magic numbers come from the host (div_magic; 0: d = 1).  As integer divisions they were ~60 instructions per table entry.
__device__ __forceinline__ int conv_div_small(int n, int d, uint32_t magic, int& rem) {
  const int q = magic ? (int)__umulhi((uint32_t)n, magic) : n;
  rem = n - q * d;
  return q;
}
// Tap table of the split's K-tile t (K-tile kt_lo + t of the call) into buffer t & 1 of ktab ([2][BK]): per k of the tile {byte offset of tap (c, i, j) relative to the window's top-left tap (signed),
// tap number i KW + j}; a k behind K gets tap NO_TAP, the bit no validity word ever sets.  Threads 0 .. BK - 1 (one wave per K-tile for 2-byte
// elements, two for bytes) while the others wait for it at the K loop's barrier.
template <int ES, int BK, int NO_TAP, typename A>
__device__ __forceinline__ void conv_fill_ktab(const A& a, int2* ktab, int kt_lo, int t, int tid) {
  if (tid < BK) {
    const int k = (kt_lo + t) * BK + tid;
    int rem, kj;
    const int ci = conv_div_small(k, a.KH * a.KW, a.khw_magic, rem);
    const int ki = conv_div_small(rem, a.KW, a.kw_magic, kj);
    ktab[(t & 1) * BK + tid] = k < a.K ? make_int2(ES * ((ci * a.H + ki * a.dh) * a.W + kj * a.dw - (a.ph * a.W + a.pw)), rem) : make_int2(0, NO_TAP);
  }
}

// -1 when tap `tp` of a pixel with validity words w0 (taps 0 .. 63; narrow windows: 0 .. 31) and w1 (64 .. 127) lies inside the image, else 0
template <bool WIDE>
__device__ __forceinline__ int conv_tap_ok(uint64_t w0, uint64_t w1, int tp) {
  if constexpr (WIDE)
    return -(int)((((tp & 64) ? w1 : w0) >> (tp & 63)) & 1ull);
  else
    return __builtin_amdgcn_sbfe((uint32_t)w0, tp, 1);
}

// Epilogue: the lane's 4 x 2 accumulator fragments (AV: f32x4, or int4 for int8 x int8) -> y in NCHW, v = fp32(acc) * channel_scale(n) rounded
// to the output dtype, then + bias rounded again (the reference's order).  D row = pixel (lane >> 4) * 4 + r of fragment i, D column = channel
// lane & 15 of fragment j; the lane's four rows are four neighbouring pixels of one channel plane - ONE 8- / 16-byte store when they lie in one
// image, the plane size is a multiple of 4 and y is aligned (r5; before: four 2-byte stores, each with its own integer division by the plane size
// - the epilogue and the prologue were a third of a (8,128,56,56) -> 128 call, profiles/r05_qconv2d_ablations.jsonl).  PL > 1 (packed sub-byte
// weights): the tile's 128 columns are (128 / PL) packed rows x PL planes; plane pl holds channels pl * P + p.
// WORDING: the two places where the units' epilogues were written differently - m / L and the test for a channel behind N, down to how the
// channel sum is parenthesised.  hipcc's listing follows the wording, so each unit keeps its own behind this parameter: with the 8-bit wording
// qconv_mfma.hip's one-byte-weight kernels come out 12-14 instructions shorter, with the 16-bit wording qconv_a8.hip's 11 longer.  Measured with
// one wording for both: the 8-bit one costs qconv_mfma.hip's six reduce kernels an SGPR each; the 16-bit one costs qconv_a8.hip no register (16
// of its kernels use fewer) but moves an instruction in front of their K loops.  CONV_EPI_16BIT: m / L through the fp32 reciprocal, corrected (m < 2^24,
// conv_geometry_ok), a channel behind N becomes -1.  CONV_EPI_8BIT: integer division, the channel tested directly.
enum { CONV_EPI_16BIT = 0, CONV_EPI_8BIT = 1 };
template <int DT, int PL, int WORDING, typename AV, typename A, typename SC>
__device__ __forceinline__ void conv_store_tile(const A& a, const AV (&acc)[4][2], int m0, int nt, int wm, int wn, int lane, SC channel_scale) {
  using E = Elem<DT>;
  using T = typename E::T;
  constexpr int BN = 128;
  T* yg = reinterpret_cast<T*>(a.y);
  const int M = a.M, N = a.N, P = N / (PL > 1 ? PL : 2), L = a.OH * a.OW;
  const float r_l = 1.0f / (float)L;
  const bool vec = (L & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & (4 * sizeof(T) - 1)) == 0;
  int bq[4], lq[4];  // image and offset inside the plane of the first of the lane's four pixels of fragment i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + (lane >> 4) * 4;
    int b, l;
    if constexpr (WORDING == CONV_EPI_16BIT) {
      b = (int)((float)m * r_l), l = m - b * L;
      if (l < 0) {
        --b;
        l += L;
      } else if (l >= L) {
        ++b;
        l -= L;
      }
    } else {
      b = m / L, l = m - b * L;
    }
    bq[i] = b;
    lq[i] = l;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int n;
    if constexpr (PL > 1) {
      constexpr int RPT = BN / PL;
      const int tc = wn * 32 + j * 16 + (lane & 15);
      const int p = nt * RPT + (tc % RPT);
      n = p < P ? p + (tc / RPT) * P : -1;
      if (n < 0) continue;
    } else if constexpr (WORDING == CONV_EPI_16BIT) {
      n = nt * BN + (wn * 32 + j * 16 + (lane & 15));
      n = n < N ? n : -1;
      if (n < 0) continue;
    } else {
      n = nt * BN + wn * 32 + j * 16 + (lane & 15);
      if (n >= N) continue;
    }
    const float sc = channel_scale(n);
    const bool has_bias = a.bias != nullptr;
    const float bv = has_bias ? E::to_f32(reinterpret_cast<const T*>(a.bias)[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + (lane >> 4) * 4;
      if (m >= M) continue;
      T out[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) out[r] = scale_round_add_round<DT>((float)acc[i][j][r], sc, has_bias, bv);
      T* dst = yg + ((size_t)bq[i] * N + n) * L + lq[i];
      if (vec && m + 3 < M) {  // (L % 4 == 0 and m % 4 == 0: the four pixels are in one image, aligned)
        if constexpr (sizeof(T) == 2)
          *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(out);
        else
          *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(out);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (m + r < M) {
            int bb = bq[i], ll = lq[i] + r;
            while (ll >= L) {  // an image ends inside the lane's four pixels (planes of fewer than 4 pixels: more than once)
              ll -= L;
              ++bb;
            }
            yg[((size_t)bb * N + n) * L + ll] = out[r];
          }
      }
    }
  }
}

// park a split's partial tile ([S][tiles][8 waves][8 fragments][64 lanes] of AV): one 1 KiB store per wave and fragment
template <typename AV>
__device__ __forceinline__ void conv_park_tile(void* partials, int sp, int nt, int wave, int lane, const AV (&acc)[4][2]) {
  AV* mine = reinterpret_cast<AV*>(partials) + ((size_t)(sp * gridDim.y + blockIdx.y) * gridDim.x + nt) * (8 * 8 * 64) + (wave * 8) * 64 + lane;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) mine[(i * 2 + j) * 64] = acc[i][j];
}

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

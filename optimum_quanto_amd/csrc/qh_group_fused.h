// Shared pieces of the two group-fused int4 / int2 GEMMs: qbits_mfma_fused.hip (16-bit activations, route mfma_fused4) and qbits_a8_fused.hip
// (int8 / e4m3 / e5m2 activations, routes a8_fused_*).  Both are one structure: workgroup = 8 waves, BM tokens x 128 features, wave = all BM tokens
// x 16 features, K-tile = one group of 128, LDS-DMA ring of two stages one tile ahead, the scale / shift tables of the workgroup's groups parked in
// LDS, group accumulators double-buffered so that the fold of tile kt-1 is sliced over the matrix steps of tile kt, the group sums of the
// activation from an all-ones matrix product, split-K through the tail of qh_mfma.h, a 4-features-per-lane epilogue.  One copy of: the table fill
// (element form), the table / group-sum reads of the fold, the fold element, the two-stage loop driver, the split-K glue, the epilogue, the weight
// piece's DMA source and swizzled read offsets; on the host the planner (token tile and K split), the tile count, the workspace formula and the
// "no scratch" rule.  The kernels, their Args and their operand construction stay in the units.
// Functions where hipcc compiles the call to the instructions of the pasted code (checked on the listings of both units), macros in the style of
// QH_SPLITK_* (qh_mfma.h) where it does not: as __forceinline__ templates the table fill, the loop driver, the split-K glue, the epilogue and even
// the one-line read offset each gave both kernels other registers or another instruction order.
#pragma once
#include <type_traits>

#include "qh_mfma.h"
#include "qh_quantize.h"

namespace qh {
namespace gf {

constexpr int BK = 128, NF = 128, WAVES = 8, STAGES = 2;  // NF: output features per workgroup, whatever the weight width
static_assert(NF == 128 && WAVES * 64 == 512, "QH_GF_FILL_TABLES: feature tid & 127, groups tid >> 7, + 4, ...");

// ---- prologue: scale / shift of the workgroup's NF features x NK groups -> SZ[(g * 2 + {0, 1}) * NF + f], element by element -------------------
// thread -> feature tid & 127 (plane f / PR, packed row f % PR), groups (tid >> 7), +4, ...: no division in front of the loop.  Integer
// zero-points (INT_SHIFT) are stored as the 16-bit type E::T: exact.
#define QH_GF_FILL_TABLES(E, INT_SHIFT, PR, SZ, SCALE, SHIFT, TID, P0, P, G, KT0, NK)                                        \
  {                                                                                                                         \
    using qh_T = typename E::T;                                                                                             \
    const int qh_f = (TID) & (qh::gf::NF - 1);                                                                              \
    int qh_p = (P0) + (qh_f & ((PR) - 1));                                                                                  \
    qh_p = qh_p < (P) ? qh_p : (P) - 1;                                                                                     \
    const size_t qh_row = (size_t)(qh_p + (qh_f / (PR)) * (P)) * (G) + (KT0);                                               \
    for (int qh_g = (TID) >> 7; qh_g < (NK); qh_g += (qh::gf::WAVES * 64) >> 7) {                                           \
      (SZ)[(qh_g * 2 + 0) * qh::gf::NF + qh_f] = reinterpret_cast<const qh_T*>(SCALE)[qh_row + qh_g];                       \
      if constexpr (INT_SHIFT)                                                                                              \
        (SZ)[(qh_g * 2 + 1) * qh::gf::NF + qh_f] = E::from_f32((float)(int8_t) reinterpret_cast<const uint8_t*>(SHIFT)[qh_row + qh_g]); \
      else                                                                                                                  \
        (SZ)[(qh_g * 2 + 1) * qh::gf::NF + qh_f] = reinterpret_cast<const qh_T*>(SHIFT)[qh_row + qh_g];                     \
    }                                                                                                                       \
  }

// ---- the fold's inputs: scale and shift term of the lane's 4 consecutive features (floc) for group g, XS[token of this lane, g] per fragment -----
// HAS_OFFSET: the weight operand carries Mma<DT>::OFFSET on top of the nibble (128 / 1024 in qbits_mfma_fused.hip) and the shift term takes it
// back; kernels whose operands are the plain codes get z / s * z - selected at compile time, not by an offset of 0: z + 0 * s is NaN for an
// infinite scale and another instruction sequence.  s * (q - zp) = s * q - (s * zp): one fp32 rounding of the product, stated in the oracle.
template <int DT, bool INT_SHIFT, bool HAS_OFFSET>
__device__ __forceinline__ void load_sz(const typename Elem<DT>::T* sz, int g, int floc, float (&s4)[4], float (&z4)[4]) {
  using E = Elem<DT>;
  typename E::T s4t[4], z4t[4];
  *reinterpret_cast<uint2*>(s4t) = *reinterpret_cast<const uint2*>(sz + (g * 2 + 0) * NF + floc);
  *reinterpret_cast<uint2*>(z4t) = *reinterpret_cast<const uint2*>(sz + (g * 2 + 1) * NF + floc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    s4[r] = E::to_f32(s4t[r]);
    const float z = E::to_f32(z4t[r]);
    if constexpr (HAS_OFFSET)
      z4[r] = INT_SHIFT ? s4[r] * (z + Mma<DT>::OFFSET) : z + Mma<DT>::OFFSET * s4[r];
    else
      z4[r] = INT_SHIFT ? s4[r] * z : z;
  }
}
template <int BM, int MI>
__device__ __forceinline__ void load_xs(const float* xs_slot, int kt_prev, int fi, float (&xsp)[MI]) {
#pragma unroll
  for (int i = 0; i < MI; ++i) xsp[i] = xs_slot[(kt_prev & 1) * BM + i * 16 + fi];
}

// ---- one element of the fold of a group: acc = fma(-z, XS, fma(s, P_g, acc)); slice q (0 .. 4 MI - 1) is feature r = q & 3 of fragment q >> 2 ----
// Two FMAs, as asm: left as C++, hipcc SINKS the whole fold (pure arithmetic whose result nobody reads before the next fold) out of the matrix
// steps to the end of the loop body, where it runs as one block while the matrix pipe idles (and its SLP vectorizer turns it into v_pk_* there:
// both units are built with -fno-slp-vectorize).  The operands were produced a tile ago (pg) or by LDS reads hipcc waits for.  int32 group
// accumulators (int8 activations) are converted in front.
template <class GV, int MI>
__device__ __forceinline__ void fold_slice(f32x4 (&acc)[MI], const GV (&pg)[MI], int q, const float (&s4)[4], const float (&z4)[4],
                                           const float (&xsp)[MI]) {
  const int i = q >> 2, r = q & 3;
  float v = acc[i][r];
  if constexpr (std::is_same<GV, f32x4>::value) {
    asm volatile("v_fmac_f32 %0, %1, %2\n\tv_fma_f32 %0, -%3, %4, %0" : "+v"(v) : "v"(s4[r]), "v"(pg[i][r]), "v"(z4[r]), "v"(xsp[i]));
  } else {
    float p;
    asm volatile("v_cvt_f32_i32 %1, %2\n\tv_fmac_f32 %0, %3, %1\n\tv_fma_f32 %0, -%4, %5, %0"
                 : "+v"(v), "=&v"(p)
                 : "v"(pg[i][r]), "v"(s4[r]), "v"(z4[r]), "v"(xsp[i]));
  }
  acc[i][r] = v;
}

// ---- the K loop over a two-stage ring: the stage of tile kt is its parity, the group accumulators alternate A, B, A ... ------------------------
// TILE(kt, accumulate into, fold from, have_prev tag, stage tag); FINAL_FOLD(set of the last tile); then nothing is in flight any more.
#define QH_GF_FOR_EACH_TILE(NK, TILE, FINAL_FOLD, A, B)                                                                      \
  do {                                                                                                                      \
    using yes = std::integral_constant<bool, true>;                                                                         \
    using st0 = std::integral_constant<int, 0>;                                                                             \
    using st1 = std::integral_constant<int, 1>;                                                                             \
    static_assert(qh::gf::STAGES == 2, "unrolled over two stages");                                                         \
    TILE(0, A, B, std::integral_constant<bool, false>{}, st0{});                                                            \
    int kt = 1;                                                                                                             \
    for (; kt + 2 <= (NK); kt += 2) {                                                                                       \
      TILE(kt, B, A, yes{}, st1{});                                                                                         \
      TILE(kt + 1, A, B, yes{}, st0{});                                                                                     \
    }                                                                                                                       \
    if (kt < (NK)) {                                                                                                        \
      TILE(kt, B, A, yes{}, st1{}); /* NK even: the last tile landed in set B */                                            \
      FINAL_FOLD(B);                                                                                                        \
    } else {                                                                                                                \
      FINAL_FOLD(A);                                                                                                        \
    }                                                                                                                       \
    /* the re-requested tiles past the end: nothing may land in LDS after the kernel moved on */                            \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                        \
  } while (0)

// ---- split-K: fp32 partial tiles through the workspace, the last workgroup of a tile adds them in split order (the tail of qh_mfma.h) ----------
// RETURNS from the kernel in every workgroup but the tile's last arriver.  The flag word is the first of SMEM (the ring is drained);
// (BM == 64 ? 4 : 2) splits x MI fragments = 16 float4 registers of loads in flight per wait.
#define QH_GF_SPLITK(BM, MI, ACC, PARTIALS, COUNTERS, S, SP, TID, SMEM)                                                      \
  {                                                                                                                         \
    const int qh_tile = blockIdx.y * gridDim.x + blockIdx.x;                                                                \
    int* const qh_flag = reinterpret_cast<int*>(SMEM);                                                                      \
    QH_SPLITK_ARRIVE(MI, qh::gf::WAVES * 64, PARTIALS, qh_tile * (S) + (SP), ACC, (COUNTERS) + qh_tile, qh_flag, TID, (void)0, (void)0); \
    if (*qh_flag != (S) - 1) return;                                                                                        \
    QH_SPLITK_SUM(MI, qh::gf::WAVES * 64, ((BM) == 64 ? 4 : 2), MI, PARTIALS, qh_tile, S, ACC, (COUNTERS) + qh_tile, TID, (void)0); \
  }

// ---- epilogue: 4 consecutive features (packed rows PL .. PL + 3 of plane PLANE) of one token per fragment: 8-byte stores, per element on the ragged
// edge.  STORE_ROW: the condition under which token m is stored; SCALE: a statement on the fp32 value v in front of everything else (the activation
// scale of the quantized-activation kernel); the element stored is round_add_round (qh_common.h) of v.
#define QH_GF_EPILOGUE(DT, MI, ACC, Y, BIAS, M0, FI, N, P, PL, PLANE, STORE_ROW, SCALE)                                      \
  {                                                                                                                         \
    using qh_E = qh::Elem<DT>;                                                                                              \
    using qh_T = typename qh_E::T;                                                                                          \
    qh_T* const qh_y = reinterpret_cast<qh_T*>(Y);                                                                          \
    const bool qh_has_bias = (BIAS) != nullptr;                                                                             \
    const int qh_pl = (PL);                     /* first of the lane's 4 packed rows */                                    \
    const int qh_n0 = qh_pl + (PLANE) * (P);    /* 4 consecutive output features n0 .. n0 + 3 */                           \
    float qh_bv[4] = {0.f, 0.f, 0.f, 0.f};                                                                                  \
    if (qh_has_bias) {                                                                                                      \
      _Pragma("unroll") for (int qh_r = 0; qh_r < 4; ++qh_r)                                                                \
        qh_bv[qh_r] = qh_pl + qh_r < (P) ? qh_E::to_f32(reinterpret_cast<const qh_T*>(BIAS)[qh_n0 + qh_r]) : 0.f;           \
    }                                                                                                                       \
    _Pragma("unroll") for (int qh_i = 0; qh_i < (MI); ++qh_i) {                                                             \
      const int m = (M0) + qh_i * 16 + (FI);                                                                                \
      if (STORE_ROW) {                                                                                                      \
        qh_T qh_out[4];                                                                                                     \
        _Pragma("unroll") for (int qh_r = 0; qh_r < 4; ++qh_r) {                                                            \
          float v = (ACC)[qh_i][qh_r];                                                                                      \
          SCALE;                                                                                                            \
          qh_out[qh_r] = qh::round_add_round<DT>(v, qh_has_bias, qh_bv[qh_r]);                                              \
        }                                                                                                                   \
        if (qh_pl + 3 < (P) && ((N) & 3) == 0) {                                                                            \
          *reinterpret_cast<uint2*>(qh_y + (size_t)m * (N) + qh_n0) = *reinterpret_cast<const uint2*>(qh_out);              \
        } else {                                                                                                            \
          _Pragma("unroll") for (int qh_r = 0; qh_r < 4; ++qh_r)                                                            \
            if (qh_pl + qh_r < (P)) qh_y[(size_t)m * (N) + qh_n0 + qh_r] = qh_out[qh_r];                                    \
        }                                                                                                                   \
      }                                                                                                                     \
    }                                                                                                                       \
  }

// ---- the same epilogue storing OUTPUT CODES (quantized-activation kernel, QOUT): what quanto::quantize_symmetric(y, activation dtype, None, out_scale)
// makes of the element the epilogue above stores.  Per element the two kernels back to back: t as above - the accumulator times the activation scale sx
// (rounded to fp32 in front of anything else), rounded to T, the bias added, rounded again - then the rule of qh_quantize.h on t: T(fp32(t) / fp32(os))
// with a correctly rounded divide, clamp_target, pack4.  A lane's 4 consecutive features of a token are one dword of codes: P % 4 == 0 (the launcher's
// N % 8 / N % 16) and pl % 4 == 0 make (m * N + n0) a multiple of 4, the launcher checks the base; per byte on the ragged edge; rows m >= M are not stored.
template <int DT, int ODT, int MI>
__device__ __forceinline__ void epilogue_codes(const f32x4 (&acc)[MI], void* yq, const void* bias, float sx, float os, int M, int m0, int fi, int N,
                                               int P, int pl, int plane) {
  using E = Elem<DT>;
  using T = typename E::T;
  uint8_t* const y = reinterpret_cast<uint8_t*>(yq);
  const bool has_bias = bias != nullptr;
  const int n0 = pl + plane * P;  // 4 consecutive output features n0 .. n0 + 3
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (has_bias) {
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = pl + r < P ? E::to_f32(reinterpret_cast<const T*>(bias)[n0 + r]) : 0.f;
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = m0 + i * 16 + fi;
    if (m < M) {
      float q[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) q[r] = epilogue_code<DT, ODT>(acc[i][r], sx, has_bias, bv[r], os);  // of the element QH_GF_EPILOGUE stores
      const uint32_t codes = pack4<ODT>(q);
      if (pl + 3 < P) {
        *reinterpret_cast<uint32_t*>(y + (size_t)m * N + n0) = codes;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (pl + r < P) y[(size_t)m * N + n0 + r] = (uint8_t)(codes >> (8 * r));
      }
    }
  }
}

// ---- the weight tile in LDS: 128-byte rows (one packed row x 128 k), 16-byte chunk c of row r at position c ^ (r & 7) --------------------------
// DMA source of weight piece `piece` (8 packed rows = 1 KiB, one per wave): lane -> row lane >> 3, position lane & 7 holds chunk pos ^ (row & 7);
// byte offset from the packed tensor ((N / VPI) * K < 4 GiB, checked by the launcher)
__device__ __forceinline__ uint32_t weight_piece_src(int piece, int lane, int p0, int P, int K) {
  const int r = piece * 8 + (lane >> 3), c = (lane & 7) ^ (r & 7);
  int p = p0 + r;
  p = p < P ? p : P - 1;
  return (uint32_t)((size_t)p * K + c * 16);
}
// read offset of chunk CHUNK of packed row R of the tile from the stage's base (the weight tile lies X_BYTES behind it)
#define QH_GF_WEIGHT_OFF(X_BYTES, R, CHUNK) ((X_BYTES) + (R) * 128 + (((CHUNK) ^ ((R) & 7)) << 4))

// ================================================================ host ================================================================
// What tells the two units apart when planning: the measured time of one tile (us; 64- / 128-token), the names of the knobs that force a
// token tile / a split (experiments, tests), and the bytes of an activation element and of a weight tile (the LDS layout).
struct Unit {
  float t_tile64, t_tile128;
  const char *env_bm, *env_split;
  int act_bytes, w_bytes;
};

// [STAGES x (activation tile | weight tile)] [xs: 2 x bm fp32 group sums] [sz: groups x 2 x NF features of a 16-bit type]
inline int lds_bytes(const Unit& u, int groups, int bm) { return STAGES * (bm * BK * u.act_bytes + u.w_bytes) + 2 * bm * 4 + groups * 2 * NF * 2; }

// output tiles of NF features x bm tokens: the same count for either weight width (int4: 64 packed rows, int2: 32); N is even
inline int tiles_of(int64_t M, int64_t N, int bm) { return (int)(((N + NF - 1) / NF) * ((M + bm - 1) / bm)); }

// Token tile and K split, chosen together from a small time model fitted to r3's sweeps (profiles/r03_fused_int4_gemm.md; us):
//   t = 5.8 + rounds * groups_per_workgroup * t_tile + tail,   rounds = ceil(workgroups / 256 CUs),
//   t_tile = 0.68 (64-token tiles) / 1.2 (128-token tiles),     tail = 3.5 + 0.5 per MB of fp32 partial tiles when K is split
//   (1.2 per MB until the partial tiles were laid out fragment-major: whole lines per write-through store instruction).
// 128 tokens per workgroup halve the activation bytes per weight byte, but a short prefill then leaves CUs idle ((512,4096,4096) is
// 128 tiles of 128 tokens on 256 CUs: 46.7 us against 28.5 with 64-token tiles); a split costs its tail (a 32 / 64 KiB partial tile
// per workgroup through the fabric and back, arrival counter, one more round trip for the last workgroup), so it pays for few
// tiles or long K only: (128,4096,4096) 27.6 / 20.0 / 16.2 / 17.9 us with 1 / 2 / 4 / 8 splits, (128,14336,4096) 83 / 48 / 34 / 34,
// (256,4096,4096) 27.9 / 21.5 / 20.8 / 28.7, but (512,4096,4096) 29.4 / 36.1.  The scale tables of a workgroup's groups must fit the LDS next
// to the ring (K = 14336 with 128-token tiles needs a split for that alone).
// The quantized-activation kernel runs the same model with its tile times, 0.45 / 0.75 (r6 sweep, profiles/r06_w4a8_*): 128-token tiles once they
// alone give every CU a workgroup, 64-token tiles (two workgroups per CU) below; K split for few tiles.  int2 runs the same model: its tile is the
// int4 tile with half the weight bytes (16 + 4 instead of 16 + 8 KiB through the vector L1 per group at bm = 128), the tile count and the matrix
// steps are the same, and the model's job - which token tile and split - does not move with that.
struct Plan {
  int bm, S;
  float us;
};
inline float model_us(const Unit& u, int tiles, int nk, int bm, int S) {
  const int wgs = tiles * S, rounds = (wgs + 255) / 256;
  const float tail = S > 1 ? 3.5f + 0.5f * (float)wgs * (float)(bm * 512) * 1e-6f : 0.f;
  return 5.8f + (float)rounds * (float)nk * (bm == 64 ? u.t_tile64 : u.t_tile128) + tail;
}
inline Plan make_plan(const Unit& u, int64_t M, int64_t N, int G) {
  const int fbm = env_int(u.env_bm, 0), fs = env_int(u.env_split, 0);
  Plan best{0, 0, 0.f};
  for (int bm = 64; bm <= 128; bm += 64) {
    if ((fbm == 64 || fbm == 128) && bm != fbm) continue;
    const int tiles = tiles_of(M, N, bm);
    for (int S = 1; S <= 8; S *= 2) {
      if (G % S) break;
      const int nk = G / S;
      if (fs > 0 ? (S != fs) : (S > 1 && nk < 4)) continue;
      if (lds_bytes(u, nk, bm) > kMaxLdsBytes) continue;
      if (S > 1 && !ws_counters_fit(tiles)) continue;
      const float us = model_us(u, tiles, nk, bm, S);
      if (best.bm == 0 || us < best.us * 0.97f) best = Plan{bm, S, us};  // ties: the smaller tile, fewer splits
    }
  }
  return best;  // bm == 0: no configuration fits (a forced split that does not divide the groups, tables that never fit)
}

// [counters (zero on entry, zero on exit) | fp32 partial tiles]; 0 when K is not split (the group sums of the activation come from the matrix pipe)
inline size_t workspace_bytes(const Plan& p, int64_t M, int64_t N) {
  if (p.bm == 0 || p.S == 1) return 0;
  return QUANTO_HIP_WS_COUNTER_BYTES + (size_t)tiles_of(M, N, p.bm) * p.S * (WAVES * 64) * ((p.bm / 16) * 16);
}

// a split plan whose scratch the caller did not bring: unsplit, with whichever token tile lets the whole scale table fit; false: none does
inline bool settle_for_workspace(const Unit& u, Plan& p, int64_t M, int64_t N, int G, const void* workspace, size_t workspace_size) {
  if (p.S > 1 && !ws_holds(workspace, workspace_size, workspace_bytes(p, M, N))) {
    p.S = 1;
    if (lds_bytes(u, G, p.bm) > kMaxLdsBytes) p.bm = 64;
    if (lds_bytes(u, G, p.bm) > kMaxLdsBytes) return false;
  }
  return true;
}

}  // namespace gf
}  // namespace qh

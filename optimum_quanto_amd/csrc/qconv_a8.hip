// F.conv2d with QUANTIZED activations and an 8-bit weight as an IMPLICIT GEMM on the 8-bit matrix instructions: QConv2d.forward (nn/qconv2d.py:54-55)
// with an ActivationQBytesTensor input, which the reference dequantizes (activation and weight) and convolves in float.
//
//   sc[n] = round_dtype(fp32(a_scale) * fp32(w_scale[n]))                     (= torch's product of the two scale tensors in their dtype)
//   v     = round_dtype(fp32(acc[m, n]) * fp32(sc[n])),   acc[m, n] = sum_{c,i,j} xq[b, c, oh*sh - ph + i*dh, ow*sw - pw + j*dw] * wq[n, c, i, j]
//   y     = bias ? round_dtype(fp32(v) + fp32(bias[n])) : v
//
// - the W8A8 QLinear arithmetic (qbytes_mm_bias(x_q, w_q, x_scale * w_scale, bias), qmm_native8.hip's epilogue) applied to the im2col of the stored
// codes.  acc is exact int32 for int8 x int8 (the result is a pure function of the integers, split or not) and the fp32 matrix-pipe sum of exact
// products for fp8.
//
// GEMM view, tiles and gather: the tap gather of DESIGN.md 4.8, whose shared pieces (tap table, validity test, partial-tile store, split
// plan and reduce, geometry rule) live in qh_conv.h and whose LDS layout in qh_mfma.h: M = B*OH*OW pixels, N = OC, K = cin*KH*KW in the weight's (c, i, j) order; one workgroup =
// 128 pixels x 128 channels, eight waves (2 x 4, 64 pixels x 32 channels each), two LDS buffers.  A K-tile is 128 ONE-byte elements - one 128-byte
// LDS row of tile_lds_off:
//   * a thread stages one pixel (tile row tid & 127) and two 16-byte chunks of it per K-tile, kc = (tid >> 7) + 4 j: k is uniform across a wave;
//   * the k-only part of an address (byte offset of tap (c, i, j) relative to the window's top-left tap, and the tap's number) comes from a
//     128-entry LDS table per K-tile; the pixel-only part (base offset, one validity bit per tap) lives in registers; an element is one
//     range-checked BUFFER byte load whose offset is forced to 0xFFFFFFFF for a padding tap or a k behind K: it reads 0 (int8 0, fp8 +0.0), nothing
//     is masked afterwards;
//   * fragments: lane (row lane & 15, 16-byte chunk lane >> 4 of each 64-byte half of the row) - the maps of qmm_native8.hip (one K = 64 int8
//     MFMA per half: v_mfma_i32_16x16x64_i8) and of its fp8 loop (both halves as ONE K = 128 v_mfma_scale_f32_16x16x128_f8f6f4, the same k
//     assignment in both operands, A and B formats independent, block scales 2^0).
// fp8 activations x int8 weights: q = 16 hi + lo with hi = q >> 4 in [-8, 7] and lo = q & 15 in [0, 15], both exact e4m3 codes, built from the
// LDS fragment by v_perm over 16-entry code tables (qbits_a8_fused.hip's nibble scheme).  Two MX-format MFMAs per fragment into the SAME fp32
// accumulator: lo with weight block scale 2^0, hi with 2^4 - the fold 16 hi + lo happens exactly inside the matrix pipe (an e4m3 / e5m2 value times
// an integer of magnitude <= 128 is exact in fp32), no extra accumulator set, no fp32 math between the MFMAs.
// K split (grids that cannot fill the chip): split z parks its int32 / fp32 tile in `partials`, a separate kernel adds the
// splits in split order (deterministic; int32: bit-identical to the unsplit result) and runs the epilogue.
// QOUT: the quantized-output form (`y` holds codes of the activation's own type, store_codes): what quanto::quantize_symmetric(y, activation dtype,
// None, out_scale) makes of the element the epilogue above stores, from the same accumulators - the tile kernel when unsplit, the reduce kernel when
// split.  The existing instantiations compile the epilogue they had.
#include <type_traits>

#include "qh_conv.h"
#include "qh_mfma.h"
#include "qh_quantize.h"  // quotient_in, clamp_target, pack4: the rule of quantize.hip, shared with the code-storing GEMM epilogues

namespace qh {
namespace conv8 {

constexpr int BM = 128, BN = 128, BK = 128, NT = 512;
constexpr int TILE_BYTES = BM * BK;                              // one operand tile in LDS (16 KiB)
constexpr int LDS_BYTES = 2 * 2 * TILE_BYTES + 2 * BK * 8;       // two buffers + two tap tables

enum Kind { K_I8 = 0, K_F8 = 1, K_F8W8 = 2 };  // int8 x int8, fp8 x fp8, fp8 activations x int8 weights
enum { F_E4M3 = 0, F_E5M2 = 1 };              // cbsz / blgp codes of the MX-format instruction

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

static_assert(BK == kTileRowBytes, "a K-tile of one-byte elements is one LDS row of tile_lds_off");

struct Args {
  const uint8_t* x;       // [B, cin, H, W] int8 / fp8 codes
  const void* a_scale;    // one element, out dtype
  const uint8_t* w;       // [OC, K] int8 / fp8 codes
  const void* w_scale;    // [OC], out dtype
  const void* bias;       // [OC] or null
  void* y;                // [B, OC, OH, OW] out dtype
  int M, N, K;            // M = B OH OW, N = OC, K = cin KH KW
  int cin, H, W, KH, KW, OH, OW, sh, sw, ph, pw, dh, dw;
  int out_dtype;          // QUANTO_HIP_{F32, F16, BF16}
  int S;                  // K split over blockIdx.z
  void* partials;         // [S][tiles][8 waves][8 fragments][64 lanes] 16 bytes (int32 / fp32)
  uint32_t khw_magic, kw_magic;  // ceil(2^32 / (KH KW)), ceil(2^32 / KW); 0 when the divisor is 1 (conv_fill_ktab)
  const void* out_scale;  // QOUT: one element, out dtype - `y` then holds [B, OC, OH, OW] one-byte codes of the activation's type
};

// ---- epilogue (conv_store_tile): the channel's factor is the scale product rounded to the output dtype, as torch multiplies the two scale tensors
template <int DT, typename AV>
__device__ __forceinline__ void store_tile_dt(const Args& a, const AV (&acc)[4][2], int m0, int nt, int wm, int wn, int lane) {
  using E = Elem<DT>;
  using T = typename E::T;
  const float as = E::to_f32(*reinterpret_cast<const T*>(a.a_scale));
  conv_store_tile<DT, 1, CONV_EPI_8BIT>(a, acc, m0, nt, wm, wn, lane,
                                        [&](int n) { return E::to_f32(E::from_f32(as * E::to_f32(reinterpret_cast<const T*>(a.w_scale)[n]))); });
}
template <typename AV>
__device__ __forceinline__ void store_tile(const Args& a, const AV (&acc)[4][2], int m0, int nt, int wm, int wn, int lane) {
  if (a.out_dtype == QUANTO_HIP_BF16)
    store_tile_dt<QUANTO_HIP_BF16>(a, acc, m0, nt, wm, wn, lane);
  else if (a.out_dtype == QUANTO_HIP_F16)
    store_tile_dt<QUANTO_HIP_F16>(a, acc, m0, nt, wm, wn, lane);
  else
    store_tile_dt<QUANTO_HIP_F32>(a, acc, m0, nt, wm, wn, lane);
}

// ---- the same epilogue storing OUTPUT CODES (QOUT).  Per element the two kernels back to back: t = the element conv_store_tile<DT, 1, CONV_EPI_8BIT>
// stores (qh_common.h: scale_round_add_round) - fp32(acc) * sc[n] behind the asm volatile, rounded to T, the bias added, rounded again - then the rule of qh_quantize.h
// on t: T(fp32(t) / fp32(out_scale)) with a correctly rounded divide, clamp_target, pack4.  ODT: the activation's own type.  A lane's four
// accumulator rows are four neighbouring pixels of one channel plane = one dword of codes: ONE 4-byte store when they lie in one image, the plane
// size is a multiple of 4 and yq is 4-byte aligned; per byte otherwise, with conv_store_tile's walk over image ends.
template <int DT, int ODT, typename AV>
__device__ __forceinline__ void store_codes_dt(const Args& a, const AV (&acc)[4][2], int m0, int nt, int wm, int wn, int lane) {
  using E = Elem<DT>;
  using T = typename E::T;
  uint8_t* yq = reinterpret_cast<uint8_t*>(a.y);
  const int M = a.M, N = a.N, L = a.OH * a.OW;
  const float as = E::to_f32(*reinterpret_cast<const T*>(a.a_scale));
  const float os = E::to_f32(*reinterpret_cast<const T*>(a.out_scale));
  const bool vec = (L & 3) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 3) == 0;
  int bq[4], lq[4];  // image and offset inside the plane of the first of the lane's four pixels of fragment i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + (lane >> 4) * 4;
    const int b = m / L;
    bq[i] = b;
    lq[i] = m - b * L;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = nt * BN + wn * 32 + j * 16 + (lane & 15);
    if (n >= N) continue;
    const float sc = E::to_f32(E::from_f32(as * E::to_f32(reinterpret_cast<const T*>(a.w_scale)[n])));
    const bool has_bias = a.bias != nullptr;
    const float bv = has_bias ? E::to_f32(reinterpret_cast<const T*>(a.bias)[n]) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wm * 64 + i * 16 + (lane >> 4) * 4;
      if (m >= M) continue;
      float q[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) q[r] = epilogue_code<DT, ODT>((float)acc[i][j][r], sc, has_bias, bv, os);  // of the element conv_store_tile stores
      const uint32_t codes = pack4<ODT>(q);
      if (vec && m + 3 < M) {  // (L % 4 == 0 and m % 4 == 0: the four pixels are in one image, aligned)
        *reinterpret_cast<uint32_t*>(yq + ((size_t)bq[i] * N + n) * L + lq[i]) = codes;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (m + r < M) {
            int bb = bq[i], ll = lq[i] + r;
            while (ll >= L) {  // an image ends inside the lane's four pixels (planes of fewer than 4 pixels: more than once)
              ll -= L;
              ++bb;
            }
            yq[((size_t)bb * N + n) * L + ll] = (uint8_t)(codes >> (8 * r));
          }
      }
    }
  }
}
template <int ODT, typename AV>
__device__ __forceinline__ void store_codes(const Args& a, const AV (&acc)[4][2], int m0, int nt, int wm, int wn, int lane) {
  if (a.out_dtype == QUANTO_HIP_BF16)
    store_codes_dt<QUANTO_HIP_BF16, ODT>(a, acc, m0, nt, wm, wn, lane);
  else if (a.out_dtype == QUANTO_HIP_F16)
    store_codes_dt<QUANTO_HIP_F16, ODT>(a, acc, m0, nt, wm, wn, lane);
  else
    store_codes_dt<QUANTO_HIP_F32, ODT>(a, acc, m0, nt, wm, wn, lane);
}
// the code type of a kernel: the activation's own (int8 x int8 -> int8; fp8 activations: AF)
template <bool INT, int AF>
constexpr int code_dtype() { return INT ? QUANTO_HIP_I8 : AF == F_E5M2 ? QUANTO_HIP_F8_E5M2 : QUANTO_HIP_F8_E4M3FN; }

// int8 weight codes (4 per dword) -> e4m3 codes of lo = q & 15 and of hi = q >> 4 (16-entry tables, three v_perm each)
__device__ __forceinline__ uint32_t nibble_codes(uint32_t s, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
  const uint32_t q7 = s & 0x07070707u;
  const uint32_t lo = __builtin_amdgcn_perm(t1, t0, q7), hi = __builtin_amdgcn_perm(t3, t2, q7);
  return __builtin_amdgcn_perm(hi, lo, ((s >> 1) & 0x04040404u) | 0x03020100u);  // byte i from hi when bit 3 of nibble i is set
}

template <int KIND, int AF, int BF, bool WIDE, bool QOUT = false>
__global__ void __launch_bounds__(NT, 2) qconv2d_a8_kernel(const Args a) {
  constexpr int NO_TAP = WIDE ? 127 : 31;
  using AV = typename std::conditional<KIND == K_I8, i32x4, f32x4>::type;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // [2 buffers][A tile | B tile] [2 tap tables]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int m0 = blockIdx.y * BM, nt = blockIdx.x;
  const int M = a.M, N = a.N, K = a.K;
  const int S = a.S, sp = blockIdx.z;
  const int nk_all = (K + BK - 1) / BK;
  const int kt_lo = (int)((long)sp * nk_all / S), nk = (int)((long)(sp + 1) * nk_all / S) - kt_lo;
  // x as a raw buffer whose range is its true size (< 2^30 bytes): an offset of 0xFFFFFFFF reads as 0
  const __amdgpu_buffer_rsrc_t xrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.x), 0, (int)(((long)M / (a.OH * a.OW)) * a.cin * a.H * a.W), 0x00020000);

  // ---- the thread's pixel: byte offset of element (b, 0, oh sh, ow sw) and one validity bit per tap (set: inside the image) ----
  // (The one-pixel case of qconv_mfma.hip's prologue; a change to the border handling belongs in both.  Kept here in its own wording: in that
  // file's wording, as a function or as a macro, hipcc gives every kernel of this file another instruction stream - DESIGN.md 4.8.)
  uint32_t px_off;
  uint64_t ok0 = 0, ok1 = 0;
  {
    const int L = a.OH * a.OW;
    int m = m0 + (tid & 127);
    m = m < M ? m : M - 1;
    const int b = m / L, l = m - b * L, oh = l / a.OW, ow = l - oh * a.OW;
    const int ih0 = oh * a.sh - a.ph, iw0 = ow * a.sw - a.pw;
    px_off = (uint32_t)(b * a.cin * a.H * a.W + oh * a.sh * a.W + ow * a.sw);
    for (int ki = 0; ki < a.KH; ++ki)
      for (int kj = 0; kj < a.KW; ++kj) {
        const int ih = ih0 + ki * a.dh, iw = iw0 + kj * a.dw;
        const int t = ki * a.KW + kj;
        const uint64_t bit = 1ull << (t & 63);
        if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
          if (WIDE && t >= 64)
            ok1 |= bit;
          else
            ok0 |= bit;
        }
      }
  }
  int2* ktab = reinterpret_cast<int2*>(smem + 2 * 2 * TILE_BYTES);  // [2][128] {byte offset relative to px_off, tap number}

  // ---- staging registers: 2 x 16 gathered bytes, 32 weight bytes (channel tid >> 2, bytes 32 (tid & 3) ..) ----
  uint8_t g[2][16];
  uint4 rw[2];
  auto issue_loads = [&](int t) {
    const int k0 = (kt_lo + t) * BK;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kc = __builtin_amdgcn_readfirstlane(tid >> 7) + 4 * j;
      const int4* tp = reinterpret_cast<const int4*>(ktab + (t & 1) * BK + kc * 16);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int4 t0 = tp[2 * h], t1 = tp[2 * h + 1];
        const int off[4] = {t0.x, t0.z, t1.x, t1.z}, tap[4] = {t0.y, t0.w, t1.y, t1.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          g[j][4 * h + q] = __builtin_amdgcn_raw_buffer_load_b8(xrsrc, (px_off + (uint32_t)off[q]) | ~(uint32_t)conv_tap_ok<WIDE>(ok0, ok1, tap[q]), 0, 0);
      }
    }
    int n = nt * BN + (tid >> 2);
    n = n < N ? n : N - 1;
    const int kb = k0 + (tid & 3) * 32;
    const uint8_t* src = a.w + (size_t)n * K + kb;
    if (kb + 32 <= K) {
      const U4u u0 = reinterpret_cast<const U4u*>(src)[0], u1 = reinterpret_cast<const U4u*>(src)[1];
      rw[0] = make_uint4(u0.x, u0.y, u0.z, u0.w);
      rw[1] = make_uint4(u1.x, u1.y, u1.z, u1.w);
    } else {  // ragged end of the last K-tile: zero bytes behind K, nothing is read beyond the row
      uint32_t d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      for (int b = 0; b < 32; ++b)
        if (kb + b < K) d[b >> 2] |= (uint32_t)src[b] << (8 * (b & 3));
      rw[0] = make_uint4(d[0], d[1], d[2], d[3]);
      rw[1] = make_uint4(d[4], d[5], d[6], d[7]);
    }
  };
  auto pack4 = [](uint8_t b0, uint8_t b1, uint8_t b2, uint8_t b3) -> uint32_t {
    return (uint32_t)b0 | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
  };
  auto write_lds = [&](int buf) {
    uint8_t* sa = smem + buf * 2 * TILE_BYTES;
    uint8_t* sb = sa + TILE_BYTES;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      *reinterpret_cast<uint4*>(sa + tile_lds_off(tid & 127, (tid >> 7) + 4 * j)) =
          make_uint4(pack4(g[j][0], g[j][1], g[j][2], g[j][3]), pack4(g[j][4], g[j][5], g[j][6], g[j][7]),
                     pack4(g[j][8], g[j][9], g[j][10], g[j][11]), pack4(g[j][12], g[j][13], g[j][14], g[j][15]));
    const int row = tid >> 2, part = tid & 3;
    *reinterpret_cast<uint4*>(sb + tile_lds_off(row, 2 * part)) = rw[0];
    *reinterpret_cast<uint4*>(sb + tile_lds_off(row, 2 * part + 1)) = rw[1];
  };

  AV acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = AV{0, 0, 0, 0};

  auto mma_phase = [&](const uint8_t* sa, const uint8_t* sb) {
    // fragment halves h = 0, 1: 16 bytes of chunk 4 h + (lane >> 4) of the fragment's row
    uint4 fa[2][4], fb[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kc = h * 4 + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[h][i] = *reinterpret_cast<const uint4*>(sa + tile_lds_off(wm * 64 + i * 16 + (lane & 15), kc));
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[h][j] = *reinterpret_cast<const uint4*>(sb + tile_lds_off(wn * 32 + j * 16 + (lane & 15), kc));
    }
    auto cat = [](const uint4& lo, const uint4& hi) { return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w}; };
    if constexpr (KIND == K_I8) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, fa[h][i]), __builtin_bit_cast(i32x4, fb[h][j]), acc[i][j], 0, 0, 0);
    } else if constexpr (KIND == K_F8) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const i32x8 b = cat(fb[0][j], fb[1][j]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(cat(fa[0][i], fa[1][i]), b, acc[i][j], AF, BF, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
      }
    } else {
      // e4m3 codes of 0..15 (lo) and of the signed nibbles 0..7, -8..-1 (hi), four per dword
      constexpr uint32_t L0 = 0x44403800u, L1 = 0x4E4C4A48u, L2 = 0x53525150u, L3 = 0x57565554u;  // 0 1 2 3 | 4 5 6 7 | 8 .. 11 | 12 .. 15
      constexpr uint32_t H2 = 0xCACCCED0u, H3 = 0xB8C0C4C8u;                                        // -8 -7 -6 -5 | -4 -3 -2 -1
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        uint32_t w[8] = {fb[0][j].x, fb[0][j].y, fb[0][j].z, fb[0][j].w, fb[1][j].x, fb[1][j].y, fb[1][j].z, fb[1][j].w};
        uint32_t lo[8], hi[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) {
          lo[d] = nibble_codes(w[d], L0, L1, L2, L3);
          hi[d] = nibble_codes(w[d] >> 4, L0, L1, H2, H3);
        }
        const i32x8 bl = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)lo[4], (int)lo[5], (int)lo[6], (int)lo[7]};
        const i32x8 bh = i32x8{(int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3], (int)hi[4], (int)hi[5], (int)hi[6], (int)hi[7]};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const i32x8 av = cat(fa[0][i], fa[1][i]);
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bl, acc[i][j], AF, F_E4M3, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);  // lo x 2^0
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bh, acc[i][j], AF, F_E4M3, 0, 0x7F7F7F7F, 0, 0x83838383);  // hi x 2^4
        }
      }
    }
  };

  conv_fill_ktab<1, BK, NO_TAP>(a, ktab, kt_lo, 0, tid);
  if (nk > 1) conv_fill_ktab<1, BK, NO_TAP>(a, ktab, kt_lo, 1, tid);
  __syncthreads();
  issue_loads(0);
  write_lds(0);
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) issue_loads(kt + 1);
    if (kt + 2 < nk) conv_fill_ktab<1, BK, NO_TAP>(a, ktab, kt_lo, kt + 2, tid);  // into the table buffer tile kt's gather last read; visible after this iteration's barrier
    const uint8_t* sa = smem + cur * 2 * TILE_BYTES;
    mma_phase(sa, sa + TILE_BYTES);
    if (kt + 1 < nk) write_lds(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  if (S > 1) return conv_park_tile(a.partials, sp, nt, wave, lane, acc);
  if constexpr (QOUT)
    store_codes<code_dtype<KIND == K_I8, AF>()>(a, acc, m0, nt, wm, wn, lane);
  else
    store_tile(a, acc, m0, nt, wm, wn, lane);
}

// split-K tail: one wave per (output tile, wave slot) adds that slot's eight fragments over the S partial tiles in split order, then the epilogue
// (AF: the fp8 activation format, which only the code-storing epilogue needs - it names the code type)
template <bool INT, int AF = F_E4M3, bool QOUT = false>
__global__ void __launch_bounds__(64) qconv2d_a8_reduce_kernel(const Args a) {
  using AV = typename std::conditional<INT, i32x4, f32x4>::type;
  const int lane = threadIdx.x, wave = blockIdx.z, S = a.S;
  AV acc[4][2];
  QH_CONV_SPLIT_SUM(AV, a.partials, S, lane, wave, acc);
  if constexpr (QOUT)
    store_codes<code_dtype<INT, AF>()>(a, acc, blockIdx.y * BM, blockIdx.x, wave >> 2, wave & 3, lane);
  else
    store_tile(a, acc, blockIdx.y * BM, blockIdx.x, wave >> 2, wave & 3, lane);
}

template <int KIND, int AF, int BF, bool WIDE, bool QOUT>
static void launch_k(const Args& a, int ntiles, int mtiles, hipStream_t stream) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qconv2d_a8_kernel<KIND, AF, BF, WIDE, QOUT>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  hipLaunchKernelGGL((qconv2d_a8_kernel<KIND, AF, BF, WIDE, QOUT>), dim3(ntiles, mtiles, a.S), dim3(NT), LDS_BYTES, stream, a);
}
// the tile kernel, then - split - the reduce kernel; QOUT reaches whichever of the two runs the epilogue (a split tile kernel parks: it stays the
// existing instantiation)
template <int KIND, int AF, int BF, bool QOUT>
static void launch_w(const Args& a, int ntiles, int mtiles, hipStream_t stream) {
  if (a.S > 1) {
    if (a.KH * a.KW > 31)
      launch_k<KIND, AF, BF, true, false>(a, ntiles, mtiles, stream);
    else
      launch_k<KIND, AF, BF, false, false>(a, ntiles, mtiles, stream);
    hipLaunchKernelGGL((qconv2d_a8_reduce_kernel<KIND == K_I8, QOUT ? AF : F_E4M3, QOUT>), dim3(ntiles, mtiles, 8), dim3(64), 0, stream, a);
  } else if (a.KH * a.KW > 31) {
    launch_k<KIND, AF, BF, true, QOUT>(a, ntiles, mtiles, stream);
  } else {
    launch_k<KIND, AF, BF, false, QOUT>(a, ntiles, mtiles, stream);
  }
}

}  // namespace conv8

// the served (activation, weight, output) formats: int8 x int8, {e4m3fn, e5m2} x {e4m3fn, e5m2, int8}; F32 / F16 / BF16 out
int qbytes_conv2d_a8_kind(int a_dtype, int b_dtype, int out_dtype) {
  if (out_dtype != QUANTO_HIP_F32 && out_dtype != QUANTO_HIP_F16 && out_dtype != QUANTO_HIP_BF16) return -1;
  const bool af8 = a_dtype == QUANTO_HIP_F8_E4M3FN || a_dtype == QUANTO_HIP_F8_E5M2;
  const bool bf8 = b_dtype == QUANTO_HIP_F8_E4M3FN || b_dtype == QUANTO_HIP_F8_E5M2;
  if (a_dtype == QUANTO_HIP_I8 && b_dtype == QUANTO_HIP_I8) return conv8::K_I8;
  if (af8 && bf8) return conv8::K_F8;
  if (af8 && b_dtype == QUANTO_HIP_I8) return conv8::K_F8W8;
  return -1;
}

size_t conv2d_a8_workspace(int64_t M, int64_t N, int64_t K) { return conv_split_workspace<conv8::BM, conv8::BN>(M, N, conv_pick_split<conv8::BK, conv8::BM, conv8::BN>(M, N, K)); }

// *kind: the conv8::Kind that ran.  The caller has validated the arguments and the format (qbytes_conv2d_a8_kind >= 0, conv_geometry_ok).
// QOUT: `y` receives a_dtype codes at *out_scale (store_codes); plan, split and workspace do not look at the output.
template <bool QOUT>
static int conv2d_a8_run(const ConvCall& c, int* kind) {
  using namespace conv8;
  hipStream_t stream = c.stream;
  const int k = qbytes_conv2d_a8_kind(c.a_dtype, c.b_dtype, c.out_dtype);
  if (k < 0 || !conv_geometry_ok(c.g)) return QUANTO_HIP_ENOTSUP;
  Args a{};
  a.x = reinterpret_cast<const uint8_t*>(c.x), a.a_scale = c.a_scale, a.w = reinterpret_cast<const uint8_t*>(c.w), a.w_scale = c.scale, a.bias = c.bias, a.y = c.y;
  a.out_dtype = c.out_dtype;
  a.out_scale = c.out_scale;
  conv_set_geometry(a, c.g);
  a.S = conv_plan_split<BK, BM, BN>(a.M, a.N, a.K, c.workspace, c.workspace_bytes);
  a.partials = c.workspace;
  const int ntiles = (a.N + BN - 1) / BN, mtiles = (a.M + BM - 1) / BM;
  const bool ae5 = c.a_dtype == QUANTO_HIP_F8_E5M2, be5 = c.b_dtype == QUANTO_HIP_F8_E5M2;
  if (k == K_I8) {
    launch_w<K_I8, 0, 0, QOUT>(a, ntiles, mtiles, stream);
  } else if (k == K_F8) {
    if (ae5)
      be5 ? launch_w<K_F8, F_E5M2, F_E5M2, QOUT>(a, ntiles, mtiles, stream) : launch_w<K_F8, F_E5M2, F_E4M3, QOUT>(a, ntiles, mtiles, stream);
    else
      be5 ? launch_w<K_F8, F_E4M3, F_E5M2, QOUT>(a, ntiles, mtiles, stream) : launch_w<K_F8, F_E4M3, F_E4M3, QOUT>(a, ntiles, mtiles, stream);
  } else {
    ae5 ? launch_w<K_F8W8, F_E5M2, F_E4M3, QOUT>(a, ntiles, mtiles, stream) : launch_w<K_F8W8, F_E4M3, F_E4M3, QOUT>(a, ntiles, mtiles, stream);
  }
  *kind = k;
  return launch_status();
}

// out_scale == nullptr: y = out_dtype[B, OC, OH, OW]; otherwise the same convolution with the layer's output quantization in its epilogue: y = a_dtype
// codes of the out_dtype-rounded output at *out_scale
int qbytes_conv2d_a8(const ConvCall& c, int* kind) { return !c.out_scale ? conv2d_a8_run<false>(c, kind) : conv2d_a8_run<true>(c, kind); }

}  // namespace qh

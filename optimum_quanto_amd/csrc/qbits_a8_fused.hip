// qbits_mm with QUANTIZED activations (W4A8, r6; W2A8 and e5m2, r7): int4 weights x int8 activations on v_mfma_i32_16x16x64_i8 and int4 weights x fp8 activations on
// v_mfma_scale_f32_16x16x128_f8f6f4 - the 8-bit matrix rates (2 x bf16) for the one activation x weight combination of the reference's
// tests/tensor/ops/test_linear_dispatch.py:22-42 that still dequantized its activation (tensor/weights/awq/qbits.py:57-58 does the same on CUDA;
// BASELINE.md lists the configuration: "W int4 / A fp8").
//
//   y[m, n] = s_x * sum_g ( s[n,g] * sum_{k in g} a[m,k] q[n,k]  -  z[n,g] * sum_{k in g} a[m,k] ) (+ bias[n])
//
// a = the stored int8 / e4m3 activation values (per-tensor scale s_x, tensor/activations/qbytes.py:28-43), q = the stored nibbles 0..15,
// z = shift (float shifts) or s * zero_point.  Products of the stored values are exact (int32 accumulation for int8; an e4m3 value times an integer
// below 16 is exact in fp32), scale / shift are applied to the fp32 accumulator per group in group order, s_x once at the end - the arithmetic contract of
// the other fused kernels.  For int8 activations the result is a pure function of the integers: bit-identical to an fp32 fma chain
// over the exact group sums (oracle/quanto_oracle.py::qbits_mm_a8_chain), whichever tile or split computes it in the unsplit form.
//
// Structure: the group-fused GEMM of qh_group_fused.h, which holds what this kernel shares with qbits_mfma_fused.hip (workgroup = 8 waves, BM tokens x 128
// features, wave = all BM tokens x 16 features, K-tile = one group of 128, LDS-DMA ring of two stages, scale tables parked in LDS, group accumulators
// double-buffered so that the fold of tile kt-1 is sliced over the matrix steps of tile kt, split-K with a deterministic last-arriver reduce, the planner),
// with 1-byte activations (128-byte LDS rows) and:
//   * int8: a weight operand is the lane's nibble plane of 16 packed bytes - ((raw >> 4 plane) & 0x0F0F0F0F), TWO VALU per four weights (the bf16 kernel: one
//     per weight) -, two K = 64 MFMAs per fragment and group, int32 group accumulator -> v_cvt_f32_i32 + two FMAs in the fold;
//   * fp8: nibbles -> e4m3 codes through a 16-entry byte table (two v_perm over the low / high half of the table + one v_perm that picks by bit 3: seven
//     VALU per four weights), ONE K = 128 MX-format MFMA (unit block scales) per fragment and group;
//   * the group sums of a come from the matrix pipe as well (an all-ones weight operand, wave w for token fragment w), exact.
// W2A8 (r7): int2 weights take the same tile with four planes per packed byte (packed [N/4, K], row p = features p, p + N/4, p + N/2, p + 3N/4 in bits
// 0-1 .. 6-7): 32 packed rows = 128 features per workgroup (4 KiB of weights per tile, requested by waves 0..3), a wave's 16 matrix rows = 4 packed rows x
// 4 planes; the operand is ((raw >> 2 plane) & 0x03030303) for int8 and ONE v_perm into the codes 0, 1, 2, 3 of the e4m3 table for fp8.  Codes 0..3 are exact
// e4m3 values, so nothing else changes.  e5m2 activations (r7): the MX-format instruction takes its A and B formats independently - the weight operand (A)
// stays e4m3, the activation operand (B) is read as bf8 (blgp = 1) in the product and in the all-ones group sum; an e5m2 value times an integer below 16 is
// exact in fp32, as for e4m3.  Instantiated: {bf16, fp16} x {int8, e4m3, e5m2} x {float shift, zero-point} x {64, 128 tokens} x {int4, int2}, each
// storing y or (QOUT) the codes of y at the layer's output scale.
#include "qh_kernels.h"
#include "qh_group_fused.h"

namespace qh {
namespace a8 {

using namespace gf;  // BK, NF, WAVES, STAGES and the shared pieces

// weight geometry of a workgroup: VPI features per packed byte (planes), PR packed rows (NF / VPI), RW packed rows per wave (16 features / VPI),
// WP waves that request a weight piece of 8 rows x 128 B per tile (int4: all eight, 8 KiB; int2: waves 0..3, 4 KiB)
template <int BITS>
struct WGeo {
  static constexpr int VPI = 8 / BITS, PR = NF / VPI, RW = 16 / VPI, W_BYTES = PR * BK, WP = W_BYTES / 1024;
  static_assert((BITS == 2 || BITS == 4) && WP <= WAVES && WP * 1024 == W_BYTES, "weight geometry");
};
template <int BM, int BITS>
struct Geo {
  static constexpr int MI = BM / 16;
  static constexpr int X_BYTES = BM * BK, STAGE_BYTES = X_BYTES + WGeo<BITS>::W_BYTES;
  static constexpr int XP = BM / 8 / WAVES;  // activation DMA pieces (8 rows x 128 B = 1 KiB) per wave and tile
  static_assert(XP >= 1 && (MI == 4 || MI == 8), "tile geometry");
};

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

enum { A_I8 = 0, A_F8E4M3 = 1, A_F8E5M2 = 2 };

struct Args {
  const uint8_t* a;      // [M, K] int8 / e4m3 activation values
  const void* a_scale;   // device scalar of the output dtype: the per-tensor activation scale
  const uint8_t* w;      // packed [N/VPI, K]
  const void* scale;     // [N*G]
  const void* shift;     // [N*G]
  const void* bias;      // [N] or null
  void* y;               // [M, N]
  int M, N, K, G;
  int S;                 // K split: blockIdx.z handles groups [z * G / S, (z + 1) * G / S)
  int* counters;         // [tiles] arrival counters, zero on entry and on exit (S > 1)
  float* partials;       // [tiles][S][MI][512 lanes] float4
  int ablate;            // QUANTO_HIP_A8_ABLATE (timing experiments, WRONG results): 1 no fold, 2 no matrix steps, 4 the DMA re-reads tile 0, 8 no weight unpack
  const void* out_scale; // QOUT kernels only: one element of the output dtype, the per-tensor scale of the codes they store into `y` ([M, N] bytes)
};

template <int AK>
struct Acc {
  using V = f32x4;
};
template <>
struct Acc<A_I8> {
  using V = i32x4;
};

// QOUT: the quantized-output form (`y` holds codes of the activation's own type, gf::epilogue_codes); the existing instantiations compile the epilogue they had
template <int DT, int AK, bool INT_SHIFT, int BM, int BITS, bool QOUT = false>
__global__ void __launch_bounds__(WAVES * 64, 1) qbits_a8_fused_kernel(const Args a) {
  using E = Elem<DT>;
  using T = typename E::T;
  using GV = typename Acc<AK>::V;  // group accumulator
  constexpr int MI = Geo<BM, BITS>::MI, XP = Geo<BM, BITS>::XP, X_BYTES = Geo<BM, BITS>::X_BYTES, STAGE_BYTES = Geo<BM, BITS>::STAGE_BYTES;
  constexpr int VPI = WGeo<BITS>::VPI, PR = WGeo<BITS>::PR, RW = WGeo<BITS>::RW, WP = WGeo<BITS>::WP;
  // B operand format of the MX-format instruction: bf8 for e5m2 activations, fp8 otherwise; the weight operand (A) is always e4m3 codes
  constexpr int BFMT = AK == A_F8E5M2 ? 1 : 0;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // layout: [STAGES x (activation tile | weight tile)] [xs: 2 x BM fp32 group sums of a] [sz: G x 2 x 128 features of T]
  float* xs_slot = reinterpret_cast<float*>(smem + STAGES * STAGE_BYTES);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = a.M, N = a.N, K = a.K, G = a.G;
  const int P = N >> (VPI == 2 ? 1 : 2);  // packed rows = features per plane
  const int p0 = blockIdx.x * PR, m0 = blockIdx.y * BM;
  const int S = a.S, sp = blockIdx.z;
  const int nk = G / S;  // one tile per group; this workgroup's groups are kt0 .. kt0 + nk - 1
  const int kt0 = sp * nk;
  const int fi = lane & 15, fg = lane >> 4;
  T* sz = reinterpret_cast<T*>(smem + STAGES * STAGE_BYTES + 2 * BM * 4);

  // ---- DMA sources: activation pieces of 8 rows x 128 B (lane -> row lane >> 3, position lane & 7 holds chunk pos ^ (row & 7)), one weight piece per wave
  uint32_t xsrc[XP];
#pragma unroll
  for (int u = 0; u < XP; ++u) {
    const int row = 8 * (wave * XP + u) + (lane >> 3);
    const int c = (lane & 7) ^ (row & 7);
    int m = m0 + row;
    m = m < M ? m : M - 1;
    xsrc[u] = (uint32_t)((size_t)m * K + c * 16);  // M * K < 4 GiB, checked by the launcher
  }
  const uint32_t wsrc = weight_piece_src(WP == WAVES ? wave : wave & (WP - 1), lane, p0, P, K);  // int2: waves >= WP request nothing
  const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr_t)smem;
  auto issue_tile = [&](int kt_tile, int stage) {
    if (a.ablate & 4) kt_tile = 0;
    const uint32_t st = __builtin_amdgcn_readfirstlane(lds_base + stage * STAGE_BYTES);
#pragma unroll
    for (int u = 0; u < XP; ++u) glds16(a.a + (size_t)(kt0 + kt_tile) * BK, xsrc[u], st + (wave * XP + u) * 1024);
    if (WP == WAVES || wave < WP) glds16(a.w + (size_t)(kt0 + kt_tile) * BK, wsrc, st + X_BYTES + wave * 1024);  // wave-uniform
  };
  const int last = nk - 1;

  // ---- prologue: tiles 0 and 1 requested, tables parked, ONE drain ----
  issue_tile(0, 0);
  issue_tile(nk > 1 ? 1 : 0, 1);
  QH_GF_FILL_TABLES(E, INT_SHIFT, PR, sz, a.scale, a.shift, tid, p0, P, G, kt0, nk);
  const float sx = E::to_f32(*reinterpret_cast<const T*>(a.a_scale));
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // hand-counted waits start from a known state

  // ---- fragment read offsets: 16-byte chunk 4 h + fg of the lane's row (h = half of the 128-byte row); (row & 7) == (fi & 7) for every fragment ----
  // weight row of matrix row fi: packed row wave * RW + fi % RW, plane fi / RW (int4: 8 rows x 2 planes, int2: 4 rows x 4 planes per wave)
  int xoff[2], woff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) xoff[h] = fi * 128 + (((4 * h + fg) ^ (fi & 7)) << 4);
  {
    const int r = wave * RW + (fi & (RW - 1));
#pragma unroll
    for (int h = 0; h < 2; ++h) woff[h] = QH_GF_WEIGHT_OFF(X_BYTES, r, 4 * h + fg);
  }
  const uint32_t nib_shift = (fi / RW) * BITS;
  // the lane's 4 consecutive matrix rows 4 fg .. 4 fg + 3 = 4 consecutive packed rows of plane 4 fg / RW: 4 consecutive features inside the block
  const int fplane = (4 * fg) / RW, froff = (4 * fg) % RW;
  const int floc = fplane * PR + wave * RW + froff;

  f32x4 acc[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint32_t nibmask = BITS == 4 ? 0x0F0F0F0Fu : 0x03030303u;
  asm volatile("" : "+s"(nibmask));
  // e4m3 codes of 0..15 (bias 7): 0, 1 = 0x38, 2 = 0x40, 3 = 0x44, 4..7 = 0x48 + 2 (q - 4), 8..15 = 0x50 + (q - 8)
  uint32_t t_lo0 = 0x44403800u, t_lo1 = 0x4E4C4A48u, t_hi0 = 0x53525150u, t_hi1 = 0x57565554u;
  asm volatile("" : "+v"(t_lo0), "+v"(t_lo1), "+v"(t_hi0), "+v"(t_hi1));

  GV accgA[MI], accgB[MI];
  float s4[4], z4[4], xsp[MI];
  const int my_xs = wave < MI ? wave : -1;
  auto load_fold_inputs = [&](int g) {  // of group g of this workgroup, folded one tile later; the operands are the plain codes: no offset in the shift term
    load_sz<DT, INT_SHIFT, false>(sz, g, floc, s4, z4);
    load_xs<BM>(xs_slot, g, fi, xsp);
  };

  constexpr int STEPS = AK == A_I8 ? 2 * MI : MI;   // matrix steps per tile
  constexpr int FPS = 4 * MI / STEPS;               // fold elements per step: 2 (int8) / 4 (fp8)
  auto tile = [&](int kt, GV (&cg)[MI], const GV (&pg)[MI], auto have_prev_tag, auto stage_tag) {
    constexpr bool have_prev = decltype(have_prev_tag)::value;
    constexpr int stage = decltype(stage_tag)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // tile kt (requested a tile ago; nothing younger is in flight)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // fragment / table reads and the sum store of the previous tile
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue_tile(kt + 1 < nk ? kt + 1 : last, 1 - stage);
    const uint8_t* st = smem + stage * STAGE_BYTES;
    uint4 w[2];
    w[0] = *reinterpret_cast<const uint4*>(st + woff[0]);
    w[1] = *reinterpret_cast<const uint4*>(st + woff[1]);
    // activation fragments: both 16-byte halves of every token fragment, two fragments ahead of their matrix step
    uint4 xl[MI], xh[MI];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      xl[i] = *reinterpret_cast<const uint4*>(st + xoff[0] + i * 2048);
      xh[i] = *reinterpret_cast<const uint4*>(st + xoff[1] + i * 2048);
    }
    if constexpr (have_prev) load_fold_inputs(kt - 1);
    // weight operand of the tile: the lane's nibble plane of its 32 packed bytes
    uint32_t op[8];
    {
      const uint32_t raw[8] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w};
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const uint32_t s = raw[d] >> nib_shift;
        if (a.ablate & 8) {
          op[d] = raw[d];
        } else if constexpr (AK == A_I8) {
          op[d] = s & nibmask;
        } else if constexpr (BITS == 2) {
          op[d] = __builtin_amdgcn_perm(t_lo1, t_lo0, s & nibmask);  // codes 0..3: bytes of t_lo0
        } else {
          const uint32_t q7 = s & 0x07070707u;
          const uint32_t lo = __builtin_amdgcn_perm(t_lo1, t_lo0, q7), hi = __builtin_amdgcn_perm(t_hi1, t_hi0, q7);
          const uint32_t sel = ((s >> 1) & 0x04040404u) | 0x03020100u;  // byte i of the result: byte i of lo, or of hi when bit 3 of the nibble is set
          op[d] = __builtin_amdgcn_perm(hi, lo, sel);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      if constexpr (AK == A_I8) {
        // step order (i0,h0) (i1,h0) (i0,h1) (i1,h1) per pair of token fragments: the two dependent K = 64 products of a fragment are one independent
        // matrix instruction apart
        const int i = 2 * (s >> 2) + (s & 1), h = (s >> 1) & 1;
        const i32x4 wa = h == 0 ? i32x4{(int)op[0], (int)op[1], (int)op[2], (int)op[3]} : i32x4{(int)op[4], (int)op[5], (int)op[6], (int)op[7]};
        const uint4& xv = h == 0 ? xl[i] : xh[i];
        if (!(a.ablate & 2)) cg[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa, __builtin_bit_cast(i32x4, xv), h == 0 ? i32x4{0, 0, 0, 0} : cg[i], 0, 0, 0);
      } else {
        const int i = s;
        const i32x8 wa = i32x8{(int)op[0], (int)op[1], (int)op[2], (int)op[3], (int)op[4], (int)op[5], (int)op[6], (int)op[7]};
        const i32x8 xa = i32x8{(int)xl[i].x, (int)xl[i].y, (int)xl[i].z, (int)xl[i].w, (int)xh[i].x, (int)xh[i].y, (int)xh[i].z, (int)xh[i].w};
        if (!(a.ablate & 2)) cg[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wa, xa, f32x4{0.f, 0.f, 0.f, 0.f}, 0, BFMT, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);  // e4m3 x e4m3 / bf8, scales 2^0
      }
      if constexpr (have_prev) {
        if (!(a.ablate & 1)) {
#pragma unroll
          for (int q = s * FPS; q < (s + 1) * FPS; ++q) fold_slice(acc, pg, q, s4, z4, xsp);
        }
      }
      // the fragment two ahead, once per token fragment (int8: fragments 2p+2, 2p+3 behind steps 0 and 2 of pair p - their registers are free: the
      // fragments of pair p+1 are not in use yet)
      const int inext = AK == A_I8 ? 2 * (s >> 2) + 2 + ((s >> 1) & 1) : s + 2;
      if ((AK != A_I8 || (s & 1) == 0) && inext < MI) {
        xl[inext] = *reinterpret_cast<const uint4*>(st + xoff[0] + inext * 2048);
        xh[inext] = *reinterpret_cast<const uint4*>(st + xoff[1] + inext * 2048);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // group sums of a for this wave's token fragment: the same matrix instruction against an all-ones weight operand (exact)
    if (my_xs >= 0) {
      const uint4 al = *reinterpret_cast<const uint4*>(st + xoff[0] + my_xs * 2048), ah = *reinterpret_cast<const uint4*>(st + xoff[1] + my_xs * 2048);
      float sum;
      if constexpr (AK == A_I8) {
        const i32x4 ones = i32x4{0x01010101, 0x01010101, 0x01010101, 0x01010101};
        i32x4 cx = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, __builtin_bit_cast(i32x4, al), i32x4{0, 0, 0, 0}, 0, 0, 0);
        cx = __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, __builtin_bit_cast(i32x4, ah), cx, 0, 0, 0);
        sum = (float)cx[0];
      } else {
        const i32x8 ones = i32x8{0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838};  // e4m3 1.0
        const i32x8 xa = i32x8{(int)al.x, (int)al.y, (int)al.z, (int)al.w, (int)ah.x, (int)ah.y, (int)ah.z, (int)ah.w};
        const f32x4 cx = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ones, xa, f32x4{0.f, 0.f, 0.f, 0.f}, 0, BFMT, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        sum = cx[0];
      }
      // the matrix instruction must run with all 64 lanes: without this barrier hipcc sinks it into the lane < 16 branch below (EXEC = 0xFFFF), where the
      // K = 128 MX-format form returned wrong sums (r6 visit 3: profiles/r06_w4a8_fp8_exec_masked_mfma.md)
      asm volatile("" : "+v"(sum));
      if (lane < 16) xs_slot[(kt & 1) * BM + my_xs * 16 + lane] = sum;  // every row of the product holds the sum: row 0 leaves it for the fold one tile later
    }
  };
  auto final_fold = [&](const GV (&pg)[MI]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    load_fold_inputs(nk - 1);
#pragma unroll
    for (int q = 0; q < 4 * MI; ++q) fold_slice(acc, pg, q, s4, z4, xsp);
  };
  QH_GF_FOR_EACH_TILE(nk, tile, final_fold, accgA, accgB);
  if (S > 1) QH_GF_SPLITK(BM, MI, acc, a.partials, a.counters, S, sp, tid, smem);
  // x activation scale (the product is rounded to fp32 before anything else happens to it), (+ bias)
  if constexpr (QOUT) {
    // ... and what quantize_symmetric makes of that element at the layer's output scale: the split-K tile's last arriver gets here with the summed accumulators
    constexpr int ODT = AK == A_I8 ? QUANTO_HIP_I8 : AK == A_F8E4M3 ? QUANTO_HIP_F8_E4M3FN : QUANTO_HIP_F8_E5M2;
    const float os = E::to_f32(*reinterpret_cast<const T*>(a.out_scale));
    epilogue_codes<DT, ODT, MI>(acc, a.y, a.bias, sx, os, M, m0, fi, N, P, p0 + wave * RW + froff, fplane);
  } else {
    QH_GF_EPILOGUE(DT, MI, acc, a.y, a.bias, m0, fi, N, P, p0 + wave * RW + froff, fplane, m < M, v = v * sx; asm volatile("" : "+v"(v)));
  }
}

// tile times of the time model (r6 sweep, us per 64- / 128-token tile), the forcing knobs, 1-byte activations, the weight tile of either width
inline Unit unit(int bits) { return Unit{0.45f, 0.75f, "QUANTO_HIP_A8_BM", "QUANTO_HIP_A8_SPLIT", 1, bits == 2 ? WGeo<2>::W_BYTES : WGeo<4>::W_BYTES}; }

template <int DT, int AK, bool INT_SHIFT, int BM, int BITS, bool QOUT>
static int launch_bm(const Args& a, hipStream_t stream) {
  const int lds = lds_bytes(unit(BITS), a.G / a.S, BM);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qbits_a8_fused_kernel<DT, AK, INT_SHIFT, BM, BITS, QOUT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            lds);
  const dim3 grid((unsigned)((a.N + NF - 1) / NF), (unsigned)((a.M + BM - 1) / BM), (unsigned)a.S);
  hipLaunchKernelGGL((qbits_a8_fused_kernel<DT, AK, INT_SHIFT, BM, BITS, QOUT>), grid, dim3(WAVES * 64), lds, stream, a);
  return launch_status();
}
template <int DT, int AK, int BITS, bool QOUT>
static int launch(const Args& a, int bm, bool int_shift, hipStream_t stream) {
  if (int_shift) return bm == 64 ? launch_bm<DT, AK, true, 64, BITS, QOUT>(a, stream) : launch_bm<DT, AK, true, 128, BITS, QOUT>(a, stream);
  return bm == 64 ? launch_bm<DT, AK, false, 64, BITS, QOUT>(a, stream) : launch_bm<DT, AK, false, 128, BITS, QOUT>(a, stream);
}
template <int DT, int BITS, bool QOUT>
static int launch_act(const Args& a, int a_dtype, int bm, bool int_shift, hipStream_t stream) {
  switch (a_dtype) {
    case QUANTO_HIP_I8:
      return launch<DT, A_I8, BITS, QOUT>(a, bm, int_shift, stream);
    case QUANTO_HIP_F8_E4M3FN:
      return launch<DT, A_F8E4M3, BITS, QOUT>(a, bm, int_shift, stream);
    default:
      return launch<DT, A_F8E5M2, BITS, QOUT>(a, bm, int_shift, stream);
  }
}
template <int DT, bool QOUT>
static int launch_bits(const Args& a, int bits, int a_dtype, int bm, bool int_shift, hipStream_t stream) {
  return bits == 2 ? launch_act<DT, 2, QOUT>(a, a_dtype, bm, int_shift, stream) : launch_act<DT, 4, QOUT>(a, a_dtype, bm, int_shift, stream);
}

}  // namespace a8

// Served: bits 4 with N % 8 == 0, bits 2 with N % 16 == 0 (N / VPI packed rows per plane, a multiple of 4: every lane's four output features are one
// aligned 8-byte store), group size 128 (per-channel with K = 128 included), activations int8 / e4m3fn / e5m2.
bool qbits_a8_supported(int64_t M, const PackedGeom& g, int a_dtype, int dtype) {
  if (!((g.bits == 4 || g.bits == 2) && g.C == 128 && (g.N % (4 * g.vpi) == 0) && (g.K % 128 == 0) && M >= 1 &&
        (dtype == QUANTO_HIP_BF16 || dtype == QUANTO_HIP_F16) &&
        (a_dtype == QUANTO_HIP_I8 || a_dtype == QUANTO_HIP_F8_E4M3FN || a_dtype == QUANTO_HIP_F8_E5M2) && g.N < (1 << 30) && g.K < (1 << 30) &&
        M * g.K < (1ll << 32) && g.N * g.K < (1ll << 33) && grid_yz_fits(M, 64)))  // grid.y = token tiles of the smaller tile the plan may take
    return false;
  return gf::make_plan(a8::unit(g.bits), M, g.N, (int)g.G).bm != 0;
}

size_t qbits_a8_workspace(int64_t M, const PackedGeom& g) {
  return gf::workspace_bytes(gf::make_plan(a8::unit(g.bits), M, g.N, (int)g.G), M, g.N);
}

// out_scale == nullptr: y = dtype[M, N]; otherwise the code-storing kernels: y = a_dtype[M, N] codes at the per-tensor scale out_scale[0], 16-byte aligned
template <bool QOUT>
static int mm_a8(const QbitsCall& c) {
  const int64_t M = c.M;
  const PackedGeom& g = c.g;
  if (!qbits_a8_supported(M, g, c.a_dtype, c.dtype)) return QUANTO_HIP_ENOTSUP;
  if ((reinterpret_cast<uintptr_t>(c.x) | reinterpret_cast<uintptr_t>(c.packed) | (QOUT ? reinterpret_cast<uintptr_t>(c.y) : 0)) % 16) return QUANTO_HIP_EALIGN;
  const gf::Unit unit = a8::unit(g.bits);
  gf::Plan p = gf::make_plan(unit, M, g.N, (int)g.G);
  if (!gf::settle_for_workspace(unit, p, M, g.N, (int)g.G, c.workspace, c.workspace_bytes)) return QUANTO_HIP_EINVAL;
  const a8::Args a{reinterpret_cast<const uint8_t*>(c.x), c.a_scale, c.packed, c.scale, c.shift, c.bias, c.y, (int)M, (int)g.N, (int)g.K, (int)g.G, p.S,
                   reinterpret_cast<int*>(c.workspace),
                   p.S > 1 ? ws_partials(c.workspace) : nullptr,
                   env_int("QUANTO_HIP_A8_ABLATE", 0),
                   c.out_scale};
  return c.dtype == QUANTO_HIP_BF16 ? a8::launch_bits<QUANTO_HIP_BF16, QOUT>(a, g.bits, c.a_dtype, p.bm, c.int_shift, c.stream)
                                    : a8::launch_bits<QUANTO_HIP_F16, QOUT>(a, g.bits, c.a_dtype, p.bm, c.int_shift, c.stream);
}

// c.x = the activation codes (a_dtype) at a_scale.  y = dtype[M, N]; or, with an out_scale, the product with the output quantization of the layer in its
// epilogue (gf::epilogue_codes): y = a_dtype[M, N] codes of the dtype-rounded product at the per-tensor scale out_scale[0] - bit-identical to
// quantize_symmetric of the float form.  Same gate, same plan, same workspace.
int qbits_mm_a8(const QbitsCall& c) { return !c.out_scale ? mm_a8<false>(c) : mm_a8<true>(c); }

}  // namespace qh

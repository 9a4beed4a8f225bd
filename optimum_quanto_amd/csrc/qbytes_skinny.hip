// qbytes_mm for small batches (2 < M <= 256 in passes of 64, e.g. batched decode with int8 / fp8 weights): weight-streaming MFMA kernel.
//
// The 8-bit sibling of qbits_skinny.hip - HBM-bound like the GEMV, products on the matrix cores so that the cost per weight
// byte does not grow with M:
//   * a block of 4 waves owns 64 output features (16 weight rows per wave) and streams them over its K-range in tiles of 128
//     k through a 4..8-stage LDS-DMA ring (`global_load_lds_dwordx4`, counted vmcnt, one s_barrier per pair of tiles);
//   * lane (i = lane & 15, g = lane >> 4) of a wave fetches the 32 bytes k = 32g .. 32g+31 of row i with two ds_read_b128
//     and converts them in registers (int8: 2 x v_cvt_f32_i32 SDWA + v_cvt_pk_bf16_f32 per pair; fp8: v_cvt_pk_f32_fp8 +
//     pack) into the A operands of the tile's four k-steps: step t uses bytes 8t .. 8t+7 of the lane's 32, i.e.
//     k = 32g + 8t .. +7.  The activation fragment of step t is read with the same k assignment (16-byte chunk 4g + t of
//     the token's 256-byte row) - an MFMA is invariant under a k permutation applied to both operands;
//   * the per-channel scale (and bias) is applied once, to the fp32 accumulator, in the epilogue - no per-group work;
//   * K is split across workgroups when N alone cannot occupy the chip, and M > 64 runs in passes of 64 rows: same scheme,
//     same split-K tail and workspace contract (zeroed arrival counters, system-coherent partial sums: qh_mfma.h).
#include <cstdlib>

#include "qh_kernels.h"
#include "qh_mfma.h"

namespace qh {
namespace skinny8 {

constexpr int BK = 128;  // k per tile = bytes per weight row and tile

using namespace w8;  // qh_mfma.h: W_I8 .. W_F8E4M3FNUZ, convert_pair

struct Args {
  const void* x;      // [M, K] activations (M <= 64 per launch)
  const uint8_t* w;   // [N, K] one byte per weight
  const void* scale;  // [N]
  const void* bias;   // [N] or null
  void* y;            // [M, N]
  int M, N, K;
  int S;              // K split (see qbits_skinny.hip)
  int* counters;
  float* partials;
  int nt;             // non-temporal weight DMA (single-pass calls)
};

// Several Linears sharing their input in one launch (MULTI, see qbits_skinny.hip): the feature blocks of all segments form
// one grid, a block takes weight / scale / bias / output pointers and N from its segment.
constexpr int MAX_SEGS = QUANTO_HIP_MAX_MULTI;
struct Segs {
  const uint8_t* w[MAX_SEGS];
  const void* scale[MAX_SEGS];
  const void* bias[MAX_SEGS];
  void* y[MAX_SEGS];
  int N[MAX_SEGS];
  int first_fb[MAX_SEGS];  // first feature block of each segment (INT_MAX for unused slots)
};

template <int DT, int FMT, int TF, int STAGES, bool MULTI = false>
__global__ void __launch_bounds__(256) qbytes_skinny_kernel(Args a, const Segs segs) {
  using E = Elem<DT>;
  using T = typename E::T;
  using V8 = typename Mma<DT>::V8;
  constexpr int WAVES = 4;
  constexpr int ROWS = 16 * WAVES;    // weight rows (= output features) per block
  constexpr int W_BYTES = ROWS * BK;  // 8 KiB: 2 KiB per wave
  constexpr int X_BYTES = TF * 16 * BK * 2;
  constexpr int STAGE_BYTES = W_BYTES + X_BYTES;
  constexpr int XP = TF * 4 / WAVES;  // 1 KiB activation DMA pieces per wave and tile (TF = 1: waves 0..TF*4-1 only)
  constexpr int XPI = XP > 0 ? XP : 1;
  constexpr int PER = 2 + XPI;        // DMA instructions per wave and tile (upper bound used for vmcnt accounting)
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = a.S;
  const int fbg = S > 1 ? blockIdx.x / S : blockIdx.x, sp = S > 1 ? blockIdx.x - fbg * S : 0;  // global feature block
  int fb = fbg;
  if constexpr (MULTI) {
    int seg = 0;
#pragma unroll
    for (int i = 1; i < MAX_SEGS; ++i) seg += fbg >= segs.first_fb[i];
    fb = fbg - segs.first_fb[seg];
    a.w = segs.w[seg];
    a.scale = segs.scale[seg];
    a.bias = segs.bias[seg];
    a.y = segs.y[seg];
    a.N = segs.N[seg];
  }
  const int M = a.M, N = a.N, K = a.K;
  const int n_blk = fb * ROWS;
  const int nk = K / BK / S;
  const int kt0 = sp * nk;

  // ---- per-lane DMA sources ---------------------------------------------------------------------------------------------
  // weights: the wave's 16 rows x 128 B as two 1 KiB pieces of 8 rows; lane -> row lane>>3, position lane&7 holds chunk pos ^ (row & 7)
  const uint8_t* wsrc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = wave * 16 + h * 8 + (lane >> 3), c = (lane & 7) ^ (r & 7);
    const int n = n_blk + r < N ? n_blk + r : N - 1;
    wsrc[h] = a.w + (size_t)n * K + c * 16 + (size_t)kt0 * BK;
  }
  // activations: 1 KiB pieces of 4 token rows (256 B each); piece u' covers tile rows 4u' .. 4u'+3
  const uint8_t* xsrc[XPI];
  constexpr int XPIECES = TF * 4;
#pragma unroll
  for (int u = 0; u < XPI; ++u) {
    const int piece = XP > 0 ? wave * XP + u : wave;  // TF = 1 with 4 waves: one piece per wave
    const int row = 4 * piece + (lane >> 4);
    const int c = (lane & 15) ^ (row & 15);
    const int m = row < M ? row : M - 1;
    xsrc[u] = reinterpret_cast<const uint8_t*>(reinterpret_cast<const T*>(a.x) + (size_t)m * K + c * 8 + (size_t)kt0 * BK);
  }
  const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr_t)smem;
  auto issue = [&](int kt, int stage) {
    const uint32_t st = __builtin_amdgcn_readfirstlane(lds_base + stage * STAGE_BYTES);
    if (a.nt) {
      glds16_nt(wsrc[0] + (size_t)kt * BK, st + (wave * 2 + 0) * 1024);
      glds16_nt(wsrc[1] + (size_t)kt * BK, st + (wave * 2 + 1) * 1024);
    } else {
      glds16(wsrc[0] + (size_t)kt * BK, st + (wave * 2 + 0) * 1024);
      glds16(wsrc[1] + (size_t)kt * BK, st + (wave * 2 + 1) * 1024);
    }
#pragma unroll
    for (int u = 0; u < XPI; ++u) {
      const int piece = XP > 0 ? wave * XP + u : wave;
      if (piece < XPIECES) glds16(xsrc[u] + (size_t)kt * (BK * 2), st + W_BYTES + piece * 1024);
    }
  };
  // r6: the lane's four scale / bias values are requested HERE, in front of the first DMA (the oldest entries of the in-order vector-memory queue), not
  // after the K loop: the epilogue used to open with a global round trip (~1 us of a 7-10 us call).  As asm: hipcc would drain the DMA queue at a load it sees.
  uint32_t sc_raw[4], bv_raw[4];
  {
    const int nq = n_blk + wave * 16 + 4 * (lane >> 4);
    // no bias: the same loads from the scale vector (unused) - a branch-free sequence, so that nothing but these asm statements ever writes the
    // destination registers before the counted wait (tests/test_build_invariants.py reads the listing for exactly that)
    const T* bsrc = reinterpret_cast<const T*>(a.bias != nullptr ? a.bias : a.scale);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nq + r < N ? nq + r : N - 1;
      asm volatile("global_load_ushort %0, %1, off" : "=v"(sc_raw[r]) : "v"(reinterpret_cast<const T*>(a.scale) + n) : "memory");
      asm volatile("global_load_ushort %0, %1, off" : "=v"(bv_raw[r]) : "v"(bsrc + n) : "memory");
    }
  }
#pragma unroll
  for (int t = 0; t < STAGES - 2; ++t)
    if (t < nk) issue(t, t);

  // ---- fragment read offsets ------------------------------------------------------------------------------------------------
  const int fi = lane & 15, fg = lane >> 4;
  const int wrow = wave * 16 + fi;
  int woff[2];  // 16-byte chunks 2g and 2g+1 of the lane's row
#pragma unroll
  for (int h = 0; h < 2; ++h) woff[h] = wrow * 128 + (((2 * fg + h) ^ (wrow & 7)) << 4);
  int xoff[TF][4];  // k-step t: chunk 4g + t of the token's row
#pragma unroll
  for (int tf = 0; tf < TF; ++tf) {
    const int row = tf * 16 + fi;
#pragma unroll
    for (int t = 0; t < 4; ++t) xoff[tf][t] = W_BYTES + row * 256 + (((4 * fg + t) ^ (row & 15)) << 4);
  }

  f32x4 acc[TF];
#pragma unroll
  for (int tf = 0; tf < TF; ++tf) acc[tf] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute_tile = [&](const uint8_t* st) {
    uint4 wr[2];
    wr[0] = *reinterpret_cast<const uint4*>(st + woff[0]);
    wr[1] = *reinterpret_cast<const uint4*>(st + woff[1]);
    // every activation fragment of the tile up front, pinned by the scheduling barrier (r5, as qbits_skinny.hip: hipcc otherwise reads one
    // fragment, waits, issues its MFMAs, TF x 4 times per tile - one exposed LDS latency each)
    V8 xb[TF][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int tf = 0; tf < TF; ++tf) xb[tf][t] = *reinterpret_cast<const V8*>(st + xoff[tf][t]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      // k-step t: bytes 8t .. 8t+7 of the lane's 32 = dwords (2t, 2t+1) -> four operand dwords
      const uint32_t d0 = (t & 1) ? wr[t >> 1].z : wr[t >> 1].x, d1 = (t & 1) ? wr[t >> 1].w : wr[t >> 1].y;
      uint32_t op[4];
      op[0] = convert_pair<DT, FMT>(d0, 0);
      op[1] = convert_pair<DT, FMT>(d0, 1);
      op[2] = convert_pair<DT, FMT>(d1, 0);
      op[3] = convert_pair<DT, FMT>(d1, 1);
      const V8 wa = __builtin_bit_cast(V8, make_uint4(op[0], op[1], op[2], op[3]));
#pragma unroll
      for (int tf = 0; tf < TF; ++tf) acc[tf] = Mma<DT>::run(wa, xb[tf][t], acc[tf]);
    }
  };

  // Tiles are consumed in pairs per barrier; ring of STAGES (even) stages, tiles kt .. kt+STAGES-1 in flight
  int cur = 0;
  for (int kt = 0; kt < nk; kt += 2) {
    const bool pair = kt + 1 < nk;
    const int last = pair ? kt + 1 : kt;
    const int younger = nk - 1 - last < STAGES - 4 ? nk - 1 - last : STAGES - 4;
    wait_vmcnt<(STAGES - 4) * PER, PER>(younger);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int nxt = cur + 1 == STAGES ? 0 : cur + 1;
    {
      const int s0 = cur >= 2 ? cur - 2 : cur + STAGES - 2, s1 = s0 + 1 == STAGES ? 0 : s0 + 1;
      if (kt + STAGES - 2 < nk) issue(kt + STAGES - 2, s0);
      if (kt + STAGES - 1 < nk) issue(kt + STAGES - 1, s1);
    }
    compute_tile(smem + cur * STAGE_BYTES);
    if (pair) compute_tile(smem + nxt * STAGE_BYTES);
    cur = nxt + 1 == STAGES ? 0 : nxt + 1;
  }

  // ---- split-K: the last block of a feature block to arrive adds the partial sums in split order, one split per wait (qh_mfma.h) ----
  if (S > 1) {
    int* flag = reinterpret_cast<int*>(smem);
    QH_SPLITK_ARRIVE(TF, 256, a.partials, blockIdx.x, acc, a.counters + fbg, flag, tid, (void)0, (void)0);
    if (*flag != S - 1) return;
    QH_SPLITK_SUM(TF, 256, 1, TF, a.partials, fbg, S, acc, a.counters + fbg, tid, (void)0);
  }

  // ---- epilogue: per-channel scale on the accumulator, optional bias; a lane holds 4 consecutive features of one token ----------
  T* yg = reinterpret_cast<T*>(a.y);
  const int n0 = n_blk + wave * 16 + 4 * fg;
  float sc[4], bv[4];
  const bool has_bias = a.bias != nullptr;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // long since complete (requested ahead of the first tile)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    asm volatile("" : "+v"(sc_raw[r]), "+v"(bv_raw[r]));
    sc[r] = E::to_f32(__builtin_bit_cast(T, (uint16_t)sc_raw[r]));
    bv[r] = has_bias ? E::to_f32(__builtin_bit_cast(T, (uint16_t)bv_raw[r])) : 0.f;
  }
#pragma unroll
  for (int tf = 0; tf < TF; ++tf) {
    const int m = tf * 16 + fi;
    if (m < M) {
      T out[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) out[r] = scale_round_add_round<DT>(acc[tf][r], sc[r], has_bias, bv[r]);
      if (n0 + 3 < N && (N & 3) == 0) {
        *reinterpret_cast<uint2*>(yg + (size_t)m * N + n0) = *reinterpret_cast<const uint2*>(out);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < N) yg[(size_t)m * N + n0 + r] = out[r];
      }
    }
  }
}


constexpr int lds_bytes(int tf, int stages) { return stages * (64 * BK + tf * 16 * BK * 2); }

// Everything the host decides about a call (see skinny::Plan in qbits_skinny.hip, which this follows): qbytes_skinny_supported / _workspace, their
// _multi forms and the launch read it and nothing else.  Made per call, never kept.
struct Plan {
  // the call (make_plan): what the supported / workspace entries answer
  bool served, multi;
  int S, grid;         // K split, workgroups = feature blocks of 64 * S
  size_t workspace;    // bytes the split this shape asks for needs (0: unsplit), whatever the caller then brought
  // one pass of up to 64 rows (plan_pass): what only the launch needs
  int rows, tf;        // rows of x and their token fragments of 16: 1, 2 or 4
  int stages;          // DMA ring depth
  int lds;             // dynamic LDS bytes
};

// `N`: all features of the launch (multi: the Linears' N added up); `workspace_bytes`: what the caller's split may use (queries: SIZE_MAX)
// Three steps, as in qbits_skinny.hip: plan_format ("served": the supported entries), make_plan (+ split, grid, workspace), plan_pass (+ ring).
constexpr int fragments(int64_t rows) { return rows <= 16 ? 1 : (rows <= 32 ? 2 : 4); }
static Plan plan_format(int64_t M, int64_t N, int64_t K, int a_dtype, int b_dtype, int out_dtype, bool multi) {
  Plan p{};
  p.multi = multi;
  const bool bd = b_dtype == QUANTO_HIP_I8 || b_dtype == QUANTO_HIP_F8_E4M3FN || b_dtype == QUANTO_HIP_F8_E5M2 || b_dtype == QUANTO_HIP_F8_E4M3FNUZ;
  p.served = bd && a_dtype == out_dtype && (out_dtype == QUANTO_HIP_BF16 || out_dtype == QUANTO_HIP_F16) && K % BK == 0 && M >= 1 &&
             M <= QUANTO_HIP_SKINNY_MAX_M && N >= 1 && N < (1 << 30) && K < (1 << 30);
  return p;
}

static Plan make_plan(int64_t M, int64_t N, int64_t K, int a_dtype, int b_dtype, int out_dtype, bool multi, size_t workspace_bytes) {
  Plan p = plan_format(M, N, K, a_dtype, b_dtype, out_dtype, multi);
  if (!p.served) return p;
  // split: same rule as qbits_skinny.hip - 250-500 blocks, at least 8 tiles per block; one counter per feature block of 64
  const int blocks = (int)((N + 63) / 64), tiles = (int)(K / BK);
  int s = 1;
  while (s < 8 && blocks * s * 2 <= 512 && tiles % (s * 2) == 0 && tiles / (s * 2) >= 8) s *= 2;
  const int forced = env_int("QUANTO_HIP_SKINNY_SPLIT", 0);  // experiments
  if (forced > 0 && tiles % forced == 0) s = forced;
  if (!ws_counters_fit(blocks)) s = 1;
  // [counters (zero on entry, zero on exit) | fp32 partial sums]; the passes of M > 64 reuse it
  p.workspace = s == 1 ? 0 : QUANTO_HIP_WS_COUNTER_BYTES + (size_t)blocks * s * 256 * fragments(M > 64 ? 64 : M) * 16;
  p.S = workspace_bytes >= p.workspace ? s : 1;
  p.grid = blocks * p.S;
  return p;
}

// The ring of one pass of `rows` rows (the short last pass of M > 64 has fewer fragments than the others): 4 stages (48 / 64 KiB: two to three
// blocks per CU, which hide each other's barrier and reduction stalls - see the measurements in qbits_skinny.hip) unless the experiment knob asks
// for the deep ring (8 stages, 6 with four fragments: one block per CU); the multi-Linear launch keeps the default ring
static void plan_pass(Plan& p, int rows) {
  p.rows = rows;
  p.tf = fragments(rows);
  const bool deep = !p.multi && env_int("QUANTO_HIP_SKINNY_LDS_KB", 50) >= 100;
  p.stages = deep ? (p.tf == 4 ? 6 : 8) : 4;
  p.lds = lds_bytes(p.tf, p.stages);
}

// ---- plan -> instantiation: the only place that names them ----------------------------------------------------------------------------------------
template <int DT, int FMT, int TF, int STAGES, bool MULTI>
static int launch_k(const Plan& p, const Args& a, const Segs& segs, hipStream_t stream) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qbytes_skinny_kernel<DT, FMT, TF, STAGES, MULTI>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            p.lds);
  hipLaunchKernelGGL((qbytes_skinny_kernel<DT, FMT, TF, STAGES, MULTI>), dim3(p.grid), dim3(256), p.lds, stream, a, segs);
  return launch_status();
}
// (the multi form of the deep rings is one no plan asks for: it was instantiated before, and still is)
template <int DT, int FMT, int TF, int STAGES>
static int launch_m(const Plan& p, const Args& a, const Segs& segs, bool multi, hipStream_t stream) {
  return multi ? launch_k<DT, FMT, TF, STAGES, true>(p, a, segs, stream) : launch_k<DT, FMT, TF, STAGES, false>(p, a, segs, stream);
}

template <int DT, int FMT>
static int launch(const Plan& p, const Args& a, const Segs& segs, bool multi, hipStream_t stream) {
  if (p.stages == 4) {
    if (p.tf == 1) return launch_m<DT, FMT, 1, 4>(p, a, segs, multi, stream);
    if (p.tf == 2) return launch_m<DT, FMT, 2, 4>(p, a, segs, multi, stream);
    return launch_m<DT, FMT, 4, 4>(p, a, segs, multi, stream);
  }
  if (p.tf == 1) return launch_m<DT, FMT, 1, 8>(p, a, segs, multi, stream);
  if (p.tf == 2) return launch_m<DT, FMT, 2, 8>(p, a, segs, multi, stream);
  return launch_m<DT, FMT, 4, 6>(p, a, segs, multi, stream);
}

// One host path: `l.nseg` Linears sharing x (the plain op is nseg = 1, the kernel without the segment lookup), `N` all features of the launch.
static int run(const void* x, const Linears& l, int64_t M, int64_t N, int64_t K, int a_dtype, int b_dtype, int out_dtype, void* workspace,
               size_t workspace_bytes, hipStream_t stream) {
  const bool multi = l.nseg > 1;
  // split-K only with a workspace (whose counter words the caller guarantees to be zero); without one: one block per feature block
  const size_t ws_bytes = ws_holds(workspace, workspace_bytes, 0) ? workspace_bytes : 0;
  Plan p = make_plan(M, N, K, a_dtype, b_dtype, out_dtype, multi, ws_bytes);
  if (!p.served) return QUANTO_HIP_ENOTSUP;
  if (l.align % 16) return QUANTO_HIP_EALIGN;
  Segs segs;
  fill_segments(
      l.nseg, segs.first_fb,
      [&](int i, int j) {
        segs.w[i] = reinterpret_cast<const uint8_t*>(l.w[j]);
        segs.scale[i] = l.scale[j];
        segs.bias[i] = l.bias[j];
        segs.y[i] = l.y[j];
        segs.N[i] = l.N[j];
      },
      [&](int i) { return l.N[i] / 64; });
  for (int64_t m0 = 0; m0 < M; m0 += 64) {  // passes of up to 64 rows; multi: M <= 64
    const int rows = (int)(M - m0 < 64 ? M - m0 : 64);
    if (rows != p.rows) plan_pass(p, rows);
    const Args a{reinterpret_cast<const uint8_t*>(x) + (size_t)m0 * K * 2, segs.w[0], segs.scale[0], segs.bias[0],
                 reinterpret_cast<uint8_t*>(segs.y[0]) + (size_t)m0 * N * 2, rows, segs.N[0], (int)K, p.S, reinterpret_cast<int*>(workspace),
                 p.S > 1 ? ws_partials(workspace) : nullptr, env_int("QUANTO_HIP_SKINNY_NT", M <= 64 ? 1 : 0)};
    int r;
#define QH_FMT(DT)                                                                                            \
  r = b_dtype == QUANTO_HIP_I8 ? launch<DT, W_I8>(p, a, segs, multi, stream)                                  \
      : b_dtype == QUANTO_HIP_F8_E4M3FN ? launch<DT, W_F8E4M3>(p, a, segs, multi, stream)                     \
      : b_dtype == QUANTO_HIP_F8_E4M3FNUZ ? launch<DT, W_F8E4M3FNUZ>(p, a, segs, multi, stream)               \
                                        : launch<DT, W_F8E5M2>(p, a, segs, multi, stream)
    if (out_dtype == QUANTO_HIP_BF16) {
      QH_FMT(QUANTO_HIP_BF16);
    } else {
      QH_FMT(QUANTO_HIP_F16);
    }
#undef QH_FMT
    if (r != QUANTO_HIP_OK) return r;
  }
  return QUANTO_HIP_OK;
}

}  // namespace skinny8

bool qbytes_skinny_supported(const QbytesShape& s) { return skinny8::plan_format(s.M, s.N, s.K, s.a_dtype, s.b_dtype, s.out_dtype, false).served; }
// 0 as well when the shape is not served
size_t qbytes_skinny_workspace(const QbytesShape& s) {
  return skinny8::make_plan(s.M, s.N, s.K, s.a_dtype, s.b_dtype, s.out_dtype, false, SIZE_MAX).workspace;
}

int qbytes_mm_skinny(const QbytesCall& c) {
  return skinny8::run(c.a, gather_linears(c.a, 1, &c.b, &c.scales, nullptr, &c.bias, &c.y, &c.N), c.M, c.N, c.K, c.a_dtype, c.b_dtype, c.out_dtype,
                      c.workspace, c.workspace_bytes, c.stream);
}

// ---- several Linears with a shared input in one launch (3 <= M <= 64), see qbits_skinny.hip ------------------------------------
// all features of the launch; 0: not a group this launch takes
static int64_t multi_total(int nseg, const int64_t* N, int64_t M) {
  if (nseg < 1 || nseg > skinny8::MAX_SEGS || M < 1 || M > 64) return 0;
  int64_t t = 0;
  for (int i = 0; i < nseg; ++i) {
    if (N[i] <= 0 || N[i] % 64) return 0;
    t += N[i];
  }
  return t;
}

bool qbytes_skinny_multi_supported(int nseg, const int64_t* N, int64_t M, int64_t K, int a_dtype, int b_dtype, int out_dtype) {
  const int64_t total = multi_total(nseg, N, M);
  return total > 0 && skinny8::plan_format(M, total, K, a_dtype, b_dtype, out_dtype, true).served;
}

size_t qbytes_skinny_multi_workspace(int nseg, const int64_t* N, int64_t M, int64_t K) {
  const int64_t total = multi_total(nseg, N, M);
  return total > 0 ? skinny8::make_plan(M, total, K, QUANTO_HIP_BF16, QUANTO_HIP_I8, QUANTO_HIP_BF16, true, SIZE_MAX).workspace : 0;
}

int qbytes_mm_skinny_multi(const QbytesMultiCall& c) {
  const int64_t total = multi_total(c.count, c.N, c.M);
  if (total <= 0) return QUANTO_HIP_ENOTSUP;
  return skinny8::run(c.a, gather_linears(c.a, c.count, c.b, c.scales, nullptr, c.bias, c.y, c.N), c.M, total, c.K, c.a_dtype, c.b_dtype, c.out_dtype,
                      c.workspace, c.workspace_bytes, c.stream);
}

}  // namespace qh

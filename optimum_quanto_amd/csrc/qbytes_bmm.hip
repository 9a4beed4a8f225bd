// torch.bmm / torch.matmul on two int8 ActivationQBytesTensors - the q k^T and p v of an eager attention block of a model quantized with
// activations = qint8 - as ONE batched int8 x int8 product on the 8-bit matrix instructions.  The reference's handler (tensor/activations/qbytes_ops.py:
// 175-186) casts both operands to fp32, runs an fp32 bmm, multiplies by the scale product and casts: five launches and an fp32 GEMM.
//
//   y[b, m, n] = T( float( sum_k a[b, m, k] * w[b, k, n] ) * scale ),   T in {bf16, fp16, fp32}
//
// - the sum exact in int32 (v_mfma_i32_16x16x64_i8; |sum| <= K * 128 * 128 < 2^31 for K <= 131071), ONE round-to-nearest-even int32 -> fp32, ONE fp32
// multiply by the scalar `scale` read from device memory, ONE rounding to T.  For K <= 1024 every partial sum of the fp32 sequence is an exact integer
// (< 2^24), so the result is bit-identical to it; beyond, the fp32 bmm rounds partial sums in an unspecified order and this kernel returns the correctly
// rounded value of the exact sum - the only observable difference.
//
// Operands are views: a pointer plus byte strides.  a [B, M, K] has K contiguous; w [B, K, N] comes in both forms that reach aten.bmm - K contiguous
// ("NT": matmul(a, b.transpose(1, 2)) on a 3-D b) or N contiguous ("NN": the contiguous [B, K, N] tensor matmul's reshape makes of a 4-D
// k.transpose(2, 3)).  Any batch stride, 0 (an expanded operand) included.  y is dense [B, M, N].
//
// One workgroup = 256 threads = one 64 x 64 output tile of one batch member; wave w owns rows 16 w .. 16 w + 15 and all 64 columns (four i32x4
// accumulators).  The batch index is folded into the linear workgroup index with the tile indices (grid.x = B * tiles < 2^31), never grid.z.
// K is walked in steps of 64 through two LDS images per buffer, [row][k] of a and [n][k] of w, rows padded to 80 bytes (the 16 lanes of a fragment
// read then touch 16 distinct 16-byte slots); two buffers: the loads of step t + 1 are in flight while step t multiplies.  A fragment is one 16-byte LDS
// read per operand per MFMA with the lane map of qmm_native8.hip / qconv_a8.hip: row lane & 15, 16-byte chunk lane >> 4.
// NN form: the transposition happens while staging - a thread takes a 4 (k) x 4 (n) byte block (four loads along n from four consecutive k rows),
// transposes it in registers with v_perm and writes four dwords into the [n][k] image.  Sixteen neighbouring lanes cover 64 contiguous bytes of one k
// row, so the 4 x 4 block keeps the requests whole lines; its loads are at most 4 bytes wide.
//
// Loads.  The width per operand is chosen on the host from the alignment of its pointer and strides: 16 bytes (K-contiguous operands only), 4 bytes, or
// single bytes.  No load touches a byte outside [row start, row start + row length) of the row it reads: a chunk that crosses the end of its row (the
// ragged last K-step) is read in narrower pieces up to the row's last byte, a chunk behind the end not at all, and both enter the MFMA as zeros; tile
// rows and columns outside the problem read the tile's last row or column of the problem again - their products are never stored.
//
// The epilogue's fp32 math is written on scalars and the unit is compiled with -fno-slp-vectorize (csrc/Makefile): packed fp32 next to MFMAs,
// profiles/r05_packed_fp32_op_sel_next_to_mfma.md.  No split-K, no workspace, no atomics.
#include <type_traits>

#include "qh_kernels.h"

namespace qh {
namespace bmm8 {

constexpr int BM = 64, BN = 64, BK = 64, NT = 256;
constexpr int ROW = BK + 16;        // bytes of one padded LDS row
constexpr int TILE_BYTES = BM * ROW;  // one operand tile (BM == BN)
constexpr int64_t kMaxK = 131071;   // the last K with K * 128 * 128 < 2^31

typedef __attribute__((ext_vector_type(4))) int i32x4;

struct Args {
  const uint8_t* a;    // [B, M, K] int8, K contiguous
  const uint8_t* w;    // [B, K, N] int8, K or N contiguous
  const float* scale;  // one fp32 element on the device
  void* y;             // [B, M, N] out dtype, dense
  int64_t M, N;
  int K;
  int64_t a_batch, a_row;       // byte strides of a
  int64_t w_batch, w_k, w_n;    // byte strides of w (one of w_k, w_n is 1)
  int mtiles, ntiles;           // B * mtiles * ntiles < 2^31
  int out_dtype;                // QUANTO_HIP_{F32, F16, BF16}
};

// Four bytes p[0 .. 4) of a row as one dword.  W: the alignment the host established for p - 4 and up: one dword load; 1: byte loads.
template <int W>
__device__ __forceinline__ uint32_t load4(const uint8_t* p) {
  if constexpr (W >= 4) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// A whole 16-byte chunk of a row.
template <int W>
__device__ __forceinline__ uint4 load16(const uint8_t* p) {
  if constexpr (W == 16) return *reinterpret_cast<const uint4*>(p);
  return make_uint4(load4<W>(p), load4<W>(p + 4), load4<W>(p + 8), load4<W>(p + 12));
}
// The end of a row: the bytes p[0 .. min(valid, 4)), zeros behind `valid` (<= 0: nothing is read).
template <int W>
__device__ __forceinline__ uint32_t load_tail4(const uint8_t* p, int valid) {
  if (valid >= 4) return load4<W>(p);
  uint32_t b0 = 0, b1 = 0, b2 = 0;
  if (valid > 0) b0 = p[0];
  if (valid > 1) b1 = p[1];
  if (valid > 2) b2 = p[2];
  return b0 | (b1 << 8) | (b2 << 16);
}
// ... of a 16-byte chunk: whole dwords while they lie inside the row, then bytes.
template <int W>
__device__ __forceinline__ uint4 load_tail16(const uint8_t* p, int valid) {
  if (valid >= 16) return load16<W>(p);
  constexpr int W4 = W >= 4 ? 4 : 1;
  return make_uint4(load_tail4<W4>(p, valid), load_tail4<W4>(p + 4, valid - 4), load_tail4<W4>(p + 8, valid - 8), load_tail4<W4>(p + 12, valid - 12));
}

// ---- epilogue: lane (column lane & 15, rows 4 (lane >> 4) + r) of the wave's four 16 x 16 fragments - the C / D map of every 16 x 16 MFMA ----
template <int DT>
__device__ __forceinline__ void store_tile_dt(const Args& g, const i32x4 (&acc)[4], int b, int64_t m0, int64_t n0, int rows, int cols, int wave, int lane) {
  using E = Elem<DT>;
  using T = typename E::T;
  const float sc = *g.scale;
  T* y = reinterpret_cast<T*>(g.y) + ((int64_t)b * g.M + m0) * g.N + n0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nl = j * 16 + (lane & 15);
    if (nl >= cols) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ml = wave * 16 + (lane >> 4) * 4 + r;
      if (ml >= rows) continue;
      y[(int64_t)ml * g.N + nl] = scale_round_add_round<DT>((float)acc[j][r], sc, false, 0.f);  // v_cvt_f32_i32 (RNE), one multiply; no bias in this product
    }
  }
}

// AW / WW: load width of a / of w (16, 4 or 1 bytes; the NN form takes 4 or 1).  NN: w has N contiguous.
template <int AW, int WW, bool NN>
__global__ void __launch_bounds__(NT) qbytes_bmm_kernel(const Args g) {
  static_assert(!NN || WW <= 4, "the 4 x 4 block of the NN form is loaded in dwords or bytes");
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * 2 * TILE_BYTES];  // [2 buffers][a tile | w tile]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = g.mtiles * g.ntiles;
  const int bid = (int)blockIdx.x;
  const int b = bid / tiles, t = bid - b * tiles;
  const int mt = t / g.ntiles, nt = t - mt * g.ntiles;
  const int64_t m0 = (int64_t)mt * BM, n0 = (int64_t)nt * BN;
  const int rows = g.M - m0 < BM ? (int)(g.M - m0) : BM, cols = g.N - n0 < BN ? (int)(g.N - n0) : BN;
  const int K = g.K;
  const int nk = (K + BK - 1) / BK;

  // ---- staging: a and the NT form of w - tile row tid >> 2, 16-byte chunk tid & 3; NN form - 4 x 4 block (n block tid & 15, k block tid >> 4).
  // Tile rows behind M (columns behind N) are never stored, so nothing has to be zero there: such a thread reads the tile's last row (column) again -
  // a row of the problem, inside its bounds.  Only k behind K must enter the MFMA as zeros: the last, ragged K-step reads narrower (load_tail*).
  const int sr = tid >> 2, sc = tid & 3;
  const int nb = tid & 15, kb = tid >> 4;
  const uint8_t* pa = g.a + (int64_t)b * g.a_batch + (m0 + (sr < rows ? sr : rows - 1)) * g.a_row + 16 * sc;
  const uint8_t* pw = NN ? g.w + (int64_t)b * g.w_batch + (int64_t)(4 * kb) * g.w_k + n0
                         : g.w + (int64_t)b * g.w_batch + (n0 + (sr < cols ? sr : cols - 1)) * g.w_n + 16 * sc;
  // NN: a block whose four columns exist is one dword (four bytes) per k row; the others read each byte at its column clamped to the last one
  const bool n_whole = 4 * nb + 4 <= cols;
  int nc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) nc[q] = 4 * nb + q < cols ? 4 * nb + q : cols - 1;
  auto nn_bytes = [&](const uint8_t* p) -> uint32_t {
    return (uint32_t)p[nc[0]] | ((uint32_t)p[nc[1]] << 8) | ((uint32_t)p[nc[2]] << 16) | ((uint32_t)p[nc[3]] << 24);
  };
  auto nn_row = [&](const uint8_t* p) -> uint32_t { return n_whole ? load4<WW>(p + 4 * nb) : nn_bytes(p); };

  uint4 ra, rw;  // a chunk; w chunk (NT) / the four dwords of the 4 x 4 block, one per k row (NN)
  // WHOLE: the K-step lies inside K - straight-line loads; otherwise the ragged last step
  auto issue_loads = [&](int kt, auto whole) {
    constexpr bool WHOLE = decltype(whole)::value;
    const int k0 = kt * BK;
    if constexpr (WHOLE)
      ra = load16<AW>(pa + k0);
    else
      ra = load_tail16<AW>(pa + k0, K - k0 - 16 * sc);
    if constexpr (NN) {
      const uint8_t* p = pw + (int64_t)k0 * g.w_k;
      const int k = k0 + 4 * kb;
      if constexpr (WHOLE) {
        if (n_whole)  // one branch around all four rows: the loads of either side go out back to back
          rw = make_uint4(load4<WW>(p + 4 * nb), load4<WW>(p + g.w_k + 4 * nb), load4<WW>(p + 2 * g.w_k + 4 * nb), load4<WW>(p + 3 * g.w_k + 4 * nb));
        else
          rw = make_uint4(nn_bytes(p), nn_bytes(p + g.w_k), nn_bytes(p + 2 * g.w_k), nn_bytes(p + 3 * g.w_k));
      } else {
        rw = make_uint4(0u, 0u, 0u, 0u);
        if (k < K) rw.x = nn_row(p);
        if (k + 1 < K) rw.y = nn_row(p + g.w_k);
        if (k + 2 < K) rw.z = nn_row(p + 2 * g.w_k);
        if (k + 3 < K) rw.w = nn_row(p + 3 * g.w_k);
      }
    } else {
      if constexpr (WHOLE)
        rw = load16<WW>(pw + k0);
      else
        rw = load_tail16<WW>(pw + k0, K - k0 - 16 * sc);
    }
  };
  auto issue = [&](int kt) {
    if ((kt + 1) * BK <= K)
      issue_loads(kt, std::true_type{});
    else
      issue_loads(kt, std::false_type{});
  };
  auto write_lds = [&](int buf) {
    uint8_t* sa = smem + buf * 2 * TILE_BYTES;
    uint8_t* sb = sa + TILE_BYTES;
    *reinterpret_cast<uint4*>(sa + sr * ROW + 16 * sc) = ra;
    if constexpr (NN) {
      // rw.{x,y,z,w} = bytes n .. n + 3 of k rows k .. k + 3  ->  one dword (k .. k + 3) per n.  v_perm selects 0-3: second operand, 4-7: first.
      const uint32_t lo01 = __builtin_amdgcn_perm(rw.y, rw.x, 0x05010400u), hi01 = __builtin_amdgcn_perm(rw.y, rw.x, 0x07030602u);
      const uint32_t lo23 = __builtin_amdgcn_perm(rw.w, rw.z, 0x05010400u), hi23 = __builtin_amdgcn_perm(rw.w, rw.z, 0x07030602u);
      uint8_t* d = sb + (4 * nb) * ROW + 4 * kb;
      *reinterpret_cast<uint32_t*>(d) = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
      *reinterpret_cast<uint32_t*>(d + ROW) = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
      *reinterpret_cast<uint32_t*>(d + 2 * ROW) = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
      *reinterpret_cast<uint32_t*>(d + 3 * ROW) = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
    } else {
      *reinterpret_cast<uint4*>(sb + sr * ROW + 16 * sc) = rw;
    }
  };

  i32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = i32x4{0, 0, 0, 0};

  if (nk > 0) {
    issue(0);
    write_lds(0);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) issue(kt + 1);
    const uint8_t* sa = smem + cur * 2 * TILE_BYTES;
    const uint8_t* sb = sa + TILE_BYTES;
    const int frag = (lane & 15) * ROW + (lane >> 4) * 16;  // row lane & 15, chunk lane >> 4
    const i32x4 fa = *reinterpret_cast<const i32x4*>(sa + wave * 16 * ROW + frag);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const i32x4 fb = *reinterpret_cast<const i32x4*>(sb + j * 16 * ROW + frag);
      acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa, fb, acc[j], 0, 0, 0);
    }
    if (kt + 1 < nk) write_lds(cur ^ 1);  // the buffer step kt - 1 read: every wave passed the barrier behind those reads
    __syncthreads();
    cur ^= 1;
  }

  if (g.out_dtype == QUANTO_HIP_BF16)
    store_tile_dt<QUANTO_HIP_BF16>(g, acc, b, m0, n0, rows, cols, wave, lane);
  else if (g.out_dtype == QUANTO_HIP_F16)
    store_tile_dt<QUANTO_HIP_F16>(g, acc, b, m0, n0, rows, cols, wave, lane);
  else
    store_tile_dt<QUANTO_HIP_F32>(g, acc, b, m0, n0, rows, cols, wave, lane);
}

template <int AW, int WW, bool NN>
static void launch_k(const Args& g, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL((qbytes_bmm_kernel<AW, WW, NN>), dim3(blocks), dim3(NT), 0, stream, g);
}
template <int AW>
static void launch_w(const Args& g, int ww, bool nn, unsigned blocks, hipStream_t stream) {
  if (nn)
    ww >= 4 ? launch_k<AW, 4, true>(g, blocks, stream) : launch_k<AW, 1, true>(g, blocks, stream);
  else if (ww == 16)
    launch_k<AW, 16, false>(g, blocks, stream);
  else
    ww == 4 ? launch_k<AW, 4, false>(g, blocks, stream) : launch_k<AW, 1, false>(g, blocks, stream);
}

// the widest load every row start of an operand is aligned for: its pointer and the strides that are walked (a dimension of one element has none)
static int load_width(const void* p, int64_t batch_stride, int64_t batches, int64_t row_stride, int64_t rows) {
  const uint64_t u = reinterpret_cast<uintptr_t>(p) | (uint64_t)(batches > 1 ? batch_stride : 0) | (uint64_t)(rows > 1 ? row_stride : 0);
  return u % 16 == 0 ? 16 : u % 4 == 0 ? 4 : 1;
}

}  // namespace bmm8
}  // namespace qh

extern "C" int quanto_hip_qbytes_bmm(const void* a, const void* w, const void* scale, void* y, int64_t B, int64_t M, int64_t N, int64_t K,
                                     int64_t a_batch_stride, int64_t a_row_stride, int64_t w_batch_stride, int64_t w_k_stride, int64_t w_n_stride,
                                     int out_dtype, void* stream) {
  using namespace qh;
  using namespace qh::bmm8;
  if (B < 0 || M < 0 || N < 0 || K < 0 || a_batch_stride < 0 || a_row_stride < 0 || w_batch_stride < 0 || w_k_stride < 0 || w_n_stride < 0)
    return QUANTO_HIP_EINVAL;
  if (out_dtype != QUANTO_HIP_F32 && out_dtype != QUANTO_HIP_F16 && out_dtype != QUANTO_HIP_BF16) return QUANTO_HIP_ENOTSUP;
  if (w_k_stride != 1 && w_n_stride != 1) return QUANTO_HIP_ENOTSUP;
  if (K > kMaxK) return QUANTO_HIP_ENOTSUP;
  constexpr int64_t kLimit = (int64_t)1 << 31;
  const int64_t mtiles = (M + BM - 1) / BM, ntiles = (N + BN - 1) / BN;  // (M, N < 2^63 - 64 or the sums wrap negative: refused below)
  if (mtiles < 0 || ntiles < 0 || mtiles >= kLimit || ntiles >= kLimit || B >= kLimit) return QUANTO_HIP_ENOTSUP;
  if (mtiles * ntiles >= kLimit || B * (mtiles * ntiles) >= kLimit) return QUANTO_HIP_ENOTSUP;
  if (B == 0 || M == 0 || N == 0) return QUANTO_HIP_OK;
  // (an empty a or w - K = 0 - is never read and may be null)
  if (!scale || !y || (K > 0 && (!a || !w))) return QUANTO_HIP_EINVAL;

  Args g{};
  g.a = reinterpret_cast<const uint8_t*>(a), g.w = reinterpret_cast<const uint8_t*>(w), g.scale = reinterpret_cast<const float*>(scale), g.y = y;
  g.M = M, g.N = N, g.K = (int)K;
  g.a_batch = a_batch_stride, g.a_row = a_row_stride, g.w_batch = w_batch_stride, g.w_k = w_k_stride, g.w_n = w_n_stride;
  g.mtiles = (int)mtiles, g.ntiles = (int)ntiles, g.out_dtype = out_dtype;
  const bool nn = w_k_stride != 1;  // K contiguous wins when both are 1: its chunks load 16 bytes wide
  const int aw = load_width(a, a_batch_stride, B, a_row_stride, M);
  const int ww = nn ? load_width(w, w_batch_stride, B, w_k_stride, K) : load_width(w, w_batch_stride, B, w_n_stride, N);
  const unsigned blocks = (unsigned)(B * mtiles * ntiles);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (aw == 16)
    launch_w<16>(g, ww, nn, blocks, s);
  else if (aw == 4)
    launch_w<4>(g, ww, nn, blocks, s);
  else
    launch_w<1>(g, ww, nn, blocks, s);
  const int r = launch_status();
  if (r == QUANTO_HIP_OK) set_last_kernel("bmm_i8");
  return r;
}

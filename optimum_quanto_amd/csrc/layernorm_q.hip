// QLayerNorm with its output quantization in the same launch: the float row is read once, the int8 / fp8 codes are stored - the float output of the
// two-op sequence (F.layer_norm, then quanto::quantize_symmetric at the module's output scale: nn/qlayernorm.py + the output hook of nn/qmodule.py)
// is never written.  With a 16-bit T the sequence moves 2 + 2 + 2 + 1 bytes per element, this kernel 2 + 1.
//
//   codes[r, :] = Q( T( (x[r, :] - mean_r) * rstd_r * w + b ), out_scale ),   T in {bf16, fp16, fp32},  codes int8 / e4m3fn / e5m2
//
// over a [rows, n] view: n = prod(normalized_shape) elements contiguous inside a row, any row stride >= n (in elements); codes dense [rows, n].
// w and b (n elements of T each) may be null; out_scale is one element of T in device memory, read here - nothing is synchronised on the host.
//
// Numerics.  Statistics in fp32, two passes over the row held in registers: the mean first, then the mean of the squared deviations from THAT mean
// (never E[x^2] - mean^2, which cancels for rows whose mean is large against their spread).  rstd = 1 / sqrt(var + eps) with the correctly rounded
// fp32 sqrt and divide hipcc emits by default (no v_rsq_f32 approximation).  The affine step is fp32 and rounded ONCE to T - the element the float
// module would have stored - and the rule of qh_quantize.h is applied to that element: clamp_target<ODT>(quotient_in<IDT>(t, os)), pack4<ODT>; the same
// copy every other code-storing epilogue uses.  So the codes are those of the two-op sequence up to the last bits of the statistics (a reduction order
// is nobody's contract): a code differs from the sequence's only where the float element lands on the other side of a rounding boundary.
//
// Shape.  n > kWaveRowMaxN: one row per workgroup of 256 threads, up to four units of 8 elements per thread (kMaxN = 256 * 8 * 4); the two sums cross
// the four waves through LDS (one barrier each, a slot array per pass).  n <= kWaveRowMaxN: one row per wave, four rows per workgroup, up to two units
// per lane, no LDS and no barrier.  Unit u of thread t is elements 8 (u * threads + t) .. + 7: neighbouring lanes read neighbouring 16 bytes.  Wave
// sums are __shfl_xor butterflies (qh::wave_sum): every lane ends with the same bits.
// Loads are 16 bytes wide when x, w, b and the row stride in bytes are multiples of 16 (chosen on the host), element by element otherwise; the ragged
// last unit of a row is always read element by element up to the row's last one, a unit behind the end not at all.  Codes leave as one 8-byte store per
// unit, two 4-byte stores, or bytes - by the alignment of yq and n, chosen on the host; the ragged unit stores a dword while four codes remain, then
// bytes.  No load or store touches a byte outside its row.  No atomics, no workspace, no MFMA.
#include "qh_kernels.h"
#include "qh_quantize.h"

namespace qh {
namespace lnq {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int NT = 256;  // threads of a workgroup
constexpr int E = 8;     // elements of a unit
constexpr int kBlockUnits = 4, kWaveUnits = 2;
constexpr int kMaxN = QUANTO_HIP_LAYER_NORM_Q_MAX_N;
constexpr int kWaveRowMaxN = kWave * E * kWaveUnits;  // 1024: the longest row one wave holds
static_assert(kMaxN == NT * E * kBlockUnits, "the row of a workgroup: four units of eight elements per thread");

struct Args {
  const void* x;
  const void* w;   // null: no elementwise affine
  const void* b;   // null: no bias
  const void* os;  // one element of T
  uint8_t* yq;     // [rows, n] codes, dense
  int64_t rows, row_stride;  // row stride of x in elements
  int n;
  float eps;
  int store_width;  // 8, 4 or 1: what yq + r * n is aligned for at every row r
};

// The elements p[0 .. min(valid, 8)) of a row as fp32, zeros behind `valid` (> 0).  VEC: p is 16-byte aligned and whole units are read 16 bytes wide.
template <int IDT, bool VEC>
__device__ __forceinline__ void load_unit(const typename Elem<IDT>::T* p, int valid, float (&v)[E]) {
  using El = Elem<IDT>;
  using T = typename El::T;
  if (valid >= E) {
    if constexpr (VEC) {
      __attribute__((aligned(16))) T e[E];
      reinterpret_cast<u32x4*>(e)[0] = reinterpret_cast<const u32x4*>(p)[0];
      if constexpr (sizeof(T) == 4) reinterpret_cast<u32x4*>(e)[1] = reinterpret_cast<const u32x4*>(p)[1];
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = El::to_f32(e[k]);
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = El::to_f32(p[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      v[k] = 0.f;
      if (k < valid) v[k] = El::to_f32(p[k]);
    }
  }
}

// The codes of one unit: p + [0, min(valid, 8)).  `width`: the alignment of p (8, 4 or 1 bytes).
__device__ __forceinline__ void store_unit(uint8_t* p, int valid, uint32_t lo, uint32_t hi, int width) {
  if (valid >= E && width == 8) {
    *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
    return;
  }
  int k = 0;
  if (width >= 4) {
    if (valid >= 4) *reinterpret_cast<uint32_t*>(p) = lo, k = 4;
    if (valid >= E) *reinterpret_cast<uint32_t*>(p + 4) = hi, k = E;
  }
  for (; k < valid && k < E; ++k) p[k] = (uint8_t)((k < 4 ? lo : hi) >> (8 * (k & 3)));
}

// The sum of `s` over the threads of a row, the same bits in every thread: the wave's butterfly, then (one row per workgroup) the four waves' sums
// through `slots`, added in one order by everybody.
template <bool WAVE_ROW>
__device__ __forceinline__ float row_sum(float s, float* slots, int wave, int lane) {
  s = wave_sum(s);
  if constexpr (WAVE_ROW) return s;
  if (lane == 0) slots[wave] = s;
  __syncthreads();
  return (slots[0] + slots[1]) + (slots[2] + slots[3]);
}

template <int IDT, int ODT, bool VEC, bool WAVE_ROW>
__global__ void __launch_bounds__(NT) layer_norm_q_kernel(const Args g) {
  using El = Elem<IDT>;
  using T = typename El::T;
  constexpr int UNITS = WAVE_ROW ? kWaveUnits : kBlockUnits;
  constexpr int THREADS = WAVE_ROW ? kWave : NT;  // threads of a row
  __shared__ float slots[2][NT / kWave];

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t row = WAVE_ROW ? (int64_t)blockIdx.x * (NT / kWave) + wave : (int64_t)blockIdx.x;
  if constexpr (WAVE_ROW) {
    if (row >= g.rows) return;  // a whole wave: this form has no barrier
  }
  const int t = WAVE_ROW ? lane : tid;
  const int n = g.n;
  const T* x = reinterpret_cast<const T*>(g.x) + row * g.row_stride;

  // ---- the row, once: unit u of this thread is elements [8 (u THREADS + t), + 8) ----
  float v[UNITS][E];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    const int start = (u * THREADS + t) * E;
    if (start < n) {
      load_unit<IDT, VEC>(x + start, n - start, v[u]);
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k) v[u][k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < E; ++k) s += v[u][k];
  }
  // (true divides by n: a row whose sum is exact in fp32 gets the correctly rounded mean - a constant row its own value, deviations exactly zero)
  const float mean = row_sum<WAVE_ROW>(s, slots[0], wave, lane) / (float)n;

  // ---- deviations from that mean, in place; elements behind the row's end stay zero ----
  float ss = 0.f;
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    const int start = (u * THREADS + t) * E;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const float d = start + k < n ? v[u][k] - mean : 0.f;
      v[u][k] = d;
      ss += d * d;
    }
  }
  const float var = row_sum<WAVE_ROW>(ss, slots[1], wave, lane) / (float)n;
  const float rstd = 1.f / __builtin_sqrtf(var + g.eps);  // correctly rounded sqrt and divide (hipcc's default for fp32)

  // ---- affine in fp32, one rounding to T, the rule of qh_quantize.h on that element ----
  const T* w = reinterpret_cast<const T*>(g.w);
  const T* b = reinterpret_cast<const T*>(g.b);
  const float os = El::to_f32(*reinterpret_cast<const T*>(g.os));
  uint8_t* yq = g.yq + row * (int64_t)n;
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    const int start = (u * THREADS + t) * E;
    if (start >= n) continue;
    const int valid = n - start;
    float wv[E], bv[E];
    if (w) load_unit<IDT, VEC>(w + start, valid, wv);
    if (b) load_unit<IDT, VEC>(b + start, valid, bv);
    float q[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      float y = v[u][k] * rstd;
      if (w) y *= wv[k];
      if (b) y += bv[k];
      asm volatile("" : "+v"(y));  // rounded to fp32 first, then once to T (no single-rounding v_fma_mixlo_f16)
      const T e = El::from_f32(y);  // the element the float module stores
      q[k] = clamp_target<ODT>(quotient_in<IDT>(El::to_f32(e), os));
    }
    store_unit(yq + start, valid, pack4<ODT>(q), pack4<ODT>(q + 4), g.store_width);
  }
}

template <int IDT, int ODT>
static void launch_form(const Args& g, bool vec, hipStream_t stream) {
  if (g.n <= kWaveRowMaxN) {
    const unsigned blocks = (unsigned)((g.rows + NT / kWave - 1) / (NT / kWave));
    if (vec)
      hipLaunchKernelGGL((layer_norm_q_kernel<IDT, ODT, true, true>), dim3(blocks), dim3(NT), 0, stream, g);
    else
      hipLaunchKernelGGL((layer_norm_q_kernel<IDT, ODT, false, true>), dim3(blocks), dim3(NT), 0, stream, g);
  } else {
    const unsigned blocks = (unsigned)g.rows;
    if (vec)
      hipLaunchKernelGGL((layer_norm_q_kernel<IDT, ODT, true, false>), dim3(blocks), dim3(NT), 0, stream, g);
    else
      hipLaunchKernelGGL((layer_norm_q_kernel<IDT, ODT, false, false>), dim3(blocks), dim3(NT), 0, stream, g);
  }
}

template <int IDT>
static void launch_out(const Args& g, int out_dtype, bool vec, hipStream_t stream) {
  if (out_dtype == QUANTO_HIP_I8)
    launch_form<IDT, QUANTO_HIP_I8>(g, vec, stream);
  else if (out_dtype == QUANTO_HIP_F8_E4M3FN)
    launch_form<IDT, QUANTO_HIP_F8_E4M3FN>(g, vec, stream);
  else
    launch_form<IDT, QUANTO_HIP_F8_E5M2>(g, vec, stream);
}

static int elem_bytes(int dtype) { return dtype == QUANTO_HIP_F32 ? 4 : 2; }

// the rule of both entries: what the kernel serves
static int supported(int64_t rows, int64_t n, int dtype, int out_dtype) {
  if (rows < 0 || n < 0) return QUANTO_HIP_EINVAL;
  if (dtype != QUANTO_HIP_F32 && dtype != QUANTO_HIP_F16 && dtype != QUANTO_HIP_BF16) return QUANTO_HIP_ENOTSUP;
  if (out_dtype != QUANTO_HIP_I8 && out_dtype != QUANTO_HIP_F8_E4M3FN && out_dtype != QUANTO_HIP_F8_E5M2) return QUANTO_HIP_ENOTSUP;
  if (n > kMaxN || rows >= ((int64_t)1 << 31)) return QUANTO_HIP_ENOTSUP;
  return QUANTO_HIP_OK;
}

}  // namespace lnq
}  // namespace qh

extern "C" int quanto_hip_layer_norm_q_supported(int64_t rows, int64_t n, int dtype, int out_dtype) {
  return qh::lnq::supported(rows, n, dtype, out_dtype);
}

extern "C" int quanto_hip_layer_norm_q(const void* x, const void* weight, const void* bias, const void* out_scale, void* yq, int64_t rows, int64_t n,
                                       int64_t row_stride, float eps, int dtype, int out_dtype, void* stream) {
  using namespace qh;
  using namespace qh::lnq;
  if (row_stride < 0) return QUANTO_HIP_EINVAL;
  const int r = supported(rows, n, dtype, out_dtype);
  if (r != QUANTO_HIP_OK) return r;
  if (rows > 1 && row_stride < n) return QUANTO_HIP_EINVAL;  // rows that overlap
  if (rows == 0 || n == 0) return QUANTO_HIP_OK;
  if (!x || !out_scale || !yq) return QUANTO_HIP_EINVAL;

  Args g{};
  g.x = x, g.w = weight, g.b = bias, g.os = out_scale, g.yq = reinterpret_cast<uint8_t*>(yq);
  g.rows = rows, g.row_stride = rows > 1 ? row_stride : n, g.n = (int)n, g.eps = eps;
  // the widest access every row start is aligned for: the pointers and, when more than one row is walked, the row strides in bytes
  const uint64_t in = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias) |
                      (uint64_t)(rows > 1 ? row_stride * elem_bytes(dtype) : 0);
  const uint64_t out = reinterpret_cast<uintptr_t>(yq) | (uint64_t)(rows > 1 ? n : 0);
  const bool vec = in % 16 == 0;
  g.store_width = out % 8 == 0 ? 8 : out % 4 == 0 ? 4 : 1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == QUANTO_HIP_BF16)
    launch_out<QUANTO_HIP_BF16>(g, out_dtype, vec, s);
  else if (dtype == QUANTO_HIP_F16)
    launch_out<QUANTO_HIP_F16>(g, out_dtype, vec, s);
  else
    launch_out<QUANTO_HIP_F32>(g, out_dtype, vec, s);
  const int st = launch_status();
  if (st == QUANTO_HIP_OK) set_last_kernel("layer_norm_q");
  return st;
}

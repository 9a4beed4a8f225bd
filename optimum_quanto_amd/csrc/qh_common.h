// Shared device helpers for libquanto_hip (gfx950 only: wave64, OCP fp8, v_dot2 bf16, MFMA 16x16x32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/quanto_hip.h"

namespace qh {

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int kWave = 64;
constexpr int kMaxLdsBytes = 160 * 1024;  // LDS of a CU: the most dynamic shared memory a workgroup can ask for

// qbits GEMV load policy used when QUANTO_HIP_GEMV_VARIANT is unset (see qbits_gemv.hip): bit 0 = x / scale loads first,
// bit 1 = non-temporal weight loads.  Measured (r2, hipGraph replay, us per launch, variant 0 / 1 / 2 / 3): (1,4096,4096) 4.54 /
// 4.93 / 4.57 / 4.70, (1,4096,11008) 7.49 / 8.33 / 7.40 / 7.99, fused gate+up 2 x (1,4096,14336) 15.5 / 16.0 / 14.2 / 15.4:
// non-temporal loads pay once the stream is long, forcing the small loads to the front never does (hipcc already
// issues them first where it matters).
#ifndef QUANTO_HIP_GEMV_DEFAULT_VARIANT
#define QUANTO_HIP_GEMV_DEFAULT_VARIANT 2
#endif

// ---- element traits for the three float dtypes of the ABI ------------------------------------
template <int DT>
struct Elem;
template <>
struct Elem<QUANTO_HIP_F32> {
  using T = float;
  static __device__ __forceinline__ float to_f32(T v) { return v; }
  static __device__ __forceinline__ T from_f32(float f) { return f; }
};
template <>
struct Elem<QUANTO_HIP_F16> {
  using T = _Float16;
  static __device__ __forceinline__ float to_f32(T v) { return (float)v; }
  static __device__ __forceinline__ T from_f32(float f) { return (_Float16)f; }  // RNE
};
template <>
struct Elem<QUANTO_HIP_BF16> {
  using T = __bf16;
  static __device__ __forceinline__ float to_f32(T v) { return (float)v; }
  static __device__ __forceinline__ T from_f32(float f) { return (__bf16)f; }  // v_cvt_pk_bf16_f32, RNE
};

// ---- the output element of every product (include/quanto_hip.h; DESIGN.md "Parity") -----------------
// THE rounding rule, its one copy: the product rounded to the output type T, the bias added to that in fp32, the sum rounded to T again -
// the reference's order (tensor/weights/qbytes.py:79-81, tensor/function.py:45-46).  `v`: the product in fp32; `bias` is read only with has_bias.
// A kernel that holds the bias as a pointer that may be null (the GEMVs, naive_mm.hip) calls it once per case - bias ? f(.., true, bias[n]) :
// f(.., false, 0.f) - so that the load stays under the test; loading into a value first cost naive_mm.hip's kernels two SGPRs.
template <int DT>
__device__ __forceinline__ typename Elem<DT>::T round_add_round(float v, bool has_bias, float bias) {
  using E = Elem<DT>;
  if (has_bias) v = E::to_f32(E::from_f32(v)) + bias;
  return E::from_f32(v);
}
// the same on accumulator x scale (library/qbytes_mm.py:47-49): the fp32 product is rounded to fp32 in front of anything else, with and without a
// bias - the empty asm keeps hipcc from fusing the multiply into a single-rounding form (v_fma_mixlo_f16, or an fma with the bias add)
template <int DT>
__device__ __forceinline__ typename Elem<DT>::T scale_round_add_round(float acc, float scale, bool has_bias, float bias) {
  float v = acc * scale;
  asm volatile("" : "+v"(v));
  return round_add_round<DT>(v, has_bias, bias);
}

// ---- 8-bit weight/activation decoders ---------------------------------------------------------
// e4m3fnuz has no hardware path on gfx950 (the native fp8 is OCP e4m3fn): decode in software.
__device__ __forceinline__ float decode_e4m3fnuz(uint32_t b) {
  b &= 0xFFu;
  if (b == 0x80u) return __builtin_nanf("");
  const uint32_t e = (b >> 3) & 0xFu, m = b & 7u;
  float v = e == 0 ? (float)m * 0x1p-10f : __builtin_bit_cast(float, ((e + 119u) << 23) | (m << 20));
  return (b & 0x80u) ? -v : v;
}

// e4m3fnuz on the OCP converters (r4): an fnuz byte is the e4m3fn value of the same bits times 1/2 (exponent bias 8 instead of 7; the
// subnormals m * 2^-10 = fn's m * 2^-9 halved), except for the three patterns the two formats disagree on: 0x7F / 0xFF are +-240 in fnuz
// (NaN in fn) and 0x80 is fnuz's only NaN (-0 in fn).  The hardware converts with scale 0.5 (a power of two: exact), the three patterns are
// patched - they are rare but real: the absmax element of every row quantizes to +-240.
__device__ __forceinline__ float fnuz_fix_f32(float half_of_fn, uint32_t byte) {
  float v = half_of_fn;
  if ((byte & 0x7Fu) == 0x7Fu) v = (byte & 0x80u) ? -240.f : 240.f;
  if (byte == 0x80u) v = __builtin_nanf("");
  return v;
}
// two T elements (bytes 2p, 2p + 1 of `word`); MAX_T / NAN_T: 240.0 and a quiet NaN in T
template <uint32_t MAX_T, uint32_t NAN_T>
__device__ __forceinline__ uint32_t fnuz_fix_pair(uint32_t converted, uint32_t word, int p) {
  const uint32_t b0 = (word >> (16 * p)) & 0xFFu, b1 = (word >> (16 * p + 8)) & 0xFFu;
  uint32_t lo = converted & 0xFFFFu, hi = converted >> 16;
  if ((b0 & 0x7Fu) == 0x7Fu) lo = MAX_T | ((b0 & 0x80u) << 8);
  if ((b1 & 0x7Fu) == 0x7Fu) hi = MAX_T | ((b1 & 0x80u) << 8);
  if (b0 == 0x80u) lo = NAN_T;
  if (b1 == 0x80u) hi = NAN_T;
  return lo | (hi << 16);
}
__device__ __forceinline__ uint32_t fnuz_pair_bf16(uint32_t word, int p) {
  const uint32_t c = __builtin_bit_cast(uint32_t, p == 0 ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)word, 0.5f, false)
                                                         : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)word, 0.5f, true));
  return fnuz_fix_pair<0x4370u, 0x7FC0u>(c, word, p);
}
__device__ __forceinline__ uint32_t fnuz_pair_f16(uint32_t word, int p) {
  const uint32_t c = __builtin_bit_cast(uint32_t, p == 0 ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)word, 0.5f, false)
                                                         : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)word, 0.5f, true));
  return fnuz_fix_pair<0x5B80u, 0x7E00u>(c, word, p);
}

// The one family of byte decoders, by the QUANTO_HIP_* code of the stored element: every kernel that turns 8-bit codes into fp32 goes through it.
// byte `i` (a literal after unrolling) of a dword -> fp32.  fp8 / bf8: the byte select of v_cvt_f32_fp8 / v_cvt_f32_bf8 is an immediate.
template <int QDT>
__device__ __forceinline__ float byte_f32(uint32_t d, int i) {
  const uint32_t b = (d >> (8 * i)) & 0xFFu;
  if constexpr (QDT == QUANTO_HIP_I8) {
    return (float)(int8_t)b;
  } else if constexpr (QDT == QUANTO_HIP_U8) {
    return (float)b;  // v_cvt_f32_ubyteN
  } else if constexpr (QDT == QUANTO_HIP_F8_E4M3FN) {
    switch (i) {
      case 0: return __builtin_amdgcn_cvt_f32_fp8((int)d, 0);
      case 1: return __builtin_amdgcn_cvt_f32_fp8((int)d, 1);
      case 2: return __builtin_amdgcn_cvt_f32_fp8((int)d, 2);
      default: return __builtin_amdgcn_cvt_f32_fp8((int)d, 3);
    }
  } else if constexpr (QDT == QUANTO_HIP_F8_E5M2) {
    switch (i) {
      case 0: return __builtin_amdgcn_cvt_f32_bf8((int)d, 0);
      case 1: return __builtin_amdgcn_cvt_f32_bf8((int)d, 1);
      case 2: return __builtin_amdgcn_cvt_f32_bf8((int)d, 2);
      default: return __builtin_amdgcn_cvt_f32_bf8((int)d, 3);
    }
  } else {
    static_assert(QDT == QUANTO_HIP_F8_E4M3FNUZ, "byte_f32: 8-bit element types only");
    return decode_e4m3fnuz(b);
  }
}
// the four bytes of a dword -> four fp32.  fp8 / bf8: two v_cvt_pk_f32_fp8 / bf8; e4m3fnuz: the fn value / 2 + the three patched patterns
template <int QDT>
__device__ __forceinline__ void dword_f32(uint32_t w, float (&f)[4]) {
  if constexpr (QDT == QUANTO_HIP_F8_E4M3FN || QDT == QUANTO_HIP_F8_E4M3FNUZ) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    if constexpr (QDT == QUANTO_HIP_F8_E4M3FN) {
      f[0] = lo.x; f[1] = lo.y; f[2] = hi.x; f[3] = hi.y;
    } else {
      f[0] = fnuz_fix_f32(lo.x * 0.5f, w & 0xFFu);
      f[1] = fnuz_fix_f32(lo.y * 0.5f, (w >> 8) & 0xFFu);
      f[2] = fnuz_fix_f32(hi.x * 0.5f, (w >> 16) & 0xFFu);
      f[3] = fnuz_fix_f32(hi.y * 0.5f, w >> 24);
    }
  } else if constexpr (QDT == QUANTO_HIP_F8_E5M2) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
    f[0] = lo.x; f[1] = lo.y; f[2] = hi.x; f[3] = hi.y;
  } else {
    static_assert(QDT == QUANTO_HIP_I8, "dword_f32: int8, e4m3fn, e5m2, e4m3fnuz");
    f[0] = (float)(int8_t)(w & 0xFFu);
    f[1] = (float)(int8_t)((w >> 8) & 0xFFu);
    f[2] = (float)(int8_t)((w >> 16) & 0xFFu);
    f[3] = (float)(int8_t)(w >> 24);
  }
}
// one stored byte -> fp32
template <int QDT>
__device__ __forceinline__ float decode8(uint8_t b) {
  return byte_f32<QDT>(b, 0);
}

// ---- wave-level sum (64 lanes) ------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
// the same sum on the DPP ladder (six v_add_f32_dpp, no LDS crossbar); only lane 63 holds the total
__device__ __forceinline__ float wave_sum_lane63(float v) {
  v += dpp_f<0xB1>(v);        // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);        // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);       // row_half_mirror
  v += dpp_f<0x140>(v);       // row_mirror  -> every lane of a 16-lane row holds the row sum
  v += dpp_f<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  v += dpp_f<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3 -> lane 63 holds the total
  return v;
}

// Generic PackedTensor geometry for an axis-0 weight [N, K] with group size C (C == K when
// per-channel): grouped rows R = N*K/C, packed rows row_dim = ceil(R / vpi).
struct PackedGeom {
  int64_t N, K, C, G, R, row_dim;
  int bits, vpi;
};
inline PackedGeom make_geom(int64_t N, int64_t K, int bits, int group_size) {
  PackedGeom g;
  g.N = N;
  g.K = K;
  g.bits = bits;
  g.vpi = 8 / bits;
  g.C = group_size > 0 ? group_size : K;
  g.G = K / g.C;
  g.R = N * g.G;
  g.row_dim = (g.R + g.vpi - 1) / g.vpi;
  return g;
}

// Experiment knobs.  The product dispatch reads NO environment variable per call: the switch QUANTO_HIP_EXPERIMENT is read once,
// when the library first needs it; unless it was set to a non-zero value at that moment every knob is its default and env_int /
// env_ptr are a load and a branch.  With the switch on, the knobs are read on every call, so that one process can A/B variants
// (scripts/ab.py flips a variable between hipGraph captures; the GPU tests force the tile configurations the same way).
inline bool experiments_enabled() {
  static const bool on = [] {
    const char* e = getenv("QUANTO_HIP_EXPERIMENT");
    return e != nullptr && atoi(e) != 0;
  }();
  return on;
}
inline int env_int(const char* name, int dflt) {
  if (!experiments_enabled()) return dflt;
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
// debugging aid: a device address handed over as text (scripts/skinny_timeline.py), null when unset
inline void* env_ptr(const char* name) {
  if (!experiments_enabled()) return nullptr;
  const char* e = getenv(name);
  return e ? reinterpret_cast<void*>(strtoull(e, nullptr, 0)) : nullptr;
}

// ---- split-K workspace: [QUANTO_HIP_WS_COUNTER_BYTES of arrival counters | partial sums] (include/quanto_hip.h) ----------------
// one counter per tile (feature block) that a workgroup split counts its arrivals on: more tiles than the region holds run unsplit
inline bool ws_counters_fit(int64_t tiles) { return (size_t)tiles * 4 <= QUANTO_HIP_WS_COUNTER_BYTES; }
// the partial sums start behind the counter region whatever the problem, so no call reads an earlier call's partials as counters
inline float* ws_partials(void* workspace) { return reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(workspace) + QUANTO_HIP_WS_COUNTER_BYTES); }
// whether the caller's workspace can hold a split that needs `need` bytes (16-byte stores); a kernel without one runs unsplit
inline bool ws_holds(const void* workspace, size_t workspace_bytes, size_t need) {
  return workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 16 == 0;
}

// ---- launch grids: a kernel that puts a tile count in grid.y / grid.z takes at most this many (hipDeviceProp_t::maxGridSize[1] and [2]
// are 65536 on gfx950; the convolutions' rules always used 65535).  A support rule bounds its tile count with it, so that AUTO steps down
// to another kernel instead of reaching a launch that cannot succeed (tests/test_size_limits_cpu.py).
constexpr int64_t kMaxGridYZ = 65535;
inline bool grid_yz_fits(int64_t items, int64_t tile) { return (items + tile - 1) / tile <= kMaxGridYZ; }

// ---- several Linears that share their input in one launch (q/k/v, gate/up): host side of the streaming kernels' segment tables ----------------
// What the caller handed over, per Linear; the plain op is nseg = 1.  `shift` stays null for the 8-bit products.  `align` ors x and every weight
// pointer: the streaming kernels want all of them 16-byte aligned.
struct Linears {
  int nseg;
  const void* w[QUANTO_HIP_MAX_MULTI];
  const void* scale[QUANTO_HIP_MAX_MULTI];
  const void* shift[QUANTO_HIP_MAX_MULTI];
  const void* bias[QUANTO_HIP_MAX_MULTI];
  void* y[QUANTO_HIP_MAX_MULTI];
  int N[QUANTO_HIP_MAX_MULTI];
  uintptr_t align;
};
// 1 <= nseg <= QUANTO_HIP_MAX_MULTI is the caller's check; `shift` / `bias` may be null arrays.  The plain op passes the addresses of its arguments.
inline Linears gather_linears(const void* x, int nseg, const void* const* w, const void* const* scale, const void* const* shift, const void* const* bias,
                              void* const* y, const int64_t* N) {
  Linears l{};
  l.nseg = nseg;
  l.align = reinterpret_cast<uintptr_t>(x);
  for (int i = 0; i < nseg; ++i) {
    l.w[i] = w[i];
    l.scale[i] = scale[i];
    l.shift[i] = shift ? shift[i] : nullptr;
    l.bias[i] = bias ? bias[i] : nullptr;
    l.y[i] = y[i];
    l.N[i] = (int)N[i];
    l.align |= reinterpret_cast<uintptr_t>(w[i]);
  }
  return l;
}
// The one fill of the four segment tables (GemvSegs, GemvSegs8, skinny::Segs, skinny8::Segs: kernel arguments whose members differ in name and type,
// hence `put(slot, linear)`, which copies one Linear's pointers and N).  Slot i < nseg holds Linear i and first[i] its first workgroup, with
// `blocks(i)` workgroups per Linear; the unused slots repeat Linear 0 and are never selected: first = INT_MAX.  Returns the workgroups of all Linears.
template <class Put, class Blocks>
inline int fill_segments(int nseg, int (&first)[QUANTO_HIP_MAX_MULTI], Put put, Blocks blocks) {
  int total = 0;
  for (int i = 0; i < QUANTO_HIP_MAX_MULTI; ++i) {
    put(i, i < nseg ? i : 0);
    first[i] = i < nseg ? total : 0x7FFFFFFF;
    if (i < nseg) total += blocks(i);
  }
  return total;
}

}  // namespace qh

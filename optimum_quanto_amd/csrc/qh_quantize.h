// The per-element rule of quanto::quantize_symmetric (library/quantize.py:26-55), one copy for quantize.hip and for the product epilogues that store
// output codes (epilogue_code below: qh_group_fused.h, qconv_a8.hip, qmm_native8.hip): code = cast(clamp(round?(T(x / scale)))).
//
// Bit-exactness with the torch sequence: the quotient is an fp32 divide, correctly rounded (no reciprocal multiply), rounded to the tensor dtype T -
// what aten's div does through its opmath type; integer targets are then rounded half-to-even in T (exact: |q| <= 256 after the clamp matters only)
// and clamped to [-128, 127]; float8 targets are clamped to the finite range and converted by the hardware's round-to-nearest-even OCP converters.
#pragma once
#include "qh_common.h"

namespace qh {

template <int ODT>
__device__ __forceinline__ float clamp_target(float q) {
  if constexpr (ODT == QUANTO_HIP_I8) {
    q = __builtin_rintf(q);
    return __builtin_fminf(__builtin_fmaxf(q, -128.f), 127.f);
  } else if constexpr (ODT == QUANTO_HIP_F8_E4M3FN) {
    return __builtin_fminf(__builtin_fmaxf(q, -448.f), 448.f);
  } else {
    return __builtin_fminf(__builtin_fmaxf(q, -57344.f), 57344.f);
  }
}

template <int ODT>
__device__ __forceinline__ uint32_t pack4(const float* q) {
  if constexpr (ODT == QUANTO_HIP_I8) {
    return ((uint32_t)(int)q[0] & 0xFFu) | (((uint32_t)(int)q[1] & 0xFFu) << 8) | (((uint32_t)(int)q[2] & 0xFFu) << 16) |
           (((uint32_t)(int)q[3] & 0xFFu) << 24);
  } else if constexpr (ODT == QUANTO_HIP_F8_E4M3FN) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w, true);
  } else {
    int w = __builtin_amdgcn_cvt_pk_bf8_f32(q[0], q[1], 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(q[2], q[3], w, true);
  }
}

// x / s rounded to the tensor dtype IDT, as fp32: the value the clamp sees
template <int IDT>
__device__ __forceinline__ float quotient_in(float x, float s) {
  using E = Elem<IDT>;
  return E::to_f32(E::from_f32(x / s));
}

// The output code of a product epilogue, before pack4: the element the float epilogue would store (qh_common.h: scale_round_add_round), then the rule
// above on it at the output scale os.  DT: the tensor dtype T of the product; ODT: the code type.  The QOUT epilogues are pinned bit for bit against the
// two-kernel sequence.
template <int DT, int ODT>
__device__ __forceinline__ float epilogue_code(float acc, float scale, bool has_bias, float bias, float os) {
  return clamp_target<ODT>(quotient_in<DT>(Elem<DT>::to_f32(scale_round_add_round<DT>(acc, scale, has_bias, bias)), os));
}

}  // namespace qh

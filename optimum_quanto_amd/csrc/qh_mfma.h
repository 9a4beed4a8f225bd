// Building blocks shared by the MFMA kernels: the 16x16x32 bf16 / fp16 MFMA trait, LDS-DMA issue, the vmcnt ladder and the 8-bit
// pair converter.
#pragma once
#include "qh_common.h"

namespace qh {

// ---- v_mfma_f32_16x16x32_{bf16,f16} and the constants of the 128+q / 1024+q int4 operands --------------------------------
// MAGIC | q is exactly OFFSET + q in the 16-bit type (two per dword); ONE2 is (1.0, 1.0), the all-ones operand of the group sums.
template <int DT>
struct Mma;
template <>
struct Mma<QUANTO_HIP_BF16> {
  using V8 = bf16x8;
  static __device__ __forceinline__ f32x4 run(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
  static constexpr uint32_t MAGIC = 0x43004300u, ONE2 = 0x3F803F80u;
  static constexpr float OFFSET = 128.f;
};
template <>
struct Mma<QUANTO_HIP_F16> {
  using V8 = f16x8;
  static __device__ __forceinline__ f32x4 run(V8 a, V8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
  static constexpr uint32_t MAGIC = 0x64006400u, ONE2 = 0x3C003C00u;
  static constexpr float OFFSET = 1024.f;
};

// two floats that are EXACT in the 16-bit type (int8 / fp8 codes) -> one dword with one instruction (v_cvt_pk_bf16_f32 / v_cvt_pkrtz_f16_f32).
// The fp16 form rounds toward zero: not for values that need rounding (qbits_mfma_large.hip has its own round-to-nearest pack).
template <int DT>
__device__ __forceinline__ uint32_t pack_exact(float a, float b) {
  if constexpr (DT == QUANTO_HIP_BF16) {
    bf16x2 r;
    r.x = (__bf16)a;
    r.y = (__bf16)b;
    return __builtin_bit_cast(uint32_t, r);
  } else {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
  }
}

// ---- LDS-DMA, 16 bytes per lane (inline asm: through the builtin hipcc puts a vmcnt(0) in front of every ds_read that follows) ----
// M0 is written and not restored: on gfx9+ the compiler only needs M0 for constructs these kernels do not contain (movrel, GWS,
// sendmsg, its own LDS-DMA builtins), and two SALU instructions per piece matter in a one-wave-per-SIMD instruction stream where
// every issue slot next to an MFMA is accounted for.
#ifndef QH_GLDS_POLICY
#define QH_GLDS_POLICY ""  // cache policy bits of the operand DMA (probes: " sc1", " nt", " sc0 sc1": profiles/r06_glds_cache_policy_ab.jsonl)
#endif
// wave-uniform 64-bit base in SGPRs + per-lane 32-bit byte offset
__device__ __forceinline__ void glds16(const void* sbase, uint32_t voff, uint32_t lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, %1" QH_GLDS_POLICY
      :
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}
// per-lane flat address
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, off"
      :
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}
// non-temporal flavour for a weight stream read once per pass (MI355X_MICROARCH.md "nt-weights": issued -> landed 18 % sooner on
// one-shot streams)
__device__ __forceinline__ void glds16_nt(const void* gsrc, uint32_t lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %0, off nt"
      :
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}

// s_waitcnt vmcnt(n * PER) for n = 0 .. MAXN / PER: the immediate must be a literal, hence the ladder
template <int MAXN, int PER>
__device__ __forceinline__ void wait_vmcnt(int younger_tiles) {
  if constexpr (MAXN > 0) {
    if (younger_tiles * PER >= MAXN) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MAXN) : "memory");
      return;
    }
    wait_vmcnt<MAXN - PER, PER>(younger_tiles);
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// ---- 8-bit weight codes -> 16-bit MFMA operands (qbytes_skinny.hip, qmm_mfma_large.hip) ------------------------------------
// The format is a template argument of the kernels: these numbers are part of their names.
namespace w8 {

enum { W_I8 = 0, W_F8E4M3 = 1, W_F8E5M2 = 2, W_DENSE = 3, W_F8E4M3FNUZ = 4 };  // W_DENSE: weights already in the activation dtype (qmm_mfma_large.hip's weights-direct loop only; no convert_pair)

// bytes (2p, 2p+1) of `word` -> two 16-bit elements.  int8: 3 VALU ops (2 x v_cvt_f32_i32 with SDWA byte select + one packed
// conversion).  fp8 / bf8: ONE op - gfx950's v_cvt_scalef32_pk_{bf16,f16}_{fp8,bf8} converts a pair straight to the 16-bit type
// (scale 1.0: exact, every e4m3 / e5m2 value is representable in bf16 and fp16) instead of cvt_pk_f32_fp8 + a packed narrowing.
template <int DT, int FMT>
__device__ __forceinline__ uint32_t convert_pair(uint32_t word, int p) {
  if constexpr (FMT == W_I8) {
    const float f0 = p == 0 ? (float)(int8_t)(word & 0xFFu) : (float)(int8_t)((word >> 16) & 0xFFu);
    const float f1 = p == 0 ? (float)(int8_t)((word >> 8) & 0xFFu) : (float)(int8_t)(word >> 24);
    return pack_exact<DT>(f0, f1);
  } else if constexpr (FMT == W_F8E4M3FNUZ) {
    return DT == QUANTO_HIP_BF16 ? fnuz_pair_bf16(word, p) : fnuz_pair_f16(word, p);  // qh_common.h: fn / 2 + three patched patterns
  } else if constexpr (FMT == W_F8E4M3) {
    if constexpr (DT == QUANTO_HIP_BF16)
      return __builtin_bit_cast(uint32_t, p == 0 ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)word, 1.0f, false)
                                                 : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)word, 1.0f, true));
    else
      return __builtin_bit_cast(uint32_t, p == 0 ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)word, 1.0f, false)
                                                 : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)word, 1.0f, true));
  } else {
    static_assert(FMT == W_F8E5M2, "convert_pair: 8-bit formats only");
    if constexpr (DT == QUANTO_HIP_BF16)
      return __builtin_bit_cast(uint32_t, p == 0 ? __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8((int)word, 1.0f, false)
                                                 : __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8((int)word, 1.0f, true));
    else
      return __builtin_bit_cast(uint32_t, p == 0 ? __builtin_amdgcn_cvt_scalef32_pk_f16_bf8((int)word, 1.0f, false)
                                                 : __builtin_amdgcn_cvt_scalef32_pk_f16_bf8((int)word, 1.0f, true));
  }
}

}  // namespace w8

}  // namespace qh

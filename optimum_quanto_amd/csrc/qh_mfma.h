// Building blocks shared by the MFMA kernels: the 16x16x32 bf16 / fp16 MFMA trait, LDS-DMA issue, the vmcnt ladder, the split-K
// tail, the 16-bit packers and the 8-bit format codes with their converters to 16-bit operands.
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
// The fp16 form rounds toward zero: not for values that need rounding (pack_rne below).
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
// two fp32 -> one dword of the 16-bit type, round to nearest even: dequantized sub-byte weights (qbits_mfma_large.hip; qconv_mfma.hip has
// conv::pack_rne in another wording - the register counts that keep the two apart are recorded there)
template <int DT>
__device__ __forceinline__ uint32_t pack_rne(float a, float b) {
  if constexpr (DT == QUANTO_HIP_BF16) {
    bf16x2 r;
    r.x = (__bf16)a;
    r.y = (__bf16)b;
    return __builtin_bit_cast(uint32_t, r);
  } else {
    f16x2 r;
    r.x = (_Float16)a;
    r.y = (_Float16)b;
    return __builtin_bit_cast(uint32_t, r);
  }
}

// ---- an operand tile staged through registers into LDS (qmm_mfma.hip, qconv_mfma.hip, qconv_a8.hip) --------------------------------
// 128-byte rows (one K-tile of a row) of eight 16-byte chunks; chunk kc of row r sits at position kc ^ (r & 7): the fragment reads (16 rows x 4
// chunks) and the staging writes are conflict-free
constexpr int kTileRowBytes = 128;
__device__ __forceinline__ int tile_lds_off(int row, int kc) { return row * kTileRowBytes + ((kc ^ (row & 7)) << 4); }

// ---- LDS-DMA, 16 bytes per lane (inline asm: through the builtin hipcc puts a vmcnt(0) in front of every ds_read that follows) ----
// M0 is written and not restored: on gfx9+ the compiler only needs M0 for constructs these kernels do not contain (movrel, GWS,
// sendmsg, its own LDS-DMA builtins), and two SALU instructions per piece matter in a one-wave-per-SIMD instruction stream where
// every issue slot next to an MFMA is accounted for.
#ifndef QH_GLDS_POLICY
#define QH_GLDS_POLICY ""  // cache policy bits of the operand DMA (probes: " sc1", " nt", " sc0 sc1": profiles/r06_glds_cache_policy_ab.jsonl)
#endif
typedef __attribute__((address_space(3))) void* lds_ptr_t;  // (uint32_t)(uintptr_t)(lds_ptr_t)smem: the LDS byte address glds16 takes
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

// ---- split-K tail: the last workgroup of a tile to arrive adds the partial sums of all S splits ------------------------------
// Used by qbits_skinny.hip, qbytes_skinny.hip, qbits_mfma_fused.hip, qbits_a8_fused.hip and qmm_mfma_large.hip:
//   QH_SPLITK_ARRIVE(...);                   park the partial, count the arrival in the LDS word *flag
//   if (*flag != S - 1) return;              every workgroup but the tile's last arriver is done
//   QH_SPLITK_SUM(...);                      reset the counter, acc = the S partials added in split order
// Workspace (include/quanto_hip.h): one arrival counter per tile, zero on entry and reset by the last arriver; the partial of split sp of
// tile t is slot t * S + sp: NF fragments x NT threads of float4, fragment-major (every store / load instruction covers whole lines:
// partial lines are what the write-through path is slow at).
// Coherence: the workgroups of one tile may run on different XCDs, whose L2s are not coherent with each other.  An agent-scope fence
// would be correct but writes back / invalidates a whole L2 (measured: 23 -> 57 us); instead the few KiB of partials travel with
// system-coherent (sc0 sc1) 16-byte stores and loads, and the only ordering needed is "my stores are acknowledged (vmcnt(0)) before
// my workgroup's arrival is counted".
// Macros, not functions: hipcc optimizes a called function on its own before it inlines it, and the tail as two __forceinline__
// templates changed the loops and the registers of every kernel that used it (qbits_skinny 134 -> 132 VGPRs, the convolution reduce
// 132 -> 110); pasted in place, each kernel compiles to the same instructions as with its own copy.
//
// PARTIALS: float* behind the counters; SLOT: this workgroup's slot; ACC: the accumulator as f32x4*; COUNTER: int* of the tile's counter;
// FLAG: int* into LDS; ACKED / COUNTED: statements run once the stores are acknowledged / the arrival is counted (qbits_skinny.hip's
// timeline probes).  s_nop: gfx9 hazard "VMEM store of > 64 bits, then VALU write of its data VGPRs" - hipcc cannot see into the asm.
#define QH_SPLITK_ARRIVE(NF, NT, PARTIALS, SLOT, ACC, COUNTER, FLAG, TID, ACKED, COUNTED)                                           \
  {                                                                                                                           \
    float* const qh_mine = (PARTIALS) + ((size_t)(SLOT) * (NF) * (NT) + (TID)) * 4;                                              \
    _Pragma("unroll") for (int qh_f = 0; qh_f < (NF); ++qh_f) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1"   \
                                                                           ::"v"(qh_mine + qh_f * ((NT) * 4)), "v"((ACC)[qh_f])   \
                                                                           : "memory");                                          \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                             \
    ACKED;                                                                                                                       \
    __syncthreads();                                                                                                             \
    if ((TID) == 0) *(FLAG) = __hip_atomic_fetch_add((COUNTER), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);                 \
    __syncthreads();                                                                                                             \
    COUNTED;                                                                                                                     \
  }
// In the last arriver, after RESET (a statement run once the counter is reset: qmm_mfma_large.hip's barrier before it reuses the flag
// word): QB splits x FB fragments of loads in flight per wait (a system-coherent load is a ~2 us round trip: one per split
// made the tail ~12 of the 21.7 us of a (128,4096,4096) fused int4 call with four splits); a batch past the last split re-loads it and
// drops it.  Adding in split order makes the result independent of which workgroup arrived last.
#define QH_SPLITK_SUM(NF, NT, QB, FB, PARTIALS, TILE, S, ACC, COUNTER, TID, RESET)                                                  \
  {                                                                                                                              \
    if ((TID) == 0) __hip_atomic_store((COUNTER), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); /* leave the workspace as found */ \
    RESET;                                                                                                                       \
    _Pragma("unroll") for (int qh_f = 0; qh_f < (NF); ++qh_f)(ACC)[qh_f] = f32x4{0.f, 0.f, 0.f, 0.f};                           \
    for (int qh_q0 = 0; qh_q0 < (S); qh_q0 += (QB)) {                                                                            \
      if constexpr ((FB) == (NF)) {                                                                                              \
        QH_SPLITK_BATCH_(NF, NT, QB, FB, 0, PARTIALS, TILE, S, ACC, TID);                                                        \
      } else {                                                                                                                   \
        _Pragma("unroll") for (int qh_f0 = 0; qh_f0 < (NF); qh_f0 += (FB)) QH_SPLITK_BATCH_(NF, NT, QB, FB, qh_f0, PARTIALS, TILE, S, ACC, TID); \
      }                                                                                                                          \
    }                                                                                                                            \
  }
// fragments F0 .. F0 + FB - 1 of splits qh_q0 .. qh_q0 + QB - 1
#define QH_SPLITK_BATCH_(NF, NT, QB, FB, F0, PARTIALS, TILE, S, ACC, TID)                                                            \
  {                                                                                                                              \
    f32x4 qh_v[QB][FB];                                                                                                          \
    _Pragma("unroll") for (int qh_j = 0; qh_j < (QB); ++qh_j) {                                                                  \
      const int qh_q = qh_q0 + qh_j < (S) ? qh_q0 + qh_j : (S) - 1;                                                              \
      const float* const qh_theirs = (PARTIALS) + ((size_t)((TILE) * (S) + qh_q) * (NF) * (NT) + (TID)) * 4;                     \
      _Pragma("unroll") for (int qh_e = 0; qh_e < (FB); ++qh_e) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1"           \
                                                                              : "=v"(qh_v[qh_j][qh_e])                           \
                                                                              : "v"(qh_theirs + ((F0) + qh_e) * ((NT) * 4))      \
                                                                              : "memory");                                       \
    }                                                                                                                            \
    /* the waits tie the uses below to the loads */                                                                              \
    _Pragma("unroll") for (int qh_j = 0; qh_j < (QB); ++qh_j) _Pragma("unroll") for (int qh_e = 0; qh_e < (FB); ++qh_e)          \
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(qh_v[qh_j][qh_e])::"memory");                                                     \
    _Pragma("unroll") for (int qh_j = 0; qh_j < (QB); ++qh_j) if (qh_q0 + qh_j < (S)) {                                          \
      _Pragma("unroll") for (int qh_e = 0; qh_e < (FB); ++qh_e) _Pragma("unroll") for (int qh_r = 0; qh_r < 4; ++qh_r)           \
        (ACC)[(F0) + qh_e][qh_r] += qh_v[qh_j][qh_e][qh_r];                                                                      \
    }                                                                                                                            \
  }

// ---- 8-bit weight codes -> 16-bit MFMA operands (qbytes_skinny.hip, qmm_mfma_large.hip, qmm_mfma.hip, qconv_mfma.hip) ----------
// The format is a template argument of the kernels: these numbers are part of their names.  A unit's own enum continues them with the formats
// only it has (qmm_mfma.hip: W_I4; qconv_mfma.hip: W_I4R ..).
namespace w8 {

enum { W_I8 = 0, W_F8E4M3 = 1, W_F8E5M2 = 2, W_DENSE = 3, W_F8E4M3FNUZ = 4 };  // W_DENSE: weights already in the activation dtype (qmm_mfma_large.hip's weights-direct loop only; no convert_pair)
// the QUANTO_HIP_* code of a format's bytes, which the byte decoders of qh_common.h take
constexpr int byte_dtype(int fmt) {
  return fmt == W_I8 ? QUANTO_HIP_I8 : fmt == W_F8E4M3 ? QUANTO_HIP_F8_E4M3FN : fmt == W_F8E4M3FNUZ ? QUANTO_HIP_F8_E4M3FNUZ : QUANTO_HIP_F8_E5M2;
}

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

// 16 one-byte weights -> 16 elements of the activation dtype, two 16-byte LDS chunks (qmm_mfma.hip, qconv_mfma.hip): through fp32
// (qh_common.h: dword_f32), every int8 / fp8 value is exact in bf16 and fp16
template <int DT, int FMT>
__device__ __forceinline__ void convert16(const uint4& w, uint4& c0, uint4& c1) {
  static_assert(FMT == W_I8 || FMT == W_F8E4M3 || FMT == W_F8E5M2, "convert16: int8, e4m3fn, e5m2");
  const uint32_t in[4] = {w.x, w.y, w.z, w.w};
  uint32_t out[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    float f[4];
    dword_f32<byte_dtype(FMT)>(in[d], f);
    out[2 * d] = pack_exact<DT>(f[0], f[1]);
    out[2 * d + 1] = pack_exact<DT>(f[2], f[3]);
  }
  c0 = make_uint4(out[0], out[1], out[2], out[3]);
  c1 = make_uint4(out[4], out[5], out[6], out[7]);
}

}  // namespace w8

}  // namespace qh

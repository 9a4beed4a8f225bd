// The internal interface between c_api.hip and the kernel units: what a call carries (the *Call structs, field names = the ABI's own) and the
// declaration of every function c_api.hip calls in a unit, once, with names.  Every unit includes this header, so a definition that drifts from its
// declaration is a compile error in that unit instead of a link error (or a silently different overload).  Host code only.
#pragma once
#include "qh_common.h"

namespace qh {

int launch_status();  // hipGetLastError() -> quanto_hip_status (defined in c_api.hip)
void set_last_kernel(const char* name);

// ---- what a call carries ------------------------------------------------------------------------------------------------------------------------
// qbits_mm: y[M, N] = x[M, K] @ dequantize(packed, scale, shift)^T + bias.  a_scale / a_dtype / out_scale: qbits_mm_a8 only (x = the activation
// codes; out_scale != nullptr: y = a_dtype codes at out_scale[0]).
struct QbitsCall {
  const void *x, *a_scale;
  const uint8_t* packed;
  const void *scale, *shift, *bias, *out_scale;
  void* y;
  int64_t M;
  PackedGeom g;
  int a_dtype, dtype;
  bool int_shift;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t stream;
};
// `count` int4 g128 Linears with the same K applied to the same x
struct QbitsMultiCall {
  const void* x;
  int count;
  const uint8_t* const* packed;
  const void *const *scale, *const *shift, *const *bias;
  void* const* y;
  const int64_t* N;
  int64_t M, K;
  int dtype;
  bool int_shift;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t stream;
};

// qbytes_mm: the problem the *_supported / *_workspace rules of the 8-bit product look at ...
struct QbytesShape {
  int64_t M, N, K;
  int a_dtype, b_dtype, out_dtype;
};
// ... and the call: y[M, N] = (a[M, K] @ b[N, K]^T) * scales[N] + bias.  out_scale != nullptr (native8 only): y = a_dtype codes at out_scale[0].
struct QbytesCall : QbytesShape {
  const void *a, *b, *scales, *bias, *out_scale;
  void* y;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t stream;
};
struct QbytesMultiCall {
  const void* a;
  int count;
  const void *const *b, *const *scales, *const *bias;
  void* const* y;
  const int64_t* N;
  int64_t M, K;
  int a_dtype, b_dtype, out_dtype;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t stream;
};

// One conv2d call: x [B, cin, H, W], weight [OC, cin (depthwise: 1), KH, KW], y [B, OC, OH, OW]; filled once per C entry, behind check_conv2d_args.
struct ConvGeom {
  int64_t B, cin, H, W, OC, KH, KW, OH, OW;
  int sh, sw, ph, pw, dh, dw;
  int64_t M() const { return B * OH * OW; }    // GEMM rows: output pixels
  int64_t K() const { return cin * KH * KW; }  // GEMM depth, in the weight's (c, i, j) order
};
// a_scale / out_scale: the a8 product; shift / wg / int_shift: int4 / int2 weights (w = the packed bytes, wg their geometry, out_dtype the float dtype)
struct ConvCall {
  const void *x, *a_scale, *w, *scale, *shift, *bias, *out_scale;
  void* y;
  ConvGeom g;
  PackedGeom wg;
  int a_dtype, b_dtype, out_dtype;
  bool int_shift;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t stream;
};

// ---- unpack.hip -----------------------------------------------------------------------------------------------------------------------------------
int unpack_dispatch(const uint8_t* packed, uint8_t* unpacked, int64_t packed_numel, int bits, hipStream_t stream);
int dequantize_qbits_dispatch(const uint8_t* packed, const void* scale, const void* shift, void* out, const PackedGeom& g, int dtype, bool int_shift,
                              hipStream_t stream);
// ---- quantize.hip ---------------------------------------------------------------------------------------------------------------------------------
int quantize_symmetric(const void* x, const void* scale, void* out, int64_t numel, int64_t inner, int scale_mode, int in_dtype, int out_dtype,
                       hipStream_t stream);
int dequantize_symmetric(const void* q, const void* scale, void* out, int64_t numel, int q_dtype, int out_dtype, hipStream_t stream);
int quantize_affine(const void* x, const void* scale, const void* shift, void* out, int64_t numel, int64_t C, int bits, int dtype, bool int_shift,
                    hipStream_t stream);
int quantize_affine_packed(const void* x, const void* scale, const void* shift, void* out, int64_t rows, int64_t C, int bits, int dtype, bool int_shift,
                           hipStream_t stream);
int pack_weights(const uint8_t* unpacked, uint8_t* packed, int64_t rows, int64_t cols, int bits, hipStream_t stream);

// ---- the two matmul products: what a route (a row of c_api.hip's tables) is made of, then every route by unit ------------------------------------
using QbitsRule = bool(int64_t M, const PackedGeom& g, int dtype);         // "<route>_supported"
using QbitsWorkspace = size_t(int64_t M, const PackedGeom& g, int dtype);  // "<route>_workspace": bytes, for a problem the rule serves
using QbitsLaunch = int(const QbitsCall& c);
using QbytesRule = bool(const QbytesShape& s);
using QbytesWorkspace = size_t(const QbytesShape& s);
using QbytesLaunch = int(const QbytesCall& c);
// naive_mm.hip
QbitsLaunch qbits_mm_naive;
QbytesLaunch qbytes_mm_naive;
// qbits_gemv.hip, qbytes_gemv.hip
QbitsRule qbits_gemv_supported;
QbitsLaunch qbits_mm_gemv;
int qbits_mm_gemv_multi(const QbitsMultiCall& c);
QbytesRule qbytes_gemv_supported;
QbytesLaunch qbytes_mm_gemv;
int qbytes_mm_gemv_multi(const QbytesMultiCall& c);
// qbits_mmv.hip
QbitsRule qbits_mmv_supported;
QbitsLaunch qbits_mm_mmv;
// qbits_skinny.hip, qbytes_skinny.hip
QbitsRule qbits_skinny_supported;
QbitsWorkspace qbits_skinny_workspace;
QbitsLaunch qbits_mm_skinny;
bool qbits_skinny_multi_supported(int count, const int64_t* N, int64_t M, int64_t K, int dtype);
size_t qbits_skinny_multi_workspace(int count, const int64_t* N, int64_t M, int64_t K);
int qbits_mm_skinny_multi(const QbitsMultiCall& c);
QbytesRule qbytes_skinny_supported;
QbytesWorkspace qbytes_skinny_workspace;
QbytesLaunch qbytes_mm_skinny;
bool qbytes_skinny_multi_supported(int count, const int64_t* N, int64_t M, int64_t K, int a_dtype, int b_dtype, int out_dtype);
size_t qbytes_skinny_multi_workspace(int count, const int64_t* N, int64_t M, int64_t K);
int qbytes_mm_skinny_multi(const QbytesMultiCall& c);
// qmm_mfma.hip
QbitsRule qbits_mfma_supported;
QbitsWorkspace qbits_mfma_workspace;
QbitsLaunch qbits_mm_mfma;
QbytesRule qbytes_mfma_supported;
QbytesLaunch qbytes_mm_mfma;
// qbits_mfma_fused.hip
QbitsRule qbits_mfma_fused_supported;
QbitsWorkspace qbits_mfma_fused_workspace;
QbitsLaunch qbits_mm_mfma_fused;
float qbits_mfma_fused_cost(int64_t M, const PackedGeom& g);
bool qbits_mfma_fused_needs_workspace(const PackedGeom& g);
// qbits_mfma_large.hip
QbitsRule qbits_mfma_large_supported;
QbitsLaunch qbits_mm_mfma_large;
// qmm_f32.hip: fp32 activations
QbitsRule qbits_gemv_f32_supported, qbits_mm_f32_supported;
QbitsLaunch qbits_mm_gemv_f32, qbits_mm_f32;
QbytesRule qbytes_gemv_f32_supported, qbytes_mm_f32_supported;
QbytesLaunch qbytes_mm_gemv_f32, qbytes_mm_f32;
// qbits_a8_fused.hip: quantized activations x int4 / int2 weights
bool qbits_a8_supported(int64_t M, const PackedGeom& g, int a_dtype, int dtype);
size_t qbits_a8_workspace(int64_t M, const PackedGeom& g);
QbitsLaunch qbits_mm_a8;
// qmm_mfma_large.hip, qmm_native8.hip (each also a dense 16-bit GEMM: the second half of dequantize + dense)
QbytesRule qbytes_mfma_large_supported, qbytes_native8_supported;
QbytesWorkspace qbytes_mfma_large_workspace, qbytes_native8_workspace;
QbytesLaunch qbytes_mm_mfma_large, qbytes_mm_native8;
bool dense_mm_wd_supported(int64_t M, int64_t N, int64_t K, int dtype);
int dense_mm_wd(const void* x, const void* w, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int dtype, hipStream_t stream);
bool dense_mm_large_supported(int64_t M, int64_t N, int64_t K, int dtype);
int dense_mm_large(const void* x, const void* w, const void* bias, void* y, int64_t M, int64_t N, int64_t K, int dtype, hipStream_t stream);

// ---- convolutions ---------------------------------------------------------------------------------------------------------------------------------
// qconv_mfma.hip
size_t conv2d_workspace(int64_t M, int64_t N, int64_t K);
size_t conv2d_dense_weight_bytes(int64_t N, int64_t K);
bool conv2d_rows_eligible(const ConvGeom& g);
int qdense_conv2d_rows(const ConvCall& c);                // w: the dense 16-bit weight, out_dtype its dtype
int qbytes_conv2d_mfma(const ConvCall& c, bool* rows);    // *rows: whether the row form ran
int qbits_conv2d_mfma(const ConvCall& c);
// qconv_a8.hip
int qbytes_conv2d_a8_kind(int a_dtype, int b_dtype, int out_dtype);
size_t conv2d_a8_workspace(int64_t M, int64_t N, int64_t K);
int qbytes_conv2d_a8(const ConvCall& c, int* kind);       // *kind: the conv8::Kind that ran
// qconv_depthwise.hip
int qbytes_conv2d_depthwise(const ConvCall& c, bool* strip);  // *strip: whether the strip form ran

}  // namespace qh

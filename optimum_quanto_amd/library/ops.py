"""The ``quanto::`` operator library for this backend.

Schemas kept verbatim from the reference so existing call sites work unchanged:

* ``quanto::unpack(Tensor self, int bits) -> Tensor``                          library/unpack.py:18
* ``quanto::qbytes_mm(Tensor A, Tensor B, Tensor scales) -> Tensor``            library/qbytes_mm.py:22
* ``quanto::quantize_symmetric(Tensor base, ScalarType dtype, int? axis, Tensor scale) -> Tensor``   library/quantize.py:22-24
* ``quanto::quantize_affine(Tensor base, int bits, int axis, int? group_size, Tensor scale, Tensor shift) -> Tensor``  :58-61

New ops (the reference has no fused int4 product outside its CUDA-only AWQ/Marlin ops; the schema follows its own
template, library/extensions/README.md:24-48 and cuda/__init__.py:82-94):

* ``quanto::qbits_mm(Tensor input, Tensor packed, Tensor scale, Tensor shift, Tensor? bias, int bits, int? group_size,
  int out_features, int in_features) -> Tensor``
* ``quanto::dequantize_qbits(Tensor packed, Tensor scale, Tensor shift, int bits, int? group_size, int out_features,
  int in_features) -> Tensor``

Dispatch: the ``default`` implementations are plain torch and serve CPU tensors (quantize-time work and the CPU
plumbing config).  The ``CUDA`` key - which is what a ROCm device uses - always goes to ``libquanto_hip.so``;
if the library cannot be loaded the call raises: there is no silent fallback for device tensors.

When ``optimum.quanto`` itself is already imported in the process the ops exist; we then only (re)register the
``CUDA`` implementations, which is how this backend plugs into an unmodified reference install.
"""
from typing import Optional, Union

import os

import torch

from ..tensor.dtypes import dtype_info
from ..tensor.grouping import group, ungroup
from . import hip
from .hip import quanto_hip

__all__ = []

_lib_def = torch.library.Library("quanto", "FRAGMENT")
_lib_impl = torch.library.Library("quanto", "IMPL")


def _op_exists(name: str) -> bool:
    try:
        return hasattr(torch.ops.quanto, name) and getattr(torch.ops.quanto, name) is not None
    except (AttributeError, RuntimeError):
        return False


# the reference's own ops: when it defined them already, their CUDA implementation is replaced by ours (plug-in mode)
_REFERENCE_OPS = ("unpack", "qbytes_mm", "quantize_symmetric", "quantize_affine")


def _register(name: str, schema: str, cuda, default=None, cpu=None):
    """Define ``quanto::name`` with its ``default`` (CompositeExplicitAutograd), ``cpu`` and ``cuda`` implementations, unless another definer
    (the reference package) already did: then only a reference op gets ``cuda`` registered, over the reference's own."""
    if not _op_exists(name):
        _lib_def.define(name + schema)
        for key, fn in (("CompositeExplicitAutograd", default), ("CPU", cpu), ("CUDA", cuda)):
            if fn is not None:
                _lib_impl.impl(name, fn, key)
    elif name in _REFERENCE_OPS:
        import warnings

        with warnings.catch_warnings():  # intended: silence torch's override notice
            warnings.simplefilter("ignore")
            try:
                _lib_impl.impl(name, cuda, "CUDA", allow_override=True)
            except TypeError:  # older torch without allow_override
                _lib_impl.impl(name, cuda, "CUDA")


# ------------------------------------------------------------------------------------------------
# quanto::unpack
# ------------------------------------------------------------------------------------------------
def unpack_default(packed: torch.Tensor, bits: int) -> torch.Tensor:
    """Planes of ``bits`` bits, concatenated along dim 0 (library/unpack.py:21-54)."""
    planes = [(packed >> (bits * i)) & ((1 << bits) - 1) for i in range(8 // bits)]
    return torch.cat(planes).to(torch.uint8)


def unpack_hip(packed: torch.Tensor, bits: int) -> torch.Tensor:
    return quanto_hip.lib.unpack(packed, bits)


_register("unpack", "(Tensor self, int bits) -> Tensor", unpack_hip, default=unpack_default)


# ------------------------------------------------------------------------------------------------
# quanto::qbytes_mm
# ------------------------------------------------------------------------------------------------
def _qbytes_mm_dense(activations, weights, output_scales):
    """Generic path (library/qbytes_mm.py:25-33): scale the weights, then a dense matmul."""
    activations = activations.to(output_scales.dtype)
    if weights.dtype.is_floating_point:
        weights = weights.to(output_scales.dtype)
    return torch.matmul(activations, (output_scales * weights).t())


def _qbytes_mm_int(activations, weights, output_scales):
    """int8 x int8 (library/qbytes_mm.py:36-50): exact int32 product, fp32 rescale."""
    k, n = activations.shape[-1], weights.shape[0]
    acc = torch._int_mm(activations.reshape(-1, k), weights.t()).reshape(activations.shape[:-1] + (n,))
    return (acc.to(torch.float32) * output_scales.t()).to(output_scales.dtype)


def qbytes_mm_default(activations, weights, output_scales):
    return _qbytes_mm_dense(activations, weights, output_scales)


def qbytes_mm_cpu(activations, weights, output_scales):
    """CPU selection logic of library/qbytes_mm.py:91-105."""
    if activations.dtype == torch.int8 and weights.dtype == torch.int8:
        return _qbytes_mm_int(activations, weights, output_scales)
    k = activations.shape[-1]
    if activations.dtype == torch.bfloat16 and weights.dtype == torch.int8 and k % 4 == 0:
        n = weights.shape[0]
        out = torch._weight_int8pack_mm(activations.reshape(-1, k), weights, output_scales.flatten())
        return out.reshape(activations.shape[:-1] + (n,))
    return _qbytes_mm_dense(activations, weights, output_scales)


def qbytes_mm_hip(activations, weights, output_scales, bias=None):
    """ROCm: one fused kernel, scales applied to the fp32 accumulator (csrc/qbytes_gemv.hip, csrc/qmm_mfma.hip)."""
    assert activations.ndim >= 1 and weights.ndim == 2
    n = weights.shape[0]
    if output_scales.numel() != n:
        # per-tensor weight scale or an exotic broadcast: expand to one scale per output feature
        output_scales = (output_scales * torch.ones((1, n), dtype=output_scales.dtype, device=output_scales.device))
        if output_scales.numel() != n:
            raise ValueError(f"qbytes_mm: cannot broadcast scales of shape {tuple(output_scales.shape)} to {n} features")
    return quanto_hip.lib.qbytes_mm(activations, weights, output_scales, bias)


def qbytes_mm_bias_default(activations, weights, output_scales, bias):
    """What tensor/weights/qbytes.py:73-81 computes: the product in the output dtype, then the bias added."""
    out = torch.ops.quanto.qbytes_mm(activations, weights, output_scales)
    return out if bias is None else out + bias


def qbytes_mm_bias_hip(activations, weights, output_scales, bias):
    return qbytes_mm_hip(activations, weights, output_scales, bias)


_register("qbytes_mm", "(Tensor A, Tensor B, Tensor scales) -> Tensor", qbytes_mm_hip, default=qbytes_mm_default, cpu=qbytes_mm_cpu)
# new op: the same product with the bias of the Linear fused into the kernel epilogue (rounded product + bias, rounded again:
# bit-identical to the two-op sequence) - saves one elementwise kernel per biased Linear
_register("qbytes_mm_bias", "(Tensor A, Tensor B, Tensor scales, Tensor? bias) -> Tensor", qbytes_mm_bias_hip, default=qbytes_mm_bias_default)


def _requantize_output(out, dtype, out_scale):
    """The second op of every ``*_q`` sequence (nn/qmodule.py:281-299): the float output re-quantized per-tensor to the activations' own 8-bit dtype."""
    return torch.ops.quanto.quantize_symmetric(out, dtype, None, out_scale.to(out.dtype).reshape(()))


# The three ``*_q`` ops below have one shape on a ROCm device: a predicate answers "this call goes to the code-storing kernel" - then the binding is
# called, which raises for what the library does not serve - otherwise the two-op sequence (``*_q_default``) runs on the existing ops: the caller
# always gets the sequence's codes.
def qbytes_mm_q_default(activations, weights, output_scales, bias, out_scale):
    """The two-op sequence of a quantized-activation layer (tensor/weights/qbytes.py:72-81, then the output hook): the product in the scales' dtype."""
    return _requantize_output(torch.ops.quanto.qbytes_mm_bias(activations, weights, output_scales, bias), activations.dtype, out_scale)


def _w8a8_codes_kernel_takes(activations, weights, output_scales, out_scale) -> int:
    """The predicate of ``qbytes_mm_q_hip``: the split-K workspace bytes (>= 0) when this call goes to the code-storing W8A8 kernel
    (csrc/qmm_native8.hip), negative otherwise.  Taken: one scale per feature of a 2-D weight, a scalar output scale, 1-byte activations, a served call
    shape (fp32 scales, mixed operand dtypes, K not a multiple of 64 and the size limits are not), and contiguous views of both operands that start on a
    16-byte boundary (a non-contiguous operand is copied by the binding and therefore aligned).  An activation that does not end in K also goes to the
    binding: for its shape error, as in the float product."""
    if not (weights.ndim == 2 and output_scales.numel() == weights.shape[0] and out_scale.numel() == 1):
        return -1
    n, k = weights.shape
    if activations.ndim == 0 or activations.shape[-1] != k:
        return 0
    if activations.dtype.itemsize != 1 or k == 0:
        return -1
    if (activations.data_ptr() | weights.data_ptr()) % 16 and (
            (activations.is_contiguous() and activations.data_ptr() % 16) or (weights.is_contiguous() and weights.data_ptr() % 16)):
        return -1
    return quanto_hip.lib.qbytes_mm_q_workspace(activations.numel() // k, n, k, activations.dtype, weights.dtype, output_scales.dtype)


def qbytes_mm_q_hip(activations, weights, output_scales, bias, out_scale):
    """ROCm: the product kernel's epilogue stores the codes (csrc/qmm_native8.hip) when the predicate says so; every other call runs the two-op sequence
    on the existing kernels - the caller always gets codes."""
    ws_bytes = _w8a8_codes_kernel_takes(activations, weights, output_scales, out_scale)
    if ws_bytes >= 0:
        return quanto_hip.lib.qbytes_mm_q(activations, weights, output_scales, bias, out_scale, _ws_bytes=ws_bytes)
    return qbytes_mm_q_default(activations, weights, output_scales, bias, out_scale)


# new op: the product of a W8A8 layer with the layer's output quantization fused into the kernel epilogue - bit-identical to
# quantize_symmetric(qbytes_mm_bias(...)), one launch and no [M, N] float tensor
_register("qbytes_mm_q", "(Tensor A, Tensor B, Tensor scales, Tensor? bias, Tensor out_scale) -> Tensor", qbytes_mm_q_hip, default=qbytes_mm_q_default)


# ------------------------------------------------------------------------------------------------
# quanto::qbytes_bmm: torch.bmm / torch.matmul on two int8 quantized activations (the q k^T and p v of an eager attention block)
# ------------------------------------------------------------------------------------------------
def qbytes_bmm_default(a, b, scale, out_dtype):
    """The two statements of the reference's aten.bmm handler (tensor/activations/qbytes_ops.py:175-186): an fp32 bmm of the casts, times the scale
    product, cast."""
    out = torch.bmm(a.to(torch.float32), b.to(torch.float32))
    return (out * scale).to(out_dtype)


def _bmm_kernel_takes(a, b, scale, out_dtype) -> bool:
    """The predicate of ``qbytes_bmm_hip``: int8 x int8, both 3-D with matching sizes, a one-element scale, a float32 / float16 / bfloat16 output,
    K <= 131071 (the int32 accumulator) and fewer than 2^31 workgroups (64 x 64 output tiles over all batch members).  No shape class is routed
    back on speed: profiles/qbmm_vs_sequence.jsonl."""
    lib = quanto_hip.lib
    if not (a.dtype == torch.int8 and b.dtype == torch.int8 and a.ndim == 3 and b.ndim == 3 and scale.numel() == 1 and out_dtype in lib.BMM_OUT_DTYPES):
        return False
    (nb, m, k), n = a.shape, b.shape[2]
    if b.shape[0] != nb or b.shape[1] != k or k > lib.BMM_MAX_K:
        return False
    return nb * (-(-m // 64) * -(-n // 64)) < (1 << 31)


def qbytes_bmm_hip(a, b, scale, out_dtype):
    """ROCm: one launch of csrc/qbytes_bmm.hip when the predicate says so; everything else runs the fp32 sequence on the device."""
    if _bmm_kernel_takes(a, b, scale, out_dtype):
        return quanto_hip.lib.qbytes_bmm(a, b, scale, out_dtype)
    return qbytes_bmm_default(a, b, scale, out_dtype)


# new op: the batched product of two int8 quantized activations on the 8-bit matrix instructions - the exact int32 sum, rounded once to fp32,
# times the scale product, rounded once to out_dtype.  For K <= 1024 every fp32 partial sum of the sequence above is an exact integer, so the kernel
# is bit-identical to it; for larger K the fp32 bmm rounds partial sums in an unspecified order and the kernel returns the correctly rounded value of
# the exact sum - the only observable difference.  On the CPU the default runs.
_register("qbytes_bmm", "(Tensor a, Tensor b, Tensor scale, ScalarType out_dtype) -> Tensor", qbytes_bmm_hip, default=qbytes_bmm_default)


def qbytes_conv2d_default(input, weight, scales, bias, stride, padding, dilation):
    """What the reference computes for F.conv2d on a WeightQBytesTensor (nn/qconv2d.py:54-55 -> qfallback): dequantize, float convolution."""
    w = scales.reshape(-1, 1, 1, 1).to(input.dtype) * weight.to(input.dtype)
    groups = input.shape[1] // weight.shape[1]  # 1, or the channel count of a depthwise layer (weight [OC, 1, KH, KW])
    return torch.nn.functional.conv2d(input, w, bias, tuple(stride), tuple(padding), tuple(dilation), groups)


def qbytes_conv2d_hip(input, weight, scales, bias, stride, padding, dilation):
    return quanto_hip.lib.qbytes_conv2d(input, weight, scales, bias, tuple(stride), tuple(padding), tuple(dilation))


# new op: dense convolution with an int8 / fp8 weight as an implicit GEMM on the device (csrc/qconv_mfma.hip): no im2col tensor
_register("qbytes_conv2d", "(Tensor input, Tensor weight, Tensor scales, Tensor? bias, int[] stride, int[] padding, int[] dilation) -> Tensor",
          qbytes_conv2d_hip, default=qbytes_conv2d_default)


def qbytes_conv2d_a8_default(input, input_scale, weight, weight_scale, bias, stride, padding, dilation):
    """What the reference computes for F.conv2d(ActivationQBytesTensor, WeightQBytesTensor) (qfallback): both dequantized, float convolution in the
    weight scale's dtype."""
    dt = weight_scale.dtype
    x = input.to(dt) * input_scale.to(dt)
    w = weight.to(dt) * weight_scale.reshape(-1, 1, 1, 1).to(dt)
    return torch.nn.functional.conv2d(x, w, None if bias is None else bias.to(dt), tuple(stride), tuple(padding), tuple(dilation), 1)


def qbytes_conv2d_a8_hip(input, input_scale, weight, weight_scale, bias, stride, padding, dilation):
    lib = quanto_hip.lib
    stride, padding, dilation = tuple(stride), tuple(padding), tuple(dilation)
    if input_scale.numel() == 1 and lib.qbytes_conv2d_a8_supported(input, weight, weight_scale.dtype, stride, padding, dilation):
        return lib.qbytes_conv2d_a8(input, input_scale, weight, weight_scale, bias, stride, padding, dilation)
    return qbytes_conv2d_a8_default(input, input_scale, weight, weight_scale, bias, stride, padding, dilation)


# new op: dense convolution of quantized activation codes with an 8-bit weight on the 8-bit matrix instructions (csrc/qconv_a8.hip): no im2col, no
# dequantized activation or weight
_register("qbytes_conv2d_a8", "(Tensor input, Tensor input_scale, Tensor weight, Tensor weight_scale, Tensor? bias, int[] stride, int[] padding, "
          "int[] dilation) -> Tensor", qbytes_conv2d_a8_hip, default=qbytes_conv2d_a8_default)


def qbytes_conv2d_a8_q_default(input, input_scale, weight, weight_scale, bias, out_scale, stride, padding, dilation):
    """The two-op sequence of a QConv2d with quantized activations: the convolution in the weight scale's dtype, then the output hook."""
    out = torch.ops.quanto.qbytes_conv2d_a8(input, input_scale, weight, weight_scale, bias, stride, padding, dilation)
    return _requantize_output(out, input.dtype, out_scale)


def qbytes_conv2d_a8_q_hip(input, input_scale, weight, weight_scale, bias, out_scale, stride, padding, dilation):
    """ROCm: the convolution kernel's epilogue stores the codes (csrc/qconv_a8.hip) exactly when ``qbytes_conv2d_a8_hip`` takes that kernel and the
    output scale is a scalar; every other call runs the two-op sequence on the existing ops - the caller always gets codes."""
    lib = quanto_hip.lib
    stride, padding, dilation = tuple(stride), tuple(padding), tuple(dilation)
    if (input_scale.numel() == 1 and out_scale.numel() == 1
            and lib.qbytes_conv2d_a8_supported(input, weight, weight_scale.dtype, stride, padding, dilation)):
        return lib.qbytes_conv2d_a8_q(input, input_scale, weight, weight_scale, bias, out_scale, stride, padding, dilation)
    return qbytes_conv2d_a8_q_default(input, input_scale, weight, weight_scale, bias, out_scale, stride, padding, dilation)


# new op: the convolution of a QConv2d with quantized activations with the layer's output quantization fused into the kernel epilogue - bit-identical
# to quantize_symmetric(qbytes_conv2d_a8(...)), one launch and no [B, OC, OH, OW] float tensor
_register("qbytes_conv2d_a8_q", "(Tensor input, Tensor input_scale, Tensor weight, Tensor weight_scale, Tensor? bias, Tensor out_scale, int[] stride, "
          "int[] padding, int[] dilation) -> Tensor", qbytes_conv2d_a8_q_hip, default=qbytes_conv2d_a8_q_default)


# ------------------------------------------------------------------------------------------------
# quanto::quantize_symmetric / quantize_affine (quantize-time, plain torch on every device)
# ------------------------------------------------------------------------------------------------
def _check_symmetric_args(base: torch.Tensor, axis: Union[int, None], scale: torch.Tensor) -> Union[int, None]:
    """Argument contract of library/quantize.py:26-49; returns the normalised axis (None, 0 or -1)."""
    if axis is None:
        if scale.ndim > 0:
            raise ValueError("Scale must be a scalar when quantizing per-tensor")
        return None
    if base.ndim == 1:
        raise ValueError("1D Tensors cannot be quantized per-axis")
    if axis == base.ndim - 1:
        axis = -1
    if axis not in (0, -1):
        raise ValueError("Quantization is only supported along the first or last axis.")
    if base.shape[axis] == 1:
        raise ValueError(f"Cannot quantize Tensor of shape {base.shape} along axis {axis} of size 1")
    if torch.squeeze(scale).ndim > 1:
        raise ValueError("Quantizing along multiple axis is not supported")
    if scale.ndim != base.ndim:
        raise ValueError(
            "When quantizing per-axis, the scale must be broadcastable to the base (Tip: try to add missing dims of length zero).")
    return axis


def quantize_symmetric(base: torch.Tensor, dtype: torch.dtype, axis: Union[int, None], scale: torch.Tensor) -> torch.Tensor:
    """clamp(round(base / scale)) to ``dtype`` (library/quantize.py:26-55; float8 targets are not rounded first)."""
    _check_symmetric_args(base, axis, scale)
    data = base / scale
    if not dtype.is_floating_point:
        data = torch.round(data)
    info = dtype_info(dtype)
    return torch.clamp(data, min=info.min, max=info.max).to(dtype)


def quantize_symmetric_hip(base: torch.Tensor, dtype: torch.dtype, axis: Union[int, None], scale: torch.Tensor) -> torch.Tensor:
    """Device tensors: the one-pass kernel (csrc/quantize.hip) for int8 / OCP float8 targets; the formats the hardware
    converters do not produce (e4m3fnuz) and non-float bases keep the elementwise torch sequence - still on the device."""
    axis = _check_symmetric_args(base, axis, scale)
    lib = quanto_hip.lib
    if dtype in lib.QUANTIZE_TARGETS and base.dtype in (torch.float32, torch.float16, torch.bfloat16) and (
            axis is None or scale.numel() == base.shape[axis]):
        return lib.quantize_symmetric(base, dtype, axis, scale)
    return quantize_symmetric(base, dtype, axis, scale)


def quantize_affine(base: torch.Tensor, bits: int, axis: int, group_size: Union[int, None], scale: torch.Tensor,
                    shift: torch.Tensor) -> torch.Tensor:
    """uint8 in [0, 2^bits): round((base + shift) / scale), or round(base / scale) + zero-point (library/quantize.py:66-78)."""
    if axis not in (0, -1):
        raise ValueError("axis parameter must be 0 (first axis) or -1 (last axis)")
    if group_size is not None:
        base = group(base, axis=axis, group_size=group_size)
    if shift.dtype.is_floating_point:
        data = torch.round((base + shift) / scale)
    else:
        data = torch.round(base / scale) + shift
    return torch.clamp(data, min=0, max=2**bits - 1).to(torch.uint8)


_register("quantize_symmetric", "(Tensor base, ScalarType dtype, int? axis, Tensor scale) -> Tensor", quantize_symmetric_hip,
          default=quantize_symmetric)


def quantize_affine_hip(base: torch.Tensor, bits: int, axis: int, group_size: Union[int, None], scale: torch.Tensor,
                        shift: torch.Tensor) -> torch.Tensor:
    """Device tensors: the one-pass kernel (csrc/quantize.hip) for the layout of the hot path - axis-0 2-D weights with
    one scale/shift per group; every other case keeps the torch sequence on the device."""
    if axis not in (0, -1):
        raise ValueError("axis parameter must be 0 (first axis) or -1 (last axis)")
    if (axis == 0 and base.ndim == 2 and bits in (2, 4) and base.dtype in (torch.float32, torch.float16, torch.bfloat16)
            and (group_size is None or base.shape[1] % group_size == 0)):
        rows = base.numel() // (group_size or base.shape[1])
        if scale.numel() == rows and shift.numel() == rows and shift.dtype in (base.dtype, torch.uint8, torch.int8):
            return quanto_hip.lib.quantize_affine(base, bits, group_size, scale, shift)
    return quantize_affine(base, bits, axis, group_size, scale, shift)


_register("quantize_affine", "(Tensor base, int bits, int axis, int? group_size, Tensor scale, Tensor shift) -> Tensor", quantize_affine_hip,
          default=quantize_affine)


# ------------------------------------------------------------------------------------------------
# quanto::layer_norm_q: the LayerNorm of a model with quantized activations and its output quantization in one launch
# ------------------------------------------------------------------------------------------------
def layer_norm_q_default(input, normalized_shape, weight, bias, eps: float, out_scale, dtype):
    """The two-op sequence of the reference's QLayerNorm (nn/qlayernorm.py:52-53, then the output hook of nn/qmodule.py): the float layer norm,
    quantized per-tensor at ``out_scale``."""
    y = torch.nn.functional.layer_norm(input, tuple(normalized_shape), weight, bias, eps)
    return torch.ops.quanto.quantize_symmetric(y, dtype, None, out_scale)


def _layer_norm_q_kernel_takes(input, normalized_shape, weight, bias, out_scale, dtype) -> bool:
    """The predicate of ``layer_norm_q_hip``: a plain float32 / float16 / bfloat16 tensor on the device that ends in ``normalized_shape``, weight and
    bias (each may be absent) of that shape in the same dtype, a one-element output scale on the device, an int8 / float8_e4m3fn / float8_e5m2 code
    type, n = prod(normalized_shape) within the row one workgroup holds in registers (``LAYER_NORM_Q_MAX_N``), fewer than 2^31 rows, and the
    normalized dimensions contiguous inside the input (leading dimensions that do not collapse to one row stride are the binding's business: it
    copies).  No shape class is routed back on speed: the kernel is 1.35-1.79x the sequence on every measured one (profiles/layernorm_q_vs_sequence.jsonl)."""
    lib = quanto_hip.lib
    nd = len(normalized_shape)
    if not (type(input) is torch.Tensor and input.is_cuda and input.dtype in lib.LAYER_NORM_Q_DTYPES and 0 < nd <= input.dim()
            and tuple(input.shape[input.dim() - nd:]) == tuple(normalized_shape)):
        return False
    n = 1
    for d in normalized_shape:
        n *= d
    for p in (weight, bias):
        if p is not None and not (type(p) in (torch.Tensor, torch.nn.Parameter) and p.is_cuda and p.dtype == input.dtype and p.numel() == n):
            return False
    if not (out_scale.is_cuda and out_scale.numel() == 1 and lib.layer_norm_q_supported(input.numel() // n if n else 0, n, input.dtype, dtype)):
        return False
    expect = 1
    for size, stride in zip(reversed(input.shape[input.dim() - nd:]), reversed(input.stride()[input.dim() - nd:])):
        if size != 1 and stride != expect:
            return False
        expect *= size
    return True


def layer_norm_q_hip(input, normalized_shape, weight, bias, eps: float, out_scale, dtype):
    """ROCm: one launch of csrc/layernorm_q.hip when the predicate says so; every other call runs the two-op sequence on the device - the caller always
    gets the sequence's contract."""
    if _layer_norm_q_kernel_takes(input, normalized_shape, weight, bias, out_scale, dtype):
        return quanto_hip.lib.layer_norm_q(input, normalized_shape, weight, bias, eps, out_scale, dtype)
    return layer_norm_q_default(input, normalized_shape, weight, bias, eps, out_scale, dtype)


# new op: F.layer_norm and the per-tensor quantization of its output in one launch - the float row is read once and the codes are stored.  Statistics
# in fp32 (two passes), the affine result rounded once to the input dtype, then the rule of quanto::quantize_symmetric: the codes of the sequence up to
# the last bits of the statistics (at most one code step, on a few elements in 10^5: tests/test_layernorm_q_gpu.py).  On the CPU the default runs.
_register("layer_norm_q", "(Tensor input, int[] normalized_shape, Tensor? weight, Tensor? bias, float eps, Tensor out_scale, ScalarType dtype) -> Tensor",
          layer_norm_q_hip, default=layer_norm_q_default)


# ------------------------------------------------------------------------------------------------
# quanto::dequantize_qbits and quanto::qbits_mm (new ops)
# ------------------------------------------------------------------------------------------------
def dequantize_qbits_default(packed, scale, shift, bits: int, group_size: Optional[int], out_features: int, in_features: int):
    """Reference sequence: unpack, trim, remove shift, scale, ungroup (tensor/packed.py:101-104, tensor/qbits.py:27-49)."""
    rows = (out_features * in_features) // group_size if group_size is not None else out_features
    data = torch.ops.quanto.unpack(packed, bits)[:rows]
    if not shift.dtype.is_floating_point:
        data = data.to(torch.int8) - shift.to(torch.int8)
    out = scale * data
    if shift.dtype.is_floating_point:
        out -= shift
    return ungroup(out, axis=0, orig_shape=torch.Size([out_features, in_features]))


def dequantize_qbits_hip(packed, scale, shift, bits: int, group_size: Optional[int], out_features: int, in_features: int):
    return quanto_hip.lib.dequantize_qbits(packed, scale, shift, bits, group_size, out_features, in_features)


def qbits_mm_default(input, packed, scale, shift, bias, bits: int, group_size: Optional[int], out_features: int, in_features: int):
    """x @ dequantize(W).T (+ bias): what tensor/function.py:41-47 computes through qfallback."""
    w = torch.ops.quanto.dequantize_qbits(packed, scale, shift, bits, group_size, out_features, in_features)
    out = torch.matmul(input, w.t())
    return out if bias is None else out + bias


def qbits_mm_hip(input, packed, scale, shift, bias, bits: int, group_size: Optional[int], out_features: int, in_features: int):
    return quanto_hip.lib.qbits_mm(input, packed, scale, shift, bias, bits, group_size, out_features, in_features)


_register("dequantize_qbits", "(Tensor packed, Tensor scale, Tensor shift, int bits, int? group_size, int out_features, int in_features) -> Tensor",
          dequantize_qbits_hip, default=dequantize_qbits_default)
_register("qbits_mm", "(Tensor input, Tensor packed, Tensor scale, Tensor shift, Tensor? bias, int bits, int? group_size, "
          "int out_features, int in_features) -> Tensor", qbits_mm_hip, default=qbits_mm_default)


# ------------------------------------------------------------------------------------------------
# quanto::qbits_mm_a8 (r6; int2 weights and e5m2 activations r7): F.linear(quantized activation, int4 / int2 weight) without dequantizing the activation
# ------------------------------------------------------------------------------------------------
def qbits_mm_a8_default(input, input_scale, packed, scale, shift, bias, bits: int, group_size: Optional[int], out_features: int, in_features: int):
    """What the reference computes (tensor/weights/awq/qbits.py:57-58, tensor/function.py:41-47): dequantize the activation, then the float product."""
    x = None
    if input.is_cuda:  # r6: cast + multiply in one pass (bit-identical: csrc/quantize.hip dequantize_symmetric)
        x = quanto_hip.lib.dequantize_symmetric(input, input_scale.to(scale.dtype))
    if x is None:
        x = input.to(scale.dtype) * input_scale.to(scale.dtype)
    return torch.ops.quanto.qbits_mm(x, packed, scale, shift, bias, bits, group_size, out_features, in_features)


def _a8_max_tiles() -> int:
    """The tile cap below; QUANTO_HIP_A8_MAX_TILES overrides it while experiments are on, read on every call with C's atoi rules like the
    library's own knobs."""
    return hip._c_atoi(os.environ.get("QUANTO_HIP_A8_MAX_TILES", "512")) if hip._EXPERIMENT else 512


# int2 weights x int8 activations run 15-20 % slower than int4 x int8 on the same tiles (r7 sweep, profiles/r07_w2a8_crossover.jsonl: (512,4096,4096)
# 35.5 vs 30.5 us) and lose to the dequantize-first sequence at the int4 cap: (512,14336,4096) = 448 tiles 111 vs 122 us, (2048,4096,4096) = 512 tiles
# 112 vs 108.  int2 x e5m2 and int4 x e5m2 keep the int4 cap (2048,4096,4096: 98 / 89 vs 106).
_A8_MAX_TILES_W2_INT8 = 448


def _a8_kernel_takes(input, input_scale, scale, bits: int, group_size: Optional[int], out_features: int, in_features: int) -> bool:
    """Whether this call goes to the W4A8 / W2A8 kernel (csrc/qbits_a8_fused.hip): one predicate for ``qbits_mm_a8_hip`` and ``qbits_mm_a8_q_hip``."""
    lib = quanto_hip.lib
    m = input.numel() // in_features if in_features else 0
    # batched-decode sizes keep the weight-streaming kernels (the activation is dequantized: M x K elements, nothing next to the weight stream);
    # above 64 rows the stored integers / fp8 values go to the 8-bit matrix instructions
    # ... while the output's 128 x 128 tiles are all resident at once (two workgroups per CU): the kernel moves 24 KiB through a CU's vector L1 per tile
    # and group and is bound by that, not by the matrix pipe; beyond one residency round the dequantize-first sequence on the dense bf16 GEMM is faster
    # (r6 sweep, profiles/r06_w4a8_crossover.jsonl: (2048,4096,4096) 93 vs 109 us, (4096,4096,4096) 184 vs 146, (768,14336,4096) 137 vs 114)
    # one 128-token x 128-feature tile per workgroup for int4 (64 packed rows) and int2 (32 packed rows x 4 planes) alike
    tiles = -(-m // 128) * -(-out_features // 128)
    cap = _a8_max_tiles()
    if bits == 2 and input.dtype == torch.int8:
        cap = min(cap, _A8_MAX_TILES_W2_INT8)
    return (64 < m and tiles <= cap and input.dtype in lib.A8_DTYPES and input_scale.numel() == 1
            and lib.qbits_mm_a8_workspace(m, out_features, in_features, bits, group_size, input.dtype, scale.dtype) >= 0)


def qbits_mm_a8_hip(input, input_scale, packed, scale, shift, bias, bits: int, group_size: Optional[int], out_features: int, in_features: int):
    if _a8_kernel_takes(input, input_scale, scale, bits, group_size, out_features, in_features):
        return quanto_hip.lib.qbits_mm_a8(input, input_scale, packed, scale, shift, bias, bits, group_size, out_features, in_features)
    return qbits_mm_a8_default(input, input_scale, packed, scale, shift, bias, bits, group_size, out_features, in_features)


_register("qbits_mm_a8", "(Tensor input, Tensor input_scale, Tensor packed, Tensor scale, Tensor shift, Tensor? bias, int bits, int? group_size, "
          "int out_features, int in_features) -> Tensor", qbits_mm_a8_hip, default=qbits_mm_a8_default)


def qbits_mm_a8_q_default(input, input_scale, packed, scale, shift, bias, out_scale, bits: int, group_size: Optional[int], out_features: int,
                          in_features: int):
    """The two-op sequence of a W4A8 / W2A8 layer: quanto::qbits_mm_a8 in the scales' dtype, then the output hook."""
    out = torch.ops.quanto.qbits_mm_a8(input, input_scale, packed, scale, shift, bias, bits, group_size, out_features, in_features)
    return _requantize_output(out, input.dtype, out_scale)


def qbits_mm_a8_q_hip(input, input_scale, packed, scale, shift, bias, out_scale, bits: int, group_size: Optional[int], out_features: int,
                      in_features: int):
    """ROCm: the a8 kernel's epilogue stores the codes exactly when quanto::qbits_mm_a8 runs that kernel for this call (_a8_kernel_takes: not up to 64
    rows, beyond the tile cap, or formats the kernel does not take), the output scale is a scalar and the view of the codes is aligned; every other call
    runs the two-op sequence on the existing ops - the caller always gets codes.  (A contiguous view of the codes that does not start on a 16-byte
    boundary is copied for the sequence: the a8 kernel of quanto::qbits_mm_a8 answers QUANTO_HIP_EALIGN to it; non-contiguous views are copied by the
    bindings anyway.)"""
    misaligned = input.is_contiguous() and input.data_ptr() % 16 != 0
    if out_scale.numel() == 1 and not misaligned and _a8_kernel_takes(input, input_scale, scale, bits, group_size, out_features, in_features):
        return quanto_hip.lib.qbits_mm_a8_q(input, input_scale, packed, scale, shift, bias, out_scale, bits, group_size, out_features, in_features)
    if misaligned:
        input = input.clone()
    return qbits_mm_a8_q_default(input, input_scale, packed, scale, shift, bias, out_scale, bits, group_size, out_features, in_features)


# new op: the product of a W4A8 / W2A8 layer with the layer's output quantization fused into the kernel epilogue - bit-identical to
# quantize_symmetric(qbits_mm_a8(...)), one launch and no [M, N] float tensor
_register("qbits_mm_a8_q", "(Tensor input, Tensor input_scale, Tensor packed, Tensor scale, Tensor shift, Tensor? bias, Tensor out_scale, int bits, "
          "int? group_size, int out_features, int in_features) -> Tensor", qbits_mm_a8_q_hip, default=qbits_mm_a8_q_default)


def qbits_conv2d_default(input, packed, scale, shift, bias, bits: int, group_size: Optional[int], weight_size, stride, padding, dilation):
    """What the reference computes for F.conv2d on a WeightQBitsTensor (nn/qconv2d.py:54-55 -> qfallback): dequantize, float convolution."""
    oc, c, kh, kw = weight_size
    w = torch.ops.quanto.dequantize_qbits(packed, scale, shift, bits, group_size, oc, c * kh * kw).reshape(oc, c, kh, kw)
    return torch.nn.functional.conv2d(input, w.to(input.dtype), bias, tuple(stride), tuple(padding), tuple(dilation), 1)


def qbits_conv2d_hip(input, packed, scale, shift, bias, bits: int, group_size: Optional[int], weight_size, stride, padding, dilation):
    return quanto_hip.lib.qbits_conv2d(input, packed, scale, shift, bias, bits, group_size, tuple(weight_size), tuple(stride), tuple(padding),
                                       tuple(dilation))


# new op: dense convolution with a packed int4 weight as an implicit GEMM on the device (csrc/qconv_mfma.hip, W_I4R staging): no im2col tensor,
# no dequantized weight in memory
_register("qbits_conv2d", "(Tensor input, Tensor packed, Tensor scale, Tensor shift, Tensor? bias, int bits, int? group_size, int[] weight_size, "
          "int[] stride, int[] padding, int[] dilation) -> Tensor", qbits_conv2d_hip, default=qbits_conv2d_default)


# several Linears applied to the same input in one launch (q/k/v, gate/up of a decoder layer at decode time)
def qbits_mm_multi_default(input, packed, scale, shift, bias, bits: int, group_size: Optional[int], out_features, in_features: int):
    return [torch.ops.quanto.qbits_mm(input, packed[i], scale[i], shift[i], bias[i], bits, group_size, out_features[i], in_features)
            for i in range(len(packed))]


def qbits_mm_multi_hip(input, packed, scale, shift, bias, bits: int, group_size: Optional[int], out_features, in_features: int):
    return quanto_hip.lib.qbits_mm_multi(input, packed, scale, shift, bias, bits, group_size, list(out_features), in_features)


_register("qbits_mm_multi", "(Tensor input, Tensor[] packed, Tensor[] scale, Tensor[] shift, Tensor?[] bias, int bits, int? group_size, "
          "int[] out_features, int in_features) -> Tensor[]", qbits_mm_multi_hip, default=qbits_mm_multi_default)


def qbytes_mm_multi_default(activations, weights, output_scales, bias):
    return [torch.ops.quanto.qbytes_mm_bias(activations, weights[i], output_scales[i], bias[i]) for i in range(len(weights))]


def qbytes_mm_multi_hip(activations, weights, output_scales, bias):
    return quanto_hip.lib.qbytes_mm_multi(activations, list(weights), list(output_scales), list(bias))


# the 8-bit counterpart: several WeightQBytes Linears applied to the same (float) input in one launch
_register("qbytes_mm_multi", "(Tensor A, Tensor[] B, Tensor[] scales, Tensor?[] bias) -> Tensor[]", qbytes_mm_multi_hip,
          default=qbytes_mm_multi_default)

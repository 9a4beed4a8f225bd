"""``QConv2d`` (optimum/quanto/nn/qconv2d.py:26-55).

The forward is the reference's: ``_conv_forward(input, self.qweight, self.bias)``, i.e. ``F.conv2d`` with a quantized
weight.  In the reference that call falls back to "dequantize the weight, run the float convolution".  Here the weight
tensors intercept ``F.conv2d`` (tensor/weights.py, ``conv2d_as_gemm``): on a ROCm device a dense (``groups == 1``)
convolution is lowered to im2col + the same fused ``quanto::qbytes_mm`` / ``quanto::qbits_mm`` kernels that serve QLinear -
the [N, C, kh, kw] weight *is* the [N, C*kh*kw] GEMM operand, byte for byte, in both storage formats.  Everything else
(grouped convolutions, CPU tensors) keeps the reference behaviour.

QConv2d with quantized activations: when the input reaching ``F.conv2d`` is an ``ActivationQBytesTensor`` (per-tensor scale) and the weight
is int8 / e4m3fn / e5m2, a dense convolution on a ROCm device runs ``quanto::qbytes_conv2d_a8`` (csrc/qconv_a8.hip): the stored 1-byte codes of
both go to the 8-bit matrix instructions, gathered inside the kernel - no dequantized activation, no im2col - with the W8A8 QLinear arithmetic
(integer / fp8 products scaled by ``input_scale * weight_scale``).  Served pairs: int8 x int8, fp8 x fp8 and fp8 x int8.  Int8 activations
with fp8 weights, e4m3fnuz, int4 / int2 weights, grouped convolutions, fp16 outputs with e5m2 activations and calls that want a gradient
keep the dequantizing route.

Fused output quantization: a frozen module marked by ``fuse_output_quantization`` (model_api.py) takes its output codes from that kernel's
epilogue (``quanto::qbytes_conv2d_a8_q``) whenever the call is one ``quanto::qbytes_conv2d_a8`` would serve - the float [B, OC, OH, OW] output
is never written and the output hook passes the codes through.  Bit-identical to the convolution followed by the hook; every other call
(CPU tensors, float inputs, a gradient wanted, ``padding_mode != "zeros"``) runs the forward below.
"""
from typing import Optional

import torch

from ..tensor import Optimizer, WeightQBytesTensor, qtype
from ..tensor.weights import conv2d_a8_eligible
from .module import QModuleMixin, register_qmodule

__all__ = ["QConv2d"]


# constructor arguments that describe the convolution geometry, copied verbatim from the float module
_GEOMETRY = ("in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "padding_mode")


@register_qmodule(torch.nn.Conv2d)
class QConv2d(QModuleMixin, torch.nn.Conv2d):
    @classmethod
    def qcreate(cls, module, weights: qtype, activations: Optional[qtype] = None, optimizer: Optional[Optimizer] = None,
                device: Optional[torch.device] = None):
        geometry = {name: getattr(module, name) for name in _GEOMETRY}
        return cls(**geometry, bias=module.bias is not None, dtype=module.weight.dtype, device=device, weights=weights,
                   activations=activations, optimizer=optimizer)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if self._fuse_output_quantization and self._codes_from_epilogue(input):
            # marked by fuse_output_quantization: convolution and output quantization in one op (quanto::qbytes_conv2d_a8_q), bit-identical to the
            # convolution followed by the output hook - which then passes these codes through
            w = self.weight
            codes = torch.ops.quanto.qbytes_conv2d_a8_q(input._data, input._scale, w._data, w._scale, self.bias, self.output_scale,
                                                        list(self.stride), list(self.padding), list(self.dilation))
            return self._output_from_codes(codes)
        # F.conv2d is intercepted by the weight's __torch_function__ (im2col + fused GEMM on a ROCm device)
        return self._conv_forward(input, self.qweight, self.bias)

    def _codes_from_epilogue(self, input) -> bool:
        """Whether this call is the one the fused op computes (QModuleMixin._takes_stored_codes), and what is the convolution's own: an 8-bit
        weight, zero padding, and a call ``quanto::qbytes_conv2d_a8`` serves (conv2d_a8_eligible: ROCm device, scalar input scale, dense, a served
        format pair, no gradient wanted - the op has no backward)."""
        w = self.weight
        if not (self._takes_stored_codes(input) and type(w) is WeightQBytesTensor and self.padding_mode == "zeros"):
            return False
        return conv2d_a8_eligible(input, w, self.bias, self.stride, self.padding, self.dilation, self.groups)

"""``QLayerNorm`` (optimum/quanto/nn/qlayernorm.py:26-53): the LayerNorm of a model with quantized activations.

The reference's behaviour comes first: the weights are never quantized, ``forward`` is the float ``F.layer_norm`` and the output hook quantizes its
result at ``output_scale`` - on every device, bit for bit.  What it is for: in a ViT or BERT block q / k / v and fc1 are fed by a LayerNorm; when its
output is an ``ActivationQBytesTensor`` those Linears take the int8 x int8 / fp8 x fp8 route on the 8-bit matrix units instead of bf16 x int8.

Fused output quantization: a module marked by ``fuse_output_quantization`` (model_api.py) calls ``quanto::layer_norm_q`` on a plain float input when no
gradient is wanted - on a ROCm device one launch of csrc/layernorm_q.hip reads the float row once and stores the codes (the float output is never
written); the output hook passes them through.  The codes are those of the two-op sequence up to the last bits of the statistics.  Every other call (a
quantized input, which dequantizes through ``qfallback``; a gradient wanted; the hook removed) runs the forward below.

The class is NOT registered as the counterpart of ``torch.nn.LayerNorm``: the default ``quantize()`` leaves LayerNorms as float modules, as before;
``quantize(..., layernorm=True)`` / ``requantize(..., layernorm=True)`` opt in.
"""
from typing import Optional

import torch

from ..tensor import Optimizer, qtype
from .module import QModuleMixin

__all__ = ["QLayerNorm"]


class QLayerNorm(QModuleMixin, torch.nn.LayerNorm):
    @classmethod
    def qcreate(cls, module, weights: Optional[qtype] = None, activations: Optional[qtype] = None, optimizer: Optional[Optimizer] = None,
                device: Optional[torch.device] = None):
        if activations is None:
            return None
        dtype = None if module.weight is None else module.weight.dtype
        # (weights / optimizer: a LayerNorm's weights are never quantized)
        return cls(module.normalized_shape, module.eps, module.elementwise_affine, module.bias is not None, dtype=dtype, device=device,
                   weights=None, activations=activations, optimizer=None)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if self._fuse_output_quantization and self._codes_from_kernel(input):
            # marked by fuse_output_quantization: layer norm and output quantization in one op (quanto::layer_norm_q) - the output hook then passes
            # these codes through
            codes = torch.ops.quanto.layer_norm_q(input, list(self.normalized_shape), self.weight, self.bias, self.eps, self.output_scale,
                                                  self.activation_qtype.dtype)
            return self._output_from_codes(codes)
        return torch.nn.functional.layer_norm(input, self.normalized_shape, self.weight, self.bias, self.eps)

    def _codes_from_kernel(self, input) -> bool:
        """Whether this call is the one the fused op computes: a plain float tensor reaches a module whose output hook is still in place, and no
        gradient is wanted (the op has no backward)."""
        if not (type(input) is torch.Tensor and input.is_floating_point() and "output" in self._quantize_hooks):
            return False
        return not (torch.is_grad_enabled() and (input.requires_grad or (self.weight is not None and self.weight.requires_grad)
                                                 or (self.bias is not None and self.bias.requires_grad)))

"""``QLinear`` - the entry point of the hot path (optimum/quanto/nn/qlinear.py:26-50)."""
from typing import Optional

import torch

from ..tensor import Optimizer, QTensor, WeightQBitsTensor, WeightQBytesTensor, qtype
from .module import QModuleMixin, register_qmodule

__all__ = ["QLinear"]


@register_qmodule(torch.nn.Linear)
class QLinear(QModuleMixin, torch.nn.Linear):
    @classmethod
    def qcreate(cls, module, weights: qtype, activations: Optional[qtype] = None, optimizer: Optional[Optimizer] = None,
                device: Optional[torch.device] = None):
        return cls(module.in_features, module.out_features, module.bias is not None, dtype=module.weight.dtype,
                   device=device, weights=weights, activations=activations, optimizer=optimizer, quantize_input=True)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        # F.linear is intercepted by the weight's __torch_function__ and lands on quanto::qbytes_mm / quanto::qbits_mm.  For a plain
        # activation tensor the weight class's handler is called directly: the same code path minus torch's override dispatch
        # (C++ -> handle_torch_function -> Python, ~2 us of the ~15 us a decode-shaped call costs on the host)
        w = self.qweight
        if self._fuse_output_quantization and self._codes_from_epilogue(input, w):
            # marked by fuse_output_quantization: product and output quantization in one op (quanto::qbytes_mm_q), bit-identical to the product
            # followed by the output hook - which then passes these codes through
            # (8-bit weights: quanto::qbytes_mm_q; int4 / int2 weights: quanto::qbits_mm_a8_q on the packed data as stored)
            if isinstance(w, WeightQBitsTensor):
                n, k = w.shape
                codes = torch.ops.quanto.qbits_mm_a8_q(input._data, input._scale, w._data._data, w._scale, w._shift, self.bias, self.output_scale,
                                                       w._data.bits, w._group_size, n, k)
            else:
                codes = torch.ops.quanto.qbytes_mm_q(input._data, w._data, input._scale * w._scale, self.bias, self.output_scale)
            return self._output_from_codes(codes)
        if type(input) is torch.Tensor and isinstance(w, QTensor):
            return type(w).__torch_function__(torch.nn.functional.linear, (type(w),), (input, w, self.bias))
        return torch.nn.functional.linear(input, w, bias=self.bias)

    def _codes_from_epilogue(self, input, w) -> bool:
        """Whether this call is the one the fused op computes (QModuleMixin._takes_stored_codes), and what is the Linear's own: a scalar input scale
        against an 8-bit weight of the same dtype or an int4 / int2 weight (the marking checked its format), no gradient wanted (the op has no
        backward)."""
        sub_byte = isinstance(w, WeightQBitsTensor)
        if not (self._takes_stored_codes(input) and (sub_byte or type(w) is WeightQBytesTensor)):
            return False
        if input._scale.numel() != 1 or not (sub_byte or input._data.dtype == w._data.dtype):
            return False
        return not (torch.is_grad_enabled() and (input.requires_grad or w.requires_grad or (self.bias is not None and self.bias.requires_grad)))

#!/usr/bin/env python3
"""QConv2d with QUANTIZED activations on the device: quanto::qbytes_conv2d_a8 (csrc/qconv_a8.hip) against the route such a call took before it
(dequantize the activation + F.unfold + quanto::qbytes_mm_bias) and against the 16-bit implicit convolution (quanto::qbytes_conv2d) on the
dequantized input.  One JSON line per shape and (activation, weight) format; hipGraph-timed, best of five replays (scripts/auto_vs_best.py)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import optimum_quanto_amd as Q  # noqa: E402
from auto_vs_best import _time_graph  # noqa: E402
from optimum_quanto_amd.library.hip import quanto_hip  # noqa: E402
from optimum_quanto_amd.tensor.weights import conv2d_as_gemm  # noqa: E402

# (B, C, H = W, OC, k, stride, padding), all bf16 out
SHAPES = [(8, 128, 28, 128, 3, 1, 1), (8, 128, 56, 128, 3, 1, 1), (8, 256, 56, 256, 3, 1, 1), (8, 64, 112, 128, 3, 2, 1), (8, 64, 56, 256, 1, 1, 0),
          (32, 512, 7, 512, 3, 1, 1), (1, 512, 7, 512, 3, 1, 1), (8, 3, 224, 64, 7, 2, 3)]
PAIRS = [("qint8", "qint8"), ("qfloat8_e4m3fn", "qfloat8_e4m3fn"), ("qfloat8_e4m3fn", "qint8")]  # (activations, weights)
if len(sys.argv) > 1:
    PAIRS = [tuple(p.split(":")) for p in sys.argv[1:]]

for (B, C, H, OC, k, s, p) in SHAPES:
    for act, wq in PAIRS:
        torch.manual_seed(0)
        conv = torch.nn.Conv2d(C, OC, k, stride=s, padding=p).to(torch.bfloat16)
        q = Q.QConv2d.from_module(conv, weights=getattr(Q, wq))
        Q.freeze(q)
        q = q.cuda()
        w = q.weight
        x = torch.randn(B, C, H, H, device="cuda").to(torch.bfloat16)
        qx = Q.quantize_activation(x, qtype=getattr(Q, act), scale=Q.absmax_scale(x, qtype=getattr(Q, act)))
        xdq = qx.dequantize()
        scale = w._scale.reshape(-1, 1).expand(OC, 1).contiguous()
        data2d = w._data.reshape(OC, -1)
        gemm = lambda a: torch.ops.quanto.qbytes_mm_bias(a, data2d, scale, q.bias)  # noqa: E731
        new = lambda: torch.ops.quanto.qbytes_conv2d_a8(qx._data, qx._scale, w._data, w._scale, q.bias, [s, s], [p, p], [1, 1])  # noqa: E731
        with torch.no_grad():
            new()
            kernel = quanto_hip.lib.last_kernel()
            t_new = _time_graph(new, 5)
            t_routed = _time_graph(lambda: torch.nn.functional.conv2d(qx, w, q.bias, s, p), 5)
            t_old = _time_graph(lambda: conv2d_as_gemm(qx, w, q.bias, (s, s), (p, p), (1, 1), 1, gemm), 5)
            t_16 = _time_graph(lambda: torch.ops.quanto.qbytes_conv2d(xdq, w._data, w._scale, q.bias, [s, s], [p, p], [1, 1]), 5)
        OHW = (H + 2 * p - k) // s + 1
        print(json.dumps({"activations": act, "weights": wq, "B": B, "C": C, "H": H, "OC": OC, "k": k, "stride": s, "pad": p, "M": B * OHW * OHW,
                          "K": C * k * k, "kernel": kernel, "a8_conv_us": round(t_new, 1), "routed_F_conv2d_us": round(t_routed, 1),
                          "dequant_unfold_gemm_us": round(t_old, 1), "implicit16_on_dequantized_us": round(t_16, 1)}), flush=True)

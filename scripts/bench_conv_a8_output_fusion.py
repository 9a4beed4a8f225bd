#!/usr/bin/env python3
"""Fused output quantization of QConv2d with quantized activations (quanto::qbytes_conv2d_a8_q) against the two-op sequence it replaces -
quanto::qbytes_conv2d_a8, then quanto::quantize_symmetric - per shape and format, with a bias, bf16.  Launch-inclusive, the method of bench.py (its
timed_replay: warm-up, the calls captured in one hipGraph, clock ramp, device events around one replay).  The two variants alternate, ROUNDS times each; a
line reports the median and the spread (min .. max) of each variant's rounds in us per call, and "fused_not_slower": median(fused) <= median(sequence) +
the sequence's own spread.  One JSON line per (shape, format); the codes of both variants are compared first (bit-identical or the line says so).  The
shapes are those of scripts/time_conv2d_a8.py; codes and scales are random with an output of order one: the time does not depend on the
values."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (timed_replay)
import optimum_quanto_amd  # noqa: E402,F401  (registers the ops)
from optimum_quanto_amd.library.hip import quanto_hip  # noqa: E402

ACTS = {"int8": torch.int8, "e4m3": torch.float8_e4m3fn}
QMAX = {torch.int8: 127.0, torch.float8_e4m3fn: 448.0}
RMS = {"int8": 74.0, "e4m3": 4.0}
# (B, C, H = W, OC, k, stride, padding)
SHAPES = [(8, 128, 28, 128, 3, 1, 1), (8, 128, 56, 128, 3, 1, 1), (8, 256, 56, 256, 3, 1, 1), (8, 64, 112, 128, 3, 2, 1), (8, 64, 56, 256, 1, 1, 0),
          (32, 512, 7, 512, 3, 1, 1), (1, 512, 7, 512, 3, 1, 1), (8, 3, 224, 64, 7, 2, 3)]


def operands(B, C, H, OC, k, act, dev):
    gen = torch.Generator(device="cpu").manual_seed(B + C + H + OC + k)
    dtype = ACTS[act]

    def codes(shape):
        return torch.randint(-128, 128, shape, dtype=torch.int8, generator=gen) if act == "int8" else (torch.randn(shape, generator=gen) * 4).to(dtype)

    x, w = codes((B, C, H, H)), codes((OC, C, k, k))
    x_scale = torch.tensor([1.0 / (RMS[act] * (C * k * k) ** 0.5)], dtype=torch.bfloat16)
    w_scale = ((torch.rand((OC, 1, 1, 1), generator=gen) + 0.5) / RMS[act]).to(torch.bfloat16)
    bias = torch.randn(OC, generator=gen).to(torch.bfloat16)
    return [t.to(dev) for t in (x, x_scale, w, w_scale, bias)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="timed replays per variant, alternating")
    ap.add_argument("--ramp-ms", type=float, default=100.0)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv_a8_output_fusion: needs a ROCm device (no fallback)")
    dev = torch.device("cuda", 0)
    lib = quanto_hip.lib
    for (B, C, H, OC, k, s, p) in SHAPES:
        for act in ACTS:
            dtype = ACTS[act]
            x, x_scale, w, w_scale, bias = operands(B, C, H, OC, k, act, dev)
            tail = ([s, s], [p, p], [1, 1])
            y = torch.ops.quanto.qbytes_conv2d_a8(x, x_scale, w, w_scale, bias, *tail)
            unfused_route = lib.last_kernel()
            out_scale = (torch.quantile(y.abs().float().reshape(-1)[:1 << 22], 0.9) / QMAX[dtype]).to(torch.bfloat16)

            def sequence():
                return torch.ops.quanto.quantize_symmetric(torch.ops.quanto.qbytes_conv2d_a8(x, x_scale, w, w_scale, bias, *tail), dtype, None, out_scale)

            def fused():
                return torch.ops.quanto.qbytes_conv2d_a8_q(x, x_scale, w, w_scale, bias, out_scale, *tail)

            want = sequence()
            got = fused()
            route = lib.last_kernel()
            identical = bool(torch.equal(got.view(torch.uint8), want.view(torch.uint8)))
            OHW = y.shape[-1]
            del y, want, got
            times = {"sequence": [], "fused": []}
            for _ in range(args.rounds):
                for variant, fn in (("sequence", sequence), ("fused", fused)):
                    _, ms = bench.timed_replay(fn, args.steps, args, None, dev)
                    times[variant].append(ms * 1e3 / args.steps)
            med = {v: statistics.median(t) for v, t in times.items()}
            spread = {v: max(t) - min(t) for v, t in times.items()}
            print(json.dumps({
                "B": B, "C": C, "H": H, "OC": OC, "k": k, "stride": s, "pad": p, "M": B * OHW * OHW, "K": C * k * k, "activations": act, "weights": act,
                "dtype": "bf16", "bias": True, "unfused_route": unfused_route, "fused_route": route, "codes_identical": identical,
                "store_form": "one dword per lane and pixel fragment",
                "sequence_us": round(med["sequence"], 2), "sequence_min_max_us": [round(min(times["sequence"]), 2), round(max(times["sequence"]), 2)],
                "fused_us": round(med["fused"], 2), "fused_min_max_us": [round(min(times["fused"]), 2), round(max(times["fused"]), 2)],
                "speedup": round(med["sequence"] / med["fused"], 3), "fused_not_slower": bool(med["fused"] <= med["sequence"] + spread["sequence"]),
                "method": f"{'eager' if args.eager else 'hipGraph replay'} of {args.steps} calls, {args.rounds} alternating rounds, launch-inclusive device events",
            }), flush=True)


if __name__ == "__main__":
    main()

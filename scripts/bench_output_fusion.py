#!/usr/bin/env python3
"""Fused output quantization (quanto::qbytes_mm_q) against the two-op sequence it replaces - quanto::qbytes_mm_bias, then quanto::quantize_symmetric - per
shape and format.  Launch-inclusive, the method of bench.py (its timed_replay: warm-up, the calls captured in one hipGraph, clock ramp, device events
around one replay).  The two variants alternate, ROUNDS times each; a line reports the median and the spread (min .. max) of each variant's rounds in us
per call, and "fused_not_slower": median(fused) <= median(sequence) + the sequence's own spread.  One JSON line per (shape, format); the codes of both
variants are compared first (bit-identical or the line says so)."""
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

SHAPES = [(4096, 4096, 4096), (512, 4096, 4096), (512, 14336, 4096), (32, 4096, 4096)]  # (M, N, K)
FORMATS = {"int8": torch.int8, "e4m3": torch.float8_e4m3fn}
QMAX = {torch.int8: 127.0, torch.float8_e4m3fn: 448.0}


def operands(M, N, K, dtype, dev):
    gen = torch.Generator(device="cpu").manual_seed(M + N + K)
    if dtype == torch.int8:
        a = torch.randint(-128, 128, (M, K), dtype=torch.int8, generator=gen)
        b = torch.randint(-128, 128, (N, K), dtype=torch.int8, generator=gen)
        base = 1.0 / (74.0 * 74.0 * K ** 0.5)  # outputs of order one
    else:
        a, b = torch.randn((M, K), generator=gen).to(dtype), torch.randn((N, K), generator=gen).to(dtype)
        base = 1.0 / K ** 0.5
    scales = ((torch.rand((N, 1), generator=gen) + 0.5) * base).to(torch.bfloat16)
    bias = torch.randn(N, generator=gen).to(torch.bfloat16)
    return a.to(dev), b.to(dev), scales.to(dev), bias.to(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="timed replays per variant, alternating")
    ap.add_argument("--ramp-ms", type=float, default=100.0)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_output_fusion: needs a ROCm device (no fallback)")
    dev = torch.device("cuda", 0)
    lib = quanto_hip.lib
    for M, N, K in SHAPES:
        for name, dtype in FORMATS.items():
            a, b, scales, bias = operands(M, N, K, dtype, dev)
            y = torch.ops.quanto.qbytes_mm_bias(a, b, scales, bias)
            out_scale = (y.abs().max().float() / QMAX[dtype] * 0.7).to(torch.bfloat16)

            def sequence():
                return torch.ops.quanto.quantize_symmetric(torch.ops.quanto.qbytes_mm_bias(a, b, scales, bias), dtype, None, out_scale)

            def fused():
                return torch.ops.quanto.qbytes_mm_q(a, b, scales, bias, out_scale)

            want = sequence()
            got = fused()
            route = lib.last_kernel()
            identical = bool(torch.equal(got.view(torch.uint8), want.view(torch.uint8)))
            del y, want, got
            times = {"sequence": [], "fused": []}
            for _ in range(args.rounds):
                for variant, fn in (("sequence", sequence), ("fused", fused)):
                    _, ms = bench.timed_replay(fn, args.steps, args, None, dev)
                    times[variant].append(ms * 1e3 / args.steps)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            print(json.dumps({
                "M": M, "N": N, "K": K, "format": name, "mid_dtype": "bf16", "bias": True, "fused_route": route, "codes_identical": identical,
                "sequence_us": round(med["sequence"], 2), "sequence_min_max_us": [round(min(times["sequence"]), 2), round(max(times["sequence"]), 2)],
                "fused_us": round(med["fused"], 2), "fused_min_max_us": [round(min(times["fused"]), 2), round(max(times["fused"]), 2)],
                "speedup": round(med["sequence"] / med["fused"], 3), "fused_not_slower": bool(med["fused"] <= med["sequence"] + spread["sequence"]),
                "method": f"{'eager' if args.eager else 'hipGraph replay'} of {args.steps} calls, {args.rounds} alternating rounds, launch-inclusive device events",
            }), flush=True)


if __name__ == "__main__":
    main()

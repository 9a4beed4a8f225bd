#!/usr/bin/env python3
"""Fused output quantization of W4A8 / W2A8 layers (quanto::qbits_mm_a8_q) against the two-op sequence it replaces - quanto::qbits_mm_a8, then
quanto::quantize_symmetric - per shape and format, both with a bias, bf16.  Launch-inclusive, the method of bench.py (its timed_replay: warm-up, the calls
captured in one hipGraph, clock ramp, device events around one replay).  The two variants alternate, ROUNDS times each; a line reports the median and the
spread (min .. max) of each variant's rounds in us per call, and "fused_not_slower": median(fused) <= median(sequence) + the sequence's own spread.  One
JSON line per (shape, format); the codes of both variants are compared first (bit-identical or the line says so).  The weights are random packed bytes
with scales that keep the output of order one: the time does not depend on the values."""
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

ACTS = {"int8": torch.int8, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
QMAX = {torch.int8: 127.0, torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}
A_RMS = {"int8": 74.0, "e4m3": 1.0, "e5m2": 1.0}
LARGE = [(128, 4096, 4096), (512, 4096, 4096), (2048, 4096, 4096), (512, 14336, 4096)]  # (M, N, K)
CASES = [(s, 4, act) for s in LARGE for act in ("int8", "e4m3")] + [((512, 4096, 4096), 2, "e5m2")]


def operands(M, N, K, bits, act, dev):
    gen = torch.Generator(device="cpu").manual_seed(M + N + K + bits)
    dtype = ACTS[act]
    a = torch.randint(-128, 128, (M, K), dtype=torch.int8, generator=gen) if act == "int8" else torch.randn((M, K), generator=gen).to(dtype)
    packed = torch.randint(0, 256, (N * bits // 8, K), dtype=torch.int16, generator=gen).to(torch.uint8)
    groups = N * K // 128
    qrms = 4.6 if bits == 4 else 1.1  # rms of a uniform nibble / crumb around its mean
    scale = ((torch.rand((groups, 1), generator=gen) + 0.5) / (A_RMS[act] * qrms * K ** 0.5)).to(torch.bfloat16)
    shift = (scale.float() * ((1 << bits) - 1) / 2).to(torch.bfloat16)  # float shifts: the mean of the codes
    bias = torch.randn(N, generator=gen).to(torch.bfloat16)
    a_scale = torch.tensor([1.0], dtype=torch.bfloat16)
    return [t.to(dev) for t in (a, a_scale, packed, scale, shift, bias)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="timed replays per variant, alternating")
    ap.add_argument("--ramp-ms", type=float, default=100.0)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_a8_output_fusion: needs a ROCm device (no fallback)")
    dev = torch.device("cuda", 0)
    lib = quanto_hip.lib
    for (M, N, K), bits, act in CASES:
        dtype = ACTS[act]
        a, a_scale, packed, scale, shift, bias = operands(M, N, K, bits, act, dev)
        tail = (bits, 128, N, K)
        y = torch.ops.quanto.qbits_mm_a8(a, a_scale, packed, scale, shift, bias, *tail)
        unfused_route = lib.last_kernel()
        out_scale = (torch.quantile(y.abs().float().reshape(-1), 0.9) / QMAX[dtype]).to(torch.bfloat16)

        def sequence():
            return torch.ops.quanto.quantize_symmetric(torch.ops.quanto.qbits_mm_a8(a, a_scale, packed, scale, shift, bias, *tail), dtype, None, out_scale)

        def fused():
            return torch.ops.quanto.qbits_mm_a8_q(a, a_scale, packed, scale, shift, bias, out_scale, *tail)

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
            "M": M, "N": N, "K": K, "weights": f"int{bits}", "activations": act, "dtype": "bf16", "bias": True, "unfused_route": unfused_route,
            "fused_route": route, "codes_identical": identical, "store_form": "one dword per lane and token fragment",
            "sequence_us": round(med["sequence"], 2), "sequence_min_max_us": [round(min(times["sequence"]), 2), round(max(times["sequence"]), 2)],
            "fused_us": round(med["fused"], 2), "fused_min_max_us": [round(min(times["fused"]), 2), round(max(times["fused"]), 2)],
            "speedup": round(med["sequence"] / med["fused"], 3), "fused_not_slower": bool(med["fused"] <= med["sequence"] + spread["sequence"]),
            "method": f"{'eager' if args.eager else 'hipGraph replay'} of {args.steps} calls, {args.rounds} alternating rounds, launch-inclusive device events",
        }), flush=True)


if __name__ == "__main__":
    main()

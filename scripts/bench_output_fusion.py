#!/usr/bin/env python3
"""Fused output quantization against the two-op sequence it replaces - the product op, then quanto::quantize_symmetric - per layer kind, shape and format,
with a bias, bf16:  --layer w8a8  quanto::qbytes_mm_q against quanto::qbytes_mm_bias;  --layer a8  quanto::qbits_mm_a8_q against quanto::qbits_mm_a8
(W4A8 / W2A8);  --layer conv  quanto::qbytes_conv2d_a8_q against quanto::qbytes_conv2d_a8 (the shapes of scripts/time_conv2d_a8.py).  Default:
all three.  Launch-inclusive, the method of bench.py (its timed_replay: warm-up, the calls captured in one hipGraph, clock ramp, device events around one
replay).  The two variants alternate, ROUNDS times each; a line reports the median and the spread (min .. max) of each variant's rounds in us per call,
and "fused_not_slower": median(fused) <= median(sequence) + the sequence's own spread.  One JSON line per case; the codes of both variants are compared
first (bit-identical or the line says so).  Operands are random with an output of order one: the time does not depend on the values."""
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
ops = torch.ops.quanto


# A layer kind is a generator of cases: (the keys that lead its JSON line, the keys behind "codes_identical", the unfused op's route or None when the
# line does not report it, sequence(), fused()); the two callables hold their case's operands as default arguments, not the loop's variables.
def w8a8_cases(dev):
    for M, N, K in [(4096, 4096, 4096), (512, 4096, 4096), (512, 14336, 4096), (32, 4096, 4096)]:
        for name in ("int8", "e4m3"):
            dtype = ACTS[name]
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
            args = tuple(t.to(dev) for t in (a, b, scales, bias))
            out_scale = (ops.qbytes_mm_bias(*args).abs().max().float() / QMAX[dtype] * 0.7).to(torch.bfloat16)
            yield (dict(M=M, N=N, K=K, format=name, mid_dtype="bf16", bias=True), {}, None,
                   lambda args=args, dtype=dtype, s=out_scale: ops.quantize_symmetric(ops.qbytes_mm_bias(*args), dtype, None, s),
                   lambda args=args, s=out_scale: ops.qbytes_mm_q(*args, s))


def a8_cases(dev):
    large = [(128, 4096, 4096), (512, 4096, 4096), (2048, 4096, 4096), (512, 14336, 4096)]  # (M, N, K)
    a_rms = {"int8": 74.0, "e4m3": 1.0, "e5m2": 1.0}
    for (M, N, K), bits, act in [(s, 4, act) for s in large for act in ("int8", "e4m3")] + [((512, 4096, 4096), 2, "e5m2")]:
        dtype = ACTS[act]
        gen = torch.Generator(device="cpu").manual_seed(M + N + K + bits)
        a = torch.randint(-128, 128, (M, K), dtype=torch.int8, generator=gen) if act == "int8" else torch.randn((M, K), generator=gen).to(dtype)
        packed = torch.randint(0, 256, (N * bits // 8, K), dtype=torch.int16, generator=gen).to(torch.uint8)  # random packed bytes
        qrms = 4.6 if bits == 4 else 1.1  # rms of a uniform nibble / crumb around its mean
        scale = ((torch.rand((N * K // 128, 1), generator=gen) + 0.5) / (a_rms[act] * qrms * K ** 0.5)).to(torch.bfloat16)
        shift = (scale.float() * ((1 << bits) - 1) / 2).to(torch.bfloat16)  # float shifts: the mean of the codes
        bias = torch.randn(N, generator=gen).to(torch.bfloat16)
        args = tuple(t.to(dev) for t in (a, torch.tensor([1.0], dtype=torch.bfloat16), packed, scale, shift, bias))
        tail = (bits, 128, N, K)
        y = ops.qbits_mm_a8(*args, *tail)
        unfused_route = quanto_hip.lib.last_kernel()
        out_scale = (torch.quantile(y.abs().float().reshape(-1), 0.9) / QMAX[dtype]).to(torch.bfloat16)
        del y
        yield (dict(M=M, N=N, K=K, weights=f"int{bits}", activations=act, dtype="bf16", bias=True),
               dict(store_form="one dword per lane and token fragment"), unfused_route,
               lambda args=args, tail=tail, dtype=dtype, s=out_scale: ops.quantize_symmetric(ops.qbits_mm_a8(*args, *tail), dtype, None, s),
               lambda args=args, tail=tail, s=out_scale: ops.qbits_mm_a8_q(*args, s, *tail))


def conv_cases(dev):
    rms = {"int8": 74.0, "e4m3": 4.0}
    # (B, C, H = W, OC, k, stride, padding)
    for B, C, H, OC, k, s, p in [(8, 128, 28, 128, 3, 1, 1), (8, 128, 56, 128, 3, 1, 1), (8, 256, 56, 256, 3, 1, 1), (8, 64, 112, 128, 3, 2, 1),
                                 (8, 64, 56, 256, 1, 1, 0), (32, 512, 7, 512, 3, 1, 1), (1, 512, 7, 512, 3, 1, 1), (8, 3, 224, 64, 7, 2, 3)]:
        for act in ("int8", "e4m3"):
            dtype = ACTS[act]
            gen = torch.Generator(device="cpu").manual_seed(B + C + H + OC + k)

            def codes(shape):
                return torch.randint(-128, 128, shape, dtype=torch.int8, generator=gen) if act == "int8" else (torch.randn(shape, generator=gen) * 4).to(dtype)

            x, w = codes((B, C, H, H)), codes((OC, C, k, k))
            x_scale = torch.tensor([1.0 / (rms[act] * (C * k * k) ** 0.5)], dtype=torch.bfloat16)
            w_scale = ((torch.rand((OC, 1, 1, 1), generator=gen) + 0.5) / rms[act]).to(torch.bfloat16)
            bias = torch.randn(OC, generator=gen).to(torch.bfloat16)
            args = tuple(t.to(dev) for t in (x, x_scale, w, w_scale, bias))
            tail = ([s, s], [p, p], [1, 1])
            y = ops.qbytes_conv2d_a8(*args, *tail)
            unfused_route = quanto_hip.lib.last_kernel()
            out_scale = (torch.quantile(y.abs().float().reshape(-1)[:1 << 22], 0.9) / QMAX[dtype]).to(torch.bfloat16)
            OHW = y.shape[-1]
            del y
            yield (dict(B=B, C=C, H=H, OC=OC, k=k, stride=s, pad=p, M=B * OHW * OHW, K=C * k * k, activations=act, weights=act, dtype="bf16", bias=True),
                   dict(store_form="one dword per lane and pixel fragment"), unfused_route,
                   lambda args=args, tail=tail, dtype=dtype, s=out_scale: ops.quantize_symmetric(ops.qbytes_conv2d_a8(*args, *tail), dtype, None, s),
                   lambda args=args, tail=tail, s=out_scale: ops.qbytes_conv2d_a8_q(*args, s, *tail))


LAYERS = {"w8a8": w8a8_cases, "a8": a8_cases, "conv": conv_cases}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--layer", action="append", choices=sorted(LAYERS), help="repeatable; default: all three")
    ap.add_argument("--steps", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="timed replays per variant, alternating")
    ap.add_argument("--ramp-ms", type=float, default=100.0)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_output_fusion: needs a ROCm device (no fallback)")
    dev = torch.device("cuda", 0)
    for layer in args.layer or ["w8a8", "a8", "conv"]:
        for head, extra, unfused_route, sequence, fused in LAYERS[layer](dev):
            want = sequence()
            got = fused()
            route = quanto_hip.lib.last_kernel()
            identical = bool(torch.equal(got.view(torch.uint8), want.view(torch.uint8)))
            del want, got
            times = {"sequence": [], "fused": []}
            for _ in range(args.rounds):
                for variant, fn in (("sequence", sequence), ("fused", fused)):
                    _, ms = bench.timed_replay(fn, args.steps, args, None, dev)
                    times[variant].append(ms * 1e3 / args.steps)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            print(json.dumps({
                **head, **({} if unfused_route is None else {"unfused_route": unfused_route}), "fused_route": route, "codes_identical": identical, **extra,
                "sequence_us": round(med["sequence"], 2), "sequence_min_max_us": [round(min(times["sequence"]), 2), round(max(times["sequence"]), 2)],
                "fused_us": round(med["fused"], 2), "fused_min_max_us": [round(min(times["fused"]), 2), round(max(times["fused"]), 2)],
                "speedup": round(med["sequence"] / med["fused"], 3), "fused_not_slower": bool(med["fused"] <= med["sequence"] + spread["sequence"]),
                "method": f"{'eager' if args.eager else 'hipGraph replay'} of {args.steps} calls, {args.rounds} alternating rounds, launch-inclusive device events",
            }), flush=True)


if __name__ == "__main__":
    main()

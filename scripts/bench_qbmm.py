#!/usr/bin/env python3
"""quanto::qbytes_bmm (csrc/qbytes_bmm.hip: one int8 x int8 launch on the 8-bit matrix instructions) against the sequence it replaces -
``qbytes_bmm_default``: both operands cast to fp32, an fp32 bmm, the multiply by the scale product, the cast - on the same tensors, bf16 output.
The two products of an eager attention block per (B = batch x heads, s, d): q k^T, [B, s, d] x the contiguous [B, d, s] tensor that matmul's reshape
makes of k.transpose(2, 3) (N contiguous), and p v, [B, s, s] x [B, s, d].  Launch-inclusive, the method of bench.py (its timed_replay: warm-up, the
calls captured in one hipGraph, clock ramp, device events around one replay).  The two variants alternate, ROUNDS times each; a line reports the median
and the spread (min .. max) of each variant's rounds in us per call, and "kernel_not_slower": median(kernel) <= median(sequence) + the sequence's own
spread - the yardstick is the sequence on the same box in the same run.  One JSON line per case; the outputs of both variants are compared first (all K
here are <= 2048; bit-identical is guaranteed for K <= 1024).  Operands are full-range random codes: the time does not depend on them."""
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
from optimum_quanto_amd.library.ops import qbytes_bmm_default  # noqa: E402

SHAPES = [(96, 197, 64), (128, 512, 64), (32, 2048, 128)]  # (B, s, d)


def cases(dev):
    for B, s, d in SHAPES:
        gen = torch.Generator(device="cpu").manual_seed(B + s + d)
        codes = lambda *shape: torch.randint(-128, 128, shape, dtype=torch.int8, generator=gen).to(dev)  # noqa: E731
        scale = torch.tensor(1.0 / (74.0 * 74.0 * d ** 0.5), dtype=torch.float32, device=dev)
        yield dict(product="q_kT", B=B, s=s, d=d, M=s, N=s, K=d, w="N contiguous"), codes(B, s, d), codes(B, d, s), scale
        yield dict(product="p_v", B=B, s=s, d=d, M=s, N=d, K=s, w="N contiguous"), codes(B, s, s), codes(B, s, d), scale


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="timed replays per variant, alternating")
    ap.add_argument("--ramp-ms", type=float, default=100.0)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_qbmm: needs a ROCm device (no fallback)")
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16
    for head, a, w, scale in cases(dev):
        sequence = lambda a=a, w=w, scale=scale: qbytes_bmm_default(a, w, scale, dtype)  # noqa: E731
        kernel = lambda a=a, w=w, scale=scale: torch.ops.quanto.qbytes_bmm(a, w, scale, dtype)  # noqa: E731
        want = sequence()
        got = kernel()
        route = quanto_hip.lib.last_kernel()
        identical = bool(torch.equal(got, want))
        del want, got
        times = {"sequence": [], "kernel": []}
        for _ in range(args.rounds):
            for variant, fn in (("sequence", sequence), ("kernel", kernel)):
                _, ms = bench.timed_replay(fn, args.steps, args, None, dev)
                times[variant].append(ms * 1e3 / args.steps)
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        print(json.dumps({
            **head, "dtype": "bf16", "route": route, "outputs_identical": identical,
            "sequence_us": round(med["sequence"], 2), "sequence_min_max_us": [round(min(times["sequence"]), 2), round(max(times["sequence"]), 2)],
            "kernel_us": round(med["kernel"], 2), "kernel_min_max_us": [round(min(times["kernel"]), 2), round(max(times["kernel"]), 2)],
            "speedup": round(med["sequence"] / med["kernel"], 3), "kernel_not_slower": bool(med["kernel"] <= med["sequence"] + spread["sequence"]),
            "method": f"{'eager' if args.eager else 'hipGraph replay'} of {args.steps} calls, {args.rounds} alternating rounds, launch-inclusive device events",
        }), flush=True)


if __name__ == "__main__":
    main()

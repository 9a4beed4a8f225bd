#!/usr/bin/env python3
"""quanto::layer_norm_q (csrc/layernorm_q.hip: one launch reads the float row and stores the codes) against the sequence it replaces -
``layer_norm_q_default``: F.layer_norm, then quanto::quantize_symmetric on the existing kernel - on the same tensors, bf16 input with weight and bias,
int8 and e4m3 codes.  Shapes (rows, n): a ViT-base block (8 x 197 tokens, 768), and hidden sizes 4096 / 8192 at 32 .. 4096 rows.  Launch-inclusive, the
method of bench.py (its timed_replay: warm-up, the calls captured in one hipGraph, clock ramp, device events around one replay).  The two variants
alternate, ROUNDS times each; a line reports the median and the spread (min .. max) of each variant's rounds in us per call, and
"kernel_not_slower": median(kernel) <= median(sequence) + the sequence's own spread - the yardstick is the sequence on the same box in the same run.
One JSON line per case; the codes of both variants are compared first (the share that differs, and the largest distance in codes)."""
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
from optimum_quanto_amd.library.ops import layer_norm_q_default  # noqa: E402

SHAPES = [(8 * 197, 768), (32, 4096), (512, 4096), (4096, 4096), (2048, 8192)]  # (rows, n)
CODES = {"int8": (torch.int8, 127.0), "e4m3": (torch.float8_e4m3fn, 448.0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=50, help="calls per captured graph")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="timed replays per variant, alternating")
    ap.add_argument("--ramp-ms", type=float, default=100.0)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_layernorm_q: needs a ROCm device (no fallback)")
    dev = torch.device("cuda", 0)
    T = torch.bfloat16
    for rows, n in SHAPES:
        gen = torch.Generator(device="cpu").manual_seed(rows + n)
        x = (torch.randn((rows, n), generator=gen) * 1.5 + 0.3).to(T).to(dev)
        w = (1 + 0.25 * torch.randn(n, generator=gen)).to(T).to(dev)
        b = (0.5 * torch.randn(n, generator=gen)).to(T).to(dev)
        for code, (dtype, qmax) in CODES.items():
            scale = torch.tensor(0.7 * 5.0 / qmax, dtype=T, device=dev)
            sequence = lambda: layer_norm_q_default(x, [n], w, b, 1e-5, scale, dtype)  # noqa: E731
            kernel = lambda: torch.ops.quanto.layer_norm_q(x, [n], w, b, 1e-5, scale, dtype)  # noqa: E731
            want = sequence()
            got = kernel()
            route = quanto_hip.lib.last_kernel()
            differing = float((got.view(torch.uint8) != want.view(torch.uint8)).float().mean())
            distance = int((got.to(torch.float32) - want.to(torch.float32)).abs().max()) if dtype == torch.int8 else None
            del want, got
            times = {"sequence": [], "kernel": []}
            for _ in range(args.rounds):
                for variant, fn in (("sequence", sequence), ("kernel", kernel)):
                    _, ms = bench.timed_replay(fn, args.steps, args, None, dev)
                    times[variant].append(ms * 1e3 / args.steps)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            moved = rows * n * 3 + 2 * n * 2  # bytes the kernel has to move: the bf16 row in, the codes out, weight and bias once
            print(json.dumps({
                "rows": rows, "n": n, "dtype": "bf16", "codes": code, "route": route, "share_of_codes_differing": differing, "largest_int8_distance": distance,
                "sequence_us": round(med["sequence"], 2), "sequence_min_max_us": [round(min(times["sequence"]), 2), round(max(times["sequence"]), 2)],
                "kernel_us": round(med["kernel"], 2), "kernel_min_max_us": [round(min(times["kernel"]), 2), round(max(times["kernel"]), 2)],
                "speedup": round(med["sequence"] / med["kernel"], 3), "kernel_not_slower": bool(med["kernel"] <= med["sequence"] + spread["sequence"]),
                "kernel_gb_per_s": round(moved / med["kernel"] / 1e3, 1),
                "method": f"{'eager' if args.eager else 'hipGraph replay'} of {args.steps} calls, {args.rounds} alternating rounds, launch-inclusive device events",
            }), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Host-side cost of the streaming decode calls that eager decode pays: us per call of 2000 back-to-back launches (after 50), wall clock around the
loop with a device sync, for the batched-decode kernels at (32,4096,4096), the one-launch q/k/v products at M = 32 and the (1,4096,4096) GEMVs.
One JSON line per op; run it in several processes to see the spread (profiles/streaming_plan_host_path.jsonl)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimum_quanto_amd.library.hip import quanto_hip  # noqa: E402

lib, dev, dt = quanto_hip.lib, "cuda", torch.bfloat16
tree = sys.argv[1] if len(sys.argv) > 1 else ""
gen = torch.Generator(device=dev).manual_seed(0)
K, QKV = 4096, [4096, 1024, 1024]


def w4(N):
    return (torch.randint(0, 256, (N * K // 2,), generator=gen, device=dev, dtype=torch.uint8),
            torch.rand((N * K // 128,), generator=gen, device=dev).to(dt) * 0.01, torch.rand((N * K // 128,), generator=gen, device=dev).to(dt))


def w8(N):
    return torch.randint(-100, 100, (N, K), generator=gen, device=dev, dtype=torch.int8), torch.rand((N,), generator=gen, device=dev).to(dt) * 0.01


def timeit(fn, n=2000):
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


x1, x32 = torch.randn((1, K), device=dev, dtype=dt), torch.randn((32, K), device=dev, dtype=dt)
p, s, z = w4(4096)
b, bs = w8(4096)
q4, q8 = [w4(N) for N in QKV], [w8(N) for N in QKV]
ops = {
    "qbits_mm (32,4096,4096)": lambda: lib.qbits_mm(x32, p, s, z, None, 4, 128, 4096, K),
    "qbytes_mm (32,4096,4096)": lambda: lib.qbytes_mm(x32, b, bs),
    "qbits_mm_multi q/k/v M=32": lambda: lib.qbits_mm_multi(x32, [w[0] for w in q4], [w[1] for w in q4], [w[2] for w in q4], None, 4, 128, QKV, K),
    "qbytes_mm_multi q/k/v M=32": lambda: lib.qbytes_mm_multi(x32, [w[0] for w in q8], [w[1] for w in q8], None),
    "qbits_mm (1,4096,4096)": lambda: lib.qbits_mm(x1, p, s, z, None, 4, 128, 4096, K),
    "qbytes_mm (1,4096,4096)": lambda: lib.qbytes_mm(x1, b, bs),
}
for name, fn in ops.items():
    us = timeit(fn)
    print(json.dumps({"op": name, "tree": tree, "route": lib.last_kernel(), "us_per_call": round(us, 3),
                      "method": "eager, 2000 back-to-back calls after 50, wall clock around the loop with a device sync"}), flush=True)

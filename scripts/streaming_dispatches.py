#!/usr/bin/env python3
"""One call per rung of the streaming decode kernels' host plans (csrc/qbits_skinny.hip, qbytes_skinny.hip, qbits_mmv.hip, the two GEMVs), to be run
under a kernel trace so that two builds of the library can be compared dispatch by dispatch (kernel name, grid, workgroup and LDS size):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python scripts/streaming_dispatches.py      # one JSON line per call
    python scripts/streaming_dispatches.py --table <dir>/.../t_kernel_trace.csv --tree <name>                 # one JSON line per dispatch of the library

The operands are random bytes: only the launches matter here (parity is the test suite's job).  profiles/streaming_plan_dispatches.jsonl holds the
tables of the commit before the units got their planners and of the one after.
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("QUANTO_HIP_EXPERIMENT", "1")  # before the library loads: the ring-depth knob below is read per call


def table(path, tree):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))  # one in-order queue: start time = dispatch order
    rows = [r for r in rows if "qh::" in r["Kernel_Name"]]
    for i, r in enumerate(rows):
        print(json.dumps({"tree": tree, "dispatch": i, "kernel": r["Kernel_Name"], "grid": [int(r[f"Grid_Size_{a}"]) for a in "XYZ"],
                          "workgroup": [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"], "lds": int(r["LDS_Block_Size"])}))


def calls():
    import torch

    from optimum_quanto_amd.library.hip import BF16, KERNEL_SKINNY, quanto_hip

    lib, c, dev, dt = quanto_hip.lib, quanto_hip.cdll, "cuda", torch.bfloat16
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(0)

    def x_of(M, K):
        return torch.randn((M, K), generator=gen, device=dev, dtype=dt)

    def w4_of(N, K, bits=4, gs=128):  # packed bytes, scale, shift of an int4 / int2 weight (gs None: per-channel)
        groups = N * (K // gs if gs else 1)
        return (torch.randint(0, 256, (N * K * bits // 8,), generator=gen, device=dev, dtype=torch.uint8),
                torch.rand((groups,), generator=gen, device=dev).to(dt) * 0.01, torch.rand((groups,), generator=gen, device=dev).to(dt))

    def w8_of(N, K, kind=None):
        b = torch.randint(-100, 100, (N, K), generator=gen, device=dev, dtype=torch.int8)
        return (b if kind is None else b.view(kind)), torch.rand((N,), generator=gen, device=dev).to(dt) * 0.01

    def say(op, shape, **more):
        torch.cuda.synchronize()
        print(json.dumps({"op": op, "shape": shape, "kernel": lib.last_kernel(), **more}), flush=True)

    def int4(M, N, K, kernel="skinny", bits=4, gs=128):
        p, s, z = w4_of(N, K, bits, gs)
        lib.qbits_mm(x_of(M, K), p, s, z, None, bits, gs, N, K, kernel=kernel)
        say("qbits_mm", [M, N, K], bits=bits, group_size=gs)

    def int8(M, N, K, kernel="skinny", kind=None):
        b, s = w8_of(N, K, kind)
        lib.qbytes_mm(x_of(M, K), b, s, kernel=kernel)
        say("qbytes_mm", [M, N, K], weight=str(b.dtype))

    # token fragments 1 / 2 / 4 on 4, 2 and 1 waves (one and two wave sets; ring depths 8 / 6 / 4 follow from fragments, waves and K)
    for N in (64, 32, 16):
        for M in (8, 17, 33):
            int4(M, N, 1024)
    int4(8, 64, 128)  # one tile: the deepest ring of 4 waves
    # group sizes 64 / 32 / 96, per-channel scales, int2
    int4(8, 64, 1024, gs=64)
    int4(33, 64, 1024, gs=32)
    int4(17, 64, 1152, gs=96)
    int4(8, 64, 1024, gs=None)
    int4(17, 64, 1024, bits=2)
    # unsplit and split; the passes of 64 rows
    int4(32, 4096, 1024)
    int4(32, 4096, 4096)
    int4(65, 256, 1024)
    int4(130, 256, 1024)
    for kind in (None, torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e4m3fnuz):
        int8(8, 64, 1024, kind=kind)
    int8(17, 64, 1024)
    int8(33, 64, 1024)
    int8(32, 4096, 1024)
    int8(32, 4096, 4096)
    int8(65, 256, 1024)
    int8(130, 256, 1024)
    # a shape that asks for a split, handed no workspace through the C entries: one block per feature block
    M, N, K = 32, 4096, 4096
    p, s, z = w4_of(N, K)
    x, y = x_of(M, K), torch.empty((M, N), device=dev, dtype=dt)
    st = c.quanto_hip_qbits_mm(x.data_ptr(), p.data_ptr(), s.data_ptr(), z.data_ptr(), 0, y.data_ptr(), M, N, K, 4, 128, BF16, BF16, KERNEL_SKINNY, 0, 0, stream)
    say("quanto_hip_qbits_mm, no workspace", [M, N, K], status=st)
    b, s = w8_of(N, K)
    st = c.quanto_hip_qbytes_mm_ws(x.data_ptr(), b.data_ptr(), s.data_ptr(), 0, y.data_ptr(), M, N, K, BF16, 3, BF16, KERNEL_SKINNY, 0, 0, stream)
    say("quanto_hip_qbytes_mm_ws, no workspace", [M, N, K], status=st)
    # several Linears in one launch: q/k/v and gate/up of Llama-3-8B
    for widths in ([4096, 1024, 1024], [14336, 14336]):
        for M in (8, 32):
            ws4 = [w4_of(N, 4096) for N in widths]
            lib.qbits_mm_multi(x_of(M, 4096), [w[0] for w in ws4], [w[1] for w in ws4], [w[2] for w in ws4], None, 4, 128, widths, 4096)
            say("qbits_mm_multi", [M, widths, 4096])
            ws8 = [w8_of(N, 4096) for N in widths]
            lib.qbytes_mm_multi(x_of(M, 4096), [w[0] for w in ws8], [w[1] for w in ws8], None)
            say("qbytes_mm_multi", [M, widths, 4096])
    # the GEMVs: 1 / 2 / 4 waves per row group, 1..4 slabs per wave, passes of rows
    for K in (1024, 4096, 14336):
        for M in (1, 3, 8):
            int4(M, 4096, K, kernel="gemv")
            int8(M, 4096, K, kernel="gemv")
    int4(8, 4096, 4096, kernel="mmv")
    int4(32, 4096, 4096, kernel="mmv")
    # the deep rings behind QUANTO_HIP_SKINNY_LDS_KB (the kernel name carries the ring depth): int4 8 / 8 / 4 stages on 4 waves, 8-bit 8 / 8 / 6
    os.environ["QUANTO_HIP_SKINNY_LDS_KB"] = "100"
    for M in (8, 17, 33):
        int4(M, 64, 1024)
        int8(M, 64, 1024)
    del os.environ["QUANTO_HIP_SKINNY_LDS_KB"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", help="a rocprofv3 kernel_trace.csv: print the library's dispatches, one JSON line each")
    ap.add_argument("--tree", default="", help="label of the build the trace was taken from")
    args = ap.parse_args()
    if args.table:
        table(args.table, args.tree)
    else:
        calls()

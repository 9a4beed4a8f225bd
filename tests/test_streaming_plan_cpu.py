"""The host plans of the weight-streaming decode kernels (csrc/qbits_skinny.hip skinny::make_plan, csrc/qbytes_skinny.hip skinny8::make_plan) decide
what the units decided before each got one planner: whether a shape is served (the status of the plan entry with the kernel forced to SKINNY) and the
K split (a split plan's workspace is 4096 + (N/16) S 64 tf 16 bytes for int4 / int2 and 4096 + ceil(N/64) S 256 tf 16 for the 8-bit weights: it
exposes S tf).  tests/golden/streaming_plan_table.json holds a seeded sweep and the answers of the library built from the commit named in its header
- the last one without these planners -, recorded by this file:

    python tests/test_streaming_plan_cpu.py --record --lib <libquanto_hip.so of that commit> --commit <its hash>

The answers are computed in a child process, where QUANTO_HIP_EXPERIMENT=1 is set before the library loads and the knobs of MODES are set in turn (the
library reads them on every call once the switch is on).  QUANTO_HIP_SKINNY_LDS_KB only deepens the DMA ring, which no plan entry reports: that mode is
recorded all the same (it must not move an answer) and the rule "a mode changes an answer" is asked of the other four.

The second half writes down, as literals, the statuses of the launch entries for argument sets that return before any launch.  Needs no device.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "streaming_plan_table.json")
F16, BF16, I8, F8_E4M3FN, F8_E5M2, F8_E4M3FNUZ = 1, 2, 3, 5, 6, 7  # quanto_hip_dtype
KERNEL_SKINNY = 5                                                   # quanto_hip_kernel
OK, EINVAL, ENOTSUP, EALIGN = 0, -1, -2, -4                         # quanto_hip_status
MODES = {"unset": {}, "split2": {"QUANTO_HIP_SKINNY_SPLIT": "2"}, "split4": {"QUANTO_HIP_SKINNY_SPLIT": "4"},
         "waves1": {"QUANTO_HIP_SKINNY_WAVES": "1"}, "waves2": {"QUANTO_HIP_SKINNY_WAVES": "2"}, "lds100": {"QUANTO_HIP_SKINNY_LDS_KB": "100"}}
MOVING_MODES = ("split2", "split4", "waves1", "waves2")  # lds100: see the module docstring
KNOBS = ("QUANTO_HIP_SKINNY_SPLIT", "QUANTO_HIP_SKINNY_WAVES", "QUANTO_HIP_SKINNY_LDS_KB")
SEED = 20261018
ROUTES = ("qbits", "qbytes", "qbits_multi", "qbytes_multi")
M_EDGES = (1, 2, 5, 8, 15, 16, 17, 18, 31, 32, 33, 34, 48, 63, 64, 65, 66, 96, 128, 129, 130, 192, 255, 256)
MULTI_WIDTHS = ([4096, 1024, 1024], [14336, 14336], [4096, 4096, 4096], [11008, 11008], [5120, 1280, 1280], [8192, 1024, 1024], [4096, 4096, 4096, 4096])


def make_cases():
    """qbits: [M, N, K, bits, group size (0: per-channel), dtype]; qbytes: [M, N, K, weight dtype, dtype]; the multi routes: [[N...], M, K, ...]."""
    import numpy as np

    rng = np.random.default_rng(SEED)

    edges = iter(M_EDGES * 40)  # every edge comes round

    def pick_m(i):
        return next(edges) if i % 3 else int(rng.integers(1, 257))

    def pick_n(i):  # mostly multiples of 64 up to 8192 (where a split can pay), some wide ones, a share that are multiples of 32 / 16 only
        r = i % 8
        if r < 5:
            return 64 * int(rng.integers(1, 129))
        if r == 5:
            return 64 * int(rng.integers(129, 449))
        return (32 if r == 6 else 16) * (2 * int(rng.integers(0, 64)) + 1)

    def pick_k(i, gs):
        if gs == 96:
            return int((192, 1152, 2880, 4800, 96 * int(rng.integers(2, 120)))[i // 10 % 5])
        return 128 if i % 12 == 0 else 1024 if i % 12 == 6 else 256 * int(rng.integers(8, 57))

    cases = {r: [] for r in ROUTES}
    for i in range(260):
        gs = (128, 128, 96, 64, 128, 32, 0, 128, 128, 64)[i % 10]
        bits = 2 if i % 7 == 4 else 4  # int2 is served with group size 128 only
        cases["qbits"].append([pick_m(i), pick_n(i), pick_k(i, gs), bits, gs, (BF16, F16)[(i // 2) % 2]])
    for i in range(120):
        cases["qbytes"].append([pick_m(i), pick_n(i) if i % 5 else int(rng.integers(1, 4097)), pick_k(i, 128), (I8, F8_E4M3FN, F8_E5M2, F8_E4M3FNUZ)[i % 4],
                                (BF16, F16)[(i // 4) % 2]])
    for i in range(80):
        if i % 2 == 0:
            widths = MULTI_WIDTHS[(i // 2) % len(MULTI_WIDTHS)]
        else:
            widths = [64 * int(rng.integers(1, 65)) for _ in range(2 + i % 3)]
            if i % 16 == 15:
                widths[-1] += 32  # not a multiple of 64: separate calls
        M = int((5, 8, 16, 17, 32, 33, 64, 65, 3, 24)[i % 10])
        K = int((4096, 2048, 8192, 14336, 1024, 5120, 11008, 128)[(i // 2) % 8])
        cases["qbits_multi"].append([widths, M, K, (BF16, F16)[(i // 3) % 2]])
        cases["qbytes_multi"].append([widths, M, K, (I8, F8_E4M3FN, F8_E5M2, F8_E4M3FNUZ)[i % 4], (BF16, F16)[(i // 3) % 2]])
    return cases


def _child(lib_path):
    """stdin: the cases; stdout: {mode: {route: [[plan status, plan workspace, workspace_size], ...]}} (multi: [status, kernel, workspace, workspace_size])."""
    assert os.environ.get("QUANTO_HIP_EXPERIMENT") == "1" and not any(k in os.environ for k in KNOBS)
    cases = json.load(sys.stdin)
    lib = ctypes.CDLL(lib_path)
    i64, ci, ip, lp = ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)

    def fn(name, restype, argtypes):
        f = getattr(lib, "quanto_hip_" + name)
        f.restype, f.argtypes = restype, argtypes
        return f

    plan4, size4 = fn("qbits_mm_plan", ci, [i64] * 3 + [ci] * 4 + [ip, lp]), fn("qbits_mm_workspace_size", i64, [i64] * 3 + [ci] * 4)
    plan8, size8 = fn("qbytes_mm_plan", ci, [i64] * 3 + [ci] * 4 + [ip, lp]), fn("qbytes_mm_workspace_size", i64, [i64] * 3 + [ci] * 4)
    mplan4, msize4 = fn("qbits_mm_multi_plan", ci, [ci, lp, i64, i64, ci, ci, ci, ip, lp]), fn("qbits_mm_multi_workspace_size", i64, [ci, lp, i64, i64, ci, ci, ci])
    mplan8 = fn("qbytes_mm_multi_plan", ci, [ci, lp, i64, i64, ci, ci, ci, ip, lp])
    k, ws = ci(-9), i64(-9)

    def asked(status):
        out = [status, k.value, ws.value]
        k.value, ws.value = -9, -9
        return out

    out = {}
    for mode, knobs in MODES.items():
        for name in KNOBS:
            os.environ.pop(name, None)
        os.environ.update(knobs)
        rows = out[mode] = {r: [] for r in ROUTES}
        for M, N, K, bits, gs, dt in cases["qbits"]:
            rows["qbits"].append(asked(plan4(M, N, K, bits, gs, dt, KERNEL_SKINNY, k, ws))[::2] + [size4(M, N, K, bits, gs, dt, KERNEL_SKINNY)])
        for M, N, K, bdt, dt in cases["qbytes"]:
            rows["qbytes"].append(asked(plan8(M, N, K, dt, bdt, dt, KERNEL_SKINNY, k, ws))[::2] + [size8(M, N, K, dt, bdt, dt, KERNEL_SKINNY)])
        for widths, M, K, dt in cases["qbits_multi"]:
            arr = (i64 * len(widths))(*widths)
            rows["qbits_multi"].append(asked(mplan4(len(widths), arr, M, K, 4, 128, dt, k, ws)) + [msize4(len(widths), arr, M, K, 4, 128, dt)])
        for widths, M, K, bdt, dt in cases["qbytes_multi"]:  # (this product has no separate size entry)
            arr = (i64 * len(widths))(*widths)
            rows["qbytes_multi"].append(asked(mplan8(len(widths), arr, M, K, dt, bdt, dt, k, ws)))
    json.dump(out, sys.stdout)


def answers(lib_path, cases):
    env = {k: v for k, v in os.environ.items() if not k.startswith("QUANTO_HIP_")}
    env["QUANTO_HIP_EXPERIMENT"] = "1"
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path], input=json.dumps(cases), capture_output=True, text=True,
                          timeout=120, env=env)
    assert proc.returncode == 0, proc.stderr
    return json.loads(proc.stdout)


def shares(rows):
    """Of the single-op cases with the knobs unset: the share with a split (a non-zero workspace), the share not served; and the modes that move an answer."""
    single = rows["unset"]["qbits"] + rows["unset"]["qbytes"]
    return {"split": sum(r[1] > 0 for r in single) / len(single), "unsupported": sum(r[0] != OK for r in single) / len(single),
            "moving_modes": [m for m in MODES if rows[m] != rows["unset"]]}


def check_shares(s):
    assert s["split"] >= 0.30, f"only {s['split']:.2f} of the single-op cases are split"
    assert s["unsupported"] <= 0.25, f"{s['unsupported']:.2f} of the single-op cases are not served"
    assert set(MOVING_MODES) <= set(s["moving_modes"]), f"modes that change no answer: {set(MOVING_MODES) - set(s['moving_modes'])}"


def test_the_sweep_covers_what_the_plans_depend_on():
    table = json.load(open(TABLE))
    cases = table["cases"]
    assert cases == make_cases() and sum(len(c) for c in cases.values()) >= 500
    q4, q8 = cases["qbits"], cases["qbytes"]
    assert all(1 <= M <= 256 for M, *_ in q4 + q8)
    for edge in (16, 17, 32, 33, 64, 65):  # the token-fragment ladder and the passes of 64
        assert sum(M == edge for M, *_ in q4) >= 3 and any(M == edge for M, *_ in q8)
    assert sum(N % 64 == 0 for _, N, *_ in q4) > len(q4) // 2 and any(N % 64 == 32 for _, N, *_ in q4) and any(N % 32 == 16 for _, N, *_ in q4)
    assert {(b, g) for *_, b, g, _ in q4} >= {(4, 128), (4, 96), (4, 64), (4, 32), (4, 0), (2, 128)} and {c[5] for c in q4} == {BF16, F16}
    assert {K for _, _, K, _, g, _ in q4 if g == 96} >= {1152, 2880, 4800} and {128, 1024} <= {K for _, _, K, *_ in q4}
    assert {c[3] for c in q8} == {I8, F8_E4M3FN, F8_E5M2, F8_E4M3FNUZ}
    assert all(2 <= len(w) <= 4 for w, *_ in cases["qbits_multi"]) and {3, 2, 4} == {len(w) for w, *_ in cases["qbits_multi"]}
    assert [4096, 1024, 1024] in [w for w, *_ in cases["qbits_multi"]] and [14336, 14336] in [w for w, *_ in cases["qbytes_multi"]]
    s = shares(table["rows"])
    check_shares(s)
    assert s == table["shares"]
    # a split's bytes are the counters plus whole token fragments: 64 lanes x 16 bytes per 16 features (int4), 256 x 16 per 64 features (8-bit)
    for (M, N, *_), (st, ws, size) in zip(q4, table["rows"]["unset"]["qbits"]):
        assert (st, ws) == (OK, size) and (ws == 0 or (ws - 4096) % ((N // 16) * 64 * 16) == 0) or (st, size) == (ENOTSUP, ENOTSUP)
    for (M, N, *_), (st, ws, size) in zip(q8, table["rows"]["unset"]["qbytes"]):
        assert (st, ws) == (OK, size) and (ws == 0 or (ws - 4096) % (-(-N // 64) * 256 * 16) == 0) or (st, size) == (ENOTSUP, ENOTSUP)
    assert any(k == KERNEL_SKINNY and ws > 0 for _, k, ws, *_ in table["rows"]["unset"]["qbits_multi"])
    assert any(k == KERNEL_SKINNY and ws > 0 for _, k, ws in table["rows"]["unset"]["qbytes_multi"])


def test_plans_are_those_of_the_commit_that_recorded_the_table():
    from optimum_quanto_amd.library.hip import quanto_hip

    table = json.load(open(TABLE))
    got = answers(quanto_hip.lib_path, table["cases"])
    for mode in MODES:
        for route in ROUTES:
            want, have = table["rows"][mode][route], got[mode][route]
            wrong = [(c, w, h) for c, w, h in zip(table["cases"][route], want, have) if w != h]
            assert len(want) == len(have) and not wrong, f"{mode} {route}: {len(wrong)} of {len(want)} plans differ from commit {table['commit']}, first {wrong[:3]}"


# ---- statuses of the launch entries, as the library answered them before the planners (none of these calls reaches a launch) ----------------------
_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
PTR = 1 << 20  # a 16-byte aligned address that is never dereferenced


_LIB = None  # --statuses: the library to ask in place of the package's


def _entry(name, argtypes):
    lib = _LIB
    if lib is None:
        from optimum_quanto_amd.library.hip import quanto_hip

        lib = quanto_hip.cdll
    fn = getattr(lib, "quanto_hip_" + name)
    fn.restype, fn.argtypes = _ci, argtypes
    return fn


def _qbits_mm(M=32, N=4096, K=4096, bits=4, gs=128, dtype=BF16, x=PTR, w=PTR, y=PTR):
    fn = _entry("qbits_mm", [_vp] * 6 + [_i64] * 3 + [_ci] * 5 + [_vp, _sz, _vp])
    return fn(x, w, PTR if w else None, PTR if w else None, None, y, M, N, K, bits, gs, dtype, dtype, KERNEL_SKINNY, None, 0, None)


def _qbytes_mm(M=32, N=4096, K=4096, b_dtype=I8, dtype=BF16, x=PTR, w=PTR, y=PTR, gs=None):
    fn = _entry("qbytes_mm_ws", [_vp] * 5 + [_i64] * 3 + [_ci] * 4 + [_vp, _sz, _vp])
    return fn(x, w, PTR if w else None, None, y, M, N, K, dtype, b_dtype, dtype, KERNEL_SKINNY, None, 0, None)


def _multi(bits4, count, widths=(4096, 1024, 1024), M=32, K=4096, ptr=PTR):
    n = (_i64 * 4)(*(list(widths) + [64] * 4)[:4])
    ptrs = (_vp * 4)(ptr, ptr, ptr, ptr)
    if bits4:
        fn = _entry("qbits_mm_multi_ws", [_vp, _ci] + [_vp] * 6 + [_i64, _i64] + [_ci] * 4 + [_vp, _sz, _vp])
        return fn(ptr, count, ptrs, ptrs, ptrs, None, ptrs, n, M, K, 4, 128, BF16, BF16, None, 0, None)
    fn = _entry("qbytes_mm_multi_ws", [_vp, _ci] + [_vp] * 5 + [_i64, _i64] + [_ci] * 3 + [_vp, _sz, _vp])
    return fn(ptr, count, ptrs, ptrs, None, ptrs, n, M, K, BF16, I8, BF16, None, 0, None)


SINGLE = [
    # (what, arguments, status of qbits_mm, status of qbytes_mm_ws; None: the entry has no such argument)
    ("served, operands at address 8", dict(x=8, w=8), EALIGN, EALIGN),
    ("served, x at address 8", dict(x=8), EALIGN, EALIGN),
    ("served, weight at address 8", dict(w=8), EALIGN, EALIGN),
    ("served over two passes (M = 130), x at address 8", dict(M=130, x=8), EALIGN, EALIGN),
    ("K = 200 (per-channel scales): not served", dict(K=200, gs=0), ENOTSUP, ENOTSUP),
    ("K = 200, operands at address 8: not served comes first", dict(K=200, gs=0, x=8, w=8), ENOTSUP, ENOTSUP),
    ("K = 200, null pointers: the entry's own check comes first", dict(K=200, gs=0, x=None, w=None, y=None), EINVAL, EINVAL),
    ("M = 257: not served", dict(M=257), ENOTSUP, ENOTSUP),
    ("M = 257, operands at address 8", dict(M=257, x=8, w=8), ENOTSUP, ENOTSUP),
    ("M = 0, null pointers", dict(M=0, x=None, w=None, y=None), OK, OK),
    ("group size 64 with N = 4064", dict(gs=64, N=4064), ENOTSUP, None),
    ("group size 64 with N = 4096, operands at address 8", dict(gs=64, x=8, w=8), EALIGN, None),
    ("group size 96 with K = 4800, operands at address 8", dict(gs=96, K=4800, x=8, w=8), EALIGN, None),
    ("group size 96 with N = 4128", dict(gs=96, K=4800, N=4128), ENOTSUP, None),
    ("int2, operands at address 8", dict(bits=2, x=8, w=8), EALIGN, None),
    ("int2 with group size 64", dict(bits=2, gs=64), ENOTSUP, None),
    ("per-channel scales, operands at address 8", dict(gs=0, x=8, w=8), EALIGN, None),
    ("N = 4104 (no multiple of 16)", dict(N=4104), ENOTSUP, None),
    ("N = 4104, weight at address 8", dict(N=4104, w=8), None, EALIGN),
    ("e4m3fnuz weight, operands at address 8", dict(b_dtype=F8_E4M3FNUZ, x=8, w=8), None, EALIGN),
    ("uint8 weight", dict(b_dtype=4), None, ENOTSUP),
]
MULTI = [
    # (what, arguments, status of qbits_mm_multi_ws, status of qbytes_mm_multi_ws)
    ("no Linear", dict(count=0), EINVAL, EINVAL),
    ("five Linears", dict(count=5), EINVAL, EINVAL),
    ("no Linear, null pointers", dict(count=0, ptr=None), EINVAL, EINVAL),
    ("five Linears, M = 0", dict(count=5, M=0), EINVAL, EINVAL),
    ("three Linears, null pointers", dict(count=3, ptr=None), EINVAL, EINVAL),
    ("three Linears, M = 0", dict(count=3, M=0), OK, OK),
    ("three Linears, K = 0", dict(count=3, K=0), EINVAL, EINVAL),
]


def test_single_entry_statuses():
    for what, args, want4, want8 in SINGLE:
        if want4 is not None:
            assert _qbits_mm(**args) == want4, f"qbits_mm, {what}"
        if want8 is not None:
            assert _qbytes_mm(**args) == want8, f"qbytes_mm_ws, {what}"


def test_multi_entry_statuses():
    for what, args, want4, want8 in MULTI:
        assert _multi(True, **args) == want4, f"qbits_mm_multi_ws, {what}"
        assert _multi(False, **args) == want8, f"qbytes_mm_multi_ws, {what}"


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        _child(sys.argv[2])
    elif sys.argv[1] == "--statuses":  # prints the status tables of the library at sys.argv[2] (to write the literals above down)
        _LIB = ctypes.CDLL(os.path.abspath(sys.argv[2]))
        for what, args, want4, want8 in SINGLE:
            print(what, None if want4 is None else _qbits_mm(**args), None if want8 is None else _qbytes_mm(**args), (want4, want8))
        for what, args, want4, want8 in MULTI:
            print(what, _multi(True, **args), _multi(False, **args), (want4, want8))
    else:
        import argparse

        ap = argparse.ArgumentParser()
        ap.add_argument("--record", action="store_true", required=True)
        ap.add_argument("--lib", required=True)
        ap.add_argument("--commit", required=True)
        args = ap.parse_args()
        cases = make_cases()
        rows = answers(os.path.abspath(args.lib), cases)
        s = shares(rows)
        check_shares(s)  # refuses to write a table that could not tell two planners apart
        with open(TABLE, "w") as f:
            json.dump({"commit": args.commit,
                       "what": "per case and mode, of that commit's library with QUANTO_HIP_EXPERIMENT=1: qbits / qbytes [status and workspace of "
                               "quanto_hip_q*_mm_plan with the kernel forced to SKINNY, quanto_hip_q*_mm_workspace_size]; qbits_multi [status, kernel, workspace "
                               "of quanto_hip_qbits_mm_multi_plan (int4, group size 128), quanto_hip_qbits_mm_multi_workspace_size]; qbytes_multi [status, "
                               "kernel, workspace of quanto_hip_qbytes_mm_multi_plan]",
                       "modes": MODES, "seed": SEED, "shares": s, "cases": cases, "rows": rows}, f, separators=(",", ":"))
            f.write("\n")
        print(f"{TABLE}: {sum(len(c) for c in cases.values())} cases x {len(MODES)} modes; {s}")

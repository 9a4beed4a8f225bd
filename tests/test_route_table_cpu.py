"""The host dispatch of qbits_mm and qbytes_mm (csrc/c_api.hip: one route table per product, read by the serve rule, the workspace rule, the planner
and the launch) answers what it answered while every kernel was spelled out in four switches.  tests/golden/route_table.json holds a seeded sweep of
about 600 problems per product and, per problem, what the host-only entries of the library built from the commit named in its header said:

* qbits_mm:  quanto_hip_qbits_mm_plan for every kernel id -1 .. 11 (status, kernel, workspace bytes), _pick, _workspace_size for AUTO;
* qbytes_mm: quanto_hip_qbytes_mm_plan for the same ids, _pick, _workspace_size for AUTO, quanto_hip_qbytes_mm_q_plan for AUTO and NATIVE8.

Recorded by this file:

    python tests/test_route_table_cpu.py --record --lib <libquanto_hip.so of that commit> --commit <its hash>

The answers are computed in a child process without any QUANTO_HIP_* variable.  Needs no device.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "route_table.json")
F32, F16, BF16, I8, U8, F8_E4M3FN, F8_E5M2, F8_E4M3FNUZ = range(8)  # quanto_hip_dtype
OK, EINVAL, ENOTSUP = 0, -1, -2                                     # quanto_hip_status
AUTO, NAIVE, GEMV, MFMA, MFMA_LARGE, SKINNY, NATIVE8, DEQUANT_MFMA, MFMA_FUSED4, MMV, MFMA_LARGE4 = range(11)  # quanto_hip_kernel
IDS = list(range(-1, 12))
QBITS_IDS = (NAIVE, GEMV, MFMA, SKINNY, DEQUANT_MFMA, MFMA_FUSED4, MMV, MFMA_LARGE4)
QBYTES_IDS = (NAIVE, GEMV, MFMA, MFMA_LARGE, SKINNY, NATIVE8)
QBITS_AUTO = {NAIVE, GEMV, MFMA, SKINNY, DEQUANT_MFMA, MFMA_FUSED4, MMV}  # MFMA_LARGE4: only for callers without a workspace, the plan entries plan with one
QBYTES_AUTO = {NAIVE, GEMV, MFMA, MFMA_LARGE, SKINNY, NATIVE8}
SEED, CASES, MIN_SEEN = 20261021, 600, 8
# M on both sides of the planners' thresholds
M_LIST = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97, 128, 192, 193, 256, 257, 512, 1024, 1025, 1536, 2048, 4096, 8192]
# (a, b, out): 16-bit x int8 / e4m3 / e5m2 / e4m3fnuz, int8 x int8, fp8 x fp8, fp32 x 8-bit -> fp32, mixed and refused combinations
TRIPLES = [(BF16, I8, BF16), (F16, I8, F16), (BF16, F8_E4M3FN, BF16), (F16, F8_E5M2, F16), (BF16, F8_E5M2, BF16), (F16, F8_E4M3FN, F16),
           (I8, I8, BF16), (I8, I8, F16), (F8_E4M3FN, F8_E4M3FN, BF16), (F8_E5M2, F8_E5M2, F16), (F32, I8, F32), (F32, F8_E4M3FN, F32),
           (F32, F8_E5M2, F32), (BF16, F8_E4M3FNUZ, BF16), (I8, I8, F32), (F8_E4M3FN, F8_E5M2, BF16), (BF16, I8, F16), (F32, I8, BF16),
           (I8, F8_E4M3FN, BF16), (BF16, I8, I8), (F16, BF16, F16), (BF16, I8, BF16)]


def _mnk(rng, i):
    M = M_LIST[(i // 3) % len(M_LIST)] if i % 3 == 0 else int(rng.integers(1, 600))
    N = 16 * int(rng.integers(1, 1025)) if i % 8 else int(rng.integers(1, 16385))
    K = 128 * int(rng.integers(1, 113)) if i % 5 else 16 * int(rng.integers(1, 897))
    return M, N, K


def make_cases():
    """{"qbits": [[M, N, K, bits, group_size, dtype]], "qbytes": [[M, N, K, a_dtype, b_dtype, out_dtype]]}"""
    import numpy as np

    rng = np.random.default_rng(SEED)
    qbits, qbytes = [], []
    for i in range(CASES):
        M, N, K = _mnk(rng, i)
        bits = 2 if i % 7 == 3 else 4
        gs = (128, 128, 128, 64, 128, 32, 0, 128, 96, 128, 64)[i % 11]
        if gs == 96:
            K = 96 * int(rng.integers(1, 150))
        dtype = (BF16, F16, BF16, F32, BF16, F16, I8, BF16, F32, F16)[i % 10] if i % 13 else BF16
        if i % 6 == 1:  # the register-streaming kernel's corner: decode batches of a small int4 g128 weight
            M, N, K, bits, gs, dtype = int(rng.integers(5, 17)), 16 * int(rng.integers(1, 257)), 128 * int(rng.integers(1, 33)), 4, 128, (BF16, F16)[i % 2]
        qbits.append([M, N, K, bits, gs, dtype])
    for i in range(CASES):
        M, N, K = _mnk(rng, i)
        if i % 4 == 1:
            K = 64 * int(rng.integers(1, 225))
        triple = TRIPLES[i % len(TRIPLES)]
        if i % 3 == 2:  # where the kernels split K (and want a workspace): few output tiles, a long K, formats the split kernels serve
            M, N, K, triple = int(rng.integers(3, 513)), 64 * int(rng.integers(1, 65)), 1024 * int(rng.integers(2, 15)), TRIPLES[i % 10]
        qbytes.append([M, N, K, *triple])
    return {"qbits": qbits, "qbytes": qbytes}


def _child(lib_path):
    """stdin: the cases; stdout: {"qbits": {"plan": [...], "pick": [...], "size": [...]}, "qbytes": {... "q_plan": [...]}}; a plan is its status when
    that is not OK, else [kernel, workspace bytes]."""
    assert not any(k.startswith("QUANTO_HIP_") for k in os.environ)
    cases = json.load(sys.stdin)
    lib = ctypes.CDLL(lib_path)
    i64, i32 = ctypes.c_int64, ctypes.c_int
    out_ptrs = [ctypes.POINTER(i32), ctypes.POINTER(i64)]
    out = {}
    for product, ints in (("qbits", 3), ("qbytes", 3)):
        plan, pick, size = (getattr(lib, f"quanto_hip_{product}_mm_{what}") for what in ("plan", "pick", "workspace_size"))
        plan.restype, plan.argtypes = i32, [i64] * 3 + [i32] * (ints + 1) + out_ptrs
        pick.restype, pick.argtypes = i32, [i64] * 3 + [i32] * ints
        size.restype, size.argtypes = i64, [i64] * 3 + [i32] * (ints + 1)
        plans = [plan]
        if product == "qbytes":
            q_plan = lib.quanto_hip_qbytes_mm_q_plan
            q_plan.restype, q_plan.argtypes = plan.restype, plan.argtypes
            plans.append(q_plan)

        def ask(fn, case, kernel):
            k, b = i32(-99), i64(-99)
            st = fn(*case, kernel, ctypes.byref(k), ctypes.byref(b))
            return st if st != OK else [k.value, b.value]

        rows = {"plan": [[ask(plan, c, k) for k in IDS] for c in cases[product]], "pick": [pick(*c) for c in cases[product]],
                "size": [size(*c, AUTO) for c in cases[product]]}
        if product == "qbytes":
            rows["q_plan"] = [[ask(q_plan, c, k) for k in (AUTO, NATIVE8)] for c in cases[product]]
        out[product] = rows
    json.dump(out, sys.stdout)


def answers(lib_path, cases):
    env = {k: v for k, v in os.environ.items() if not k.startswith("QUANTO_HIP_")}
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path], input=json.dumps(cases), capture_output=True, text=True,
                          timeout=120, env=env)
    assert proc.returncode == 0, proc.stderr
    return json.loads(proc.stdout)


def check_coverage(rows):
    """The table is not mostly one answer: every kernel AUTO returns is returned MIN_SEEN times, every kernel of a product is served and refused
    MIN_SEEN times when forced, ids of the other product are EINVAL, a tenth of the plans have a workspace."""
    for product, ids, auto in (("qbits", QBITS_IDS, QBITS_AUTO), ("qbytes", QBYTES_IDS, QBYTES_AUTO)):
        plans = rows[product]["plan"]
        valid = [p for p in plans if isinstance(p[IDS.index(AUTO)], list)]  # the arguments pass the entry's own check
        picked = [p[IDS.index(AUTO)][0] for p in valid]
        seen = {k: picked.count(k) for k in set(picked)}
        assert auto <= set(seen) and all(n >= MIN_SEEN for n in seen.values()), (product, seen)
        for k in ids:
            forced = [p[IDS.index(k)] for p in valid]
            served, refused = sum(isinstance(f, list) for f in forced), forced.count(ENOTSUP)
            if k == NAIVE:  # serves whatever the argument check lets through; that check refuses the int4 product's int8 scale dtype
                assert served == len(valid) and (product == "qbytes" or sum(p[IDS.index(k)] == ENOTSUP for p in plans) >= MIN_SEEN), (product, served)
            else:
                assert served >= MIN_SEEN and refused >= MIN_SEEN, (product, k, served, refused)
            assert all(f[0] == k for f in forced if isinstance(f, list)), (product, k)
        for k in IDS:
            if k != AUTO and k not in ids:
                assert sum(p[IDS.index(k)] == EINVAL for p in plans) >= MIN_SEEN and not any(isinstance(p[IDS.index(k)], list) for p in plans), (product, k)
        ok = [f for p in plans for f in p if isinstance(f, list)]
        assert sum(f[1] > 0 for f in ok) * 10 >= len(ok), (product, len(ok))
    q = [f for p in rows["qbytes"]["q_plan"] for f in p]
    assert sum(isinstance(f, list) for f in q) >= MIN_SEEN and q.count(ENOTSUP) >= MIN_SEEN


def test_the_sweep_covers_every_route_served_and_refused():
    table = json.load(open(TABLE))
    assert table["cases"] == make_cases() and all(len(c) == CASES for c in table["cases"].values())
    assert {c[0] for c in table["cases"]["qbits"]} >= set(M_LIST) and {tuple(c[3:]) for c in table["cases"]["qbytes"]} == set(TRIPLES)
    assert {(c[3], c[4]) for c in table["cases"]["qbits"]} >= {(4, g) for g in (128, 64, 32, 96, 0)} | {(2, 128)}
    assert {c[5] for c in table["cases"]["qbits"]} == {BF16, F16, F32, I8}
    check_coverage(table["rows"])


def test_plans_are_those_of_the_commit_that_recorded_the_table():
    from optimum_quanto_amd.library.hip import quanto_hip

    table = json.load(open(TABLE))
    got = answers(quanto_hip.lib_path, table["cases"])
    for product, want_rows in table["rows"].items():
        assert set(got[product]) == set(want_rows)
        for what, want in want_rows.items():
            wrong = [(c, w, h) for c, w, h in zip(table["cases"][product], want, got[product][what]) if w != h]
            assert not wrong, f"{product} {what}: {len(wrong)} of {len(want)} answers differ from commit {table['commit']}, first {wrong[:2]}"


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        import argparse

        ap = argparse.ArgumentParser()
        ap.add_argument("--record", action="store_true", required=True)
        ap.add_argument("--lib", required=True)
        ap.add_argument("--commit", required=True)
        args = ap.parse_args()
        cases = make_cases()
        rows = answers(os.path.abspath(args.lib), cases)
        check_coverage(rows)
        with open(TABLE, "w") as f:
            json.dump({"commit": args.commit,
                       "what": "per case and product: quanto_hip_<product>_mm_plan for kernel ids -1 .. 11 (status, or [kernel, workspace bytes] when OK), "
                               "_pick, _workspace_size(AUTO); qbytes: quanto_hip_qbytes_mm_q_plan for AUTO and NATIVE8; no QUANTO_HIP_* variable set",
                       "seed": SEED, "cases": cases, "rows": rows}, f, separators=(",", ":"))
            f.write("\n")
        print(f"{TABLE}: {CASES} cases per product, {os.path.getsize(TABLE)} bytes")

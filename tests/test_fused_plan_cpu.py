"""The planner of the two group-fused int4 / int2 GEMMs (csrc/qh_group_fused.h: token tile and K split of the routes mfma_fused4 and a8_fused_*) decides
what it decided before it became one copy.  The workspace size of a split plan is QUANTO_HIP_WS_COUNTER_BYTES + tiles(bm) * S * 512 * bm bytes, so it
exposes (bm, S) whenever S > 1 and is 0 (unsplit) or ENOTSUP otherwise; half of the sweep's M have M % 128 in 1..64, where 64- and 128-token tiles
give different tile counts.  tests/golden/fused_plan_table.json holds the sweep and the answers of the library built from the commit named in its
header - the last one with a planner per unit -, recorded by this file:

    python tests/test_fused_plan_cpu.py --record --lib <libquanto_hip.so of that commit> --commit <its hash>

The answers are computed in a child process, where QUANTO_HIP_EXPERIMENT=1 is set before the library loads and the split knobs are unset, 2 and 4 in
turn (the library reads them on every call once the switch is on).  Needs no device.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "fused_plan_table.json")
F16, BF16, I8, F8_E4M3FN, F8_E5M2 = 1, 2, 3, 5, 6  # quanto_hip_dtype
KERNEL_MFMA_FUSED4 = 8                              # quanto_hip_kernel
MODES = {"unset": None, "split2": "2", "split4": "4"}
KNOBS = ("QUANTO_HIP_FUSED4_SPLIT", "QUANTO_HIP_A8_SPLIT")
SEED, CASES = 20261017, 320
WS_COUNTER_BYTES = 4096  # include/quanto_hip.h


def make_cases():
    """[M, N, K, bits, activation dtype, output dtype]; sizes skewed to the small end, where the planner's choices change."""
    import numpy as np

    rng = np.random.default_rng(SEED)
    cases = []
    for i in range(CASES):
        if i % 2 == 0:
            M = 128 * int(rng.integers(0, 64) if i % 4 else rng.integers(0, 4)) + int(rng.integers(1, 65))  # M % 128 in 1..64
        else:
            M = int(rng.integers(1, 8193) if i % 4 == 1 else rng.integers(1, 513))
        N = 16 * int(rng.integers(1, 1025) if i % 3 == 0 else rng.integers(1, 129))
        K = 128 * int(rng.integers(1, 225) if i % 5 == 0 else 4 * rng.integers(1, 57) if i % 5 == 1 else 4 * rng.integers(1, 15))  # mostly splittable by 4
        cases.append([M, N, K, (4, 2)[(i // 2) % 2], (I8, F8_E4M3FN, F8_E5M2)[i % 3], (BF16, F16)[(i // 3) % 2]])
    return cases


def _child(lib_path):
    """stdin: the cases; stdout: {mode: {"fused4": [...], "a8": [...]}}."""
    assert os.environ.get("QUANTO_HIP_EXPERIMENT") == "1" and not any(k in os.environ for k in KNOBS)
    cases = json.load(sys.stdin)
    lib = ctypes.CDLL(lib_path)
    f4 = lib.quanto_hip_qbits_mm_workspace_size
    f4.restype, f4.argtypes = ctypes.c_int64, [ctypes.c_int64] * 3 + [ctypes.c_int] * 4
    a8 = lib.quanto_hip_qbits_mm_a8_workspace_size
    a8.restype, a8.argtypes = ctypes.c_int64, [ctypes.c_int64] * 3 + [ctypes.c_int] * 4
    out = {}
    for mode, split in MODES.items():
        for k in KNOBS:
            if split is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = split
        out[mode] = {"fused4": [f4(M, N, K, 4, 128, odt, KERNEL_MFMA_FUSED4) for M, N, K, bits, adt, odt in cases],  # the route is int4 only
                     "a8": [a8(M, N, K, bits, 128, adt, odt) for M, N, K, bits, adt, odt in cases]}
    json.dump(out, sys.stdout)


def answers(lib_path, cases):
    env = {k: v for k, v in os.environ.items() if not k.startswith("QUANTO_HIP_")}
    env["QUANTO_HIP_EXPERIMENT"] = "1"
    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path], input=json.dumps(cases), capture_output=True, text=True,
                          timeout=120, env=env)
    assert proc.returncode == 0, proc.stderr
    return json.loads(proc.stdout)


def split_share(rows):
    flat = [v for mode in rows.values() for route in mode.values() for v in route]
    return sum(v > 0 for v in flat) / len(flat)


def test_the_sweep_covers_what_the_planner_depends_on():
    table = json.load(open(TABLE))
    cases = table["cases"]
    assert cases == make_cases() and len(cases) >= 300
    assert all(1 <= M <= 8192 and N % 16 == 0 and 16 <= N <= 16384 and K % 128 == 0 and 128 <= K <= 28672 for M, N, K, *_ in cases)
    assert sum(1 <= M % 128 <= 64 for M, *_ in cases) >= len(cases) // 2  # the byte count tells 64- from 128-token tiles
    assert {(c[3], c[4]) for c in cases} == {(b, a) for b in (2, 4) for a in (I8, F8_E4M3FN, F8_E5M2)} and {c[5] for c in cases} == {BF16, F16}
    assert split_share(table["rows"]) >= 1 / 3  # S > 1 in at least a third of the rows: the table is not mostly zeros
    # a split's bytes are the counters plus whole 64-token partial tiles of 512 lanes x 16 floats
    assert all(v <= 0 or (v - WS_COUNTER_BYTES) % (512 * 64 * 2) == 0 for m in table["rows"].values() for r in m.values() for v in r)


def test_plans_are_those_of_the_commit_that_recorded_the_table():
    from optimum_quanto_amd.library.hip import quanto_hip

    table = json.load(open(TABLE))
    got = answers(quanto_hip.lib_path, table["cases"])
    for mode in MODES:
        for route in ("fused4", "a8"):
            want, have = table["rows"][mode][route], got[mode][route]
            wrong = [(c, w, h) for c, w, h in zip(table["cases"], want, have) if w != h]
            assert not wrong, f"{mode} {route}: {len(wrong)} of {len(want)} plans differ from commit {table['commit']}, first {wrong[:3]}"


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
        share = split_share(rows)
        assert share >= 1 / 3, f"only {share:.2f} of the rows have a split"
        with open(TABLE, "w") as f:
            json.dump({"commit": args.commit,
                       "what": "quanto_hip_qbits_mm_workspace_size(M, N, K, 4, 128, odt, MFMA_FUSED4) and quanto_hip_qbits_mm_a8_workspace_size(M, N, K, "
                               "bits, 128, adt, odt) of that commit's library per case [M, N, K, bits, adt, odt], QUANTO_HIP_EXPERIMENT=1, split knobs "
                               "unset / 2 / 4",
                       "seed": SEED, "cases": cases, "rows": rows}, f, separators=(",", ":"))
            f.write("\n")
        print(f"{TABLE}: {len(cases)} cases x {len(MODES)} modes x 2 routes, {share:.2f} with S > 1")

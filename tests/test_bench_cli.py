"""bench.py's launch contract, exercised where there is no GPU: `--gpus N` without a launcher spawns N ranks itself (r2's
`--gpus` was parsed and never used), the `--full` line stays short enough for the driver's ~8 KB stdout tail, and a plain run
measures the headline alone and can dump what it computed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(*argv, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=600, env=e)


def test_gpus_2_spawns_two_ranks_over_gloo():
    r = _run("--gpus", "2", "--stub", "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 prints ONE line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1 and rec["data"] == "stub"


def test_gpus_8_stub_spawns_eight_ranks():
    """What the driver does on an 8-GPU node, without the GPUs: eight ranks over gloo, barrier + max-over-ranks timing, ONE line from rank 0."""
    r = _run("--gpus", "8", "--stub", "--steps", "2", "--warmup", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 8


def test_gpus_2_without_a_device_reaches_the_process_group_then_fails_loudly():
    r = _run("--gpus", "2", "--steps", "1", "--warmup", "0")
    if r.returncode == 0:  # a box with two GPUs: the real thing ran
        assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["n_gpus"] == 2
        return
    assert "needs a ROCm device" in r.stderr  # both ranks were started and initialised; no silent single-rank run, no CPU fallback


def test_launcher_and_flag_must_agree():
    r = _run("--gpus", "2", "--stub", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 2" in r.stderr


def test_default_line_fits_the_driver_tail():
    import bench

    def fake(name):
        kind, M, K, N, desc = bench.WORKLOADS[name]
        flops, nbytes = bench.algorithmic_work(kind, M, K, N)
        roof = {"bound": "hbm", "achieved": 1234.5, "peak": 8000.0, "unit": "GB/s", "frac": 0.1543, "traffic": 123456789, "kernel": "skinny_multi",
                "launch_us": 12.345, "event_us": 12.123, "kernel_us": 10.123, "kernel_us_min": 9.876, "algorithmic_bytes": nbytes,
                "algorithmic_flops": flops}
        cpu = {"kind": "reference", "cores": 128, "path": "int4_generic", "value": 1.23456, "unit": "GB/s", "sample": "full call, 50 timed calls after 3 warm-up",
               "seconds_per_call": 0.123456, "iqr_s": 0.012345, "calls_timed": 50,
               "tinygemm": {"seconds_per_call": 0.000123, "iqr_s": 1e-6, "calls": 200, "value": 123.456, "unit": "GB/s"}}
        return {"metric": "QLinear GEMM GB/s (bf16 x int4 qbits_mm, decode)", "value": 1234.567, "unit": "GB/s", "n_gpus": 1, "steps": 200, "warmup": 5,
                "ms_per_step": 0.01234, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                "config": {"workload": desc, "name": name, "M": M, "K": K, "N": list(N) if isinstance(N, tuple) else N, "weight_buffers_rotated": 58,
                           "launch": "hipGraph replay of the K steps", "clock_ramp_ms": 300.0, "parallelism": "replicas x1 (no data-path collective)"},
                "tflops": 1.234, "gbps": 1234.5, "roofline": roof, "cpu_baseline": cpu, "ref_rocm_us": 123.45}

    def fake_layer(name):
        return {"name": name, "B": 32, "us_per_layer": 123.456, "alg_bytes": 123456789, "GBs": 1234.5, "bound": "hbm", "frac": 0.1234, "kernel_us": 12.345,
                "traffic": 123456789, "cache_resident_us_per_layer": 123.456}

    out = fake("cfg2")
    out["cpu_baseline"]["how"] = "x" * 160
    out["sub_results"] = [fake_layer(n) if n in bench.LAYER_WORKLOADS else bench.compact(fake(n)) for n in bench.DEFAULT_SUB]
    for sr in out["sub_results"]:
        bench.apply_profile(sr, {"kernel_us": 12.345, "kernel_us_min": 11.234, "traffic": 123456789}, compacted=True)
        assert "kernel_us_min" not in sr
        if sr["name"] == "int4_decode32":
            sr["ablate_us"] = {label: 12.345 for label, _ in bench.ABLATIONS}
    out["sub_results"].append({"name": "qconv2d_3x3", "shape": "(8,128,28,28)->128 3x3 pad 1", "M": 6272, "K": 1152, "N": 128, "alg_flops": 1849688064,
                               "kernel_us": 12.345, "traffic": 123456789, "int8_us": 12.34, "int8_kernel": "conv2d_mfma_rows",
                               "int8_alg_bytes": 3358976, "int8_frac_mfma": 0.0299, "int8_frac_hbm": 0.0123, "ref_rocm_int8_us": 12.34, "int4_us": 12.34,
                               "int4_kernel": "conv2d_rows_dequant_int4", "int4_alg_bytes": 3358976, "int4_frac_mfma": 0.0299, "int4_frac_hbm": 0.0123,
                               "ref_rocm_int4_us": 12.34, "dw_kernel": "conv2d_depthwise", "dw_us": 12.34, "ref_rocm_dw_us": 12.34, "dw_frac_hbm": 0.1234})
    out["sub_results"].append({"name": "cfg5", "prompt": 512, "new_tokens": 512, "fused_groups": 64, "build_s": 12.3, "int4_bytes_per_token": 3706716160,
                               "b1_tok_s": 123.4, "b1_ms_per_token": 12.345, "b32_tok_s": 1234.5, "b32_ms_per_token": 12.345,
                               "graph_b1_tok_s": 123.4, "graph_b1_ms_per_token": 12.345, "graph_b1_prefill_warmup_capture_ms": 123.4,
                               "graph_b32_tok_s": 1234.5, "graph_b32_ms_per_token": 12.345, "graph_b32_prefill_warmup_capture_ms": 123.4,
                               "b1_qh_kernel_ms_per_token": 1.234, "b32_qh_kernel_ms_per_token": 1.234,
                               "host_us_per_call": {"module": 12.3, "F_linear": 12.3, "op": 12.3, "binding": 12.3, "c_entry": 12.3}})
    out["profile_passes"] = {"ok": True, "seconds": 123.4, "trace_floor_us": 2.0, "what": "x" * 90}
    line = json.dumps(out, separators=(",", ":"))
    assert len(line) < 7200, len(line)  # the driver keeps an 8 KB stdout tail (r6 visit 10: the real line had reached 8,019 bytes; records slimmed)
    for sr in out["sub_results"]:  # enough to recompute every fraction from the line alone (alg_flops = 2 M sum(N) K)
        if sr["name"] in bench.WORKLOADS:
            assert {"name", "M", "K", "N", "us_per_step", "kernel_us", "frac", "alg_bytes", "kernel", "traffic", "cpu_s"} <= set(sr)
    assert {"northstar", "cfg3", "cfg4", "cfg4_fp8a8", "w8a8", "fp8a8", "w8a8_down512", "w4a8", "int4_prefill", "layer_decode_b1", "layer_decode_b32",
            "cfg5"} <= {sr["name"] for sr in out["sub_results"]}


def test_world_size_from_the_launcher_is_enough():
    """`torchrun --nproc-per-node N bench.py` without --gpus: the flag defaults to WORLD_SIZE (r3 exited on the mismatch)."""
    r = _run("--stub", "--steps", "2", "--warmup", "0", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 0, r.stderr[-1500:]
    assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["n_gpus"] == 1


def test_plain_run_options_are_there():
    r = _run("--help")
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = _run("--stub", "--dump-outputs", "unused")
    assert r.returncode != 0 and "--dump-outputs" in r.stderr


def _tensors(v):
    """The tensors of a nested (x, sets) structure, in order."""
    return [t for u in v for t in _tensors(u)] if isinstance(v, (list, tuple)) else [v]


def test_bench_inputs_repeat_for_the_same_arguments():
    """--dump-outputs compares two builds output for output: the inputs of a workload must be the same from run to run."""
    import torch

    import bench

    for name in ("cfg2", "northstar", "qkv_fused", "w8a8", "w4a8_512"):
        kind, M, K, N, _ = bench.WORKLOADS[name]
        M, K = min(M, 16), min(K, 256)
        N = tuple(min(n, 64) for n in N) if isinstance(N, tuple) else min(N, 64)
        a, b = (_tensors(bench.build_inputs(kind, M, K, N, torch.device("cpu"), 2, seed=1234)) for _ in range(2))
        assert len(a) == len(b) and all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, b)), name


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    import numpy as np
    import torch

    import bench

    assert bench.dump_rows(64, 32, 1 << 20) is None  # small enough: every row
    rows = bench.dump_rows(4096, 4096, bench.DUMP_BYTES)
    assert rows is not None and len(rows) * 4096 * 4 <= bench.DUMP_BYTES and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, bench.dump_rows(4096, 4096, bench.DUMP_BYTES))
    y = torch.arange(4096 * 4096, dtype=torch.float32).reshape(4096, 4096)
    bench.dump_outputs(str(tmp_path / "one"), [y])
    a = np.load(tmp_path / "one" / "y.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y.numpy()[rows])
    assert (tmp_path / "one" / ".gitignore").read_text() == "*\n"  # a dump directory made inside a checkout leaves git status clean
    bench.dump_outputs(str(tmp_path / "two"), [y[:8], y[8:16, :100]])
    assert np.array_equal(np.load(tmp_path / "two" / "y0.npy"), y[:8].numpy()) and np.load(tmp_path / "two" / "y1.npy").shape == (8, 100)


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_for_and_dumps_the_headline_output(tmp_path):
    """A plain run: the headline alone (no sub_results, CPU baseline or reference timing), K = --steps timed steps, and --dump-outputs writes
    the last step's output, whose sampled rows are the product of the seeded inputs."""
    import numpy as np
    import torch

    import bench
    from helpers import assert_close_to_exact
    from oracle import quanto_oracle as O

    r = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["unit"] == "TFLOP/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert not {"sub_results", "cpu_baseline", "ref_rocm_us", "profile_passes"} & set(rec)
    y = np.load(tmp_path / "y.npy")
    kind, M, K, N, _ = bench.WORKLOADS["cfg2"]
    rows = bench.dump_rows(M, N, bench.DUMP_BYTES)
    assert y.dtype == np.float32 and y.shape == (len(rows), N) and y.nbytes <= 64 << 20
    x, sets = bench.build_inputs(kind, M, K, N, torch.device("cuda"), 1, seed=1234)
    w, scale = sets[0]
    pick = [0, len(rows) // 2, len(rows) - 1]
    xs = x[torch.as_tensor(rows[pick], device=x.device)].float().cpu().numpy()
    want = O.qbytes_mm_exact(xs, w.cpu().numpy(), scale.float().cpu().numpy().reshape(-1))
    assert_close_to_exact(y[pick], want, "bf16", "bench.py --dump-outputs, cfg2")

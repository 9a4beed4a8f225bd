"""``oracle/reference_cpu_path.py`` - what bench.py's cpu_baseline times - is the reference's CPU QLinear path, call for call.

The reference's outputs on fixed tensors are stored in ``tests/golden/reference_cpu_path.npz`` (``tests/golden/make_cpu_path_golden.py``
writes them from a reference checkout); the restatement must reproduce every one of them bit for bit.  Host threads are pinned to one
while it runs, as they were when the vectors were written, so that the ATen reductions run in the same order."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_cpu_path.npz")


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_reference_cpu_path_restatement_equals_the_reference(one_thread):
    from oracle import reference_cpu_path as R

    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}

    def t(key, dt=None):
        a = torch.from_numpy(g[key])
        if dt == torch.float8_e4m3fn:
            return a.view(torch.float8_e4m3fn)
        return a if dt is None else a.to(dt)

    def same(got, key):
        want = torch.from_numpy(g[key])
        got = got.view(torch.uint8) if got.dtype == torch.float8_e4m3fn else got
        assert got.shape == want.shape and torch.equal(got.to(want.dtype), want), key

    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x, bias = t(f"{name}/x", dt), t(f"{name}/bias", dt)
        with torch.no_grad():
            # 8-bit: int8 (bf16 takes _weight_int8pack_mm, fp32 the generic path) and fp8
            for key, wdt in (("q8", None), ("f8", torch.float8_e4m3fn)):
                data, scale = t(f"{name}/{key}/data", wdt), t(f"{name}/{key}/scale", dt)
                same(R.qbytes_linear(x, data, scale, bias), f"{name}/{key}/linear")
                same(R.qbytes_mm_cpu(x, data, scale), f"{name}/{key}/mm")
            # int8 x int8
            same(R.qbytes_mm_cpu(t(f"{name}/i8i8/a"), t(f"{name}/q8/data"), t(f"{name}/i8i8/scale", dt)), f"{name}/i8i8/mm")
            # int4 generic class
            packed, scale, shift = t(f"{name}/q4/packed"), t(f"{name}/q4/scale", dt), t(f"{name}/q4/shift", dt)
            same(R.dequantize_qbits(packed, scale, shift, 4, 128, 96, 256), f"{name}/q4/dequantized")
            same(R.qbits_linear_generic(x, packed, scale, shift, 4, 128, 96, 256, bias), f"{name}/q4/linear")
            # int4 optimized class on CPU: TinyGemm when the scales are bf16
            if dt == torch.bfloat16:
                data, scale_shift = R.tinygemm_pack(packed, scale, shift, 128, 96, 256)
                same(data, f"{name}/tinygemm/data")
                same(scale_shift, f"{name}/tinygemm/scale_shift")
                same(R.tinygemm_linear(x, data, 128, scale_shift, 96, bias), f"{name}/tinygemm/linear")

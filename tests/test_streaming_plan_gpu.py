"""The rungs of the streaming decode kernels' host plans (csrc/qbits_skinny.hip, csrc/qbytes_skinny.hip) that the parity files do not reach: the deep
DMA rings behind QUANTO_HIP_SKINNY_LDS_KB and the unsplit run of a shape that asks for a split when the caller of the C entry brings no workspace.
Smallest shapes per rung, against exact (float64) math; the other rungs - token fragments, block widths, wave sets, group sizes, int2, passes of 64
rows, the multi launches - are driven by test_hip_parity.py and test_multi_linear.py.
"""
import numpy as np
import pytest
import torch

from optimum_quanto_amd.library.hip import KERNEL_SKINNY, quanto_hip
from oracle import quanto_oracle as O

from helpers import assert_close_to_exact, fp8_tensor, make_qbits_problem, make_qbytes_problem, to_numpy, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT_CODE = {"fp16": 1, "bf16": 2}
KIND_CODE = {None: 3, "e4m3fn": 5, "e5m2": 6}


def _qbits(p, N, K, dt):
    lib = quanto_hip.lib
    y = lib.qbits_mm(to_torch(p["x"], dt, DEV), torch.from_numpy(p["packed"]).to(DEV), to_torch(p["scale"], dt, DEV), to_torch(p["shift"], dt, DEV), None,
                     4, 128, N, K, kernel="skinny")
    assert lib.last_kernel() == "skinny"
    return to_numpy(y)


@pytest.mark.parametrize("M", [5, 17, 33, 65])
def test_deep_rings_behind_the_lds_knob(M, monkeypatch):
    """100 KiB per block: int4 on 4 waves plans 8 stages for one and two fragments (M = 5, 17) and stays at 4 for four (M = 33: six stages would need
    122 KiB); 8-bit 8 / 8 / 6 stages; M = 65: the short second pass plans its own ring.  The ABI does not report the ring depth, so this test holds that
    the deep-ring instantiations compute the right product when the knob is set; WHICH instantiation ran is in the kernel names of
    profiles/streaming_plan_dispatches.jsonl (scripts/streaming_dispatches.py sets the same knob)."""
    monkeypatch.setenv("QUANTO_HIP_SKINNY_LDS_KB", "100")
    N, K, dt = 64, 1024, "bf16"
    p = make_qbits_problem(M, N, K, dt, seed=M)
    assert_close_to_exact(_qbits(p, N, K, dt), O.qbits_mm_exact(p["x"], p["packed"], 4, p["scale"], p["shift"], 128, N, K), dt, f"int4 deep ring M={M}")
    q = make_qbytes_problem(M, N, K, dt, None, seed=M)
    y = quanto_hip.lib.qbytes_mm(to_torch(q["x"], dt, DEV), torch.from_numpy(q["data"]).to(DEV), to_torch(q["scale"], dt, DEV), kernel="skinny")
    assert quanto_hip.lib.last_kernel() == "skinny"
    assert_close_to_exact(to_numpy(y), O.qbytes_mm_exact(q["x"], q["data"], q["scale"]), dt, f"int8 deep ring M={M}")


@pytest.mark.parametrize("M", [5, 33])
def test_a_split_shape_without_a_workspace_runs_unsplit(M):
    """(M, 128, 2048) asks for a split of 2 (16 tiles, 2 feature blocks); the C entries run it with one block per feature block when handed none."""
    N, K, dt = 128, 2048, "fp16"
    c, code = quanto_hip.cdll, DT_CODE[dt]
    stream = torch.cuda.current_stream().cuda_stream
    assert c.quanto_hip_qbits_mm_workspace_size(M, N, K, 4, 128, code, KERNEL_SKINNY) > 0
    p = make_qbits_problem(M, N, K, dt, seed=M)
    x, w, s, z = to_torch(p["x"], dt, DEV), torch.from_numpy(p["packed"]).to(DEV), to_torch(p["scale"], dt, DEV), to_torch(p["shift"], dt, DEV)
    y = torch.empty((M, N), dtype=x.dtype, device=DEV)
    st = c.quanto_hip_qbits_mm(x.data_ptr(), w.data_ptr(), s.data_ptr(), z.data_ptr(), 0, y.data_ptr(), M, N, K, 4, 128, code, code, KERNEL_SKINNY, 0, 0, stream)
    assert st == 0
    assert_close_to_exact(to_numpy(y), O.qbits_mm_exact(p["x"], p["packed"], 4, p["scale"], p["shift"], 128, N, K), dt, f"int4 unsplit M={M}")
    for kind in (None, "e4m3fn"):
        assert c.quanto_hip_qbytes_mm_workspace_size(M, N, K, code, KIND_CODE[kind], code, KERNEL_SKINNY) > 0
        q = make_qbytes_problem(M, N, K, dt, kind, seed=M)
        b = fp8_tensor(q["data"], kind, DEV) if kind else torch.from_numpy(q["data"]).to(DEV)
        a, sc = to_torch(q["x"], dt, DEV), to_torch(q["scale"], dt, DEV)
        y = torch.empty((M, N), dtype=a.dtype, device=DEV)
        st = c.quanto_hip_qbytes_mm_ws(a.data_ptr(), b.data_ptr(), sc.data_ptr(), 0, y.data_ptr(), M, N, K, code, KIND_CODE[kind], code, KERNEL_SKINNY, 0, 0, stream)
        assert st == 0
        assert_close_to_exact(to_numpy(y), O.qbytes_mm_exact(q["x"], q["data"], q["scale"], kind), dt, f"8-bit {kind} unsplit M={M}")

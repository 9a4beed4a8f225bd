"""W2A8 and e5m2 activations on the 8-bit matrix kernel (csrc/qbits_a8_fused.hip): what the C entry serves, checked on the host (library loaded, no
device call).  The int4 x int8 / e4m3 plans stay what they were; int2 weights and e5m2 activations are served at group size 128 and refused elsewhere."""
import ctypes

import pytest

from optimum_quanto_amd.library.hip import F8_E4M3FN, F8_E5M2, F16, I8, BF16, quanto_hip

ENOTSUP = -2


@pytest.fixture(scope="module")
def ws():
    lib = quanto_hip.cdll
    f = lib.quanto_hip_qbits_mm_a8_workspace_size
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int64] * 3 + [ctypes.c_int] * 4
    return f


@pytest.mark.parametrize("bits,adt", [(2, I8), (2, F8_E4M3FN), (2, F8_E5M2), (4, F8_E5M2)])
@pytest.mark.parametrize("M,N,K", [(512, 4096, 4096), (65, 128, 256), (2048, 14336, 4096), (300, 512, 128)])
def test_new_formats_are_served(ws, bits, adt, M, N, K):
    for dt in (BF16, F16):
        assert ws(M, N, K, bits, 128, adt, dt) >= 0


@pytest.mark.parametrize("M,N,K", [(512, 4096, 4096), (96, 256, 2048), (130, 1024, 4096)])
def test_int2_and_e5m2_plan_like_int4(ws, M, N, K):
    """Same output tiles (128 features x the token tile) and the same time model: the same K split, hence the same scratch size."""
    want = ws(M, N, K, 4, 128, I8, BF16)
    assert want >= 0
    assert ws(M, N, K, 2, 128, I8, BF16) == want
    assert ws(M, N, K, 2, 128, F8_E5M2, BF16) == want
    assert ws(M, N, K, 4, 128, F8_E5M2, BF16) == want


@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("adt", [I8, F8_E4M3FN, F8_E5M2])
def test_group_size_other_than_128_is_refused(ws, bits, adt):
    assert ws(512, 4096, 4096, bits, 64, adt, BF16) == ENOTSUP
    assert ws(512, 4096, 4096, bits, 256, adt, BF16) == ENOTSUP


def test_int2_needs_n_multiple_of_16(ws):
    """int2: N / 4 packed rows per plane, a multiple of 4 (each lane stores four consecutive features of one plane at once); int4 keeps N % 8."""
    assert ws(512, 520, 1024, 4, 128, I8, BF16) >= 0
    assert ws(512, 520, 1024, 2, 128, I8, BF16) == ENOTSUP
    assert ws(512, 528, 1024, 2, 128, I8, BF16) >= 0


def test_python_side_takes_e5m2_activations():
    import torch

    assert torch.float8_e5m2 in quanto_hip.lib.A8_DTYPES
    assert quanto_hip.lib.qbits_mm_a8_workspace(512, 4096, 4096, 2, 128, torch.float8_e5m2, torch.bfloat16) >= 0

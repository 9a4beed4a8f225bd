"""QConv2d with quantized activations (csrc/qconv_a8.hip): the C ABI, the workspace query and the op's default, without a device."""
import ctypes
import os
import re

import pytest
import torch

import optimum_quanto_amd  # noqa: F401  (registers the quanto:: ops)
from optimum_quanto_amd.library.hip import quanto_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quanto_hip.h")

F32, F16, BF16, I8, U8, E4M3, E5M2, FNUZ = 0, 1, 2, 3, 4, 5, 6, 7
OK, EINVAL, ENOTSUP = 0, -1, -2
SERVED = [(I8, I8), (E4M3, E4M3), (E4M3, E5M2), (E5M2, E4M3), (E5M2, E5M2), (E4M3, I8), (E5M2, I8)]
SYMBOLS = ("quanto_hip_qbytes_conv2d_a8", "quanto_hip_qbytes_conv2d_a8_workspace_size")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(quanto_hip.lib_path):
        pytest.fail(f"{quanto_hip.lib_path} missing: run __graft_entry__.build() first")
    c = ctypes.CDLL(quanto_hip.lib_path)
    f = c.quanto_hip_qbytes_conv2d_a8_workspace_size
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int64] * 9 + [ctypes.c_int] * 9
    return c


def _ws(lib, a, b, o, B=8, cin=128, H=28, W=28, OC=128, KH=3, KW=3, OH=None, OW=None, s=(1, 1), p=(1, 1), d=(1, 1)):
    if OH is None:
        OH = (H + 2 * p[0] - d[0] * (KH - 1) - 1) // s[0] + 1
    if OW is None:
        OW = (W + 2 * p[1] - d[1] * (KW - 1) - 1) // s[1] + 1
    return lib.quanto_hip_qbytes_conv2d_a8_workspace_size(B, cin, H, W, OC, KH, KW, OH, OW, s[0], s[1], p[0], p[1], d[0], d[1], a, b, o)


def test_header_declares_and_library_exports_the_a8_conv_entries(lib):
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), f"{name} not declared in include/quanto_hip.h"
        assert hasattr(lib, name), f"{name} not exported by the library"


@pytest.mark.parametrize("out", [F32, F16, BF16])
@pytest.mark.parametrize("a,b", SERVED)
def test_workspace_query_serves_every_format_pair(lib, a, b, out):
    assert _ws(lib, a, b, out) >= 0
    # a grid that cannot fill the chip is split (RGB-stem-free, K = 4608): non-zero scratch, a multiple of one 128 x 128 tile of 4-byte sums
    split = _ws(lib, a, b, out, B=1, cin=512, H=7, W=7, OC=512)
    assert split > 0 and split % (128 * 128 * 4) == 0
    assert _ws(lib, a, b, out, B=0) == 0  # empty batch: nothing to split


@pytest.mark.parametrize("a,b,out", [(FNUZ, FNUZ, BF16), (FNUZ, I8, BF16), (I8, FNUZ, BF16), (E4M3, FNUZ, F16), (FNUZ, E4M3, F32),
                                     (I8, E4M3, BF16), (I8, E5M2, F16), (I8, I8, I8), (E4M3, E4M3, U8), (U8, I8, BF16), (BF16, I8, BF16)])
def test_workspace_query_refuses_unserved_formats(lib, a, b, out):
    assert _ws(lib, a, b, out) == ENOTSUP


def test_workspace_query_rejects_inconsistent_geometry(lib):
    assert _ws(lib, I8, I8, BF16, OH=27) == EINVAL
    assert _ws(lib, I8, I8, BF16, OW=29) == EINVAL
    assert _ws(lib, I8, I8, BF16, s=(0, 1), OH=28, OW=28) == EINVAL
    assert _ws(lib, I8, I8, BF16, KH=0) == EINVAL


def test_workspace_query_geometry_limits(lib):
    assert _ws(lib, I8, I8, BF16, KH=11, KW=11, p=(5, 5)) >= 0  # 121 taps
    assert _ws(lib, I8, I8, BF16, KH=12, KW=11, p=(5, 5)) == ENOTSUP  # 132 taps
    assert _ws(lib, I8, I8, BF16, B=8, cin=3, H=224, W=224, OC=64, KH=7, KW=7, s=(2, 2), p=(3, 3)) >= 0  # RGB stem, K = 147


def _qact(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if dtype == torch.int8:
        return torch.randint(-127, 128, shape, generator=g, dtype=torch.int8)
    return x.clamp(-8, 8).to(dtype)


@pytest.mark.parametrize("xdt,wdt,dt", [(torch.int8, torch.int8, torch.float32), (torch.float8_e4m3fn, torch.float8_e5m2, torch.float32),
                                        (torch.float8_e5m2, torch.int8, torch.float32), (torch.int8, torch.int8, torch.bfloat16)])
@pytest.mark.parametrize("bias", [False, True])
def test_op_default_is_conv2d_on_dequantized_tensors(xdt, wdt, dt, bias):
    assert hasattr(torch.ops.quanto, "qbytes_conv2d_a8")
    x = _qact((2, 5, 9, 11), xdt, 1)
    w = _qact((7, 5, 3, 3), wdt, 2)
    xs = torch.tensor([0.0125], dtype=dt)
    ws = (torch.rand(7, 1, 1, 1, generator=torch.Generator().manual_seed(3)) * 0.01 + 0.001).to(dt)
    b = torch.randn(7).to(dt) if bias else None
    y = torch.ops.quanto.qbytes_conv2d_a8(x, xs, w, ws, b, [2, 1], [1, 0], [1, 2])
    want = torch.nn.functional.conv2d(x.to(dt) * xs, w.to(dt) * ws, b, (2, 1), (1, 0), (1, 2))
    assert y.dtype == dt and torch.equal(y, want)

"""``quanto::qbytes_bmm`` without a device: the op and its default (the two statements the aten.bmm handler of quantized activations ran), the
handler's routing, the C entry's argument checks, the route predicate, and the build rule of csrc/qbytes_bmm.hip (-fno-slp-vectorize: no packed
fp32 next to the MFMAs, profiles/r05_packed_fp32_op_sel_next_to_mfma.md)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from optimum_quanto_amd.library import hip as hip_mod
from optimum_quanto_amd.library import ops as ops_mod
from optimum_quanto_amd.library.hip import BF16, F16, F32, I8, quanto_hip
from optimum_quanto_amd.tensor import absmax_scale, qfloat8, qint8, quantize_activation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimum_quanto_amd", "csrc")
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
OK, EINVAL, ENOTSUP = 0, -1, -2  # QUANTO_HIP_* (include/quanto_hip.h)


def _former_statements(a, b, scale, out_dtype):
    """What ``_h_bmm`` ran before the op existed (tensor/activations/qbytes_ops.py:175-186)."""
    out = torch.bmm(a.to(torch.float32), b.to(torch.float32))
    return (out * scale).to(out_dtype)


def _codes(gen, *shape):
    return torch.randint(-128, 128, shape, dtype=torch.int8, generator=gen)


def _quantized(gen, shape, dtype=torch.float32, qtype=qint8):
    t = torch.randn(shape, generator=gen).to(dtype)
    return quantize_activation(t, qtype=qtype, scale=absmax_scale(t, qtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_the_op_exists_and_its_default_is_the_former_two_statements(dtype):
    gen = torch.Generator().manual_seed(0)
    for B, M, N, K in [(1, 1, 1, 1), (3, 7, 5, 9), (2, 33, 65, 130), (4, 24, 24, 32), (1, 5, 3, 1500)]:
        a, b = _codes(gen, B, M, K), _codes(gen, B, K, N)
        scale = (torch.rand((), generator=gen) * 1e-3).to(dtype).to(torch.float32)
        got = torch.ops.quanto.qbytes_bmm(a, b, scale, dtype)
        assert got.dtype == dtype and got.shape == (B, M, N)
        assert torch.equal(got, _former_statements(a, b, scale, dtype))
        # the transposed view of the second operand as well
        bt = b.transpose(1, 2).contiguous().transpose(1, 2)
        assert torch.equal(torch.ops.quanto.qbytes_bmm(a, bt, scale, dtype), got)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_matmul_on_two_quantized_activations_gives_what_the_former_handler_gave(dtype, monkeypatch):
    calls = []
    op = torch.ops.quanto.qbytes_bmm
    monkeypatch.setattr(torch.ops.quanto, "qbytes_bmm", lambda *args: calls.append(args) or op(*args))
    gen = torch.Generator().manual_seed(1)
    # 3-D, the second operand as a transposed view
    a, b = _quantized(gen, (3, 10, 20), dtype), _quantized(gen, (3, 12, 20), dtype)
    got = torch.matmul(a, b.transpose(1, 2))
    assert type(got) is torch.Tensor and got.dtype == dtype
    assert torch.equal(got, _former_statements(a._data, b._data.transpose(1, 2), (a._scale * b._scale).to(torch.float32), dtype))
    assert len(calls) == 1 and calls[0][1].stride() == (240, 1, 20)  # the view itself reaches the op: K contiguous
    # 4-D attention: q / k made by view + transpose; matmul's reshape hands aten.bmm a contiguous [B, K, N] second operand
    bsz, s, h, d = 2, 6, 4, 8
    q, k = (_quantized(gen, (bsz, s, h * d), dtype).view(bsz, s, h, d).transpose(1, 2) for _ in range(2))
    got = torch.matmul(q, k.transpose(2, 3))
    want = _former_statements(q._data.reshape(bsz * h, s, d), k._data.transpose(2, 3).reshape(bsz * h, d, s), (q._scale * k._scale).to(torch.float32), dtype)
    assert torch.equal(got, want.view(bsz, h, s, s))
    assert len(calls) == 2 and calls[1][1].is_contiguous() and calls[1][1].shape == (bsz * h, d, s)


def test_the_other_branches_of_the_handler_do_not_reach_the_op(monkeypatch):
    calls = []
    op = torch.ops.quanto.qbytes_bmm
    monkeypatch.setattr(torch.ops.quanto, "qbytes_bmm", lambda *args: calls.append(args) or op(*args))
    gen = torch.Generator().manual_seed(2)
    a, b = _quantized(gen, (2, 5, 16)), _quantized(gen, (2, 16, 7))
    x = torch.randn((2, 5, 16), generator=gen)
    assert torch.equal(torch.bmm(x, b), torch.bmm(x, b.dequantize()))  # float x quantized
    assert torch.equal(torch.bmm(a, b.dequantize()), torch.bmm(a.dequantize(), b.dequantize()))  # quantized x float
    a8, b8 = _quantized(gen, (2, 5, 16), qtype=qfloat8), _quantized(gen, (2, 16, 7), qtype=qfloat8)
    assert torch.equal(torch.bmm(a8, b8), torch.bmm(a8.dequantize(), b8.dequantize()))  # fp8 pair: qfallback
    assert torch.equal(torch.bmm(a, b8), torch.bmm(a.dequantize(), b8.dequantize()))
    assert calls == []
    torch.bmm(a, b)
    assert len(calls) == 1


def test_the_library_exports_the_entry_and_the_binding_declares_it():
    assert hasattr(quanto_hip.cdll, "quanto_hip_qbytes_bmm")
    assert "quanto_hip_qbytes_bmm" in hip_mod._PROTOTYPES
    header = open(os.path.join(ROOT, "include", "quanto_hip.h")).read()
    assert re.search(r"\bquanto_hip_qbytes_bmm\(", header)
    assert "tensor/activations/qbytes_ops.py:175-186" in header
    assert callable(quanto_hip.lib.qbytes_bmm)


PTR = 1 << 20  # an aligned address that is never dereferenced: every case below is refused, or done, before a launch
BIG = 1 << 31


def _bmm(a=PTR, w=PTR, scale=PTR, y=PTR, B=2, M=70, N=90, K=80, a_batch=None, a_row=None, w_batch=None, w_k=None, w_n=1, out_dtype=BF16):
    fn = quanto_hip.cdll.quanto_hip_qbytes_bmm
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int64] * 9 + [ctypes.c_int, ctypes.c_void_p]
    a_row = K if a_row is None else a_row
    w_k = N if w_k is None else w_k
    a_batch = M * K if a_batch is None else a_batch
    w_batch = K * N if w_batch is None else w_batch
    return fn(a, w, scale, y, B, M, N, K, a_batch, a_row, w_batch, w_k, w_n, out_dtype, None)


# (what, arguments, status).  A served problem is shown as served by the status of its null output: the last check before the launch.
STATUSES = [
    ("null a", dict(a=None), EINVAL),
    ("null w", dict(w=None), EINVAL),
    ("null scale", dict(scale=None), EINVAL),
    ("null y", dict(y=None), EINVAL),
    ("negative B", dict(B=-1), EINVAL),
    ("negative M", dict(M=-1), EINVAL),
    ("negative N", dict(N=-1), EINVAL),
    ("negative K", dict(K=-1), EINVAL),
    ("negative batch stride of a", dict(a_batch=-1), EINVAL),
    ("negative row stride of a", dict(a_row=-80), EINVAL),
    ("negative batch stride of w", dict(w_batch=-1), EINVAL),
    ("negative k stride of w", dict(w_k=-1), EINVAL),
    ("negative n stride of w", dict(w_n=-1, w_k=1), EINVAL),
    ("a negative size ahead of an unsupported dtype", dict(M=-1, out_dtype=I8), EINVAL),
    ("int8 output", dict(out_dtype=I8), ENOTSUP),
    ("an output dtype that is no dtype", dict(out_dtype=99), ENOTSUP),
    ("neither stride of w is 1", dict(w_k=180, w_n=2), ENOTSUP),
    ("K = 131072", dict(K=131072), ENOTSUP),
    ("K = 131071 is served", dict(K=131071, y=None), EINVAL),
    ("2^31 workgroups: the batch alone", dict(B=BIG, M=1, N=1), ENOTSUP),
    ("2^31 workgroups: 2^25 x 8 x 8 tiles", dict(B=1 << 25, M=449, N=512), ENOTSUP),
    ("2^31 workgroups: the tiles of one member", dict(B=1, M=64 << 16, N=64 << 15), ENOTSUP),
    ("2^31 - 1 workgroups are served", dict(B=BIG - 1, M=64, N=1, y=None), EINVAL),
    ("2^31 - 64 workgroups are served", dict(B=(1 << 25) - 1, M=449, N=512, y=None), EINVAL),
    ("not served, even when empty", dict(B=0, out_dtype=I8), ENOTSUP),
    ("B = 0", dict(B=0), OK),
    ("M = 0", dict(M=0), OK),
    ("N = 0", dict(N=0), OK),
    ("empty, null pointers", dict(B=0, a=None, w=None, scale=None, y=None), OK),
    ("expanded operands (batch strides 0), null y", dict(a_batch=0, w_batch=0, y=None), EINVAL),
    ("K contiguous w, null y", dict(w_k=1, w_n=80, y=None), EINVAL),
    ("the three float outputs", dict(out_dtype=F32, y=None), EINVAL),
    ("the three float outputs", dict(out_dtype=F16, y=None), EINVAL),
    ("K = 0 reads neither a nor w, null y", dict(K=0, a=None, w=None, y=None), EINVAL),
]


def test_the_entry_validates_its_arguments_before_any_hip_call():
    for what, args, status in STATUSES:
        assert _bmm(**args) == status, what


def test_route_predicate_truth_table():
    takes = ops_mod._bmm_kernel_takes
    z = lambda *shape, dtype=torch.int8: torch.zeros(shape, dtype=dtype)  # noqa: E731
    one = torch.ones((), dtype=torch.float32)
    assert takes(z(2, 3, 4), z(2, 4, 5), one, torch.bfloat16)
    assert takes(z(2, 3, 4), z(2, 5, 4).transpose(1, 2), one, torch.float16)
    assert takes(z(2, 3, 4), z(2, 4, 10)[..., ::2], one, torch.float32)  # the binding copies it
    assert takes(z(2, 3, 4), z(1, 4, 5).expand(2, 4, 5), torch.ones(1, 1, 1), torch.float32)
    assert takes(z(1, 1, 131071), z(1, 131071, 1), one, torch.float32)
    assert not takes(z(1, 1, 131072), z(1, 131072, 1), one, torch.float32)
    assert not takes(z(2, 3, 4), z(2, 4, 5), torch.ones(1, 1, 5), torch.float32)  # a per-axis scale
    for f8 in (torch.float8_e4m3fn, torch.float8_e5m2):
        assert not takes(z(2, 3, 4, dtype=f8), z(2, 4, 5, dtype=f8), one, torch.float32)
        assert not takes(z(2, 3, 4), z(2, 4, 5, dtype=f8), one, torch.float32)
    assert not takes(z(3, 4), z(4, 5), one, torch.float32)  # 2-D operands
    assert not takes(z(2, 3, 4), z(4, 5), one, torch.float32)
    assert not takes(z(2, 3, 4), z(2, 4, 5), one, torch.float64)
    assert not takes(z(2, 3, 4), z(2, 4, 5, dtype=torch.uint8), one, torch.float32)
    assert not takes(z(2, 3, 4), z(3, 4, 5), one, torch.float32)  # sizes that do not match: torch.bmm's error, from the default
    # the launch's 2^31 workgroups (shapes only: meta tensors)
    m = lambda *shape: torch.empty(shape, dtype=torch.int8, device="meta")  # noqa: E731
    assert takes(m((1 << 31) - 1, 1, 1), m((1 << 31) - 1, 1, 1), one, torch.float32)
    assert not takes(m(1 << 31, 1, 1), m(1 << 31, 1, 1), one, torch.float32)


def test_the_cpu_route_of_what_the_predicate_refuses_is_the_default():
    gen = torch.Generator().manual_seed(3)
    a, b = _codes(gen, 2, 3, 4), _codes(gen, 2, 4, 5)
    scale = torch.rand((1, 1, 5), generator=gen)
    assert torch.equal(torch.ops.quanto.qbytes_bmm(a, b, scale, torch.float32), _former_statements(a, b, scale, torch.float32))


@pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")
def test_the_unit_is_built_without_packed_fp32_next_to_its_mfmas():
    proc = subprocess.run(["make", "-C", CSRC, "build/qbytes_bmm.s"], capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    text = open(os.path.join(CSRC, "build", "qbytes_bmm.s")).read()
    assert "v_mfma_i32_16x16x64_i8" in text
    packed = [ln.strip() for ln in text.splitlines() if re.search(r"\bv_pk_(add|mul|fma)_f32\b", ln)]
    assert not packed, f"hipcc packed the epilogue's fp32 math ({len(packed)} v_pk_*_f32): is -fno-slp-vectorize still applied?"
    # the product is rounded to fp32 before it is rounded to fp16: no fused multiply-and-convert (one rounding) in the epilogue
    assert not re.search(r"\bv_(fma|mad)_mix", text) and "v_cvt_f16_f32" in text
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^build/qbytes_bmm\.o: CXXFLAGS \+= -fno-slp-vectorize$", make, re.M)
    assert "qbytes_bmm.hip" in re.search(r"^SRCS\s*=\s*(.+)$", make, re.M).group(1).split()

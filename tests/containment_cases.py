"""The case table of the containment tests (tests/test_containment_cpu.py, tests/test_containment_gpu.py): one row per route of a C entry of
include/quanto_hip.h that stores into caller memory, at the smallest shape at which the route has a ragged tail.

A row holds: the entry, the forced ``quanto_hip_kernel`` (or AUTO), the shape, the formats, the ``QUANTO_HIP_*`` knobs, the ``quanto_hip_last_kernel()``
name expected (None: the entry reports none), whether the plan is expected to split K (``split``: None for a family that cannot) and whether the call needs
scratch for another reason (``scratch``: row sums, a dequantized weight).  ``counters`` marks the rows whose workspace falls under the counter contract of the
header ([QUANTO_HIP_WS_COUNTER_BYTES of arrival counters, zero on entry and restored to zero | partial sums never read before they are written]).

Every row calls the C ABI through ``quanto_hip.lib._c`` with pointers into a ``containment.Arena``: the test owns the output and the workspace.  Per entry a
``Family`` gives the plan (host only, "needs no device"), the problem (host tensors, the outputs' types and the oracle gate the route already has elsewhere in
the suite - no tolerance is defined here) and the call (a ``bias`` region - ``bias0`` ... for the multi entries - is passed where the arena has one: the
problems of this file have none, tests/exact_cases.py adds them).

Shapes follow the support rules in csrc/: M and N are no multiples of the 64 / 128 / 256 tiles where the rule allows it and the smallest legal multiple plus
one unit where it does not; K is two to twelve K-tiles.  Where a convolution row forces a K split its K has that many K-tiles (a forced split is clamped to
the K-tiles there are: 64 k per tile for 16-bit activations, 128 for 8-bit codes), with an odd channel count where the route allows one.
"""
import ctypes
import functools
import os
import re
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from helpers import (BF16, E4M3, E4M3FNUZ, E5M2, F16, F32, I8, TORCH_DT, assert_close_to_exact, make_qbits_problem, make_qbytes_problem, to_numpy,
                     to_torch)
from optimum_quanto_amd.library import ops
from optimum_quanto_amd.library.hip import quanto_hip
from optimum_quanto_amd.tensor.packing import pack_weights
from oracle import quanto_oracle as O

OK, EINVAL, ENOTSUP = 0, -1, -2
AUTO, NAIVE, GEMV, MFMA, MFMA_LARGE, SKINNY, NATIVE8, DEQUANT_MFMA, MFMA_FUSED4, MMV, MFMA_LARGE4 = range(11)
KERNEL_NAMES = {NAIVE: "naive", GEMV: "gemv", MFMA: "mfma", MFMA_LARGE: "mfma_large", SKINNY: "skinny", NATIVE8: "mfma_native8",
                DEQUANT_MFMA: "dequant_mfma", MFMA_FUSED4: "mfma_fused4", MMV: "mmv", MFMA_LARGE4: "mfma_large4"}
DT_CODE = {"fp32": F32, "fp16": F16, "bf16": BF16, "int8": I8, "e4m3fn": E4M3, "e5m2": E5M2, "e4m3fnuz": E4M3FNUZ}
DT_SIZE = {"fp32": 4, "fp16": 2, "bf16": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Row(NamedTuple):
    id: str
    entry: str                 # the C entry, without its quanto_hip_ prefix
    kernel: int                # forced quanto_hip_kernel, AUTO where the entry takes none
    shape: tuple
    fmt: tuple                 # ((key, value), ...): formats, family specific
    knobs: tuple               # ((QUANTO_HIP_* name, value), ...)
    name: Optional[str]        # quanto_hip_last_kernel() after the call
    split: Optional[bool]      # the plan splits K (None: the family has no split)
    scratch: bool = False      # workspace bytes for another reason than a split
    counters: bool = False     # the workspace is under the counter contract

    @property
    def f(self) -> dict:
        return dict(self.fmt)

    @property
    def wants_workspace(self) -> bool:
        return bool(self.split) or self.scratch


class Plan(NamedTuple):
    status: int
    kernel: Optional[int]      # what the *_plan entry resolved to (None: the entry has no kernel choice)
    ws_bytes: int
    ws_bytes_other: Optional[int] = None  # the *_workspace_size entry's answer where both exist


class Problem(NamedTuple):
    inputs: Dict[str, torch.Tensor]                      # host tensors, uploaded byte for byte
    outputs: Dict[str, Tuple[torch.dtype, tuple]]
    gate: Callable[..., None]                            # gate(outputs on the host, ws_bytes the call was given): the route's oracle gate
    elem_check: bool = True                               # the output type cannot hold the prefill pattern as a value: "every element stored" is checkable


def lib():
    return quanto_hip.lib._c


def knobs_env(row: Row, monkeypatch):
    for k, v in row.knobs:
        monkeypatch.setenv(k, str(v))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def nbytes(dtype: torch.dtype, shape) -> int:
    n = 1
    for d in shape:
        n *= d
    return n * torch.empty((), dtype=dtype).element_size()


def _seed(row: Row) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(row.id)) % (1 << 31)


# ---- qbits_mm ----------------------------------------------------------------------------------------------------------------------------------------------
def _qbits_inputs(p, dt):
    shift = torch.from_numpy(p["shift"]) if p["shift"].dtype == np.uint8 else to_torch(p["shift"], dt)
    return {"packed": torch.from_numpy(p["packed"]), "scale": to_torch(p["scale"], dt), "shift": shift}


def _qbits_want(p, x, kernel):
    """float64 product: of the reference's rounded dequantized weight for the two prefill kernels that multiply it, of the stored integers otherwise."""
    gs = p["group_size"]
    if kernel in (DEQUANT_MFMA, MFMA_LARGE4):
        w = O.dequantize_qbits_ref(p["packed"], p["bits"], p["scale"], p["shift"], 0, gs, (p["N"], p["K"]), p["dt"])
        return np.matmul(np.asarray(x, np.float64), w.astype(np.float64).T)
    return O.qbits_mm_exact(x, p["packed"], p["bits"], p["scale"], p["shift"], gs, p["N"], p["K"])


class QBitsMM:
    @staticmethod
    def plan(row: Row) -> Plan:
        (M, N, K), f = row.shape, row.f
        k, ws = ctypes.c_int(0), ctypes.c_int64(0)
        st = lib().quanto_hip_qbits_mm_plan(M, N, K, f["bits"], f["gs"], DT_CODE[f["dt"]], row.kernel, ctypes.byref(k), ctypes.byref(ws))
        other = lib().quanto_hip_qbits_mm_workspace_size(M, N, K, f["bits"], f["gs"], DT_CODE[f["dt"]], row.kernel)
        return Plan(st, k.value, ws.value, int(other))

    @staticmethod
    def problem(row: Row) -> Problem:
        (M, N, K), f = row.shape, row.f
        dt = f["dt"]
        p = make_qbits_problem(M, N, K, dt, bits=f["bits"], group_size=f["gs"] or None, seed=_seed(row))
        kernel = QBitsMM.plan(row).kernel

        def gate(out, ws_bytes=None):
            assert_close_to_exact(to_numpy(out["y"]), _qbits_want(p, p["x"], kernel), dt, row.id)

        return Problem({"x": to_torch(p["x"], dt), **_qbits_inputs(p, dt)}, {"y": (TORCH_DT[dt], (M, N))}, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        (M, N, K), f = row.shape, row.f
        code = DT_CODE[f["dt"]]
        return lib().quanto_hip_qbits_mm(a.ptr("x"), a.ptr("packed"), a.ptr("scale"), a.ptr("shift"), a.ptr("bias") or None, a.ptr("y"), M, N, K, f["bits"], f["gs"], code,
                                         code, row.kernel, ws_ptr or None, ws_bytes, _stream())


# ---- qbytes_mm_ws ------------------------------------------------------------------------------------------------------------------------------------------
def _codes_problem(M, N, K, kind, seed, scale_div):
    """Quantized activations x a quantized weight of the same kind (the NATIVE8 route), as tests/test_native8_split_gpu.py builds them."""
    rng = np.random.default_rng(seed)
    if kind == "int8":
        a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
        b = rng.integers(-128, 128, size=(N, K), dtype=np.int8)
    else:
        a = O.fp8_encode(rng.standard_normal((M, K)).astype(np.float32), kind)
        b = O.fp8_encode(rng.standard_normal((N, K)).astype(np.float32), kind)
    s = O.round_to(((rng.random((N, 1)) + 0.5) / scale_div).astype(np.float32), "bf16")
    return a, b, s


class QBytesMM:
    @staticmethod
    def _codes(row):
        f = row.f
        return DT_CODE[f["a"]], DT_CODE[f["b"]], DT_CODE[f["dt"]]

    @staticmethod
    def plan(row: Row) -> Plan:
        M, N, K = row.shape
        adt, bdt, odt = QBytesMM._codes(row)
        k, ws = ctypes.c_int(0), ctypes.c_int64(0)
        st = lib().quanto_hip_qbytes_mm_plan(M, N, K, adt, bdt, odt, row.kernel, ctypes.byref(k), ctypes.byref(ws))
        return Plan(st, k.value, ws.value, int(lib().quanto_hip_qbytes_mm_workspace_size(M, N, K, adt, bdt, odt, row.kernel)))

    @staticmethod
    def problem(row: Row) -> Problem:
        (M, N, K), f = row.shape, row.f
        dt = f["dt"]
        if f["a"] in ("int8", "e4m3fn"):  # codes x codes
            kind = f["a"]
            a, b, s = _codes_problem(M, N, K, kind, _seed(row), 1e4 if kind == "int8" else 1e2)
            if kind == "int8":
                want = O.qbytes_int_mm_ref(a, b, s, dt)

                def gate(out, ws_bytes=None):
                    np.testing.assert_array_equal(to_numpy(out["y"]), want, err_msg=row.id)
            else:
                want = np.matmul(O.fp8_decode(a, kind).astype(np.float64), O.fp8_decode(b, kind).astype(np.float64).T) * s.astype(np.float64).reshape(1, -1)

                def gate(out, ws_bytes=None):
                    assert_close_to_exact(to_numpy(out["y"]), want, dt, row.id)
            inputs = {"a": torch.from_numpy(a), "b": torch.from_numpy(b), "scales": to_torch(s, dt)}
        else:
            kind = None if f["b"] == "int8" else f["b"]
            p = make_qbytes_problem(M, N, K, dt, kind, seed=_seed(row))
            want = O.qbytes_mm_exact(p["x"], p["data"], p["scale"], kind)

            def gate(out, ws_bytes=None):
                assert_close_to_exact(to_numpy(out["y"]), want, dt, row.id)
            inputs = {"a": to_torch(p["x"], dt), "b": torch.from_numpy(p["data"]), "scales": to_torch(p["scale"], dt)}
        return Problem(inputs, {"y": (TORCH_DT[dt], (M, N))}, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        M, N, K = row.shape
        adt, bdt, odt = QBytesMM._codes(row)
        return lib().quanto_hip_qbytes_mm_ws(a.ptr("a"), a.ptr("b"), a.ptr("scales"), a.ptr("bias") or None, a.ptr("y"), M, N, K, adt, bdt, odt, row.kernel, ws_ptr or None,
                                             ws_bytes, _stream())


# ---- the two *_multi_ws entries ----------------------------------------------------------------------------------------------------------------------------
def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def _ptrs(a, names):
    return (ctypes.c_void_p * len(names))(*[a.ptr(n) for n in names])


def _bias_ptrs(a, n):
    """The members' bias regions (bias0, bias1, ...) where the arena has them; NULL for a problem without a bias."""
    return _ptrs(a, [f"bias{i}" for i in range(n)]) if a.ptr("bias0") else None


class QBitsMulti:
    """kernel = what the plan must say: GEMV / SKINNY (one launch) or AUTO (separate calls sharing the workspace: its bytes are those of
    quanto_hip_qbits_mm_multi_workspace_size, the plan entry reports 0 for that case)."""

    @staticmethod
    def plan(row: Row) -> Plan:
        (M, Ns, K), f = row.shape, row.f
        k, ws = ctypes.c_int(0), ctypes.c_int64(0)
        st = lib().quanto_hip_qbits_mm_multi_plan(len(Ns), _i64(Ns), M, K, f["bits"], f["gs"], DT_CODE[f["dt"]], ctypes.byref(k), ctypes.byref(ws))
        size = int(lib().quanto_hip_qbits_mm_multi_workspace_size(len(Ns), _i64(Ns), M, K, f["bits"], f["gs"], DT_CODE[f["dt"]]))
        if st == OK and k.value == AUTO:
            return Plan(st if size >= 0 else size, AUTO, max(size, 0), None)
        return Plan(st, k.value, ws.value, size)

    @staticmethod
    def member_kernels(row: Row):
        (M, Ns, K), f = row.shape, row.f
        return [lib().quanto_hip_qbits_mm_pick(M, n, K, f["bits"], f["gs"], DT_CODE[f["dt"]]) for n in Ns]

    @staticmethod
    def problem(row: Row) -> Problem:
        (M, Ns, K), f = row.shape, row.f
        dt = f["dt"]
        ps = [make_qbits_problem(M, n, K, dt, bits=f["bits"], group_size=f["gs"] or None, seed=_seed(row) + i) for i, n in enumerate(Ns)]
        x = ps[0]["x"]
        kernels = QBitsMulti.member_kernels(row) if row.kernel == AUTO else [row.kernel] * len(Ns)
        inputs, outputs = {"x": to_torch(x, dt)}, {}
        for i, p in enumerate(ps):
            inputs.update({f"{k}{i}": v for k, v in _qbits_inputs(p, dt).items()})
            outputs[f"y{i}"] = (TORCH_DT[dt], (M, Ns[i]))

        def gate(out, ws_bytes=None):
            for i, p in enumerate(ps):
                # separate calls: a member whose dense weight no longer fits the workspace it was given steps down to a kernel that multiplies the integers
                k = kernels[i]
                if k == DEQUANT_MFMA and ws_bytes is not None and ws_bytes < Ns[i] * K * DT_SIZE[dt]:
                    k = NAIVE
                assert_close_to_exact(to_numpy(out[f"y{i}"]), _qbits_want(p, x, k), dt, f"{row.id} member {i}")

        return Problem(inputs, outputs, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        (M, Ns, K), f = row.shape, row.f
        n, code = len(Ns), DT_CODE[f["dt"]]
        names = lambda k: [f"{k}{i}" for i in range(n)]  # noqa: E731
        return lib().quanto_hip_qbits_mm_multi_ws(a.ptr("x"), n, _ptrs(a, names("packed")), _ptrs(a, names("scale")), _ptrs(a, names("shift")), _bias_ptrs(a, n),
                                                  _ptrs(a, names("y")), _i64(Ns), M, K, f["bits"], f["gs"], code, code, ws_ptr or None, ws_bytes, _stream())


class QBytesMulti:
    @staticmethod
    def plan(row: Row) -> Plan:
        (M, Ns, K), f = row.shape, row.f
        k, ws = ctypes.c_int(0), ctypes.c_int64(0)
        st = lib().quanto_hip_qbytes_mm_multi_plan(len(Ns), _i64(Ns), M, K, DT_CODE[f["dt"]], DT_CODE[f["b"]], DT_CODE[f["dt"]], ctypes.byref(k),
                                                   ctypes.byref(ws))
        return Plan(st, k.value, ws.value, None)

    @staticmethod
    def member_kernels(row: Row):
        (M, Ns, K), f = row.shape, row.f
        return [lib().quanto_hip_qbytes_mm_pick(M, n, K, DT_CODE[f["dt"]], DT_CODE[f["b"]], DT_CODE[f["dt"]]) for n in Ns]

    @staticmethod
    def problem(row: Row) -> Problem:
        (M, Ns, K), f = row.shape, row.f
        dt, kind = f["dt"], (None if f["b"] == "int8" else f["b"])
        ps = [make_qbytes_problem(M, n, K, dt, kind, seed=_seed(row) + i) for i, n in enumerate(Ns)]
        x = ps[0]["x"]
        inputs, outputs = {"a": to_torch(x, dt)}, {}
        for i, p in enumerate(ps):
            inputs[f"b{i}"], inputs[f"scales{i}"] = torch.from_numpy(p["data"]), to_torch(p["scale"], dt)
            outputs[f"y{i}"] = (TORCH_DT[dt], (M, Ns[i]))

        def gate(out, ws_bytes=None):
            for i, p in enumerate(ps):
                assert_close_to_exact(to_numpy(out[f"y{i}"]), O.qbytes_mm_exact(x, p["data"], p["scale"], kind), dt, f"{row.id} member {i}")

        return Problem(inputs, outputs, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        (M, Ns, K), f = row.shape, row.f
        n, code = len(Ns), DT_CODE[f["dt"]]
        names = lambda k: [f"{k}{i}" for i in range(n)]  # noqa: E731
        return lib().quanto_hip_qbytes_mm_multi_ws(a.ptr("a"), n, _ptrs(a, names("b")), _ptrs(a, names("scales")), _bias_ptrs(a, n), _ptrs(a, names("y")), _i64(Ns), M, K,
                                                   code, DT_CODE[f["b"]], code, ws_ptr or None, ws_bytes, _stream())


# ---- qbits_mm_a8 -------------------------------------------------------------------------------------------------------------------------------------------
class QBitsA8:
    @staticmethod
    def plan(row: Row) -> Plan:
        (M, N, K), f = row.shape, row.f
        ws = int(lib().quanto_hip_qbits_mm_a8_workspace_size(M, N, K, f["bits"], 128, DT_CODE[f["a"]], DT_CODE[f["dt"]]))
        return Plan(OK if ws >= 0 else ws, None, max(ws, 0), None)

    @staticmethod
    def problem(row: Row) -> Problem:
        (M, N, K), f = row.shape, row.f
        dt, bits, seed = f["dt"], f["bits"], _seed(row)
        p = make_qbits_problem(2, N, K, dt, bits=bits, seed=seed)
        rng = np.random.default_rng(seed + 1)
        if f["a"] == "int8":
            codes = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
            values, sx = codes, O.round_to(np.array([0.0173], np.float32), dt)
        else:
            codes = O.fp8_encode((rng.standard_normal((M, K)) * 40).astype(np.float32), "e4m3fn")
            values, sx = O.fp8_decode(codes, "e4m3fn"), O.round_to(np.array([0.021], np.float32), dt)
        exact = f["a"] == "int8" and not row.split  # the unsplit int8 form is a pure function of the integers: the oracle's fp32 fma chain, bit for bit

        def gate(out, ws_bytes=None):
            y = to_numpy(out["y"])
            if exact:
                np.testing.assert_array_equal(y, O.qbits_mm_a8_chain(codes, sx, p["packed"], bits, p["scale"], p["shift"], 128, N, K, dt), err_msg=row.id)
            else:
                assert_close_to_exact(y, O.qbits_mm_a8_exact(values, sx, p["packed"], bits, p["scale"], p["shift"], 128, N, K), dt, row.id)

        return Problem({"a": torch.from_numpy(codes), "a_scale": to_torch(sx, dt), **_qbits_inputs(p, dt)}, {"y": (TORCH_DT[dt], (M, N))}, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        (M, N, K), f = row.shape, row.f
        code = DT_CODE[f["dt"]]
        return lib().quanto_hip_qbits_mm_a8(a.ptr("a"), a.ptr("a_scale"), a.ptr("packed"), a.ptr("scale"), a.ptr("shift"), a.ptr("bias") or None, a.ptr("y"), M, N, K,
                                            f["bits"], 128, DT_CODE[f["a"]], code, code, ws_ptr or None, ws_bytes, _stream())


# ---- qbytes_bmm --------------------------------------------------------------------------------------------------------------------------------------------
class QBytesBmm:
    SCALE = 0.0123

    @staticmethod
    def plan(row: Row) -> Plan:
        return Plan(OK, None, 0, None)  # no plan entry, no workspace

    @staticmethod
    def problem(row: Row) -> Problem:
        (B, M, N, K), f = row.shape, row.f
        rng = np.random.default_rng(_seed(row))
        a = rng.integers(-128, 128, size=(B, M, K), dtype=np.int8)
        w = rng.integers(-128, 128, size=(B, K, N), dtype=np.int8)
        stored = w if f["layout"] == "NN" else np.ascontiguousarray(w.transpose(0, 2, 1))  # NT: [B, N, K], K contiguous
        acc = np.matmul(a.astype(np.int64), w.astype(np.int64))
        tdt = TORCH_DT[f["dt"]]
        want = torch.from_numpy(acc.astype(np.float32) * np.float32(QBytesBmm.SCALE)).to(tdt)  # one round-to-nearest-even to T

        def gate(out, ws_bytes=None):
            assert torch.equal(out["y"].view(torch.uint8), want.view(torch.uint8)), f"{row.id}: differs from the int32 sum scaled in fp32 and rounded once"

        return Problem({"a": torch.from_numpy(a), "w": torch.from_numpy(stored), "scale": torch.tensor([QBytesBmm.SCALE], dtype=torch.float32)},
                       {"y": (tdt, (B, M, N))}, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        (B, M, N, K), f = row.shape, row.f
        w_k, w_n = (N, 1) if f["layout"] == "NN" else (1, K)
        return lib().quanto_hip_qbytes_bmm(a.ptr("a"), a.ptr("w"), a.ptr("scale"), a.ptr("y"), B, M, N, K, M * K, K, K * N, w_k, w_n, DT_CODE[f["dt"]], _stream())


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------------------------
class Geo(NamedTuple):
    B: int
    cin: int
    H: int
    W: int
    OC: int
    KH: int
    KW: int
    s: Tuple[int, int] = (1, 1)
    p: Tuple[int, int] = (0, 0)
    d: Tuple[int, int] = (1, 1)

    @property
    def OH(self):
        return (self.H + 2 * self.p[0] - self.d[0] * (self.KH - 1) - 1) // self.s[0] + 1

    @property
    def OW(self):
        return (self.W + 2 * self.p[1] - self.d[1] * (self.KW - 1) - 1) // self.s[1] + 1

    @property
    def K(self):
        return self.cin * self.KH * self.KW

    def args(self):
        """The positional geometry of every convolution entry."""
        return (self.B, self.cin, self.H, self.W, self.OC, self.KH, self.KW, self.OH, self.OW, self.s[0], self.s[1], self.p[0], self.p[1], self.d[0], self.d[1])


def _conv64(x, w, g: Geo, groups=1):
    """The float64 convolution of the suite's convolution tests: [B, OC, OH, OW]."""
    return torch.nn.functional.conv2d(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64)), None, g.s, g.p, g.d, groups).numpy()


def _conv_activation(g: Geo, dt, rng):
    return O.round_to(rng.standard_normal((g.B, g.cin, g.H, g.W)).astype(np.float32), dt)


def _bytes_weight(shape, kind, dt, rng):
    """int8 / fp8 weight of ``shape`` with a per-output-channel absmax scale, quantized by the oracle."""
    w = O.round_to((rng.standard_normal(shape) * 0.05).astype(np.float32), dt)
    if kind == "int8":
        scale = O.absmax_scale(w, 127.0, 0, dt)
        data = O.quantize_symmetric_int8(w, scale, dt)
        return data, scale, data.astype(np.float64)
    scale = O.absmax_scale(w, O.FP8_MAX[kind], 0, dt)
    data = O.quantize_symmetric_fp8(w, scale, kind, dt)
    return data, scale, O.fp8_decode(data, kind).astype(np.float64)


class QBytesConv2d:
    depthwise = False

    @classmethod
    def plan(cls, row: Row) -> Plan:
        g = row.shape
        if cls.depthwise:
            return Plan(OK, None, 0, None)
        ws = int(lib().quanto_hip_conv2d_workspace_size(g.B, g.OH, g.OW, g.OC, g.K))
        return Plan(OK if ws >= 0 else EINVAL, None, max(ws, 0), None)

    @classmethod
    def problem(cls, row: Row) -> Problem:
        g, f = row.shape, row.f
        dt, rng = f["dt"], np.random.default_rng(_seed(row))
        x = _conv_activation(g, dt, rng)
        wshape = (g.OC, 1 if cls.depthwise else g.cin, g.KH, g.KW)
        data, scale, w64 = _bytes_weight(wshape, f["b"], dt, rng)
        want = _conv64(x, w64 * scale.astype(np.float64).reshape(-1, 1, 1, 1), g, groups=g.cin if cls.depthwise else 1)

        def gate(out, ws_bytes=None):
            assert_close_to_exact(to_numpy(out["y"]), want, dt, row.id)

        return Problem({"x": to_torch(x, dt), "w": torch.from_numpy(data), "scales": to_torch(scale, dt)}, {"y": (TORCH_DT[dt], want.shape)}, gate)

    @classmethod
    def call(cls, row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        g, f = row.shape, row.f
        code = DT_CODE[f["dt"]]
        args = (a.ptr("x"), a.ptr("w"), a.ptr("scales"), a.ptr("bias") or None, a.ptr("y"), *g.args(), code, DT_CODE[f["b"]], code)
        if cls.depthwise:
            return lib().quanto_hip_qbytes_conv2d_depthwise(*args, _stream())
        return lib().quanto_hip_qbytes_conv2d(*args, ws_ptr or None, ws_bytes, _stream())


class QBytesConv2dDepthwise(QBytesConv2d):
    depthwise = True


class QBitsConv2d:
    @staticmethod
    def plan(row: Row) -> Plan:
        g = row.shape
        ws = int(lib().quanto_hip_qbits_conv2d_workspace_size_geom(g.B, g.cin, g.W, g.OC, g.KH, g.KW, g.OH, g.OW, g.s[1], g.d[1]))
        return Plan(OK if ws >= 0 else EINVAL, None, max(ws, 0), None)

    @staticmethod
    def problem(row: Row) -> Problem:
        g, f = row.shape, row.f
        dt, rng = f["dt"], np.random.default_rng(_seed(row))
        x = _conv_activation(g, dt, rng)
        p = make_qbits_problem(1, g.OC, g.K, dt, bits=f["bits"], group_size=f["gs"] or None, seed=_seed(row) + 1, wscale=0.05)
        # the matrix cores multiply by exactly the dense weight the reference would have materialised (include/quanto_hip.h)
        w = O.dequantize_qbits_ref(p["packed"], f["bits"], p["scale"], p["shift"], 0, f["gs"] or None, (g.OC, g.K), dt)
        want = _conv64(x, w.astype(np.float64).reshape(g.OC, g.cin, g.KH, g.KW), g)

        def gate(out, ws_bytes=None):
            assert_close_to_exact(to_numpy(out["y"]), want, dt, row.id)

        return Problem({"x": to_torch(x, dt), **_qbits_inputs(p, dt)}, {"y": (TORCH_DT[dt], want.shape)}, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        g, f = row.shape, row.f
        code = DT_CODE[f["dt"]]
        return lib().quanto_hip_qbits_conv2d(a.ptr("x"), a.ptr("packed"), a.ptr("scale"), a.ptr("shift"), a.ptr("bias") or None, a.ptr("y"), *g.args(), f["bits"], f["gs"], code,
                                             code, ws_ptr or None, ws_bytes, _stream())


class QBytesConv2dA8:
    @staticmethod
    def plan(row: Row) -> Plan:
        g, f = row.shape, row.f
        ws = int(lib().quanto_hip_qbytes_conv2d_a8_workspace_size(*g.args(), DT_CODE[f["a"]], DT_CODE[f["b"]], DT_CODE[f["dt"]]))
        return Plan(OK if ws >= 0 else ws, None, max(ws, 0), None)

    @staticmethod
    def _codes(shape, kind, rng):
        if kind == "int8":
            c = rng.integers(-128, 128, size=shape, dtype=np.int8)
            return c, c.astype(np.float64)
        c = O.fp8_encode((rng.standard_normal(shape) * 4).astype(np.float32), kind)
        return c, O.fp8_decode(c, kind).astype(np.float64)

    @staticmethod
    def problem(row: Row) -> Problem:
        g, f = row.shape, row.f
        dt, rng = f["dt"], np.random.default_rng(_seed(row))
        x, x64 = QBytesConv2dA8._codes((g.B, g.cin, g.H, g.W), f["a"], rng)
        w, w64 = QBytesConv2dA8._codes((g.OC, g.cin, g.KH, g.KW), f["b"], rng)
        xs = torch.tensor([0.0173], dtype=TORCH_DT[dt])
        ws = (torch.from_numpy(rng.random(g.OC).astype(np.float32)) * 0.004 + 0.0005).to(TORCH_DT[dt])
        sc = to_numpy(xs * ws)  # torch's product in the dtype: sc[n] = round_dtype(a_scale * w_scale[n])
        acc = _conv64(x64, w64, g)  # exact: integers (or fp8 values) in float64
        if f["a"] == "int8":
            want = O.round_to(acc.astype(np.float32) * sc.astype(np.float32).reshape(1, -1, 1, 1), dt)  # oracle.qbytes_int_mm_ref on the im2col

            def gate(out, ws_bytes=None):
                np.testing.assert_array_equal(to_numpy(out["y"]), want, err_msg=row.id)
        else:
            want = acc * sc.astype(np.float64).reshape(1, -1, 1, 1)

            def gate(out, ws_bytes=None):
                assert_close_to_exact(to_numpy(out["y"]), want, dt, row.id)

        return Problem({"x": torch.from_numpy(x), "a_scale": xs, "w": torch.from_numpy(w), "w_scale": ws}, {"y": (TORCH_DT[dt], acc.shape)}, gate)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        g, f = row.shape, row.f
        return lib().quanto_hip_qbytes_conv2d_a8(a.ptr("x"), a.ptr("a_scale"), a.ptr("w"), a.ptr("w_scale"), a.ptr("bias") or None, a.ptr("y"), *g.args(), DT_CODE[f["a"]],
                                                 DT_CODE[f["b"]], DT_CODE[f["dt"]], ws_ptr or None, ws_bytes, _stream())


# ---- elementwise quantize / pack / unpack: bit equality with the reference library's torch sequence on the host --------------------------------------
def _bits_equal(row, got, want):
    assert torch.equal(got.view(torch.uint8).reshape(-1), want.contiguous().view(torch.uint8).reshape(-1)), f"{row.id}: differs from the CPU sequence"


class Elementwise:
    """shape and fmt per entry; no plan, no workspace, no last-kernel name."""

    @staticmethod
    def plan(row: Row) -> Plan:
        return Plan(OK, None, 0, None)

    @staticmethod
    def problem(row: Row) -> Problem:
        f, gen = row.f, torch.Generator().manual_seed(_seed(row))
        e = row.entry
        if e == "unpack":
            (n,) = row.shape
            packed = torch.randint(0, 256, (n,), generator=gen, dtype=torch.int32).to(torch.uint8)
            want = torch.from_numpy(O.unpack(packed.numpy(), f["bits"]))
            return Problem({"packed": packed}, {"out": (torch.uint8, (n * 8 // f["bits"],))}, lambda out, ws_bytes=None: _bits_equal(row, out["out"], want))
        if e == "dequantize_qbits":
            N, K = row.shape
            p = make_qbits_problem(1, N, K, f["dt"], bits=f["bits"], group_size=f["gs"] or None, seed=_seed(row))
            want = to_torch(O.dequantize_qbits_ref(p["packed"], f["bits"], p["scale"], p["shift"], 0, f["gs"] or None, (N, K), f["dt"]), f["dt"])
            return Problem(_qbits_inputs(p, f["dt"]), {"out": (TORCH_DT[f["dt"]], (N, K))}, lambda out, ws_bytes=None: _bits_equal(row, out["out"], want))
        if e == "quantize_symmetric":
            rows, inner = row.shape
            tdt, target = TORCH_DT[f["dt"]], {"int8": torch.int8, "e4m3fn": torch.float8_e4m3fn}[f["out"]]
            base = (torch.randn((rows, inner), generator=gen) * 3).to(tdt)
            axis = {"tensor": None, "first": 0, "last": -1}[f["mode"]]
            sshape = {"tensor": (), "first": (rows, 1), "last": (1, inner)}[f["mode"]]
            scale = (torch.rand(sshape, generator=gen) * 0.05 + 0.01).to(tdt)
            want = ops.quantize_symmetric(base, target, axis, scale)
            return Problem({"base": base, "scale": scale}, {"out": (target, (rows, inner))}, lambda out, ws_bytes=None: _bits_equal(row, out["out"], want), elem_check=False)
        if e == "dequantize_symmetric":
            (n,) = row.shape
            tdt = TORCH_DT[f["dt"]]
            q = torch.randint(-128, 128, (n,), generator=gen, dtype=torch.int8)
            scale = torch.tensor([0.0123], dtype=torch.float64).to(tdt)
            want = scale * q.to(tdt)
            return Problem({"q": q, "scale": scale}, {"out": (tdt, (n,))}, lambda out, ws_bytes=None: _bits_equal(row, out["out"], want))
        if e in ("quantize_affine", "quantize_affine_packed"):
            N, K = row.shape
            tdt, bits, gs = TORCH_DT[f["dt"]], f["bits"], f["gs"]
            base = torch.randn((N, K), generator=gen).to(tdt)
            R = N * K // gs
            scale = (torch.rand((R, 1), generator=gen) * 0.3 + 0.1).to(tdt)
            shift = (torch.rand((R, 1), generator=gen) * 2 + 1).to(tdt)
            want = ops.quantize_affine(base, bits, 0, gs, scale, shift)
            if e == "quantize_affine":  # values below 2^bits: the prefill byte is no value
                return Problem({"base": base, "scale": scale, "shift": shift}, {"out": (torch.uint8, tuple(want.shape))}, lambda out, ws_bytes=None: _bits_equal(row, out["out"], want))
            packed = pack_weights(want, bits)
            return Problem({"base": base, "scale": scale, "shift": shift}, {"out": (torch.uint8, tuple(packed.shape))}, lambda out, ws_bytes=None: _bits_equal(row, out["out"], packed),
                           elem_check=False)
        if e == "pack":
            rows, cols = row.shape
            u = torch.randint(0, 1 << f["bits"], (rows, cols), generator=gen, dtype=torch.int32).to(torch.uint8)
            packed = pack_weights(u, f["bits"])
            return Problem({"unpacked": u}, {"out": (torch.uint8, tuple(packed.shape))}, lambda out, ws_bytes=None: _bits_equal(row, out["out"], packed), elem_check=False)
        raise KeyError(e)

    @staticmethod
    def call(row: Row, a, ws_ptr: int, ws_bytes: int) -> int:
        f, e, c, s = row.f, row.entry, lib(), _stream()
        if e == "unpack":
            return c.quanto_hip_unpack(a.ptr("packed"), a.ptr("out"), row.shape[0], f["bits"], s)
        if e == "dequantize_qbits":
            code = DT_CODE[f["dt"]]
            return c.quanto_hip_dequantize_qbits(a.ptr("packed"), a.ptr("scale"), a.ptr("shift"), a.ptr("out"), row.shape[0], row.shape[1], f["bits"], f["gs"],
                                                 code, code, s)
        if e == "quantize_symmetric":
            rows, inner = row.shape
            mode = {"tensor": 0, "first": 1, "last": 2}[f["mode"]]
            return c.quanto_hip_quantize_symmetric(a.ptr("base"), a.ptr("scale"), a.ptr("out"), rows * inner, 1 if mode == 0 else inner, mode, DT_CODE[f["dt"]],
                                                   DT_CODE[f["out"]], s)
        if e == "dequantize_symmetric":
            return c.quanto_hip_dequantize_symmetric(a.ptr("q"), a.ptr("scale"), a.ptr("out"), row.shape[0], I8, DT_CODE[f["dt"]], s)
        if e in ("quantize_affine", "quantize_affine_packed"):
            code = DT_CODE[f["dt"]]
            fn = c.quanto_hip_quantize_affine if e == "quantize_affine" else c.quanto_hip_quantize_affine_packed
            return fn(a.ptr("base"), a.ptr("scale"), a.ptr("shift"), a.ptr("out"), row.shape[0], row.shape[1], f["bits"], f["gs"], code, code, s)
        if e == "pack":
            return c.quanto_hip_pack(a.ptr("unpacked"), a.ptr("out"), row.shape[0], row.shape[1], f["bits"], s)
        raise KeyError(e)


FAMILIES = {
    "qbits_mm": QBitsMM, "qbytes_mm_ws": QBytesMM, "qbits_mm_multi_ws": QBitsMulti, "qbytes_mm_multi_ws": QBytesMulti, "qbits_mm_a8": QBitsA8,
    "qbytes_bmm": QBytesBmm, "qbytes_conv2d": QBytesConv2d, "qbytes_conv2d_depthwise": QBytesConv2dDepthwise, "qbits_conv2d": QBitsConv2d,
    "qbytes_conv2d_a8": QBytesConv2dA8, "unpack": Elementwise, "dequantize_qbits": Elementwise, "quantize_symmetric": Elementwise,
    "dequantize_symmetric": Elementwise, "quantize_affine": Elementwise, "quantize_affine_packed": Elementwise, "pack": Elementwise,
}
# entries that store into caller memory and are not in the table: their outputs already sit between guard bytes (helpers.sentinel_buffer) elsewhere;
# the plain forms of two entries of the table (the same code with workspace = NULL, which the table's "NULL, 0" pass calls)
COVERED_ELSEWHERE = {
    "quanto_hip_qbytes_mm_q_ws": "tests/test_output_fusion_gpu.py::test_no_byte_outside_the_output",
    "quanto_hip_qbits_mm_a8_q": "tests/test_a8_output_fusion_gpu.py::test_no_byte_outside_the_output",
    "quanto_hip_qbytes_conv2d_a8_q": "tests/test_conv_output_fusion_gpu.py::test_no_byte_outside_a_misaligned_output",
    "quanto_hip_layer_norm_q": "tests/test_layernorm_q_gpu.py::test_the_entry_stores_inside_its_output_only",
    "quanto_hip_qbytes_mm": "tests/test_containment_gpu.py::test_short_and_null_workspace (quanto_hip_qbytes_mm_ws with NULL, 0 is this entry)",
    "quanto_hip_qbits_mm_multi": "tests/test_containment_gpu.py::test_short_and_null_workspace (quanto_hip_qbits_mm_multi_ws with NULL, 0 is this entry)",
}


def family(row: Row):
    return FAMILIES[row.entry]


@functools.lru_cache(maxsize=None)
def _problem_cached(row_id: str) -> Problem:
    return family(BY_ID[row_id]).problem(BY_ID[row_id])


def problem(row: Row) -> Problem:
    """The row's problem, built once per session (under the row's knobs: a builder may ask the plan) and never changed."""
    return _problem_cached(row.id)


def header_kernel_names():
    """The last-kernel names include/quanto_hip.h lists for the entries of the table: every quoted lower-case name of the header that names a route, the
    code-storing ``*_q`` routes (COVERED_ELSEWHERE) left out."""
    with open(os.path.join(ROOT, "include", "quanto_hip.h")) as fh:
        text = fh.read()
    names = set(re.findall(r'"([a-z][a-z0-9_]*)"', text))
    return {n for n in names if not n.endswith("_q")}


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------
def _fmt(**kw):
    return tuple(sorted(kw.items()))


def _knobs(**kw):
    return tuple(sorted((f"QUANTO_HIP_{k}", v) for k, v in kw.items()))


def _kid(knobs):
    return "".join(f"-{k[len('QUANTO_HIP_'):].lower()}{v}" for k, v in knobs)


def _mm(entry, kernel, shape, fmt, name, split=None, scratch=False, counters=False, tag="", **knobs):
    kn = _knobs(**knobs)
    sid = "x".join("+".join(map(str, d)) if isinstance(d, (tuple, list)) else str(d) for d in shape)
    rid = f"{entry}-{name}-{sid}{('-' + tag) if tag else ''}{_kid(kn)}"
    return Row(rid, entry, kernel, tuple(tuple(d) if isinstance(d, list) else d for d in shape), fmt, kn, name, split, scratch, counters)


def _qbits(kernel, shape, name, bits=4, gs=128, dt="bf16", **kw):
    tag = f"int{bits}g{gs}" + ("" if dt == "bf16" else f"-{dt}")
    return _mm("qbits_mm", kernel, shape, _fmt(bits=bits, gs=gs, dt=dt), name, tag=tag, **kw)


def _qbytes(kernel, shape, name, a="bf16", b="int8", dt="bf16", **kw):
    return _mm("qbytes_mm_ws", kernel, shape, _fmt(a=a, b=b, dt=dt), name, tag=f"{a}x{b}", **kw)


def _conv(entry, geo: Geo, name, fmt, split=None, scratch=False, tag="", **knobs):
    kn = _knobs(**knobs)
    gid = f"b{geo.B}c{geo.cin}-{geo.H}x{geo.W}-oc{geo.OC}-k{geo.KH}x{geo.KW}s{geo.s[0]}p{geo.p[0]}"
    return Row(f"{entry}-{name}-{gid}{('-' + tag) if tag else ''}{_kid(kn)}", entry, AUTO, geo, fmt, kn, name, split, scratch, False)


def _elem(entry, shape, tag="", **fmt):
    return Row(f"{entry}-{'x'.join(map(str, shape))}{('-' + tag) if tag else ''}", entry, AUTO, tuple(shape), _fmt(**fmt), (), None, None)


def _rows():
    r = []
    # qbits_mm, bf16, int4 group 128 unless said
    r += [_qbits(NAIVE, (3, 36, 96), "naive", bits=2, gs=32), _qbits(NAIVE, (5, 34, 160), "naive", gs=0)]
    r += [_qbits(GEMV, (1, 130, 384), "gemv"), _qbits(GEMV, (3, 130, 384), "gemv"), _qbits(GEMV, (5, 132, 256), "gemv", bits=2, gs=64)]
    r += [_qbits(MMV, (5, 48, 384), "mmv"), _qbits(MMV, (17, 48, 384), "mmv")]
    r += [_qbits(SKINNY, (9, 192, 512), "skinny", split=False, counters=True, SKINNY_SPLIT=1),
          _qbits(SKINNY, (70, 192, 1024), "skinny", split=True, counters=True, SKINNY_SPLIT=2),
          _qbits(SKINNY, (70, 192, 1024), "skinny", split=True, counters=True, SKINNY_SPLIT=4),
          _qbits(AUTO, (16, 1024, 8192), "skinny", split=True, counters=True)]
    r += [_qbits(MFMA, (129, 130, 384), "mfma", scratch=True), _qbits(MFMA, (129, 130, 384), "mfma", gs=64, scratch=True)]
    r += [_qbits(MFMA_FUSED4, (65, 136, 512), "mfma_fused4", split=False, counters=True, FUSED4_SPLIT=1)]
    r += [_qbits(MFMA_FUSED4, (130, 264, 1024), "mfma_fused4", split=s > 1, counters=True, FUSED4_BM=bm, FUSED4_SPLIT=s) for bm in (64, 128) for s in (1, 2)]
    r += [_qbits(MFMA_LARGE4, (257, 258, 512), "mfma_large4")]
    r += [_qbits(DEQUANT_MFMA, (130, 258, 384), "dequant_mfma", scratch=True)]
    r += [_qbits(AUTO, (3, 66, 256), "gemv_f32", dt="fp32"), _qbits(AUTO, (70, 66, 256), "mfma_f32", dt="fp32")]
    # qbytes_mm_ws
    r += [_qbytes(k, (3, 131, 208), n, b=b) for k, n in ((NAIVE, "naive"), (GEMV, "gemv")) for b in ("int8", "e4m3fn")]
    r += [_qbytes(SKINNY, (9, 192, 512), "skinny", split=False, counters=True, SKINNY_SPLIT=1),
          _qbytes(SKINNY, (70, 192, 1024), "skinny", split=True, counters=True, SKINNY_SPLIT=2),
          _qbytes(SKINNY, (70, 192, 1024), "skinny", split=True, counters=True, SKINNY_SPLIT=4)]
    r += [_qbytes(MFMA, (129, 131, 256), "mfma")]
    r += [_qbytes(MFMA_LARGE, (257, 259, 512), "mfma_large", split=False, counters=True, LARGE_SPLIT=1),
          _qbytes(MFMA_LARGE, (129, 131, 1024), "mfma_large", split=True, counters=True, LARGE_SPLIT=2)]
    r += [_qbytes(NATIVE8, (129, 257, 1536), "mfma_native8", a=a, b=a, split=s > 1, counters=True, NATIVE8_SMALL=small, NATIVE8_SPLIT=s)
          for a in ("int8", "e4m3fn") for small in (0, 1) for s in (1, 2, 4)]
    r += [_qbytes(NATIVE8, (129, 257, 1536), "mfma_native8", a="int8", b="int8", split=True, counters=True, NATIVE8_SMALL=0, NATIVE8_SPLIT=4,
                  NATIVE8_POLL_TICKS=0)]
    r += [_qbytes(AUTO, (3, 67, 256), "gemv_f32", a="fp32", dt="fp32"), _qbytes(AUTO, (70, 67, 256), "mfma_f32", a="fp32", dt="fp32")]
    # the two *_multi_ws entries: one GEMV launch, one streaming launch (split and unsplit), separate calls on one shared workspace
    q4 = _fmt(bits=4, gs=128, dt="bf16")
    r += [_mm("qbits_mm_multi_ws", GEMV, (2, [130, 64, 258], 384), q4, "gemv_multi"),
          _mm("qbits_mm_multi_ws", SKINNY, (8, [64, 128, 192], 1024), q4, "skinny_multi", split=True, counters=True, SKINNY_SPLIT=2),
          _mm("qbits_mm_multi_ws", SKINNY, (8, [64, 128, 192], 1024), q4, "skinny_multi", split=False, counters=True, SKINNY_SPLIT=1),
          _mm("qbits_mm_multi_ws", AUTO, (100, [130, 258], 384), q4, "dequant_mfma", scratch=True, counters=True)]
    b8 = _fmt(b="int8", dt="bf16")
    r += [_mm("qbytes_mm_multi_ws", GEMV, (2, [130, 64, 258], 384), b8, "gemv_multi"),
          _mm("qbytes_mm_multi_ws", SKINNY, (8, [64, 128, 192], 1024), b8, "skinny_multi", split=True, counters=True, SKINNY_SPLIT=2),
          _mm("qbytes_mm_multi_ws", SKINNY, (8, [64, 128, 192], 1024), b8, "skinny_multi", split=False, counters=True, SKINNY_SPLIT=1),
          _mm("qbytes_mm_multi_ws", AUTO, (100, [130, 258], 384), b8, "skinny")]
    # qbits_mm_a8
    a8_names = {("int8", 4): "a8_fused_int8", ("e4m3fn", 4): "a8_fused_fp8", ("int8", 2): "a8_fused_int8_w2", ("e4m3fn", 2): "a8_fused_fp8_w2"}
    r += [_mm("qbits_mm_a8", AUTO, (65, 136 if bits == 4 else 144, 512), _fmt(a=a, bits=bits, dt="bf16"), a8_names[a, bits], split=s > 1, counters=True, A8_SPLIT=s)
          for a in ("int8", "e4m3fn") for bits in (4, 2) for s in (1, 2)]
    # qbytes_bmm
    r += [_mm("qbytes_bmm", AUTO, (3, 65, 67, 72), _fmt(layout=lay, dt=dt), "bmm_i8", tag=f"{lay}-{dt}") for lay in ("NT", "NN") for dt in ("bf16", "fp16", "fp32")]
    # qbytes_conv2d: tap gather (odd cin), row form in pixel pairs (even OW) and single pixels (odd OW); K-tiles of 64: a split of 5 needs K > 256
    tap, tap5 = Geo(2, 5, 9, 7, 19, 3, 3, p=(1, 1)), Geo(2, 29, 9, 7, 19, 3, 3, p=(1, 1))
    pairs, pairs5 = Geo(2, 8, 9, 10, 19, 3, 3, p=(1, 1)), Geo(2, 40, 9, 10, 19, 3, 3, p=(1, 1))
    single, single5 = Geo(2, 8, 9, 9, 19, 3, 3, p=(1, 1)), Geo(2, 40, 9, 9, 19, 3, 3, p=(1, 1))
    cb = _fmt(b="int8", dt="bf16")
    for small, big, name in ((tap, tap5, "conv2d_mfma"), (pairs, pairs5, "conv2d_mfma_rows"), (single, single5, "conv2d_mfma_rows")):
        two_tiles = small.K > 64  # K = 72: two K-tiles, a forced split of 2 or 5 runs as 2; K = 45: one K-tile, every forced split runs unsplit
        r += [_conv("qbytes_conv2d", small, name, cb, split=False, CONV_SPLIT=1), _conv("qbytes_conv2d", small, name, cb, split=two_tiles, CONV_SPLIT=2),
              _conv("qbytes_conv2d", small, name, cb, split=two_tiles, CONV_SPLIT=5), _conv("qbytes_conv2d", big, name, cb, split=True, CONV_SPLIT=2),
              _conv("qbytes_conv2d", big, name, cb, split=True, CONV_SPLIT=5)]
    # qbits_conv2d: int4 / int2 tap gather (per-channel scales: K = 45), the dequantize-once row route (dense weight + split scratch in one buffer)
    tap20, rows20, rows20k = Geo(2, 5, 9, 7, 20, 3, 3, p=(1, 1)), Geo(2, 8, 24, 24, 20, 3, 3, p=(1, 1)), Geo(2, 40, 24, 24, 20, 3, 3, p=(1, 1))
    r += [_conv("qbits_conv2d", tap20, f"conv2d_mfma_int{b}", _fmt(bits=b, gs=0, dt="bf16"), split=False, CONV_SPLIT=1) for b in (4, 2)]
    r += [_conv("qbits_conv2d", Geo(2, 32, 9, 7, 20, 3, 3, p=(1, 1)), "conv2d_mfma_int4", _fmt(bits=4, gs=32, dt="bf16"), split=True, CONV_SPLIT=2)]
    r += [_conv("qbits_conv2d", rows20, "conv2d_rows_dequant_int4", _fmt(bits=4, gs=24, dt="bf16"), split=False, scratch=True, CONV_SPLIT=1),
          _conv("qbits_conv2d", rows20k, "conv2d_rows_dequant_int4", _fmt(bits=4, gs=40, dt="bf16"), split=True, scratch=True, CONV_SPLIT=2),
          _conv("qbits_conv2d", rows20, "conv2d_rows_dequant_int2", _fmt(bits=2, gs=24, dt="bf16"), split=False, scratch=True, CONV_SPLIT=1)]
    # qbytes_conv2d_depthwise: general form (stride 2, multiplier 1 and 3), strip form ("same" 3 x 3 and 5 x 5)
    r += [_conv("qbytes_conv2d_depthwise", Geo(2, 5, 9, 7, 5 * m, 3, 3, s=(2, 2), p=(1, 1)), "conv2d_depthwise", cb, tag=f"m{m}") for m in (1, 3)]
    r += [_conv("qbytes_conv2d_depthwise", Geo(2, 5, 9, 8, 5, k, k, p=(k // 2, k // 2)), "conv2d_depthwise_strip", cb) for k in (3, 5)]
    # qbytes_conv2d_a8: the two dense geometries with int8 and e4m3 codes (K-tiles of 128 bytes: a split of 2 needs K > 128), fp8 codes x int8 weight
    for a, b, name in (("int8", "int8", "conv2d_a8_int8"), ("e4m3fn", "e4m3fn", "conv2d_a8_fp8")):
        fm = _fmt(a=a, b=b, dt="bf16")
        for small, big in ((tap, tap5), (pairs, pairs5)):  # K = 45 and 72 are one K-tile of codes: a forced split of 2 runs unsplit there
            r += [_conv("qbytes_conv2d_a8", small, name, fm, split=False, CONV_SPLIT=1), _conv("qbytes_conv2d_a8", small, name, fm, split=False, CONV_SPLIT=2),
                  _conv("qbytes_conv2d_a8", big, name, fm, split=True, CONV_SPLIT=2)]
    r += [_conv("qbytes_conv2d_a8", tap5, "conv2d_a8_fp8_w8", _fmt(a="e4m3fn", b="int8", dt="bf16"), split=True, CONV_SPLIT=2)]
    # elementwise: one ragged size each, a little above one workgroup's span (256 threads x 16 bytes)
    r += [_elem("unpack", (4112,), "int4-vec16", bits=4), _elem("unpack", (4101,), "int4", bits=4), _elem("unpack", (4101,), "int2", bits=2)]
    r += [_elem("dequantize_qbits", (6, 136), "int4-per-channel", bits=4, gs=0, dt="bf16"), _elem("dequantize_qbits", (6, 136), "int2-per-channel", bits=2, gs=0, dt="bf16"),
          _elem("dequantize_qbits", (11, 384), "int4g128", bits=4, gs=128, dt="bf16")]
    r += [_elem("quantize_symmetric", (7, 587), f"{m}-{o}", mode=m, out=o, dt="bf16") for m in ("tensor", "first", "last") for o in ("int8", "e4m3fn")]
    r += [_elem("dequantize_symmetric", (4109,), "int8-bf16", dt="bf16")]
    r += [_elem("quantize_affine", (33, 128), f"int{b}", bits=b, gs=128, dt="bf16") for b in (4, 2)]
    r += [_elem("quantize_affine_packed", (33, 128), f"int{b}", bits=b, gs=128, dt="bf16") for b in (4, 2)]
    r += [_elem("pack", (33, 136), f"int{b}", bits=b) for b in (4, 2)]
    return r


ROWS = _rows()
BY_ID = {row.id: row for row in ROWS}
assert len(BY_ID) == len(ROWS), "row ids are unique"
# the rows by entry, the elementwise entries together: one GPU test per group
GROUPS: Dict[str, list] = {}
for _row in ROWS:
    GROUPS.setdefault("elementwise" if FAMILIES[_row.entry] is Elementwise else _row.entry, []).append(_row)
# split-capable families: (entry, kernel name prefix) -> must appear split and unsplit
SPLIT_FAMILIES = sorted({(row.entry, row.name) for row in ROWS if row.split is not None})

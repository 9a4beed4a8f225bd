"""``quanto_hip``: ctypes binding of ``libquanto_hip.so`` (the MI355X backend, ``include/quanto_hip.h``).

This is the counterpart of the reference's ``library/extensions/hip/__init__.py:18-36`` (which binds a
single ``unpack`` kernel through pybind11): it exposes ``ext.lib.unpack(t, bits)`` with the same call
shape plus the fused products the reference lacks on ROCm.  The wrappers take torch tensors, allocate the
output with the input's options and return it by value - the reference's C++ convention
(library/extensions/cuda/unpack.cu:26-56) - and launch on torch's *current* stream under a device guard.
"""
import ctypes
import os
import re

import torch

from .extension import NativeLibrary, register_extension

__all__ = ["quanto_hip", "QuantoHipError"]

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# quanto_hip_dtype (include/quanto_hip.h)
F32, F16, BF16, I8, U8, F8_E4M3FN, F8_E5M2, F8_E4M3FNUZ = range(8)
WS_COUNTER_BYTES = 4096  # QUANTO_HIP_WS_COUNTER_BYTES
def _c_atoi(v: str) -> int:
    """The value C's ``atoi`` reads from an environment string (csrc/qh_common.h parses the knobs with it): optional blanks, a sign, leading
    digits; anything else is 0 - so that "01", "1 " or "true" mean the same thing on both sides of the binding."""
    m = re.match(r"\s*([+-]?\d+)", v or "")
    return int(m.group(1)) if m else 0


_EXPERIMENT = _c_atoi(os.environ.get("QUANTO_HIP_EXPERIMENT", "0")) != 0  # the library's knobs are live: plans are not cached
KERNEL_AUTO, KERNEL_NAIVE, KERNEL_GEMV, KERNEL_MFMA, KERNEL_MFMA_LARGE, KERNEL_SKINNY, KERNEL_NATIVE8, KERNEL_DEQUANT_MFMA, KERNEL_MFMA_FUSED4, KERNEL_MMV, KERNEL_MFMA_LARGE4 = range(11)
KERNELS = {"auto": KERNEL_AUTO, "naive": KERNEL_NAIVE, "gemv": KERNEL_GEMV, "mfma": KERNEL_MFMA, "mfma_large": KERNEL_MFMA_LARGE, "skinny": KERNEL_SKINNY,
           "mfma_native8": KERNEL_NATIVE8, "dequant_mfma": KERNEL_DEQUANT_MFMA, "mfma_fused4": KERNEL_MFMA_FUSED4, "mmv": KERNEL_MMV, "mfma_large4": KERNEL_MFMA_LARGE4}

_DTYPES = {
    torch.float32: F32,
    torch.float16: F16,
    torch.bfloat16: BF16,
    torch.int8: I8,
    torch.uint8: U8,
    torch.float8_e4m3fn: F8_E4M3FN,
    torch.float8_e5m2: F8_E5M2,
    torch.float8_e4m3fnuz: F8_E4M3FNUZ,
}


class QuantoHipError(RuntimeError):
    pass


def _dt(t: torch.Tensor) -> int:
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise QuantoHipError(f"quanto_hip: unsupported dtype {t.dtype}") from None


def _ptr(t):
    """Device address as a plain int (ctypes converts it through the entry's argtypes; building a c_void_p object per argument costs more
    than the rest of the marshalling)."""
    return 0 if t is None else t.data_ptr()


try:  # the stream handle without constructing a torch.cuda.Stream per call (what torch's own inductor / triton launchers use)
    _raw_stream = torch._C._cuda_getCurrentRawStream
    _current_device = torch._C._cuda_getDevice
except AttributeError:  # pragma: no cover - other torch builds
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream

    def _current_device():
        return torch.cuda.current_device()


class _DeviceGuard:
    """``with _DeviceGuard(d) as stream``: makes ``d`` the current device for the block and yields the raw handle of torch's current stream on it.
    ``torch.cuda.device`` is entered only when ``d`` is not already current: the context manager costs ~3 us per call, the check 0.2."""

    __slots__ = ("ctx", "index")

    def __init__(self, device: torch.device):
        index, current = device.index, _current_device()
        self.index = current if index is None else index
        self.ctx = None if index is None or index == current else torch.cuda.device(device)

    def __enter__(self) -> int:
        if self.ctx is not None:
            self.ctx.__enter__()
        return _raw_stream(self.index)

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_pvp, _pi64, _pci = ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_ci)
# name: (restype, argtypes) of every entry of include/quanto_hip.h
_PROTOTYPES = {
    "quanto_hip_abi_version": (_ci, None),
    "quanto_hip_status_string": (ctypes.c_char_p, [_ci]),
    "quanto_hip_last_kernel": (ctypes.c_char_p, None),
    "quanto_hip_stream_capture_id": (_i64, [_vp]),
    "quanto_hip_unpack": (_ci, [_vp, _vp, _i64, _ci, _vp]),
    "quanto_hip_dequantize_qbits": (_ci, [_vp] * 4 + [_i64] * 2 + [_ci] * 4 + [_vp]),
    "quanto_hip_qbits_mm": (_ci, [_vp] * 6 + [_i64] * 3 + [_ci] * 5 + [_vp, _sz, _vp]),
    "quanto_hip_qbits_mm_multi": (_ci, [_vp, _ci] + [_pvp] * 5 + [_pi64, _i64, _i64] + [_ci] * 4 + [_vp]),
    "quanto_hip_qbits_mm_multi_ws": (_ci, [_vp, _ci] + [_pvp] * 5 + [_pi64, _i64, _i64] + [_ci] * 4 + [_vp, _sz, _vp]),
    "quanto_hip_qbits_mm_multi_plan": (_ci, [_ci, _pi64, _i64, _i64] + [_ci] * 3 + [_pci, _pi64]),
    "quanto_hip_qbytes_mm_multi_ws": (_ci, [_vp, _ci] + [_pvp] * 4 + [_pi64, _i64, _i64] + [_ci] * 3 + [_vp, _sz, _vp]),
    "quanto_hip_qbytes_mm_multi_plan": (_ci, [_ci, _pi64, _i64, _i64] + [_ci] * 3 + [_pci, _pi64]),
    "quanto_hip_qbits_mm_workspace_size": (_i64, [_i64] * 3 + [_ci] * 4),
    "quanto_hip_qbits_mm_plan": (_ci, [_i64] * 3 + [_ci] * 4 + [_pci, _pi64]),
    "quanto_hip_qbits_mm_pick": (_ci, [_i64] * 3 + [_ci] * 3),
    "quanto_hip_qbits_mm_a8": (_ci, [_vp] * 7 + [_i64] * 3 + [_ci] * 5 + [_vp, _sz, _vp]),
    "quanto_hip_qbits_mm_a8_workspace_size": (_i64, [_i64] * 3 + [_ci] * 4),
    "quanto_hip_qbits_mm_a8_q": (_ci, [_vp] * 8 + [_i64] * 3 + [_ci] * 5 + [_vp, _sz, _vp]),
    "quanto_hip_qbytes_mm": (_ci, [_vp] * 5 + [_i64] * 3 + [_ci] * 4 + [_vp]),
    "quanto_hip_qbytes_mm_ws": (_ci, [_vp] * 5 + [_i64] * 3 + [_ci] * 4 + [_vp, _sz, _vp]),
    "quanto_hip_qbytes_mm_workspace_size": (_i64, [_i64] * 3 + [_ci] * 4),
    "quanto_hip_qbytes_mm_plan": (_ci, [_i64] * 3 + [_ci] * 4 + [_pci, _pi64]),
    "quanto_hip_qbytes_mm_pick": (_ci, [_i64] * 3 + [_ci] * 3),
    "quanto_hip_qbytes_mm_q_ws": (_ci, [_vp] * 6 + [_i64] * 3 + [_ci] * 4 + [_vp, _sz, _vp]),
    "quanto_hip_qbytes_mm_q_plan": (_ci, [_i64] * 3 + [_ci] * 4 + [_pci, _pi64]),
    "quanto_hip_qbytes_bmm": (_ci, [_vp] * 4 + [_i64] * 9 + [_ci, _vp]),
    "quanto_hip_layer_norm_q": (_ci, [_vp] * 5 + [_i64] * 3 + [ctypes.c_float, _ci, _ci, _vp]),
    "quanto_hip_layer_norm_q_supported": (_ci, [_i64] * 2 + [_ci] * 2),
    "quanto_hip_quantize_symmetric": (_ci, [_vp] * 3 + [_i64] * 2 + [_ci] * 3 + [_vp]),
    "quanto_hip_dequantize_symmetric": (_ci, [_vp] * 3 + [_i64] + [_ci] * 2 + [_vp]),
    "quanto_hip_quantize_affine": (_ci, [_vp] * 4 + [_i64] * 2 + [_ci] * 4 + [_vp]),
    "quanto_hip_quantize_affine_packed": (_ci, [_vp] * 4 + [_i64] * 2 + [_ci] * 4 + [_vp]),
    "quanto_hip_pack": (_ci, [_vp, _vp, _i64, _i64, _ci, _vp]),
    "quanto_hip_qbytes_conv2d": (_ci, [_vp] * 5 + [_i64] * 9 + [_ci] * 9 + [_vp, _sz, _vp]),
    "quanto_hip_qbytes_conv2d_depthwise": (_ci, [_vp] * 5 + [_i64] * 9 + [_ci] * 9 + [_vp]),
    "quanto_hip_qbytes_conv2d_a8": (_ci, [_vp] * 6 + [_i64] * 9 + [_ci] * 9 + [_vp, _sz, _vp]),
    "quanto_hip_qbytes_conv2d_a8_workspace_size": (_i64, [_i64] * 9 + [_ci] * 9),
    "quanto_hip_qbytes_conv2d_a8_q": (_ci, [_vp] * 7 + [_i64] * 9 + [_ci] * 9 + [_vp, _sz, _vp]),
    "quanto_hip_conv2d_workspace_size": (_i64, [_i64] * 5),
    "quanto_hip_qbits_conv2d_workspace_size": (_i64, [_i64] * 5),
    "quanto_hip_qbits_conv2d_workspace_size_geom": (_i64, [_i64] * 8 + [_ci] * 2),
    "quanto_hip_qbits_conv2d": (_ci, [_vp] * 6 + [_i64] * 9 + [_ci] * 10 + [_vp, _sz, _vp]),
}


class _Bindings:
    """Typed entry points; one instance per loaded library."""

    def __init__(self, cdll: ctypes.CDLL):
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(cdll, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        self._c = cdll
        if cdll.quanto_hip_abi_version() != 1:
            raise QuantoHipError("libquanto_hip.so ABI version mismatch: rebuild with __graft_entry__.build()")

    # -- helpers ----------------------------------------------------------------------------------
    def _check(self, status: int, what: str):
        if status != 0:
            msg = self._c.quanto_hip_status_string(status).decode()
            raise QuantoHipError(f"quanto_hip.{what} failed: {msg} (status {status})")

    @staticmethod
    def _require_cuda(*tensors):
        for t in tensors:
            if t is not None and not t.is_cuda:
                raise QuantoHipError("quanto_hip kernels only accept tensors on a ROCm device")

    def _stream_buffer(self, pool: str, device: torch.device, nbytes: int, stream: int, zero_counters: bool) -> torch.Tensor:
        """One growing buffer per (device, stream, capture) in ``pool`` instead of an allocation per call.  Launches on one stream use it in
        stream order; launches on different streams of one device may overlap, so each stream gets its own.  A buffer allocated while the
        stream is being captured lives in that graph's memory pool (and a zero-fill is a node of that graph, re-run on every replay): it is
        keyed by the capture id so that neither eager launches nor another capture ever see it."""
        cache = self.__dict__.setdefault(pool, {})
        capture = self._c.quanto_hip_stream_capture_id(stream)
        if capture < 0:
            self._check(int(capture), "stream_capture_id")
        key = (device, stream, capture)
        buf = cache.get(key)
        if buf is None or buf.numel() < nbytes:
            if len(cache) > 64:  # stream handles / capture ids come and go: do not keep dead buffers alive forever
                for k in [k for k in cache if k[2] != 0 and k != key]:
                    del cache[k]
            if zero_counters:
                # only the counter region has to be zero (include/quanto_hip.h: QUANTO_HIP_WS_COUNTER_BYTES; the kernels restore what they
                # use, the partial sums behind it are never read before they are written): 4 KiB of fill - under capture a 4 KiB memset
                # node per replay instead of one over the whole buffer (8-17 MB)
                buf = torch.empty((max(nbytes, 8 << 20),), dtype=torch.uint8, device=device)
                buf[:WS_COUNTER_BYTES].zero_()
            else:
                buf = torch.empty((nbytes,), dtype=torch.uint8, device=device)
            cache[key] = buf
        return buf

    def _zeroed_workspace(self, device: torch.device, nbytes: int, stream: int) -> torch.Tensor:
        """Split-K workspace: [QUANTO_HIP_WS_COUNTER_BYTES of arrival counters | fp32 partial sums] (include/quanto_hip.h), its counter region
        zero-filled once when (re)allocated and only ever handed to kernels that restore the counter words they use.  A pool of its own: the
        kernels that take scratch write from offset 0, over what would be the counter region."""
        return self._stream_buffer("_zero_ws", device, nbytes, stream, True)

    def _scratch(self, device: torch.device, nbytes: int, stream: int) -> torch.Tensor:
        """Uninitialised scratch (the dequantized weight of the prefill path, the row sums of the 128x128 kernel, the convolutions' K split)."""
        return self._stream_buffer("_scratch_ws", device, nbytes, stream, False)

    def _plan(self, which: str, key, call):
        """(kernel, workspace bytes) of a call shape, asked from the library once per (shape, format, dtype, forced kernel) and kept: the
        choice is a pure function of those (csrc/c_api.hip: plan_q*; with QUANTO_HIP_EXPERIMENT the knobs may change between calls, so
        nothing is kept then).  ``call()`` asks: (status, kernel, workspace bytes); a failed status raises and is not kept."""
        cache = self.__dict__.setdefault("_plans", {})
        hit = cache.get((which, key))
        if hit is not None:
            return hit
        st, kernel, ws = call()
        if st != 0:
            self._check(st, which + "_plan")
        plan = (kernel, ws)
        if not _EXPERIMENT:
            if len(cache) > 4096:
                cache.clear()
            cache[(which, key)] = plan
        return plan

    @staticmethod
    def _ask(entry, *args):
        """(status, kernel, workspace bytes) from one of the C ``*_plan`` entries."""
        k_out, ws_out = ctypes.c_int(0), ctypes.c_int64(0)
        st = entry(*args, ctypes.byref(k_out), ctypes.byref(ws_out))
        return st, k_out.value, ws_out.value

    def last_kernel(self) -> str:
        return self._c.quanto_hip_last_kernel().decode()

    # -- quanto::quantize_symmetric -----------------------------------------------------------------
    QUANTIZE_TARGETS = (torch.int8, torch.float8_e4m3fn, torch.float8_e5m2)

    def quantize_symmetric(self, base: torch.Tensor, dtype: torch.dtype, axis, scale: torch.Tensor) -> torch.Tensor:
        """One-pass clamp(round(base / scale)).to(dtype); ``axis`` in (None, 0, -1) as validated by the op wrapper."""
        self._require_cuda(base, scale)
        if dtype not in self.QUANTIZE_TARGETS or base.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise QuantoHipError(f"quantize_symmetric: unsupported dtypes {base.dtype} -> {dtype}")
        base = base.contiguous()
        scale = scale.to(base.dtype).contiguous()
        out = torch.empty(base.shape, dtype=dtype, device=base.device)
        if axis is None:
            mode, inner = 0, 1
        elif axis == 0:
            mode, inner = 1, (base.numel() // base.shape[0] if base.numel() else 1)
        else:
            mode, inner = 2, base.shape[-1]
        with _DeviceGuard(base.device) as stream:
            st = self._c.quanto_hip_quantize_symmetric(_ptr(base), _ptr(scale), _ptr(out), base.numel(), inner, mode, _dt(base), _dt(out), stream)
        self._check(st, "quantize_symmetric")
        return out

    def dequantize_symmetric(self, data: torch.Tensor, scale: torch.Tensor):
        """``scale * data.to(scale.dtype)`` for a per-tensor scale in one pass (tensor/qbytes.py:23-36); None when the view is not one the kernel takes (the
        caller keeps the two-kernel expression)."""
        if not (data.is_cuda and scale.is_cuda and scale.numel() == 1 and data.is_contiguous() and data.dtype in (torch.int8, torch.float8_e4m3fn, torch.float8_e5m2)
                and scale.dtype in (torch.float32, torch.float16, torch.bfloat16)):
            return None
        out = torch.empty(data.shape, dtype=scale.dtype, device=data.device)
        if data.numel() == 0:
            return out
        if (data.data_ptr() | out.data_ptr()) % 16:
            return None
        with _DeviceGuard(data.device) as stream:
            st = self._c.quanto_hip_dequantize_symmetric(_ptr(data), _ptr(scale), _ptr(out), data.numel(), _dt(data), _dt(out), stream)
        self._check(st, "dequantize_symmetric")
        return out

    def quantize_affine(self, base: torch.Tensor, bits: int, group_size, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
        """Axis-0 2-D weights only: uint8 grouped matrix [N*K/C, C] (C = group_size or K)."""
        self._require_cuda(base, scale, shift)
        N, K = base.shape
        base = base.contiguous()
        scale = scale.to(base.dtype).contiguous()
        shift = shift.contiguous() if not shift.dtype.is_floating_point else shift.to(base.dtype).contiguous()
        C = group_size or K
        out = torch.empty((N * K // C, C), dtype=torch.uint8, device=base.device)
        with _DeviceGuard(base.device) as stream:
            st = self._c.quanto_hip_quantize_affine(_ptr(base), _ptr(scale), _ptr(shift), _ptr(out), N, K, bits, group_size or 0,
                                                    _dt(base), _dt(shift), stream)
        self._check(st, "quantize_affine")
        return out

    def quantize_affine_packed(self, base: torch.Tensor, bits: int, group_size, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
        """quantize_affine + pack_weights in one pass: the packed bytes [ceil(R / (8/bits)), C] of the grouped matrix [R, C]."""
        self._require_cuda(base, scale, shift)
        N = base.shape[0]
        K = base.numel() // N
        base = base.contiguous()
        scale = scale.to(base.dtype).contiguous()
        shift = shift.contiguous() if not shift.dtype.is_floating_point else shift.to(base.dtype).contiguous()
        C = group_size or K
        rows = N * K // C
        vpi = 8 // bits
        out = torch.empty(((rows + vpi - 1) // vpi, C), dtype=torch.uint8, device=base.device)
        with _DeviceGuard(base.device) as stream:
            st = self._c.quanto_hip_quantize_affine_packed(_ptr(base), _ptr(scale), _ptr(shift), _ptr(out), N, K, bits,
                                                           group_size or 0, _dt(base), _dt(shift), stream)
        self._check(st, "quantize_affine_packed")
        return out

    def pack(self, t: torch.Tensor, bits: int) -> torch.Tensor:
        self._require_cuda(t)
        if t.dtype not in (torch.uint8, torch.int8):
            raise QuantoHipError("pack expects an 8-bit integer tensor")
        t = t.contiguous().view(torch.uint8)
        rows = t.shape[0]
        cols = t.numel() // rows if rows else 0
        row_dim = (rows + 8 // bits - 1) // (8 // bits)
        out = torch.empty((row_dim,) + tuple(t.shape[1:]), dtype=torch.uint8, device=t.device)
        with _DeviceGuard(t.device) as stream:
            self._check(self._c.quanto_hip_pack(_ptr(t), _ptr(out), rows, cols, bits, stream), "pack")
        return out

    # -- quanto::qbytes_conv2d (implicit GEMM) -----------------------------------------------------------
    @staticmethod
    def conv2d_out_size(size, k, stride, pad, dil):
        return (size + 2 * pad - dil * (k - 1) - 1) // stride + 1

    def _conv2d_scratch(self, x, B, OH, OW, OC, K, stream, geom=None):
        """(buffer, bytes) for the convolution kernels' K split - plain scratch, nothing to zero; (None, 0) when the problem needs none.  ``geom`` =
        (cin, W, KH, KW, stride_w, dil_w) of a sub-byte weight: plus the dense weight of the row form, when THIS geometry can take it."""
        if geom is None:
            nbytes = int(self._c.quanto_hip_conv2d_workspace_size(B, max(OH, 0), max(OW, 0), OC, K))
        else:
            cin, W, KH, KW, sw, dw = geom
            nbytes = int(self._c.quanto_hip_qbits_conv2d_workspace_size_geom(B, cin, W, OC, KH, KW, max(OH, 0), max(OW, 0), sw, dw))
        if nbytes <= 0:
            return None, 0
        return self._scratch(x.device, nbytes, stream), nbytes

    def _conv2d_output(self, x, OC, KH, KW, stride, padding, dilation, bias, scales=None):
        """What the three convolutions share: output sizes, the per-channel scales (one per OC, in x's dtype; None when not given), the bias in
        x's dtype and the output tensor."""
        B, _, H, W = x.shape
        OH = self.conv2d_out_size(H, KH, stride[0], padding[0], dilation[0])
        OW = self.conv2d_out_size(W, KW, stride[1], padding[1], dilation[1])
        if scales is not None:
            scales = scales.reshape(-1).to(x.dtype).contiguous()
            if scales.numel() == 1:
                scales = scales.expand(OC).contiguous()
        if bias is not None:
            bias = bias.to(x.dtype).contiguous()
        return OH, OW, scales, bias, torch.empty((B, OC, max(OH, 0), max(OW, 0)), dtype=x.dtype, device=x.device)

    @classmethod
    def conv2d_geometry_ok(cls, x_shape, w_shape, stride, padding, dilation) -> bool:
        """Python mirror of ``conv_geometry_ok`` (csrc/qh_conv.h): what the implicit-GEMM kernels index with 31-bit offsets and one grid
        dimension.  Beyond these limits the C entry returns ENOTSUP; the callers ask here first and keep the im2col / reference path instead."""
        B, C, H, W = x_shape
        OC, _, KH, KW = w_shape
        if min(stride) <= 0 or min(dilation) <= 0 or min(padding) < 0:
            return False
        OH = cls.conv2d_out_size(H, KH, stride[0], padding[0], dilation[0])
        OW = cls.conv2d_out_size(W, KW, stride[1], padding[1], dilation[1])
        K = C * KH * KW
        return (B >= 1 and OH >= 1 and OW >= 1 and K >= 1 and K < (1 << 24) and KH * KW <= 127 and B * C * H * W < (1 << 30) and B * OC * OH * OW < (1 << 31)
                and OC * K < (1 << 31) and (B * OH * OW + 127) // 128 <= 65535)

    @staticmethod
    def _qbytes_conv2d_dtypes_ok(x, w) -> bool:
        """NCHW 16-bit activations and an 8-bit OCP weight."""
        return (x.is_cuda and x.dim() == 4 and w.dim() == 4 and x.dtype in (torch.float16, torch.bfloat16) and
                w.dtype in (torch.int8, torch.float8_e4m3fn, torch.float8_e5m2))

    def qbytes_conv2d_supported(self, x, w, stride=(1, 1), padding=(0, 0), dilation=(1, 1)) -> bool:
        """What the kernel takes: NCHW 16-bit activations, an 8-bit OCP weight, and a geometry within ``conv2d_geometry_ok`` (windows of up
        to 127 taps, 31-bit offsets; any C * KH * KW: the last K-tile may be ragged, any weight alignment)."""
        return self._qbytes_conv2d_dtypes_ok(x, w) and self.conv2d_geometry_ok(tuple(x.shape), tuple(w.shape), stride, padding, dilation)

    def qbytes_conv2d_depthwise_supported(self, x, w, stride=(1, 1), padding=(0, 0), dilation=(1, 1)) -> bool:
        """Depthwise layers (r6): weight [OC, 1, KH, KW] on an input of C > 1 channels with OC a multiple of C; NCHW 16-bit activations, 8-bit OCP weight."""
        if not self._qbytes_conv2d_dtypes_ok(x, w):
            return False
        B, C, H, W = x.shape
        OC, wc, KH, KW = w.shape
        if wc != 1 or C < 2 or OC % C != 0 or min(stride) <= 0 or min(dilation) <= 0 or min(padding) < 0:
            return False
        OH = self.conv2d_out_size(H, KH, stride[0], padding[0], dilation[0])
        OW = self.conv2d_out_size(W, KW, stride[1], padding[1], dilation[1])
        # (H, W < 2^20: the C rule's clause, csrc/qconv_depthwise.hip - without it a column of 2^20 rows got ENOTSUP raised instead of the reference path)
        return (B >= 1 and OH >= 1 and OW >= 1 and B * C * H * W < (1 << 31) and B * OC * OH * OW < (1 << 31) and KH * KW <= 4096 and
                H < (1 << 20) and W < (1 << 20))

    def qbytes_conv2d(self, x, w, scales, bias, stride, padding, dilation):
        """Dense convolution with an 8-bit weight [OC, C, KH, KW] and per-channel scales: im2col happens inside the kernel's staging loads.  A weight
        [OC, 1, KH, KW] on an input of C > 1 channels is the depthwise layer (groups = C): the stencil kernel of csrc/qconv_depthwise.hip."""
        self._require_cuda(x, w, scales, bias)
        x, w = x.contiguous(), w.contiguous()
        B, C, H, W = x.shape
        OC, wc, KH, KW = w.shape
        depthwise = wc == 1 and C > 1
        OH, OW, s, bias, y = self._conv2d_output(x, OC, KH, KW, stride, padding, dilation, bias, scales)
        args = (_ptr(x), _ptr(w), _ptr(s), _ptr(bias), _ptr(y), B, C, H, W, OC, KH, KW, OH, OW, stride[0], stride[1], padding[0], padding[1],
                dilation[0], dilation[1], _dt(x), _dt(w), _dt(y))
        with _DeviceGuard(x.device) as stream:
            if depthwise:
                st = self._c.quanto_hip_qbytes_conv2d_depthwise(*args, stream)
            else:
                ws, ws_bytes = self._conv2d_scratch(x, B, OH, OW, OC, C * KH * KW, stream)
                st = self._c.quanto_hip_qbytes_conv2d(*args, _ptr(ws), ws_bytes, stream)
        self._check(st, "qbytes_conv2d_depthwise" if depthwise else "qbytes_conv2d")
        return y

    # -- quanto::qbytes_conv2d_a8 (quantized activations, 8-bit matrix instructions) ------------------------------
    def _conv2d_a8_workspace(self, x_shape, w_shape, a_dtype, b_dtype, out_dtype, stride, padding, dilation) -> int:
        """Split-K scratch bytes of csrc/qconv_a8.hip for this call, or a negative status (format / geometry not served, bad geometry); asked
        once per shape and kept."""
        adt, bdt, odt = _DTYPES.get(a_dtype), _DTYPES.get(b_dtype), _DTYPES.get(out_dtype)
        if adt is None or bdt is None or odt is None:
            return -2
        B, C, H, W = x_shape
        OC, _, KH, KW = w_shape
        OH = self.conv2d_out_size(H, KH, stride[0], padding[0], dilation[0])
        OW = self.conv2d_out_size(W, KW, stride[1], padding[1], dilation[1])
        args = (B, C, H, W, OC, KH, KW, max(OH, 0), max(OW, 0), stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], adt, bdt, odt)
        return self._plan("qbytes_conv2d_a8", args, lambda: (0, 0, int(self._c.quanto_hip_qbytes_conv2d_a8_workspace_size(*args))))[1]

    def qbytes_conv2d_a8_supported(self, x_data, w_data, out_dtype, stride=(1, 1), padding=(0, 0), dilation=(1, 1)) -> bool:
        """What csrc/qconv_a8.hip takes: NCHW int8 / e4m3fn / e5m2 activation codes on a ROCm device, an [OC, C, KH, KW] int8 (any activation
        format but int8 x fp8) or e4m3fn / e5m2 weight (fp8 activations), output dtype float32 / float16 / bfloat16, geometry within
        ``conv2d_geometry_ok``."""
        if not (x_data.is_cuda and x_data.dim() == 4 and w_data.dim() == 4 and x_data.shape[1] == w_data.shape[1]):
            return False
        if min(stride) <= 0 or min(dilation) <= 0 or min(padding) < 0:
            return False
        if not self.conv2d_geometry_ok(tuple(x_data.shape), tuple(w_data.shape), stride, padding, dilation):
            return False
        return self._conv2d_a8_workspace(tuple(x_data.shape), tuple(w_data.shape), x_data.dtype, w_data.dtype, out_dtype, stride, padding, dilation) >= 0

    def qbytes_conv2d_a8(self, x, x_scale, w, w_scale, bias, stride, padding, dilation):
        """Dense convolution of quantized activation codes ``x`` (per-tensor scale ``x_scale``, one element) with an 8-bit weight [OC, C, KH, KW]
        (per-channel scales ``w_scale``): y = conv(x, w) * round(x_scale * w_scale) (+ bias), in w_scale's dtype.  Raises QuantoHipError(ENOTSUP)
        for formats the kernel does not take."""
        return self._conv2d_a8("qbytes_conv2d_a8", x, x_scale, w, w_scale, bias, None, stride, padding, dilation)

    def qbytes_conv2d_a8_q(self, x, x_scale, w, w_scale, bias, out_scale, stride, padding, dilation):
        """``qbytes_conv2d_a8`` with the layer's output quantization in the kernel epilogue: codes in ``x.dtype`` of the convolution output at the
        per-tensor ``out_scale`` (one element), bit-identical to ``quantize_symmetric(qbytes_conv2d_a8(...), x.dtype, None, out_scale)``.  Same
        formats, plan cache entry and scratch as ``qbytes_conv2d_a8``."""
        if out_scale.numel() != 1:
            raise QuantoHipError("qbytes_conv2d_a8_q: the output scale is per-tensor (one element)")
        return self._conv2d_a8("qbytes_conv2d_a8_q", x, x_scale, w, w_scale, bias, out_scale, stride, padding, dilation)

    def _conv2d_a8(self, what, x, x_scale, w, w_scale, bias, out_scale, stride, padding, dilation):
        """The one host path of both entries: ``out_scale`` None -> the float output, else the codes."""
        self._require_cuda(x, x_scale, w, w_scale, bias, out_scale)
        if x_scale.numel() != 1:
            raise QuantoHipError(f"{what} expects a per-tensor activation scale")
        x, w = x.contiguous(), w.contiguous()
        B, C, H, W = x.shape
        OC, _, KH, KW = w.shape
        odt = w_scale.dtype
        ws_bytes = self._conv2d_a8_workspace(tuple(x.shape), tuple(w.shape), x.dtype, w.dtype, odt, stride, padding, dilation)
        if ws_bytes < 0:
            self._check(int(ws_bytes), what)
        OH = self.conv2d_out_size(H, KH, stride[0], padding[0], dilation[0])
        OW = self.conv2d_out_size(W, KW, stride[1], padding[1], dilation[1])
        s = w_scale.reshape(-1).contiguous()
        if s.numel() == 1:
            s = s.expand(OC).contiguous()
        xs = x_scale.reshape(1).to(odt).contiguous()
        if bias is not None:
            bias = bias.to(odt).contiguous()
        y = torch.empty((B, OC, max(OH, 0), max(OW, 0)), dtype=odt if out_scale is None else x.dtype, device=x.device)
        geometry = (B, C, H, W, OC, KH, KW, OH, OW, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], _dt(x), _dt(w), _DTYPES[odt])
        with _DeviceGuard(x.device) as stream:
            ws = self._scratch(x.device, ws_bytes, stream) if ws_bytes > 0 else None
            if out_scale is None:
                st = self._c.quanto_hip_qbytes_conv2d_a8(_ptr(x), _ptr(xs), _ptr(w), _ptr(s), _ptr(bias), _ptr(y), *geometry, _ptr(ws), ws_bytes, stream)
            else:
                os_ = out_scale.reshape(1).to(odt).contiguous()
                st = self._c.quanto_hip_qbytes_conv2d_a8_q(_ptr(x), _ptr(xs), _ptr(w), _ptr(s), _ptr(bias), _ptr(os_), _ptr(y), *geometry, _ptr(ws),
                                                           ws_bytes, stream)
        self._check(st, what)
        return y

    # -- quanto::qbits_conv2d (implicit GEMM, int4 dequantized while staged) -----------------------------------
    def qbits_conv2d_supported(self, x, weight_size, bits: int, group_size, stride=(1, 1), padding=(0, 0), dilation=(1, 1)) -> bool:
        """NCHW 16-bit activations, generic packed int4 / int2 weight [OC, C, KH, KW] with OC a multiple of the values per byte and groups of a
        multiple of 8 (or per-channel scales), geometry within ``conv2d_geometry_ok``."""
        oc, c, kh, kw = weight_size
        k = c * kh * kw
        return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float16, torch.bfloat16) and bits in (2, 4) and oc % (8 // bits) == 0 and
                (not group_size or (group_size % 8 == 0 and k % group_size == 0)) and oc * (k // (group_size or k)) < (1 << 31) and
                self.conv2d_geometry_ok(tuple(x.shape), tuple(weight_size), stride, padding, dilation))

    def qbits_conv2d(self, x, packed, scale, shift, bias, bits: int, group_size, weight_size, stride, padding, dilation):
        """Dense convolution with a generic packed int4 weight (its [OC, C, KH, KW] shape in ``weight_size``): im2col inside the staging loads,
        the weight dequantized there with the reference's roundings (r5: three-tap-wide windows at stride 1 dequantize the weight once into the
        scratch buffer and take the row form of the kernel on it)."""
        self._require_cuda(x, packed, scale, shift, bias)
        if x.dtype != scale.dtype:
            x = x.to(scale.dtype)
        x, packed, scale, shift = x.contiguous(), packed.contiguous(), scale.contiguous(), shift.contiguous()
        B, C, H, W = x.shape
        OC, _, KH, KW = weight_size
        OH, OW, _, bias, y = self._conv2d_output(x, OC, KH, KW, stride, padding, dilation, bias)
        with _DeviceGuard(x.device) as stream:
            ws, ws_bytes = self._conv2d_scratch(x, B, OH, OW, OC, C * KH * KW, stream, geom=(C, W, KH, KW, stride[1], dilation[1]))
            st = self._c.quanto_hip_qbits_conv2d(_ptr(x), _ptr(packed), _ptr(scale), _ptr(shift), _ptr(bias), _ptr(y), B, C, H, W, OC, KH, KW, OH, OW,
                                                 stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], bits, group_size or 0, _dt(x),
                                                 _dt(shift), _ptr(ws), ws_bytes, stream)
        self._check(st, "qbits_conv2d")
        return y

    # -- quanto::unpack ---------------------------------------------------------------------------
    def unpack(self, t: torch.Tensor, bits: int) -> torch.Tensor:
        self._require_cuda(t)
        if t.dtype != torch.uint8:
            raise QuantoHipError("unpack expects a torch.uint8 tensor")
        if bits not in (2, 4):
            raise ValueError(f"Can only unpack 2-bit or 4-bit tensors, got bits={bits}")
        t = t.contiguous()
        vpi = 8 // bits
        out_shape = (t.shape[0] * vpi,) + tuple(t.shape[1:]) if t.ndim > 0 else (vpi,)
        out = torch.empty(out_shape, dtype=torch.uint8, device=t.device)
        with _DeviceGuard(t.device) as stream:
            self._check(self._c.quanto_hip_unpack(_ptr(t), _ptr(out), t.numel(), bits, stream), "unpack")
        return out

    # -- fused unpack + dequantize ------------------------------------------------------------------
    def dequantize_qbits(self, packed, scale, shift, bits: int, group_size, out_features: int, in_features: int):
        self._require_cuda(packed, scale, shift)
        packed, scale, shift = packed.contiguous(), scale.contiguous(), shift.contiguous()
        out = torch.empty((out_features, in_features), dtype=scale.dtype, device=packed.device)
        with _DeviceGuard(packed.device) as stream:
            st = self._c.quanto_hip_dequantize_qbits(_ptr(packed), _ptr(scale), _ptr(shift), _ptr(out), out_features, in_features, bits,
                                                     group_size or 0, _dt(scale), _dt(shift), stream)
        self._check(st, "dequantize_qbits")
        return out

    # -- quanto::qbits_mm ---------------------------------------------------------------------------
    def qbits_mm(self, x, packed, scale, shift, bias, bits: int, group_size, out_features: int, in_features: int,
                 kernel: str = "auto"):
        if not (x.is_cuda and packed.is_cuda and scale.is_cuda and shift.is_cuda and (bias is None or bias.is_cuda)):
            raise QuantoHipError("quanto_hip kernels only accept tensors on a ROCm device")
        if x.dim() == 0 or x.shape[-1] != in_features:  # the kernel reads M * in_features elements: never from a smaller buffer
            raise QuantoHipError(f"qbits_mm: input of shape {tuple(x.shape)} does not end in in_features = {in_features}")
        sdt = scale.dtype
        if x.dtype != sdt:
            x = x.to(sdt)
        x2 = x if x.dim() == 2 and x.is_contiguous() else x.reshape(-1, in_features).contiguous()
        if not packed.is_contiguous():
            packed = packed.contiguous()
        if not scale.is_contiguous():
            scale = scale.contiguous()
        if not shift.is_contiguous():
            shift = shift.contiguous()
        if bias is not None and (bias.dtype != sdt or not bias.is_contiguous()):
            bias = bias.to(sdt).contiguous()
        M = x2.shape[0]
        gs = group_size or 0
        dt, zdt = _DTYPES.get(sdt), _DTYPES.get(shift.dtype)
        if dt is None or zdt is None:
            raise QuantoHipError(f"quanto_hip: unsupported dtype {sdt if dt is None else shift.dtype}")
        y = torch.empty((M, out_features), dtype=sdt, device=x.device)
        c = self._c
        k, ws_bytes = self._plan("qbits_mm", (M, out_features, in_features, bits, gs, dt, kernel),
                                 lambda: self._ask(c.quanto_hip_qbits_mm_plan, M, out_features, in_features, bits, gs, dt, KERNELS[kernel]))
        xp, pp = x2.data_ptr(), packed.data_ptr()
        if kernel == "auto" and (xp | pp) % 16:
            k, ws_bytes = KERNEL_NAIVE, 0  # misaligned view: the kernel without an alignment requirement (what AUTO does in C)
        with _DeviceGuard(x.device) as stream:
            if ws_bytes == 0:
                wp = 0
            elif k in (KERNEL_SKINNY, KERNEL_MFMA_FUSED4):
                wp = self._zeroed_workspace(x.device, ws_bytes, stream).data_ptr()  # split-K arrival counters: zero on entry, left zero by the kernel
            else:
                wp = self._scratch(x.device, ws_bytes, stream).data_ptr()
            st = c.quanto_hip_qbits_mm(xp, pp, scale.data_ptr(), shift.data_ptr(), 0 if bias is None else bias.data_ptr(), y.data_ptr(), M,
                                       out_features, in_features, bits, gs, dt, zdt, k, wp, ws_bytes, stream)
        if st != 0:
            self._check(st, "qbits_mm")
        return y if x.dim() == 2 else y.reshape(*x.shape[:-1], out_features)

    # -- quanto::qbits_mm_a8 (quantized activations x int4 / int2 weights) ---------------------------------
    A8_DTYPES = (torch.int8, torch.float8_e4m3fn, torch.float8_e5m2)

    def qbits_mm_a8_workspace(self, M: int, out_features: int, in_features: int, bits: int, group_size, a_dtype, dtype) -> int:
        """Split-K scratch bytes of the W4A8 / W2A8 kernel for this call shape, or a negative status when the format is not served (the caller then
        dequantizes the activation, as the reference does)."""
        adt, dt = _DTYPES.get(a_dtype), _DTYPES.get(dtype)
        if adt is None or dt is None:
            return -2
        gs = group_size or 0
        # one kernel: the size entry alone is the plan (its negative statuses are kept as the answer, not raised)
        return self._plan("qbits_mm_a8", (M, out_features, in_features, bits, gs, adt, dt),
                          lambda: (0, 0, int(self._c.quanto_hip_qbits_mm_a8_workspace_size(M, out_features, in_features, bits, gs, adt, dt))))[1]

    def qbits_mm_a8(self, a, a_scale, packed, scale, shift, bias, bits: int, group_size, out_features: int, in_features: int):
        """F.linear(quantized activation, int4 / int2 weight) on the 8-bit matrix instructions: ``a`` int8 / float8_e4m3fn / float8_e5m2 [..., K], ``a_scale`` its
        per-tensor scale (one element).  Raises QuantoHipError(ENOTSUP) for formats the kernel does not take."""
        return self._qbits_mm_a8("qbits_mm_a8", a, a_scale, packed, scale, shift, bias, bits, group_size, out_features, in_features)

    def qbits_mm_a8_q(self, a, a_scale, packed, scale, shift, bias, out_scale, bits: int, group_size, out_features: int, in_features: int, _out=None):
        """``quantize_symmetric(qbits_mm_a8(a, ...), a.dtype, None, out_scale)`` in one launch (csrc/qbits_a8_fused.hip, the epilogue that stores codes):
        the same plan cache, zeroed workspace and device guard as ``qbits_mm_a8``.  Raises QuantoHipError for what the library does not serve
        (QUANTO_HIP_ENOTSUP) or a misaligned view (QUANTO_HIP_EALIGN): ``ops.qbits_mm_a8_q_hip`` asks first and runs the two ops then.
        ``_out`` (tests): a contiguous [M, out_features] buffer of ``a.dtype`` to store into."""
        return self._qbits_mm_a8("qbits_mm_a8_q", a, a_scale, packed, scale, shift, bias, bits, group_size, out_features, in_features, out_scale, _out)

    def _qbits_mm_a8(self, what, a, a_scale, packed, scale, shift, bias, bits, group_size, out_features, in_features, out_scale=None, _out=None):
        """The one host path of both entries: ``out_scale`` None -> the float output in the scales' dtype, else the codes in ``a.dtype``."""
        if not (a.is_cuda and a_scale.is_cuda and packed.is_cuda and scale.is_cuda and shift.is_cuda and (bias is None or bias.is_cuda)
                and (out_scale is None or out_scale.is_cuda)):
            raise QuantoHipError("quanto_hip kernels only accept tensors on a ROCm device")
        if a.dim() == 0 or a.shape[-1] != in_features:
            raise QuantoHipError(f"{what}: input of shape {tuple(a.shape)} does not end in in_features = {in_features}")
        if a_scale.numel() != 1 or (out_scale is not None and out_scale.numel() != 1):
            raise QuantoHipError(f"{what} expects a per-tensor activation scale" + ("" if out_scale is None else " and a per-tensor output scale"))
        sdt = scale.dtype
        a2 = a if a.dim() == 2 and a.is_contiguous() else a.reshape(-1, in_features).contiguous()
        a_scale = a_scale.reshape(1).to(sdt).contiguous()
        packed, scale, shift = packed.contiguous(), scale.contiguous(), shift.contiguous()
        if bias is not None:
            bias = bias.to(sdt).contiguous()
        M = a2.shape[0]
        ws_bytes = self.qbits_mm_a8_workspace(M, out_features, in_features, bits, group_size, a2.dtype, sdt)
        if ws_bytes < 0:
            self._check(int(ws_bytes), what)
        if out_scale is None:
            y = torch.empty((M, out_features), dtype=sdt, device=a.device)
        else:
            out_scale = out_scale.reshape(1).to(sdt).contiguous()  # what quantize_symmetric does with a scale of another dtype
            y = torch.empty((M, out_features), dtype=a2.dtype, device=a.device) if _out is None else _out
        bp = 0 if bias is None else bias.data_ptr()
        with _DeviceGuard(a.device) as stream:
            wp = self._zeroed_workspace(a.device, ws_bytes, stream).data_ptr() if ws_bytes > 0 else 0
            if out_scale is None:
                st = self._c.quanto_hip_qbits_mm_a8(a2.data_ptr(), a_scale.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), bp, y.data_ptr(),
                                                    M, out_features, in_features, bits, group_size or 0, _DTYPES[a2.dtype], _DTYPES[sdt], _dt(shift), wp,
                                                    ws_bytes, stream)
            else:
                st = self._c.quanto_hip_qbits_mm_a8_q(a2.data_ptr(), a_scale.data_ptr(), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), bp,
                                                      out_scale.data_ptr(), y.data_ptr(), M, out_features, in_features, bits, group_size or 0,
                                                      _DTYPES[a2.dtype], _DTYPES[sdt], _dt(shift), wp, ws_bytes, stream)
        if st != 0:
            self._check(st, what)
        return y if a.dim() == 2 else y.reshape(*a.shape[:-1], out_features)

    # -- quanto::qbits_mm_multi ---------------------------------------------------------------------
    MAX_MULTI = 4  # QUANTO_HIP_MAX_MULTI

    def qbits_mm_multi(self, x, packed, scale, shift, bias, bits: int, group_size, out_features, in_features: int):
        """Several qbits_mm products sharing ``x`` (q/k/v, gate/up).  One kernel launch when every product is eligible for
        the decode GEMV (M <= 4, int4, group size 128: bit-identical to the separate calls) or, for batched decode (4 < M <= 64,
        every out_features a multiple of 64), for one launch of the streaming MFMA kernel over all members; otherwise the
        separate ops (each with its own kernel choice and workspace).  Returns the list of outputs."""
        n = len(packed)
        bias = list(bias) if bias is not None else [None] * n
        if not (len(scale) == len(shift) == len(bias) == len(out_features) == n) or n < 1:
            raise QuantoHipError("qbits_mm_multi: inconsistent argument lists")
        self._require_cuda(x, *packed, *scale, *shift, *bias)
        sdt = scale[0].dtype
        if x.dtype != sdt:
            x = x.to(sdt)
        lead = x.shape[:-1]
        x2 = x.reshape(-1, in_features).contiguous()
        M = x2.shape[0]
        kernel, ws_bytes = KERNEL_AUTO, 0
        if 1 <= M <= 64 and n <= self.MAX_MULTI and all(s.dtype == sdt for s in scale) and len({sh.dtype for sh in shift}) == 1:
            kernel, ws_bytes = self._multi_plan("qbits_mm_multi", self._c.quanto_hip_qbits_mm_multi_plan, out_features, M, in_features, bits,
                                                group_size or 0, _dt(scale[0]))
        if kernel == KERNEL_AUTO:
            return [self.qbits_mm(x, packed[i], scale[i], shift[i], bias[i], bits, group_size, out_features[i], in_features)
                    for i in range(n)]
        lists = ([t.contiguous() for t in packed], [t.contiguous() for t in scale], [t.contiguous() for t in shift],
                 [None if b is None else b.to(sdt).contiguous() for b in bias])
        return self._multi_launch("qbits_mm_multi", self._c.quanto_hip_qbits_mm_multi_ws, x2, lead, lists, out_features,
                                  (bits, group_size or 0, _dt(scale[0]), _dt(shift[0])), ws_bytes)

    def _multi_plan(self, which: str, entry, out_features, M: int, K: int, *args):
        """(kernel, workspace bytes) of the one launch that serves a group of products, from ``entry`` (a C ``*_multi_plan``); KERNEL_AUTO
        when none does (separate calls, each with its own plan), failed statuses included."""
        def ask():
            st, kernel, ws = self._ask(entry, len(out_features), (ctypes.c_int64 * len(out_features))(*out_features), M, K, *args)
            return (0, kernel, ws) if st == 0 else (0, KERNEL_AUTO, 0)

        return self._plan(which, (tuple(out_features), M, K) + args, ask)

    def _multi_launch(self, which: str, entry, x2, lead, lists, out_features, args, ws_bytes: int):
        """One launch of a C ``*_multi_ws`` entry over the members: x2 [M, K], one pointer array per tensor list (``lists``, then the outputs),
        ``args`` between K and the workspace; the outputs in x2's dtype, shaped as ``lead + (out_features[i],)``."""
        n, (M, K) = len(out_features), x2.shape
        ys = [torch.empty((M, nf), dtype=x2.dtype, device=x2.device) for nf in out_features]
        arrays = [(ctypes.c_void_p * n)(*[_ptr(t) for t in ts]) for ts in (*lists, ys)]
        with _DeviceGuard(x2.device) as stream:
            ws = self._zeroed_workspace(x2.device, ws_bytes, stream) if ws_bytes else None  # split-K arrival counters
            st = entry(_ptr(x2), n, *arrays, (ctypes.c_int64 * n)(*out_features), M, K, *args, _ptr(ws), ws_bytes, stream)
        self._check(st, which)
        return [y.reshape(*lead, nf) for y, nf in zip(ys, out_features)]

    # -- quanto::qbytes_mm_multi --------------------------------------------------------------------
    def qbytes_mm_multi(self, a, weights, scales, bias):
        """Several qbytes_mm products sharing the activation (q/k/v, gate/up of an int8 / fp8 model): one GEMV launch for M <= 2,
        one streaming-MFMA launch for M <= 64 when every out_features is a multiple of 64, otherwise the separate ops."""
        n = len(weights)
        bias = list(bias) if bias is not None else [None] * n
        if not (len(scales) == len(bias) == n) or n < 1:
            raise QuantoHipError("qbytes_mm_multi: inconsistent argument lists")
        self._require_cuda(a, *weights, *scales, *bias)
        K = weights[0].shape[1]
        sdt = scales[0].dtype
        one_call = (n <= self.MAX_MULTI and a.dtype.is_floating_point and a.dtype.itemsize > 1 and all(w.shape[1] == K for w in weights)
                    and all(w.dtype == weights[0].dtype for w in weights) and all(s.dtype == sdt for s in scales)
                    and all(s.numel() == w.shape[0] for s, w in zip(scales, weights)))
        kernel, ws_bytes = KERNEL_AUTO, 0
        out_features = [w.shape[0] for w in weights]
        if one_call:
            if a.dtype != sdt:
                a = a.to(sdt)
            lead = a.shape[:-1]
            a2 = a.reshape(-1, K).contiguous()
            M = a2.shape[0]
            if 1 <= M <= 64:
                kernel, ws_bytes = self._multi_plan("qbytes_mm_multi", self._c.quanto_hip_qbytes_mm_multi_plan, out_features, M, K, _dt(a2),
                                                    _dt(weights[0]), _dt(scales[0]))
        if kernel == KERNEL_AUTO:
            return [self.qbytes_mm(a, weights[i], scales[i], bias[i]) for i in range(n)]
        lists = ([w.contiguous() for w in weights], [s.reshape(-1).contiguous() for s in scales],
                 [None if b is None else b.to(sdt).contiguous() for b in bias])
        return self._multi_launch("qbytes_mm_multi", self._c.quanto_hip_qbytes_mm_multi_ws, a2, lead, lists, out_features,
                                  (_dt(a2), _dt(weights[0]), _dt(scales[0])), ws_bytes)

    # -- quanto::qbytes_mm / quanto::qbytes_mm_q ------------------------------------------------------
    @staticmethod
    def _qbytes_mm_operands(what, a, b, scales, bias, out_scale=None):
        """What both products check and normalise: (a2 [M, K], b, scales [N], bias, M, N, K, (a, b, scales) dtype codes) - every tensor on the device, one scale
        per output feature, ``a`` ending in K, float activations of another 16 / 32-bit dtype cast to the scales' (library/qbytes_mm.py:26)."""
        if not (a.is_cuda and b.is_cuda and scales.is_cuda and (bias is None or bias.is_cuda) and (out_scale is None or out_scale.is_cuda)):
            raise QuantoHipError("quanto_hip kernels only accept tensors on a ROCm device")
        N, K = b.shape
        if scales.numel() != N:
            raise QuantoHipError(f"{what} expects one scale per output feature ({N}), got {tuple(scales.shape)}")
        if a.dim() == 0 or a.shape[-1] != K:  # torch.matmul's shape error in the reference; here the kernel would read past the buffer
            raise QuantoHipError(f"{what}: input of shape {tuple(a.shape)} does not end in in_features = {K}")
        sdt = scales.dtype
        if a.dtype.is_floating_point and a.dtype.itemsize > 1 and a.dtype != sdt:
            a = a.to(sdt)
        a2 = a if a.dim() == 2 and a.is_contiguous() else a.reshape(-1, K).contiguous()
        if not b.is_contiguous():
            b = b.contiguous()
        s = scales if scales.dim() == 1 and scales.is_contiguous() else scales.reshape(-1).contiguous()
        if bias is not None and (bias.dtype != sdt or not bias.is_contiguous()):
            bias = bias.to(sdt).contiguous()
        adt, bdt, odt = _DTYPES.get(a2.dtype), _DTYPES.get(b.dtype), _DTYPES.get(sdt)
        if adt is None or bdt is None or odt is None:
            raise QuantoHipError(f"quanto_hip: unsupported dtype in {what}({a2.dtype}, {b.dtype}, {sdt})")
        return a2, b, s, bias, a2.shape[0], N, K, adt, bdt, odt

    def qbytes_mm(self, a, b, scales, bias=None, kernel: str = "auto"):
        a2, b, s, bias, M, N, K, adt, bdt, odt = self._qbytes_mm_operands("qbytes_mm", a, b, scales, bias)
        y = torch.empty((M, N), dtype=s.dtype, device=a.device)
        c = self._c
        k, ws_bytes = self._plan("qbytes_mm", (M, N, K, adt, bdt, odt, kernel),
                                 lambda: self._ask(c.quanto_hip_qbytes_mm_plan, M, N, K, adt, bdt, odt, KERNELS[kernel]))
        ap, bp = a2.data_ptr(), b.data_ptr()
        if kernel == "auto" and (ap | bp) % 16:
            k, ws_bytes = KERNEL_NAIVE, 0  # misaligned view: the kernel without an alignment requirement (what AUTO does in C)
        with _DeviceGuard(a.device) as stream:
            wp = self._zeroed_workspace(a.device, ws_bytes, stream).data_ptr() if ws_bytes > 0 else 0  # split-K arrival counters: zero on entry, left zero
            st = c.quanto_hip_qbytes_mm_ws(ap, bp, s.data_ptr(), 0 if bias is None else bias.data_ptr(), y.data_ptr(), M, N, K, adt, bdt, odt, k, wp,
                                           max(ws_bytes, 0), stream)
        if st != 0:
            self._check(st, "qbytes_mm")
        return y if a.dim() == 2 else y.reshape(*a.shape[:-1], N)

    def qbytes_mm_q_workspace(self, M: int, N: int, K: int, a_dtype, b_dtype, dtype) -> int:
        """Split-K scratch bytes of the code-storing W8A8 kernel for this call shape, or a negative status when the library does not serve it
        (QUANTO_HIP_ENOTSUP: fp32 scales, mixed operand dtypes, K not a multiple of 64, the size limits): the caller then runs the two ops.  The
        counterpart of ``qbits_mm_a8_workspace``: the status is kept as the answer, not raised.  The plan entry has one route - its kernel is
        NATIVE8 by construction (csrc/c_api.hip, quanto_hip_qbytes_mm_q_plan plans with it whatever it is asked) - so the cached plan is
        (NATIVE8, bytes or status) and the launch names that kernel itself."""
        def ask():  # (on a miss of the plan cache only: the key holds the torch dtypes)
            adt, bdt, odt = _DTYPES.get(a_dtype), _DTYPES.get(b_dtype), _DTYPES.get(dtype)
            if adt is None or bdt is None or odt is None:
                return 0, KERNEL_NATIVE8, -2
            st, _, ws = self._ask(self._c.quanto_hip_qbytes_mm_q_plan, M, N, K, adt, bdt, odt, KERNEL_AUTO)
            return 0, KERNEL_NATIVE8, ws if st == 0 else st

        return self._plan("qbytes_mm_q", (M, N, K, a_dtype, b_dtype, dtype), ask)[1]

    def qbytes_mm_q(self, a, b, scales, bias, out_scale, _ws_bytes=None):
        """``quantize_symmetric(qbytes_mm_bias(a, b, scales, bias), a.dtype, None, out_scale)`` in one launch (csrc/qmm_native8.hip, the epilogue that
        stores codes).  Raises QuantoHipError for what the library does not serve (QUANTO_HIP_ENOTSUP) or a misaligned view (QUANTO_HIP_EALIGN):
        ``ops.qbytes_mm_q_hip`` asks first and runs the two ops then.  ``_ws_bytes``: the answer of ``qbytes_mm_q_workspace`` for this call when
        the caller has it already (the op: one plan-cache lookup per call, not two)."""
        a2, b, s, bias, M, N, K, adt, bdt, odt = self._qbytes_mm_operands("qbytes_mm_q", a, b, scales, bias, out_scale)
        if out_scale.numel() != 1:
            raise QuantoHipError("qbytes_mm_q: the output scale is per-tensor (one element)")
        if out_scale.dtype != s.dtype:
            out_scale = out_scale.to(s.dtype)  # what quantize_symmetric does with a scale of another dtype
        ws_bytes = self.qbytes_mm_q_workspace(M, N, K, a2.dtype, b.dtype, s.dtype) if _ws_bytes is None else _ws_bytes
        if ws_bytes < 0:
            self._check(int(ws_bytes), "qbytes_mm_q")
        yq = torch.empty((M, N), dtype=a2.dtype, device=a.device)
        with _DeviceGuard(a.device) as stream:
            wp = self._zeroed_workspace(a.device, ws_bytes, stream).data_ptr() if ws_bytes > 0 else 0  # split-K arrival counters: zero on entry, left zero
            st = self._c.quanto_hip_qbytes_mm_q_ws(a2.data_ptr(), b.data_ptr(), s.data_ptr(), 0 if bias is None else bias.data_ptr(), out_scale.data_ptr(),
                                                   yq.data_ptr(), M, N, K, adt, bdt, odt, KERNEL_NATIVE8, wp, ws_bytes, stream)
        if st != 0:
            self._check(st, "qbytes_mm_q")
        return yq if a.dim() == 2 else yq.reshape(*a.shape[:-1], N)

    # -- quanto::qbytes_bmm (int8 x int8 batched product of two quantized activations) ------------------------
    BMM_MAX_K = 131071  # the last K for which K * 128 * 128 fits the int32 accumulator (csrc/qbytes_bmm.hip)
    BMM_OUT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)

    def qbytes_bmm(self, a, b, scale, out_dtype):
        """``(bmm(a.float(), b.float()) * scale).to(out_dtype)`` for int8 ``a`` [B, M, K] and ``b`` [B, K, N] and a one-element ``scale`` on the
        device (never read on the host), as one launch of csrc/qbytes_bmm.hip.  The operands are passed as the views they are - pointer and strides,
        an expanded batch (stride 0) included: ``a`` with K contiguous, ``b`` with K contiguous (a transposed view) or N contiguous; a view whose
        unit-stride dimension is neither is copied first.  Raises QuantoHipError for what the library does not serve: ``ops.qbytes_bmm_hip`` asks
        its predicate first."""
        self._require_cuda(a, b, scale)
        if not (a.dtype == b.dtype == torch.int8 and a.dim() == b.dim() == 3 and a.shape[0] == b.shape[0] and a.shape[2] == b.shape[1]):
            raise QuantoHipError(f"qbytes_bmm expects int8 [B, M, K] x [B, K, N], got {a.dtype}{tuple(a.shape)} x {b.dtype}{tuple(b.shape)}")
        if scale.numel() != 1 or out_dtype not in self.BMM_OUT_DTYPES:
            raise QuantoHipError("qbytes_bmm expects a one-element scale and a float32 / float16 / bfloat16 output")
        B, M, K = a.shape
        N = b.shape[2]
        if K > 1 and a.stride(2) != 1:
            a = a.contiguous()
        # (a dimension of one element is contiguous whatever stride torch reports for it)
        if K == 1 or b.stride(1) == 1:
            w_k, w_n = 1, b.stride(2)
        elif N == 1 or b.stride(2) == 1:
            w_k, w_n = b.stride(1), 1
        else:
            b = b.contiguous()
            w_k, w_n = N, 1
        scale = scale.reshape(1).to(torch.float32)
        y = torch.empty((B, M, N), dtype=out_dtype, device=a.device)
        with _DeviceGuard(a.device) as stream:
            st = self._c.quanto_hip_qbytes_bmm(a.data_ptr(), b.data_ptr(), scale.data_ptr(), y.data_ptr(), B, M, N, K, a.stride(0), a.stride(1),
                                               b.stride(0), w_k, w_n, _DTYPES[out_dtype], stream)
        if st != 0:
            self._check(st, "qbytes_bmm")
        return y

    # -- quanto::layer_norm_q (QLayerNorm with its output quantization in the same launch) ----------------------
    LAYER_NORM_Q_MAX_N = 8192  # QUANTO_HIP_LAYER_NORM_Q_MAX_N: the row one workgroup holds in registers (csrc/layernorm_q.hip)
    LAYER_NORM_Q_DTYPES = (torch.float32, torch.float16, torch.bfloat16)

    def layer_norm_q_supported(self, rows: int, n: int, dtype, out_dtype) -> bool:
        """Python mirror of ``quanto_hip_layer_norm_q_supported``: the sizes and formats csrc/layernorm_q.hip serves."""
        return (dtype in self.LAYER_NORM_Q_DTYPES and out_dtype in self.QUANTIZE_TARGETS and 0 <= n <= self.LAYER_NORM_Q_MAX_N
                and 0 <= rows < (1 << 31))

    def layer_norm_q(self, x, normalized_shape, weight, bias, eps: float, out_scale, dtype):
        """``quantize_symmetric(F.layer_norm(x, normalized_shape, weight, bias, eps), dtype, None, out_scale)`` as one launch of
        csrc/layernorm_q.hip: codes of ``dtype`` in x's shape, dense.  ``x`` is passed as the [rows, n] view it is when its leading dimensions
        collapse to one row stride >= n (a slice of a wider buffer, an offset view) and copied otherwise; the normalized dimensions must be
        contiguous.  ``out_scale``: one element on the device, never read on the host.  Raises QuantoHipError for what the library does not
        serve: ``ops.layer_norm_q_hip`` asks its predicate first."""
        self._require_cuda(x, weight, bias, out_scale)
        normalized_shape = tuple(normalized_shape)
        nd = len(normalized_shape)
        if nd == 0 or nd > x.dim() or tuple(x.shape[x.dim() - nd:]) != normalized_shape:
            raise QuantoHipError(f"layer_norm_q: input of shape {tuple(x.shape)} does not end in normalized_shape = {normalized_shape}")
        n = 1
        for d in normalized_shape:
            n *= d
        T = x.dtype
        if any(p is not None and (p.dtype != T or p.numel() != n) for p in (weight, bias)) or out_scale.numel() != 1:
            raise QuantoHipError("layer_norm_q expects weight and bias of normalized_shape in the input's dtype and a one-element output scale")
        rows = x.numel() // n if n else 0
        if not self.layer_norm_q_supported(rows, n, T, dtype):
            self._check(-2, "layer_norm_q")
        yq = torch.empty(x.shape, dtype=dtype, device=x.device)
        if rows == 0:
            return yq
        x2 = x.reshape(rows, n)  # a view wherever the leading dimensions collapse, a copy otherwise
        if (n > 1 and x2.stride(1) != 1) or (rows > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
        weight = None if weight is None else weight.contiguous()
        bias = None if bias is None else bias.contiguous()
        out_scale = out_scale.reshape(1).to(T)  # what quantize_symmetric does with a scale of another dtype
        with _DeviceGuard(x.device) as stream:
            st = self._c.quanto_hip_layer_norm_q(x2.data_ptr(), _ptr(weight), _ptr(bias), out_scale.data_ptr(), yq.data_ptr(), rows, n,
                                                 x2.stride(0) if rows > 1 else n, eps, _DTYPES[T], _DTYPES[dtype], stream)
        if st != 0:
            self._check(st, "layer_norm_q")
        return yq


class QuantoHipExtension(NativeLibrary):
    """The ``quanto_hip`` extension (name expected by the reference's tests/library/test_extensions.py:23-24)."""

    def __init__(self):
        csrc = os.path.join(_PKG_DIR, "csrc")
        super().__init__(
            "quanto_hip",
            root_dir=csrc,
            lib_path=os.path.join(_PKG_DIR, "lib", "libquanto_hip.so"),
            sources=["c_api.hip", "unpack.hip", "naive_mm.hip", "qbits_gemv.hip", "qbytes_gemv.hip", "qmm_mfma.hip", "qconv_mfma.hip", "qconv_a8.hip", "qconv_depthwise.hip", "qmm_mfma_large.hip", "qmm_large_common.h", "qbits_skinny.hip", "qbits_mmv.hip", "qbits_mfma_fused.hip", "qbits_a8_fused.hip", "qbits_mfma_large.hip", "qbytes_skinny.hip", "qmm_native8.hip", "qmm_f32.hip", "quantize.hip", "qbytes_bmm.hip", "layernorm_q.hip",
                     "qh_common.h", "qh_conv.h", "qh_group_fused.h", "qh_kernels.h", "qh_mfma.h", "qh_quantize.h", os.path.join("..", "..", "include", "quanto_hip.h")],
        )
        self._bindings = None

    @property
    def lib(self) -> _Bindings:
        if self._bindings is None:
            try:
                self._bindings = _Bindings(self.cdll)
            except OSError as e:
                raise QuantoHipError(
                    f"quanto_hip: cannot load {self.lib_path} ({e}). Build it with `python -c 'import __graft_entry__ as g; "
                    "g.build()'` (hipcc --offload-arch=gfx950). There is no fallback for ROCm tensors.") from e
        return self._bindings


quanto_hip = QuantoHipExtension()
# The reference registers its HIP extension only when a ROCm device is visible
# (library/extensions/__init__.py:24-28); same gate here, plus "the binary exists" so that a GPU box without
# the library fails loudly at first use instead of silently running something else.
if torch.version.hip is not None:
    register_extension(quanto_hip)

"""The status every argument check of the product entries with a code-storing form answers: ``quanto_hip_qbits_mm_a8`` / ``_a8_q`` and
``quanto_hip_qbytes_conv2d_a8`` / ``_a8_q`` (each pair is one body in csrc/c_api.hip) and ``quanto_hip_qbytes_mm_q_ws``.  One table per product of
argument sets that return before any launch - refused sizes, formats and geometry, empty products, null and misaligned pointers - with the status of
the float form and of the code form as literals, recorded from the library before the pairs shared a body.  The rows where the two differ are the
contract of the code forms: what they do not serve is ENOTSUP ahead of any look at M == 0 (qbits_mm_a8_q) and at the data pointers (both), so that the
caller runs the two-op sequence; the float forms answer the empty product and the null pointers first and leave the refusal to their launcher."""
import ctypes

import pytest

from optimum_quanto_amd.library.hip import BF16, F32, I8
from optimum_quanto_amd.library.hip import F8_E4M3FN as E4M3
from optimum_quanto_amd.library.hip import F8_E4M3FNUZ as E4M3FNUZ
from optimum_quanto_amd.library.hip import KERNEL_NATIVE8 as NATIVE8
from optimum_quanto_amd.library.hip import quanto_hip

OK, EINVAL, ENOTSUP, EALIGN = 0, -1, -2, -4  # QUANTO_HIP_* (include/quanto_hip.h)
_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
PTR = 1 << 20  # a 16-byte aligned address that is never dereferenced: every case below is refused, or done, before a launch
NULLS = dict(data=None, out_scale=None, y=None)


def _entry(name, argtypes):
    fn = getattr(quanto_hip.cdll, "quanto_hip_" + name)
    fn.restype, fn.argtypes = _ci, argtypes
    return fn


def _mm_a8(codes, M=300, N=512, K=4096, bits=4, group_size=128, a_dtype=I8, dtype=BF16, data=PTR, out_scale=PTR, y=PTR):
    fn = _entry("qbits_mm_a8_q" if codes else "qbits_mm_a8", [_vp] * (8 if codes else 7) + [_i64] * 3 + [_ci] * 5 + [_vp, _sz, _vp])
    return fn(data, data, data, data, data, None, *((out_scale,) if codes else ()), y, M, N, K, bits, group_size, a_dtype, dtype, dtype, None, 0, None)


def _conv2d_a8(codes, B=2, C=16, H=12, W=12, OC=32, KH=3, KW=3, OH=10, OW=10, stride=1, a_dtype=I8, b_dtype=I8, dtype=BF16, data=PTR, out_scale=PTR,
               y=PTR):
    fn = _entry("qbytes_conv2d_a8_q" if codes else "qbytes_conv2d_a8", [_vp] * (7 if codes else 6) + [_i64] * 9 + [_ci] * 9 + [_vp, _sz, _vp])
    return fn(data, data, data, data, None, *((out_scale,) if codes else ()), y, B, C, H, W, OC, KH, KW, OH, OW, stride, stride, 0, 0, 1, 1, a_dtype,
              b_dtype, dtype, None, 0, None)


def _mm_q(M=300, N=512, K=4096, a_dtype=I8, b_dtype=I8, dtype=BF16, kernel=0, data=PTR, out_scale=PTR, y=PTR):
    fn = _entry("qbytes_mm_q_ws", [_vp] * 6 + [_i64] * 3 + [_ci] * 4 + [_vp, _sz, _vp])
    return fn(data, data, data, None, out_scale, y, M, N, K, a_dtype, b_dtype, dtype, kernel, None, 0, None)


# (what, arguments, status of the float form - None: it has no such argument, or would launch -, status of the code form)
MM_A8 = [
    ("negative M", dict(M=-1), EINVAL, EINVAL),
    ("bits 3", dict(bits=3), EINVAL, EINVAL),
    ("K not a multiple of the group", dict(K=4000), EINVAL, EINVAL),
    ("fp32 dtype", dict(dtype=F32), ENOTSUP, ENOTSUP),
    ("fp32 dtype, M = 0", dict(dtype=F32, M=0), OK, ENOTSUP),
    ("fp32 dtype, null pointers", dict(dtype=F32, **NULLS), EINVAL, ENOTSUP),
    ("group size 64", dict(group_size=64), ENOTSUP, ENOTSUP),
    ("group size 64, M = 0", dict(group_size=64, M=0), OK, ENOTSUP),
    ("group size 64, null pointers", dict(group_size=64, **NULLS), EINVAL, ENOTSUP),
    ("float activations", dict(a_dtype=BF16), ENOTSUP, ENOTSUP),
    ("float activations, M = 0", dict(a_dtype=BF16, M=0), OK, ENOTSUP),
    ("float activations, null pointers", dict(a_dtype=BF16, **NULLS), EINVAL, ENOTSUP),
    ("int2 with N = 24", dict(bits=2, N=24), ENOTSUP, ENOTSUP),
    ("int2 with N = 24, M = 0, null pointers", dict(bits=2, N=24, M=0, **NULLS), OK, ENOTSUP),
    ("served, M = 0, null pointers", dict(M=0, **NULLS), OK, OK),
    ("served, null data", dict(data=None), EINVAL, EINVAL),
    ("served, null output", dict(y=None), EINVAL, EINVAL),
    ("served, misaligned operands", dict(data=PTR + 8), EALIGN, EALIGN),
    ("served, null output scale", dict(out_scale=None), None, EINVAL),
    ("served, misaligned output", dict(y=PTR + 1), None, EALIGN),
]
TAPS_144 = dict(H=16, W=16, KH=12, KW=12, OH=5, OW=5)  # beyond conv_geometry_ok (127 taps)
CONV2D_A8 = [
    ("negative batch", dict(B=-1), EINVAL, EINVAL),
    ("output size that does not follow", dict(OH=9), EINVAL, EINVAL),
    ("zero stride", dict(stride=0), EINVAL, EINVAL),
    ("int8 activations x fp8 weight", dict(b_dtype=E4M3), ENOTSUP, ENOTSUP),
    ("int8 activations x fp8 weight, null pointers", dict(b_dtype=E4M3, **NULLS), ENOTSUP, ENOTSUP),
    ("e4m3fnuz activations, empty batch", dict(a_dtype=E4M3FNUZ, B=0), ENOTSUP, ENOTSUP),
    ("integer output dtype", dict(dtype=I8), ENOTSUP, ENOTSUP),
    ("144 taps", dict(**TAPS_144), ENOTSUP, ENOTSUP),
    ("144 taps, null pointers", dict(**TAPS_144, **NULLS), EINVAL, ENOTSUP),
    ("144 taps, empty batch", dict(**TAPS_144, B=0, **NULLS), OK, OK),
    ("served, empty batch, null pointers", dict(B=0, **NULLS), OK, OK),
    ("served, empty output, null pointers", dict(H=2, W=2, OH=0, OW=0, **NULLS), OK, OK),
    ("served, null data", dict(data=None), EINVAL, EINVAL),
    ("served, null output", dict(y=None), EINVAL, EINVAL),
    ("served fp32 output, null data", dict(dtype=F32, data=None), EINVAL, EINVAL),
    ("served, null output scale", dict(out_scale=None), None, EINVAL),
]
MM_Q = [
    ("negative M", dict(M=-1), EINVAL),
    ("an id that is no kernel", dict(kernel=99), EINVAL),
    ("a kernel that stores no codes", dict(kernel=1), ENOTSUP),
    ("fp32 scales", dict(dtype=F32), ENOTSUP),
    ("fp32 scales, M = 0, null pointers", dict(dtype=F32, M=0, **NULLS), ENOTSUP),
    ("mixed operand dtypes", dict(b_dtype=E4M3), ENOTSUP),
    ("K = 100", dict(K=100, **NULLS), ENOTSUP),
    ("served, M = 0, null pointers", dict(M=0, **NULLS), OK),
    ("served, forced native8, M = 0", dict(M=0, kernel=NATIVE8), OK),
    ("served, null data", dict(data=None), EINVAL),
    ("served, null output scale", dict(out_scale=None), EINVAL),
    ("served, null output", dict(y=None), EINVAL),
    ("served, misaligned operands", dict(data=PTR + 8), EALIGN),
    ("served, misaligned output", dict(y=PTR + 1), EALIGN),
]


@pytest.mark.parametrize("call,table", [(_mm_a8, MM_A8), (_conv2d_a8, CONV2D_A8)], ids=["qbits_mm_a8", "qbytes_conv2d_a8"])
def test_both_forms_of_a_pair_answer_what_they_answered_as_two_bodies(call, table):
    for what, args, float_form, code_form in table:
        if float_form is not None:
            assert call(False, **args) == float_form, what
        assert call(True, **args) == code_form, what
    # the order differences are in the table
    assert any(f is not None and f != c for _, _, f, c in table)


def test_qbytes_mm_q_ws_statuses():
    for what, args, status in MM_Q:
        assert _mm_q(**args) == status, what

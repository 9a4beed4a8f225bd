"""The two CPU references of the elementwise quantize / dequantize tests agree, before either is used against the device.

Criterion everywhere: the numpy oracle (``O.quantize_symmetric_int8``, ``O.quantize_symmetric_fp8``, ``O.quantize_affine``, ``O.dequantize_qbytes_ref``) gives the
very bytes of the reference library's torch sequence on CPU tensors - the ``default=`` implementations of library/ops.py and ``scale * data.to(dtype)`` - on every
input set of tests/test_elementwise_values_gpu.py (the builders live in tests/helpers.py; both files import the same ones).  Where the two differ, torch is the
contract and the oracle is what gets fixed.  No tolerances: bit equality of the output bytes (NaN outputs of the dequantizer: NaN on both sides).
"""
import numpy as np
import pytest
import torch

from optimum_quanto_amd.library import ops
from oracle import quanto_oracle as O

from helpers import (AFFINE_ROTATIONS, FINITE_CODES, SCALES_16, SCALES_32, TARGETS, TORCH_DT, affine_case_16, affine_case_32, axis_first_case, axis_last_case,
                     dequantize_codes, dequantize_scales, finite_values_16, scale_tensor, symmetric_boundaries, tie_inputs, value_vector_16)


def f32(t: torch.Tensor) -> np.ndarray:
    return t.to(torch.float32).numpy()


def torch_symmetric(x, target, axis, scale) -> np.ndarray:
    """uint8 image of the reference sequence's codes."""
    return ops.quantize_symmetric(x, TARGETS[target], axis, scale).view(torch.uint8).numpy()


def oracle_symmetric(x, target, scale, dt) -> np.ndarray:
    with np.errstate(over="ignore"):  # quotients beyond fp32 / fp16 are part of the sets
        if target == "int8":
            return O.quantize_symmetric_int8(f32(x), f32(scale), dt).view(np.uint8)
        return O.quantize_symmetric_fp8(f32(x), f32(scale), target, dt)


def test_the_value_sets_hold_every_finite_pattern():
    assert finite_values_16("fp16").numel() == 63488 and finite_values_16("bf16").numel() == 65280
    for dt in ("fp16", "bf16"):
        v = value_vector_16(dt)
        assert v.numel() % 8 == 3 and v.view(torch.int16).unique().numel() == v.numel() - 3
        assert (v == 0).sum() == 3 and bool((v.view(torch.int16) == -32768).any())  # +0 (twice: the padding), -0
        tiny = torch.finfo(TORCH_DT[dt]).tiny
        assert ((v != 0) & (v.abs().to(torch.float64) < tiny)).sum() >= 2 * ((1 << (10 if dt == "fp16" else 7)) - 1)  # every subnormal


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_symmetric_every_16_bit_value_per_tensor(dt, target):
    x = value_vector_16(dt)
    for i, s in enumerate(scale_tensor(SCALES_16[dt], dt)):
        want = torch_symmetric(x, target, None, s)
        np.testing.assert_array_equal(oracle_symmetric(x, target, s, dt), want, err_msg=f"scale {SCALES_16[dt][i]}")
        if i == 0:  # scale 1: every finite code of the target occurs
            assert np.unique(want).size == FINITE_CODES[target]


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_symmetric_every_16_bit_value_per_axis(dt, target):
    for axis, (x, s) in ((0, axis_first_case(dt)), (-1, axis_last_case(dt))):
        np.testing.assert_array_equal(oracle_symmetric(x, target, s, dt), torch_symmetric(x, target, axis, s), err_msg=f"axis {axis}")


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_symmetric_on_and_next_to_every_tie(dt, target):
    b = symmetric_boundaries(target)
    for scale in SCALES_32:
        x, s = tie_inputs(b, scale, dt), scale_tensor([scale], dt)[0]
        assert x.numel() > (6 if dt == "fp32" else 1) * b.size
        np.testing.assert_array_equal(oracle_symmetric(x, target, s, dt), torch_symmetric(x, target, None, s), err_msg=f"scale {scale}")


def test_fp32_tie_set_lands_on_the_ties():
    """At scale 1 the centre of each group of seven is the boundary itself: a tie of the int8 rounding, and for float8 a value or a midpoint."""
    x = tie_inputs(symmetric_boundaries("int8"), 1.0).reshape(-1, 7)
    assert bool((x[:, 0] == torch.arange(-130, 130) + 0.5).all()) and bool((x[:, 1:4] < x[:, :1]).all()) and bool((x[:, 4:] > x[:, :1]).all())
    got = torch_symmetric(x[:, 0], "int8", None, torch.tensor(1.0)).view(np.int8)
    assert (got[got < 127] % 2 == 0).all() and (got[x[:, 0] > 127] == 127).all()  # half to even below the clamp (-128 is even), 127 from 127.5 up
    assert set(got.tolist()) == set(range(-128, 127, 2)) | {127}


def oracle_affine(base, bits, scale, shift, dt, group_size=128) -> np.ndarray:
    sh = shift.numpy() if not shift.dtype.is_floating_point else f32(shift)
    return O.quantize_affine(f32(base), bits, 0, group_size, f32(scale), sh, dt)


@pytest.mark.parametrize("int_shift", [False, True], ids=["shift", "zp"])
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_affine_every_16_bit_value(dt, bits, int_shift):
    seen = set()
    for r in range(AFFINE_ROTATIONS):
        base, scale, shift = affine_case_16(dt, bits, int_shift, r)
        want = ops.quantize_affine(base, bits, 0, 128, scale, shift).numpy()
        np.testing.assert_array_equal(oracle_affine(base, bits, scale, shift, dt), want, err_msg=f"rotation {r}")
        seen.update(np.unique(want).tolist())
    assert seen == set(range(1 << bits))  # over the rotations: a single one leaves a group's few in-range values to chance (rotation 0, int4, float shift: no 4)


@pytest.mark.parametrize("int_shift", [False, True], ids=["shift", "zp"])
@pytest.mark.parametrize("bits", [2, 4])
def test_affine_fp32_ties(bits, int_shift):
    base, scale, shift = affine_case_32(bits, int_shift)
    want = ops.quantize_affine(base, bits, 0, 128, scale, shift).numpy()
    np.testing.assert_array_equal(oracle_affine(base, bits, scale, shift, "fp32"), want)
    assert np.unique(want).size == 1 << bits


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("kind", list(TARGETS))
def test_dequantize_every_code(kind, dt):
    codes = dequantize_codes(512 + 15)
    data = codes.view(TARGETS[kind])
    for s in dequantize_scales(dt):
        want = f32(s * data.to(TORCH_DT[dt]))
        with np.errstate(over="ignore"):  # products beyond fp16 are part of the set
            got = O.dequantize_qbytes_ref(codes.numpy().view(np.int8) if kind == "int8" else codes.numpy(), f32(s), dt, None if kind == "int8" else kind)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        np.testing.assert_array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32), err_msg=f"scale {float(s)}")

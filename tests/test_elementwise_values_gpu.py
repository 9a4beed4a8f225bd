"""The elementwise quantize / dequantize kernels (csrc/quantize.hip, csrc/qh_quantize.h) at every input value, against the CPU.

Criterion everywhere: the device bytes equal the bytes of the reference library's torch sequence run on CPU tensors - the ``default=`` implementations of
library/ops.py (``quantize_symmetric``, ``quantize_affine``), ``tensor.packing.pack_weights`` and ``scale * data.to(dtype)`` - bit for bit, every element; no
tolerances.  The reference is never an op computed by the library under test: qh_quantize.h is one rule with three users (the standalone quantizer and the two
code-storing GEMM epilogues), and the fused-output tests compare those users with each other.  tests/test_elementwise_values_cpu.py shows on the same inputs (the
builders of tests/helpers.py) that the numpy oracle and the torch sequence agree.

Inputs: every finite fp16 / bf16 bit pattern (both zeros, every subnormal, quotients that overflow fp16) under eight per-tensor scales per dtype, as rows under
per-row scales and as rotated columns under per-column scales; fp32 (and the same rounded to 16 bits) on every tie of the target and three neighbours on each
side, under power-of-two and other scales; for the affine quantizers every 16-bit value up to 64 under every pairing of five scales with four shifts, and fp32
ties; every byte value through the dequantizer under every scale.  NaN / inf inputs and misaligned views are outside this file.

Denormal policy of the symmetric quantizer (``check_symmetric``): the same torch sequence also runs on the device.  Inputs at which it differs from the CPU
sequence are left out of the comparison with the kernel - their number is printed - and the case fails unless they are under 1 % of its inputs and every one of
them has |x| or |x / s| subnormal in fp32 or in the tensor dtype.

The last two tests anchor the fused epilogues to the CPU with no device op on the reference side: ``lib.qbytes_mm_q`` (int8 x int8) against the CPU quantizer
applied to ``O.qbytes_int_mm_ref`` (+ bias), ``lib.qbits_mm_a8_q`` (int8 activations, unsplit) against the CPU quantizer applied to ``O.qbits_mm_a8_chain`` -
the two oracles that reproduce the unfused kernels bit for bit (test_activations.py, test_w4a8_gpu.py).
"""
import numpy as np
import pytest
import torch

from optimum_quanto_amd.library import ops
from optimum_quanto_amd.library.hip import quanto_hip
from optimum_quanto_amd.tensor.packing import pack_weights
from oracle import quanto_oracle as O

from helpers import (AFFINE_ROTATIONS, FINITE_CODES, SCALES_16, SCALES_32, TARGETS, TORCH_DT, affine_case_16, affine_case_32, axis_first_case, axis_last_case,
                     dequantize_codes, dequantize_scales, make_qbits_problem, scale_tensor, symmetric_boundaries, tie_inputs, to_torch, value_vector_16)
from test_output_fusion_gpu import problem as w8a8_problem

pytestmark = pytest.mark.gpu
DEV = "cuda"


def u8(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().view(torch.uint8)


def check_symmetric(x, target, axis, scale, what, entries=("op", "lib")):
    """The kernel through the op and through the binding against the CPU sequence, under the denormal policy of the module docstring; returns the CPU codes."""
    tdt = TARGETS[target]
    want = u8(ops.quantize_symmetric(x, tdt, axis, scale))
    xd, sd = x.to(DEV), scale.to(DEV)
    left_out = u8(ops.quantize_symmetric(xd, tdt, axis, sd)) != want  # the torch sequence itself, on the device
    n_out = int(left_out.sum())
    print(f"{what}: {x.numel()} inputs, {n_out} left out (the device's torch sequence differs from the CPU's)")
    if n_out:
        tiny = max(torch.finfo(torch.float32).tiny, torch.finfo(x.dtype).tiny)
        ax, aq = x.to(torch.float64).abs(), (x.to(torch.float64) / scale.to(torch.float64)).abs()
        subnormal = ((ax > 0) & (ax < tiny)) | ((aq > 0) & (aq < tiny))
        assert n_out < 0.01 * x.numel(), f"{what}: {n_out} of {x.numel()} inputs left out"
        assert bool(subnormal[left_out].all()), f"{what}: {int((left_out & ~subnormal).sum())} inputs without a subnormal |x| or |x / s| differ between the two torch runs"
    for entry in entries:
        got = torch.ops.quanto.quantize_symmetric(xd, tdt, axis, sd) if entry == "op" else quanto_hip.lib.quantize_symmetric(xd, tdt, axis, sd)
        assert got.dtype == tdt and got.shape == x.shape
        bad = (u8(got) != want) & ~left_out
        if bad.any():
            i = bad.reshape(-1).nonzero()[:8, 0]
            s = scale.expand_as(x).reshape(-1)[i] if scale.ndim else scale.repeat(i.numel())
            raise AssertionError(f"{what} ({entry}): {int(bad.sum())} of {x.numel()} codes differ from the CPU sequence; x {x.reshape(-1)[i].tolist()} "
                                 f"scale {s.tolist()} got {u8(got).reshape(-1)[i].tolist()} want {want.reshape(-1)[i].tolist()}")
    return want


# ---- quantize_symmetric ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_symmetric_every_16_bit_value_per_tensor(dt, target):
    x = value_vector_16(dt)
    for value, s in zip(SCALES_16[dt], scale_tensor(SCALES_16[dt], dt)):
        want = check_symmetric(x, target, None, s, f"{dt} -> {target}, scale {value}")
        if value == 1.0:
            assert want.unique().numel() == FINITE_CODES[target], "at scale 1 every finite code of the target occurs"


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_symmetric_every_16_bit_value_per_row(dt, target):
    x, s = axis_first_case(dt)
    assert x.shape[1] % 8 and s.shape == (8, 1)
    check_symmetric(x, target, 0, s, f"{dt} -> {target}, axis 0")


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_symmetric_every_16_bit_value_per_column(dt, target):
    x, s = axis_last_case(dt)
    assert x.shape[1] == 7 and s.shape == (1, 7)
    check_symmetric(x, target, -1, s, f"{dt} -> {target}, axis -1")


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_symmetric_on_and_next_to_every_tie(dt, target):
    b = symmetric_boundaries(target)
    for value in SCALES_32:
        check_symmetric(tie_inputs(b, value, dt), target, None, scale_tensor([value], dt)[0], f"{dt} -> {target} ties, scale {value}")


# ---- quantize_affine, quantize_affine_packed, pack ---------------------------------------------------------------------------------------------------
def check_affine(base, bits, scale, shift, what):
    """quanto::quantize_affine, the one-pass quantize + pack and the pack kernel against the CPU sequence and its pack; returns the CPU codes."""
    lib = quanto_hip.lib
    want = ops.quantize_affine(base, bits, 0, 128, scale, shift)
    want_packed = pack_weights(want, bits)
    bd, sd, zd = base.to(DEV), scale.to(DEV), shift.to(DEV)
    got = torch.ops.quanto.quantize_affine(bd, bits, 0, 128, sd, zd)
    assert got.dtype == torch.uint8 and got.shape == want.shape
    bad = got.cpu() != want
    if bad.any():
        r, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.numel()} codes differ from the CPU sequence; first: x {base.reshape(-1, 128)[r, c].item()!r} "
                             f"scale {scale[r].item()!r} shift {shift[r].item()!r} got {got[r, c].item()} want {want[r, c].item()}")
    fused = lib.quantize_affine_packed(bd, bits, 128, sd, zd)
    assert torch.equal(fused.cpu(), want_packed), f"{what}: the one-pass quantize + pack differs from pack(CPU sequence)"
    assert torch.equal(lib.pack(got, bits).cpu(), want_packed), f"{what}: lib.pack of the device codes differs from pack(CPU sequence)"
    return want


@pytest.mark.parametrize("int_shift", [False, True], ids=["shift", "zp"])
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_affine_every_16_bit_value(dt, bits, int_shift):
    seen = set()
    for r in range(AFFINE_ROTATIONS):
        base, scale, shift = affine_case_16(dt, bits, int_shift, r)
        seen.update(check_affine(base, bits, scale, shift, f"{dt} int{bits} rotation {r}").unique().tolist())
    print(f"{dt} int{bits}: {AFFINE_ROTATIONS} x {base.numel()} inputs")
    assert seen == set(range(1 << bits))


@pytest.mark.parametrize("int_shift", [False, True], ids=["shift", "zp"])
@pytest.mark.parametrize("bits", [2, 4])
def test_affine_fp32_ties(bits, int_shift):
    base, scale, shift = affine_case_32(bits, int_shift)
    want = check_affine(base, bits, scale, shift, f"fp32 int{bits} ties")
    assert want.unique().numel() == 1 << bits


# ---- dequantize_symmetric ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("kind", list(TARGETS))
def test_dequantize_every_code(kind, dt):
    tdt = TORCH_DT[dt]
    bits = {2: torch.int16, 4: torch.int32}[tdt.itemsize]
    for numel in (512, 513, 527):  # 16 k + r, r = 0, 1, 15
        data = dequantize_codes(numel).view(TARGETS[kind])
        dd = data.to(DEV)
        for s in dequantize_scales(dt):
            want = s * data.to(tdt)
            got = quanto_hip.lib.dequantize_symmetric(dd, s.to(DEV))
            assert got is not None and got.dtype == tdt and got.shape == want.shape
            got = got.cpu()
            nan = torch.isnan(want)
            assert torch.equal(torch.isnan(got), nan), f"{kind} -> {dt}, scale {float(s)}: NaN codes"
            assert nan.sum() == {"int8": 0, "e4m3fn": 2, "e5m2": 6}[kind] * 2
            bad = (got.view(bits) != want.view(bits)) & ~nan
            assert not bad.any(), (f"{kind} -> {dt}, scale {float(s)}, {numel} elements: {int(bad.sum())} differ; codes {data.view(torch.uint8)[bad][:8].tolist()} "
                                   f"got {got[bad][:8].tolist()} want {want[bad][:8].tolist()}")


# ---- the fused epilogues against the CPU -------------------------------------------------------------------------------------------------------------
def cpu_codes(y: torch.Tensor, out_scale: torch.Tensor, what):
    """int8 codes of the CPU quantizer on a CPU product, with the share of elements it clamps asserted."""
    share = ((y / out_scale).to(torch.float32).abs() > 127).to(torch.float32).mean().item()
    print(f"{what}: out_scale {out_scale.item():.6g}, clamped share {share:.4f}")
    assert 0.02 <= share <= 0.25, f"{what}: the CPU sequence clamps {share:.4f} of the elements at this output scale"
    return ops.quantize_symmetric(y, torch.int8, None, out_scale)


def assert_codes_equal(got, want, what):
    assert got.dtype == torch.int8 and got.shape == want.shape
    bad = got.cpu() != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.numel()} fused codes differ from the CPU sequence"
    assert {-128, 127} <= set(want.unique().tolist())


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K", [(65, 48, 64), (300, 136, 256)])
def test_w8a8_fused_codes_equal_the_cpu_sequence(M, N, K, dt, with_bias):
    """out_scale as in test_output_fusion_gpu.py (0.7 x absmax / qmax, on that file's operands), from the CPU product."""
    a, b, scales, bias = w8a8_problem(M, N, K, "int8", dt, with_bias, seed=11)
    y = to_torch(O.qbytes_int_mm_ref(a.cpu().numpy(), b.cpu().numpy(), scales.cpu().to(torch.float32).numpy(), dt), dt)
    if with_bias:
        y = y + bias.cpu()  # quanto::qbytes_mm_bias: the rounded product plus the bias, rounded again
    out_scale = (y.abs().max().to(torch.float32) / 127.0 * 0.7).to(y.dtype)
    what = f"W8A8 {M}x{N}x{K} {dt} {'bias' if with_bias else 'nobias'}"
    want = cpu_codes(y, out_scale, what)
    got = quanto_hip.lib.qbytes_mm_q(a, b, scales, bias, out_scale.to(DEV))
    assert got is not None and quanto_hip.lib.last_kernel() == "mfma_native8_q"
    assert_codes_equal(got, want, what)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N,K,zp", [(65, 48, 128, True), (300, 136, 256, False)])
def test_w4a8_fused_codes_equal_the_cpu_sequence(monkeypatch, M, N, K, zp, dt, with_bias):
    """The W8A8 shapes with K raised to a whole group of 128 (the kernel serves nothing shorter); operands and out_scale as in test_a8_output_fusion_gpu.py
    (uniform int8 codes, activation scale 0.02, the 0.9-quantile of |y| over qmax), from the CPU product.  Unsplit: that is what the chain restates."""
    monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", "1")
    p = make_qbits_problem(1, N, K, dt, bits=4, group_size=128, zeropoint=zp, seed=M + N + K)
    rng = np.random.default_rng(7 * M + 3 * N + K)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    sx = O.round_to(np.array([0.02], np.float32), dt)
    bias = O.round_to((rng.standard_normal(N) * 0.5).astype(np.float32), dt) if with_bias else None
    y = to_torch(O.qbits_mm_a8_chain(a, sx, p["packed"], 4, p["scale"], p["shift"], 128, N, K, dt, bias), dt)
    out_scale = (torch.quantile(y.abs().to(torch.float32).reshape(-1), 0.9) / 127.0).to(y.dtype)
    what = f"W4A8 {M}x{N}x{K} {dt} {'bias' if with_bias else 'nobias'} {'zp' if zp else 'shift'}"
    want = cpu_codes(y, out_scale, what)
    shift = torch.from_numpy(p["shift"]) if zp else to_torch(p["shift"], dt)
    got = quanto_hip.lib.qbits_mm_a8_q(torch.from_numpy(a).to(DEV), to_torch(sx, dt, DEV), torch.from_numpy(p["packed"]).to(DEV), to_torch(p["scale"], dt, DEV),
                                       shift.to(DEV), None if bias is None else to_torch(bias, dt, DEV), out_scale.to(DEV), 4, 128, N, K)
    assert quanto_hip.lib.last_kernel() == "a8_fused_int8_q"
    assert_codes_equal(got, want, what)

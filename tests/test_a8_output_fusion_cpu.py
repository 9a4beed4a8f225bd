"""Fused output quantization of W4A8 / W2A8 layers, the parts that need no device: the op ``quanto::qbits_mm_a8_q`` and its default implementation, the
marking rules of ``fuse_output_quantization`` for int4 / int2 weights (one case per clause), the marked forward on CPU tensors, and the C entry
``quanto_hip_qbits_mm_a8_q`` with every refusal of its argument check (the check answers before it looks at the data pointers)."""
import ctypes
import os

import pytest
import torch

import optimum_quanto_amd
from optimum_quanto_amd import (ActivationQBytesTensor, QLinear, freeze, fuse_output_quantization, qfloat8_e4m3fn, qint2, qint4, qint8, quantize)
from optimum_quanto_amd.library import hip as hip_mod
from optimum_quanto_amd.library.hip import quanto_hip

from helpers import BF16, E4M3, E4M3FNUZ, E5M2, EALIGN, EINVAL, ENOTSUP, F16, F32, I8, OK, U8
from helpers import full_range_codes as _codes
from helpers import make_qbits_problem, quantile_out_scale, to_torch

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def test_status_codes_are_the_header_s():
    header = open(os.path.join(os.path.dirname(os.path.dirname(optimum_quanto_amd.__file__)), "include", "quanto_hip.h")).read()
    for name, value in (("QUANTO_HIP_EINVAL", EINVAL), ("QUANTO_HIP_ENOTSUP", ENOTSUP), ("QUANTO_HIP_EALIGN", EALIGN)):
        assert f"{name} = {value}" in header


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("dtype,a_scale", [(torch.int8, 0.02), (torch.float8_e4m3fn, 0.01), (torch.float8_e5m2, 1e-4)])
def test_op_default_is_the_two_op_sequence(dtype, a_scale, dt, with_bias):
    gen = torch.Generator().manual_seed(11)
    M, N, K = 7, 24, 256
    p = make_qbits_problem(1, N, K, dt, seed=3)
    a = _codes(dtype, (M, K), gen)
    args = (torch.tensor(a_scale, dtype=TDT[dt]), torch.from_numpy(p["packed"]), to_torch(p["scale"], dt), to_torch(p["shift"], dt),
            torch.randn(N, generator=gen).to(TDT[dt]) if with_bias else None)
    y = torch.ops.quanto.qbits_mm_a8(a, *args, 4, 128, N, K)
    assert y.dtype == TDT[dt] and bool(torch.isfinite(y).all())
    out_scale = quantile_out_scale(y, dtype)
    want = torch.ops.quanto.quantize_symmetric(y, dtype, None, out_scale)
    got = torch.ops.quanto.qbits_mm_a8_q(a, *args, out_scale, 4, 128, N, K)
    assert got.dtype == dtype and got.shape == (M, N)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    # a leading batch dimension is carried through, a one-element scale tensor is taken as the scalar
    got3 = torch.ops.quanto.qbits_mm_a8_q(a.reshape(1, M, K), *args, out_scale.reshape(1), 4, 128, N, K)
    assert got3.shape == (1, M, N) and torch.equal(got3.view(torch.uint8).reshape(M, N), want.view(torch.uint8))


# ---- marking ---------------------------------------------------------------------------------------------------------------------------------------
def _model(features, weights, activations, dtype=torch.bfloat16, frozen=True):
    torch.manual_seed(3)
    layers = [torch.nn.Linear(i, o, bias=(n == 0)) for n, (i, o) in enumerate(zip(features, features[1:]))]
    model = torch.nn.Sequential(*layers).to(dtype)
    quantize(model, weights=weights, activations=activations)
    if frozen:
        freeze(model)
    for layer, (si, so) in zip(model, [(0.03, 0.02), (0.02, 0.01)]):
        if isinstance(layer, QLinear) and activations is not None:
            layer.input_scale.fill_(si)
            layer.output_scale.fill_(so)
    return model


def test_served_sub_byte_layers_are_marked():
    model = _model((256, 128, 128), qint4, qint8)  # group size 128, and per-channel with 128 inputs
    assert model[0].weight._group_size == 128 and model[1].weight._group_size is None
    assert fuse_output_quantization(model) == ["0", "1"]
    assert all(m._fuse_output_quantization for m in model)
    model = _model((256, 128, 128), qint2, qfloat8_e4m3fn)
    assert fuse_output_quantization(model) == ["0", "1"]


@pytest.mark.parametrize("features,weights,activations,dtype,frozen", [
    ((192, 128), qint4, qint8, torch.bfloat16, True),
    ((256, 100), qint4, qint8, torch.bfloat16, True),
    ((256, 24), qint2, qint8, torch.bfloat16, True),
    ((256, 128, 128), qint4, qint8, torch.float32, True),
    ((256, 128, 128), qint4, qint8, torch.bfloat16, False),
    ((256, 128, 128), qint4, None, torch.bfloat16, True),
], ids=["in_features-192-group-96", "out_features-100", "int2-out_features-24", "fp32-module", "unfrozen", "no-activations"])
def test_layers_outside_the_gate_stay_unmarked(features, weights, activations, dtype, frozen):
    model = _model(features, weights, activations, dtype, frozen)
    assert fuse_output_quantization(model) == []
    assert not any(m._fuse_output_quantization for m in model)


def test_a_removed_output_hook_keeps_the_module_unmarked():
    model = _model((256, 128, 128), qint4, qint8)
    model[1].disable_output_quantization()
    assert fuse_output_quantization(model) == ["0"]
    assert not model[1]._fuse_output_quantization


def test_int2_with_24_features_would_pass_the_int4_rule():
    """The out_features rule is per weight width: 24 features are 3 x 8 (served for int4) but not a multiple of 16 (int2)."""
    assert fuse_output_quantization(_model((256, 24), qint4, qint8)) == ["0"]


# ---- the marked forward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights,activations", [(qint4, qint8), (qint2, qfloat8_e4m3fn)], ids=["qint4-qint8", "qint2-qfloat8_e4m3fn"])
def test_marked_forward_calls_the_op_once_per_layer_and_keeps_the_bits(monkeypatch, weights, activations):
    import optimum_quanto_amd.nn.module as module_mod

    model = _model((256, 128, 128), weights, activations)
    x = torch.randn(2, 5, 256, dtype=torch.bfloat16)
    keys = set(model.state_dict().keys())
    calls, quantized = [], []
    real_op, real_quantize = torch.ops.quanto.qbits_mm_a8_q, module_mod.quantize_activation

    def counting_op(*args):
        calls.append(tuple(args[0].shape))
        return real_op(*args)

    monkeypatch.setattr(torch.ops.quanto, "qbits_mm_a8_q", counting_op)
    monkeypatch.setattr(module_mod, "quantize_activation", lambda t, qtype, scale: (quantized.append(tuple(t.shape)), real_quantize(t, qtype=qtype, scale=scale))[1])
    with torch.no_grad():
        ref = model(x)
        assert calls == [] and quantized == [(2, 5, 256), (2, 5, 128), (2, 5, 128)]  # the input, then the float output of either layer
        assert fuse_output_quantization(model) == ["0", "1"]
        del quantized[:]
        out = model(x)
        assert calls == [(2, 5, 256), (2, 5, 128)]
        assert quantized == [(2, 5, 256)]  # the input hook of the first layer only: no float output was quantized in a second pass
        assert isinstance(out, ActivationQBytesTensor) and out.qtype == activations and out.shape == ref.shape == (2, 5, 128)
        assert torch.equal(out._data.view(torch.uint8), ref._data.view(torch.uint8))
        assert torch.equal(out._scale, ref._scale)
        assert set(model.state_dict().keys()) == keys  # the mark is not serialised
        # with a gradient wanted the marked module runs the existing forward
        del calls[:]
        with torch.enable_grad():
            again = model(x)
        assert calls == []
        assert torch.equal(again._data.view(torch.uint8), ref._data.view(torch.uint8))


def test_enable_false_and_disable_output_quantization_unmark():
    model = _model((256, 128, 128), qint4, qint8)
    assert fuse_output_quantization(model) == ["0", "1"]
    assert fuse_output_quantization(model, enable=False) == ["0", "1"]
    assert not any(m._fuse_output_quantization for m in model)
    assert fuse_output_quantization(model, enable=False) == []
    assert fuse_output_quantization(model) == ["0", "1"]
    model[1].disable_output_quantization()
    assert not model[1]._fuse_output_quantization
    with torch.no_grad():
        out = model(torch.randn(3, 256, dtype=torch.bfloat16))
    assert type(out) is torch.Tensor and out.dtype == torch.bfloat16  # the last layer returns its float output again


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------------------
_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
PTR = 1 << 20  # a 16-byte aligned address that is never dereferenced: every case below is refused, or done, before a launch


def _entry():
    fn = quanto_hip.cdll.quanto_hip_qbits_mm_a8_q
    fn.restype, fn.argtypes = _ci, [_vp] * 8 + [_i64] * 3 + [_ci] * 5 + [_vp, _sz, _vp]
    return fn


def _call(M=300, N=512, K=4096, bits=4, group_size=128, a_dtype=I8, dtype=BF16, shift_dtype=None, out_scale=PTR, yq=PTR, data=PTR):
    return _entry()(data, data, data, data, data, None, out_scale, yq, M, N, K, bits, group_size, a_dtype, dtype, dtype if shift_dtype is None else shift_dtype,
                    None, 0, None)


def test_the_symbol_is_exported_declared_and_bound():
    _entry()
    quanto_hip.cdll.quanto_hip_abi_version.restype = _ci
    assert quanto_hip.cdll.quanto_hip_abi_version() == 1
    assert "quanto_hip_qbits_mm_a8_q" in hip_mod._PROTOTYPES
    assert hasattr(hip_mod._Bindings, "qbits_mm_a8_q")
    header = open(os.path.join(os.path.dirname(os.path.dirname(optimum_quanto_amd.__file__)), "include", "quanto_hip.h")).read()
    assert "int quanto_hip_qbits_mm_a8_q(" in header


NOT_SERVED = {
    "fp32 dtype": dict(dtype=F32),
    "group size 64": dict(group_size=64),
    "N not a multiple of 8": dict(N=100),
    "int2 with N not a multiple of 16": dict(bits=2, N=24),
    "an unknown activation dtype": dict(a_dtype=42),
    "float activations": dict(a_dtype=BF16),
    "e4m3fnuz activations": dict(a_dtype=E4M3FNUZ),
}


@pytest.mark.parametrize("why", sorted(NOT_SERVED))
def test_every_refusal_answers_enotsup_ahead_of_the_pointers(why):
    assert _call(**NOT_SERVED[why]) == ENOTSUP, why
    assert _call(**NOT_SERVED[why], data=None, out_scale=None, yq=None) == ENOTSUP, why
    assert _call(**NOT_SERVED[why], M=0) == ENOTSUP, why


def test_einval_ealign_and_the_empty_product():
    assert _call(M=-1) == EINVAL and _call(N=0) == EINVAL and _call(K=0) == EINVAL and _call(bits=3) == EINVAL
    assert _call(out_scale=None) == EINVAL
    assert _call(yq=None) == EINVAL
    assert _call(data=None) == EINVAL
    assert _call(yq=PTR + 1) == EALIGN
    assert _call(data=PTR + 8) == EALIGN
    for a_dtype in (I8, E4M3, E5M2):
        for dtype in (BF16, F16):
            for bits, n in ((4, 8), (2, 16)):
                assert _call(M=0, N=n, bits=bits, a_dtype=a_dtype, dtype=dtype, data=None, out_scale=None, yq=None) == OK
                assert _call(M=0, N=n, bits=bits, a_dtype=a_dtype, dtype=dtype, shift_dtype=U8) == OK

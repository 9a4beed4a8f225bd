"""Fused output quantization of QConv2d with quantized activations, the parts that need no device: the op ``quanto::qbytes_conv2d_a8_q`` and its default
implementation, the C entry ``quanto_hip_qbytes_conv2d_a8_q`` with the refusals of its argument check (format and geometry answer before the data pointers
are looked at), the marking rules of ``fuse_output_quantization`` for ``QConv2d`` (one case per clause), the marked forward on CPU tensors and the
routing of a marked module to the fused op."""
import ctypes
import os
import re

import pytest
import torch

import optimum_quanto_amd
from optimum_quanto_amd import (ActivationQBytesTensor, QConv2d, freeze, fuse_output_quantization, qfloat8_e4m3fn, qfloat8_e5m2, qint4, qint8, quantize)
from optimum_quanto_amd.library import hip as hip_mod
from optimum_quanto_amd.library.hip import quanto_hip

from helpers import BF16, E4M3, E4M3FNUZ, E5M2, EINVAL, ENOTSUP, F16, F32, I8, OK, U8, quantile_out_scale

HEADER = os.path.join(os.path.dirname(os.path.dirname(optimum_quanto_amd.__file__)), "include", "quanto_hip.h")


# ---- the symbol ------------------------------------------------------------------------------------------------------------------------------------
_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
PTR = 1 << 20  # an aligned address that is never dereferenced: every case below is refused, or done, before a launch


def _entry():
    fn = quanto_hip.cdll.quanto_hip_qbytes_conv2d_a8_q
    fn.restype, fn.argtypes = _ci, [_vp] * 7 + [_i64] * 9 + [_ci] * 9 + [_vp, _sz, _vp]
    return fn


def test_the_symbol_is_exported_declared_and_bound():
    _entry()
    quanto_hip.cdll.quanto_hip_abi_version.restype = _ci
    assert quanto_hip.cdll.quanto_hip_abi_version() == 1
    assert "quanto_hip_qbytes_conv2d_a8_q" in hip_mod._PROTOTYPES
    assert hasattr(hip_mod._Bindings, "qbytes_conv2d_a8_q")
    assert re.search(r"\bint quanto_hip_qbytes_conv2d_a8_q\(", open(HEADER).read())


# ---- the default op ----------------------------------------------------------------------------------------------------------------------------------
def _codes(dtype, shape, gen):
    if dtype == torch.int8:
        return torch.randint(-128, 128, shape, dtype=torch.int8, generator=gen)
    return (torch.randn(shape, generator=gen) * 4).to(dtype)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("dtype", [torch.int8, torch.float8_e4m3fn], ids=["int8", "e4m3"])
def test_op_default_is_the_two_op_sequence(dtype, dt, with_bias):
    gen = torch.Generator().manual_seed(11)
    x, w = _codes(dtype, (2, 5, 9, 11), gen), _codes(dtype, (7, 5, 3, 3), gen)
    xs = torch.tensor([0.0125], dtype=dt)
    ws = (torch.rand(7, 1, 1, 1, generator=gen) * 0.01 + 0.001).to(dt)
    b = torch.randn(7, generator=gen).to(dt) if with_bias else None
    geometry = ([2, 1], [1, 0], [1, 2])
    y = torch.ops.quanto.qbytes_conv2d_a8(x, xs, w, ws, b, *geometry)
    assert y.dtype == dt and y.shape == (2, 7, 5, 7)
    out_scale = quantile_out_scale(y, dtype)
    want = torch.ops.quanto.quantize_symmetric(y, dtype, None, out_scale)
    got = torch.ops.quanto.qbytes_conv2d_a8_q(x, xs, w, ws, b, out_scale, *geometry)
    assert got.dtype == dtype and got.shape == (2, 7, 5, 7)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    assert len(torch.unique(got.view(torch.uint8))) > 8  # neither all zero nor all clamped
    # a one-element scale tensor is taken as the scalar
    got1 = torch.ops.quanto.qbytes_conv2d_a8_q(x, xs, w, ws, b, out_scale.reshape(1), *geometry)
    assert torch.equal(got1.view(torch.uint8), want.view(torch.uint8))


# ---- the C entry -----------------------------------------------------------------------------------------------------------------------------------
def _call(a=I8, b=I8, mid=BF16, B=8, cin=128, H=28, W=28, OC=128, KH=3, KW=3, OH=None, OW=None, s=(1, 1), p=(1, 1), d=(1, 1), out_scale=PTR, yq=PTR,
          data=PTR):
    if OH is None:
        OH = (H + 2 * p[0] - d[0] * (KH - 1) - 1) // s[0] + 1
    if OW is None:
        OW = (W + 2 * p[1] - d[1] * (KW - 1) - 1) // s[1] + 1
    return _entry()(data, data, data, data, None, out_scale, yq, B, cin, H, W, OC, KH, KW, OH, OW, s[0], s[1], p[0], p[1], d[0], d[1], a, b, mid,
                    None, 0, None)


NOT_SERVED = {
    "int8 activations x e4m3 weights": dict(a=I8, b=E4M3),
    "int8 activations x e5m2 weights": dict(a=I8, b=E5M2),
    "e4m3fnuz activations": dict(a=E4M3FNUZ, b=I8),
    "e4m3fnuz weights": dict(a=E4M3, b=E4M3FNUZ),
    "an int8 mid dtype": dict(mid=I8),
    "a uint8 mid dtype": dict(a=E4M3, b=E4M3, mid=U8),
    "an unknown mid dtype": dict(mid=42),
}


@pytest.mark.parametrize("why", sorted(NOT_SERVED))
def test_the_format_is_refused_ahead_of_the_pointers(why):
    assert _call(**NOT_SERVED[why]) == ENOTSUP, why
    assert _call(**NOT_SERVED[why], data=None, out_scale=None, yq=None) == ENOTSUP, why
    assert _call(**NOT_SERVED[why], B=0, data=None, out_scale=None, yq=None) == ENOTSUP, why


def test_the_geometry_statuses_are_the_unfused_entry_s():
    null = dict(data=None, out_scale=None, yq=None)
    for pointers in ({}, null):
        assert _call(OH=27, **pointers) == EINVAL
        assert _call(OW=29, **pointers) == EINVAL
        assert _call(s=(0, 1), OH=28, OW=28, **pointers) == EINVAL
        assert _call(KH=0, **pointers) == EINVAL
        assert _call(B=-1, **pointers) == EINVAL
        assert _call(KH=12, KW=11, p=(5, 5), **pointers) == ENOTSUP  # 132 taps: beyond the tap masks
    assert _call(KH=11, KW=11, p=(5, 5), **null) == EINVAL  # 121 taps are served: the null pointers are what is refused


@pytest.mark.parametrize("a,b", [(I8, I8), (E4M3, E4M3), (E4M3, E5M2), (E5M2, E4M3), (E5M2, E5M2), (E4M3, I8), (E5M2, I8)])
@pytest.mark.parametrize("mid", [F32, F16, BF16])
def test_served_formats_empty_output_and_null_pointers(a, b, mid):
    assert _call(a, b, mid, B=0, data=None, out_scale=None, yq=None) == OK
    assert _call(a, b, mid, B=0) == OK
    assert _call(a, b, mid, yq=None) == EINVAL
    assert _call(a, b, mid, out_scale=None) == EINVAL
    assert _call(a, b, mid, data=None) == EINVAL


# ---- marking ---------------------------------------------------------------------------------------------------------------------------------------
def _model(weights=qint8, activations=qint8, dtype=torch.bfloat16, frozen=True, **first):
    """Conv2d(8, 16, 3, padding=1) -> Conv2d(16, 8, 1) with calibrated scales set by hand; ``first`` overrides arguments of the first layer."""
    torch.manual_seed(3)
    args = dict(padding=1)
    args.update(first)
    model = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, **args), torch.nn.Conv2d(16, 8, 1)).to(dtype)
    quantize(model, weights=weights, activations=activations)
    if frozen:
        freeze(model)
    if activations is not None:
        qmax = 127.0 if activations is qint8 else torch.finfo(activations.dtype).max
        for layer, (si, so) in zip(model, [(3.0, 2.0), (2.0, 1.0)]):
            layer.input_scale.fill_(si / qmax)
            layer.output_scale.fill_(so / qmax)
    return model


SERVED_PAIRS = [(qint8, qint8), (qfloat8_e4m3fn, qfloat8_e4m3fn), (qfloat8_e5m2, qfloat8_e4m3fn), (qint8, qfloat8_e4m3fn), (qint8, qfloat8_e5m2),
                (qfloat8_e4m3fn, qfloat8_e5m2)]  # (weights, activations)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("weights,activations", SERVED_PAIRS, ids=lambda q: q.name)
def test_served_pairs_are_marked(weights, activations, dtype):
    model = _model(weights, activations, dtype)
    assert all(type(m) is QConv2d for m in model)
    keys = set(model.state_dict().keys())
    if activations is qfloat8_e5m2 and dtype == torch.float16:  # the fp16 scale product of an e5m2 scale underflows: never served
        assert fuse_output_quantization(model) == []
        return
    assert fuse_output_quantization(model) == ["0", "1"]
    assert all(m._fuse_output_quantization for m in model)
    assert set(model.state_dict().keys()) == keys  # the mark is not serialised
    assert fuse_output_quantization(model, enable=False) == ["0", "1"]
    assert not any(m._fuse_output_quantization for m in model)
    assert fuse_output_quantization(model, enable=False) == []


@pytest.mark.parametrize("why,kwargs", [
    ("groups-2", dict(groups=2)),
    ("padding-mode-reflect", dict(padding_mode="reflect")),
    ("padding-same", dict(padding="same")),
], ids=lambda v: v if isinstance(v, str) else "")
def test_a_first_layer_outside_the_gate_stays_unmarked(why, kwargs):
    model = _model(**kwargs)
    assert fuse_output_quantization(model) == ["1"]
    assert not model[0]._fuse_output_quantization and model[1]._fuse_output_quantization


@pytest.mark.parametrize("kwargs", [dict(frozen=False), dict(weights=qint4), dict(weights=qfloat8_e4m3fn, activations=qint8), dict(activations=None)],
                         ids=["unfrozen", "qint4-weights", "int8-activations-x-fp8-weights", "no-activations"])
def test_models_outside_the_gate_stay_unmarked(kwargs):
    model = _model(**kwargs)
    assert fuse_output_quantization(model) == []
    assert not any(m._fuse_output_quantization for m in model)


def test_a_removed_output_hook_keeps_the_module_unmarked_and_disabling_unmarks():
    model = _model()
    model[1].disable_output_quantization()
    assert fuse_output_quantization(model) == ["0"]
    assert not model[1]._fuse_output_quantization
    model = _model()
    assert fuse_output_quantization(model) == ["0", "1"]
    model[1].disable_output_quantization()
    assert not model[1]._fuse_output_quantization
    with torch.no_grad():
        out = model(torch.randn(2, 8, 6, 6).to(torch.bfloat16))
    assert type(out) is torch.Tensor and out.dtype == torch.bfloat16  # the last layer returns its float output again


def test_linear_and_conv_names_come_in_module_order():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 1), torch.nn.Flatten(), torch.nn.Linear(64, 64)).to(torch.bfloat16)
    quantize(model, weights=qint8, activations=qint8)
    freeze(model)
    assert fuse_output_quantization(model) == ["0", "2"]


# ---- the marked forward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights,activations", [(qint8, qint8), (qfloat8_e4m3fn, qfloat8_e4m3fn)], ids=lambda q: q.name)
def test_marked_model_on_cpu_returns_the_unmarked_model_s_codes(monkeypatch, weights, activations):
    model = _model(weights, activations)
    x = torch.randn(2, 8, 6, 7).to(torch.bfloat16)
    with torch.no_grad():
        ref = model(x)
    assert fuse_output_quantization(model) == ["0", "1"]
    calls = []
    real_op = torch.ops.quanto.qbytes_conv2d_a8_q
    monkeypatch.setattr(torch.ops.quanto, "qbytes_conv2d_a8_q", lambda *args: (calls.append(1), real_op(*args))[1])
    with torch.no_grad():
        out = model(x)
    assert calls == []  # not a ROCm device: the predicate is false and the existing forward runs
    assert isinstance(out, ActivationQBytesTensor) and out.qtype == activations and out.shape == ref.shape == (2, 8, 6, 7)
    assert torch.equal(out._data.view(torch.uint8), ref._data.view(torch.uint8))
    assert torch.equal(out._scale, ref._scale)
    assert len(torch.unique(ref._data.view(torch.uint8))) > 8


def test_marked_forward_calls_the_fused_op_once_for_the_second_layer(monkeypatch):
    import optimum_quanto_amd.nn.conv as conv_mod
    import optimum_quanto_amd.nn.module as module_mod

    model = _model()
    x = torch.randn(2, 8, 6, 7).to(torch.bfloat16)
    assert fuse_output_quantization(model) == ["0", "1"]
    calls, quantized, asked = [], [], []
    real_op, real_quantize = torch.ops.quanto.qbytes_conv2d_a8_q, module_mod.quantize_activation

    def counting_op(*args):
        calls.append(args)
        return real_op(*args)

    def eligible(input, weight, bias, stride, padding, dilation, groups):
        asked.append((tuple(stride), tuple(padding), tuple(dilation), groups))
        return True

    monkeypatch.setattr(torch.ops.quanto, "qbytes_conv2d_a8_q", counting_op)
    monkeypatch.setattr(conv_mod, "conv2d_a8_eligible", eligible)
    monkeypatch.setattr(module_mod, "quantize_activation", lambda t, qtype, scale: (quantized.append(tuple(t.shape)), real_quantize(t, qtype=qtype, scale=scale))[1])
    with torch.no_grad():
        out = model(x)
    # the first layer's input is a float tensor: its existing forward runs and its hook quantizes the output; the second layer gets codes
    assert quantized == [(2, 16, 6, 7)]
    assert asked == [((1, 1), (0, 0), (1, 1), 1)]
    assert len(calls) == 1
    input, input_scale, weight, weight_scale, bias, out_scale, stride, padding, dilation = calls[0]
    assert input.dtype == torch.int8 and tuple(input.shape) == (2, 16, 6, 7) and input_scale is not None
    assert weight is model[1].weight._data and weight_scale is model[1].weight._scale and bias is model[1].bias
    assert out_scale is model[1].output_scale
    assert (list(stride), list(padding), list(dilation)) == ([1, 1], [0, 0], [1, 1])
    assert isinstance(out, ActivationQBytesTensor) and out.qtype == qint8 and out.shape == (2, 8, 6, 7)
    assert out._scale is model[1].output_scale
    # with a float input to the second layer the marked module runs the existing forward
    del calls[:]
    with torch.no_grad():
        model[1](torch.randn(2, 16, 6, 7).to(torch.bfloat16))
    assert calls == []

"""``quanto::layer_norm_q`` and ``QLayerNorm`` without a device: the op and its default (the two statements of the reference's QLayerNorm), the inputs of
the GPU file against the float64 oracle (layernorm_q_cases.py: the accuracy condition, and why it is attainable), the module, the model API's opt-in
``layernorm=True``, ``fuse_output_quantization``, and the C entry's argument checks and size rule."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import optimum_quanto_amd as Q
from optimum_quanto_amd import (QLayerNorm, QLinear, freeze, fuse_output_quantization, qfloat8_e4m3fn, qint8, quantization_map, quantize,
                                quantize_activation, requantize)
from optimum_quanto_amd.library import hip as hip_mod
from optimum_quanto_amd.library.hip import BF16, F8_E4M3FN, F16, F32, I8, U8, quanto_hip

import layernorm_q_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENOTSUP = 0, -1, -2  # QUANTO_HIP_* (include/quanto_hip.h)


def _default_op(p):
    return torch.ops.quanto.layer_norm_q(p.x, list(p.norm), p.weight, p.bias, C.EPS, p.scale, p.dtype)


# ---- the op ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.PAIR_CASES[:8] + C.PARAM_CASES + C.ND_CASES, ids=lambda c: c.id)
def test_the_op_exists_and_its_default_is_the_two_statements(case):
    p = C.problem(case)
    got = _default_op(p)
    y = torch.nn.functional.layer_norm(p.x, p.norm, p.weight, p.bias, C.EPS)
    want = torch.ops.quanto.quantize_symmetric(y, p.dtype, None, p.scale)
    assert got.dtype == p.dtype and got.shape == p.x.shape
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


@pytest.mark.parametrize("case", C.ALL_CASES, ids=lambda c: c.id)
def test_every_input_of_the_gpu_file_meets_the_condition_on_the_cpu(case):
    """The cap is attainable on these inputs: an fp32 two-pass sequence (what the kernel computes, up to the order of its sums) stays inside it everywhere,
    and so does the default op - torch's own CPU sequence - on everything but the ``mean1000`` rows, where its x * rstd - mean * rstd form is held to
    the cap that form can meet (layernorm_q_cases.torch_cpu_cap) and to one code step."""
    p = C.problem(case)
    C.assert_condition(C.emulated_codes(p), p.want, f"fp32 two-pass emulation, {case.id}")
    if case.kind != "mean1000" or case.code != "int8":
        C.assert_condition(_default_op(p), p.want, f"default op, {case.id}")
    else:
        differing, steps, cap = C.difference(_default_op(p), p.want)
        print(f"default op, {case.id}: {differing} of {p.want.numel()} codes differ (cap of the condition {cap}, of torch's formula {C.torch_cpu_cap(p)})")
        assert steps <= 1 and differing <= C.torch_cpu_cap(p)


@pytest.mark.parametrize("case", [c for c in C.STAT_CASES if c.kind == "mean1000" and c.code == "int8"], ids=lambda c: c.id)
def test_a_one_pass_variance_fails_the_mean_1000_rows(case):
    """The statistic cases have teeth: E[x^2] - mean^2 in fp32 is far outside the condition on them."""
    p = C.problem(case)
    differing, steps, cap = C.difference(C.emulated_codes(p, one_pass=True), p.want)
    assert differing > 10 * cap


def test_the_saturating_inputs_clamp_on_both_sides():
    for case in (c for c in C.STAT_CASES if c.kind == "saturate"):
        want = C.ordinal(C.problem(case).want)
        top = {"int8": 127, "e4m3": 0x7E, "e5m2": 0x7B}[case.code]  # the largest finite code
        assert want.max() == top and (want == top).float().mean() > 0.2 and (want <= -top).float().mean() > 0.2


# ---- QLayerNorm ------------------------------------------------------------------------------------------------------------------------
def _float_ln(n=48, dtype=torch.float32, **kw):
    torch.manual_seed(n)
    m = torch.nn.LayerNorm(n, dtype=dtype, **kw)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p))
    return m


def test_from_module_shares_parameters_and_never_quantizes_weights():
    m = _float_ln()
    q = QLayerNorm.from_module(m, weights=qint8, activations=qint8)
    assert type(q) is QLayerNorm and q.weight is m.weight and q.bias is m.bias
    assert q.weight_qtype is None and q.activation_qtype == qint8 and q.optimizer is None and not q.frozen
    assert q.normalized_shape == m.normalized_shape and q.eps == m.eps
    assert "output" in q._quantize_hooks and "input" not in q._quantize_hooks
    assert QLayerNorm.from_module(m, weights=qint8, activations=None) is None
    q.freeze()
    assert q.weight is m.weight


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("qt", [qint8, qfloat8_e4m3fn], ids=lambda q: q.name)
@pytest.mark.parametrize("marked", [False, True])
def test_forward_is_the_float_layer_norm_quantized_by_the_hook(dtype, qt, marked):
    m = _float_ln(dtype=dtype)
    q = QLayerNorm.from_module(m, activations=qt)
    x = torch.randn(3, 5, 48).to(dtype)
    q.output_scale = torch.tensor(0.03, dtype=dtype)
    q._fuse_output_quantization = marked
    with torch.no_grad():
        got = q(x)
        want = quantize_activation(torch.nn.functional.layer_norm(x, (48,), m.weight, m.bias, m.eps), qtype=qt, scale=q.output_scale)
    assert isinstance(got, Q.ActivationQBytesTensor) and got.qtype == qt and got.shape == x.shape
    assert torch.equal(got._data.view(torch.uint8), want._data.view(torch.uint8)) and torch.equal(got._scale, want._scale)


def test_a_marked_module_keeps_the_float_forward_when_a_gradient_is_wanted_or_the_input_is_quantized(monkeypatch):
    calls = []
    op = torch.ops.quanto.layer_norm_q
    monkeypatch.setattr(torch.ops.quanto, "layer_norm_q", lambda *a: calls.append(a) or op(*a))
    q = QLayerNorm.from_module(_float_ln(), activations=qint8)
    q.output_scale = torch.tensor(0.03)
    q._fuse_output_quantization = True
    x = torch.randn(2, 48)
    out = q(x)  # grad enabled, parameters require grad
    assert calls == [] and isinstance(out, Q.ActivationQBytesTensor)
    with torch.no_grad():
        q(x)
        assert len(calls) == 1
        qx = quantize_activation(x, qtype=qint8, scale=torch.tensor(0.02))
        out = q(qx)  # dequantized through qfallback, as unmarked
        assert len(calls) == 1
        want = quantize_activation(torch.nn.functional.layer_norm(qx.dequantize(), (48,), q.weight, q.bias, q.eps), qtype=qint8, scale=q.output_scale)
        assert torch.equal(out._data, want._data)
        q.disable_output_quantization()
        assert not q._fuse_output_quantization
        assert type(q(x)) is torch.Tensor and len(calls) == 1


@pytest.mark.parametrize("kw", [dict(elementwise_affine=False), dict(bias=False), dict()], ids=["no-affine", "no-bias", "affine"])
def test_affine_and_bias_may_be_absent_and_the_state_dict_round_trips(kw):
    m = _float_ln(**kw)
    model = torch.nn.Sequential(m)
    weight, bias = m.weight, m.bias  # (quantize releases the float module's parameters)
    quantize(model, activations=qint8, layernorm=True)
    q = model[0]
    assert type(q) is QLayerNorm and q.weight is weight and q.bias is bias
    assert (weight is None) == (not m.elementwise_affine) and (bias is None) == (kw != {})
    assert q.elementwise_affine == m.elementwise_affine
    assert quantization_map(model) == {"0": {"weights": "none", "activations": "qint8"}}
    q.input_scale, q.output_scale = torch.tensor(0.5), torch.tensor(0.025)
    x = torch.randn(4, 48)
    with torch.no_grad():
        want = q(x)
    assert torch.equal(want._data, quantize_activation(torch.nn.functional.layer_norm(x, (48,), q.weight, q.bias, q.eps), qint8, q.output_scale)._data)
    sd = model.state_dict()
    expected = {"0.input_scale", "0.output_scale"} | ({"0.weight"} if q.weight is not None else set()) | ({"0.bias"} if q.bias is not None else set())
    assert set(sd) == expected and all(v is not None for v in sd.values())
    fresh = torch.nn.Sequential(torch.nn.LayerNorm(48, **kw))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        requantize(fresh, sd, quantization_map(model), layernorm=True)
    assert type(fresh[0]) is QLayerNorm and torch.equal(fresh[0].output_scale, q.output_scale) and float(fresh[0].input_scale) == 0.5
    with torch.no_grad():
        assert torch.equal(fresh[0](x)._data, want._data)


# ---- quantize / requantize -------------------------------------------------------------------------------------------------------------------
def _block():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.LayerNorm(32), torch.nn.Linear(32, 48), torch.nn.ReLU(), torch.nn.LayerNorm(48), torch.nn.Linear(48, 16))


def test_quantize_replaces_layernorms_only_on_request_and_honours_include_exclude():
    names = lambda m: [type(layer).__name__ for layer in m]  # noqa: E731
    model = _block()
    quantize(model, weights=qint8, activations=qint8)
    assert names(model) == ["LayerNorm", "QLinear", "ReLU", "LayerNorm", "QLinear"]
    model = _block()
    quantize(model, weights=qint8, activations=qint8, layernorm=True)
    assert names(model) == ["QLayerNorm", "QLinear", "ReLU", "QLayerNorm", "QLinear"]
    model = _block()
    quantize(model, weights=qint8, activations=qint8, layernorm=True, exclude="3")
    assert names(model) == ["QLayerNorm", "QLinear", "ReLU", "LayerNorm", "QLinear"]
    model = _block()
    quantize(model, weights=qint8, activations=qint8, layernorm=True, include=["0", "4"])
    assert names(model) == ["QLayerNorm", "Linear", "ReLU", "LayerNorm", "QLinear"]
    model = _block()
    quantize(model, weights=qint8, layernorm=True)  # no activation qtype: nothing to quantize in a LayerNorm
    assert names(model) == ["LayerNorm", "QLinear", "ReLU", "LayerNorm", "QLinear"]


def test_requantize_rebuilds_a_layernorm_the_map_names_and_restores_its_scales():
    model = _block()
    quantize(model, weights=qint8, activations=qint8, layernorm=True)
    model[0].output_scale, model[3].output_scale = torch.tensor(0.031), torch.tensor(0.017)
    model[1].input_scale = torch.tensor(0.031)
    freeze(model)
    x = torch.randn(3, 32)
    with torch.no_grad():
        want = model(x)
    sd, qmap = model.state_dict(), quantization_map(model)
    assert qmap["0"] == {"weights": "none", "activations": "qint8"} and qmap["3"] == qmap["0"]
    rebuilt = _block()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no "no quantized counterpart" warning
        requantize(rebuilt, sd, qmap, layernorm=True)
    assert type(rebuilt[0]) is QLayerNorm and type(rebuilt[3]) is QLayerNorm
    assert float(rebuilt[0].output_scale) == float(model[0].output_scale) and float(rebuilt[3].output_scale) == float(model[3].output_scale)
    with torch.no_grad():
        got = rebuilt(x)
    assert torch.equal(got._data, want._data) and torch.equal(got._scale, want._scale)
    # the default keeps saying that it has no counterpart
    with pytest.warns(UserWarning, match="no quantized counterpart for 0 \\(LayerNorm\\)"):
        requantize(_block(), sd, qmap)


# ---- fuse_output_quantization ------------------------------------------------------------------------------------------------------------
def test_fuse_output_quantization_marks_and_unmarks_qlayernorms():
    model = _block().to(torch.bfloat16)
    quantize(model, weights=qint8, activations=qint8, layernorm=True)
    assert fuse_output_quantization(model) == ["0", "3"]  # the Linears are not frozen yet; a QLayerNorm has nothing to freeze
    assert fuse_output_quantization(model, enable=False) == ["0", "3"]
    freeze(model)
    assert fuse_output_quantization(model) == ["0", "1", "3", "4"]  # named_modules() order
    assert all(model[i]._fuse_output_quantization for i in (0, 1, 3, 4))
    model[3].disable_output_quantization()
    assert not model[3]._fuse_output_quantization
    assert fuse_output_quantization(model, enable=False) == ["0", "1", "4"]
    assert fuse_output_quantization(model) == ["0", "1", "4"]  # without its hook module 3 is not marked again
    # an activation qtype outside int8 / e4m3fn / e5m2 is never marked
    other = torch.nn.Sequential(torch.nn.LayerNorm(8))
    quantize(other, activations=Q.qfloat8_e4m3fnuz, layernorm=True)
    assert type(other[0]) is QLayerNorm and fuse_output_quantization(other) == []


def test_the_class_is_exported_and_not_registered_as_a_counterpart():
    from optimum_quanto_amd import nn
    from optimum_quanto_amd.nn.module import _counterparts

    assert nn.QLayerNorm is QLayerNorm and Q.QLayerNorm is QLayerNorm
    assert torch.nn.LayerNorm not in _counterparts and QLayerNorm not in _counterparts.values()
    assert Q.quantize_module(torch.nn.LayerNorm(8), activations=qint8) is None


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entries_and_the_binding_declares_them():
    header = open(os.path.join(ROOT, "include", "quanto_hip.h")).read()
    for name in ("quanto_hip_layer_norm_q", "quanto_hip_layer_norm_q_supported"):
        assert hasattr(quanto_hip.cdll, name) and name in hip_mod._PROTOTYPES
        assert re.search(r"\b" + name + r"\(", header)
    limit = int(re.search(r"#define QUANTO_HIP_LAYER_NORM_Q_MAX_N (\d+)", header).group(1))
    assert limit == hip_mod._Bindings.LAYER_NORM_Q_MAX_N == C.LIMIT >= 8192
    make = open(os.path.join(ROOT, "optimum_quanto_amd", "csrc", "Makefile")).read()
    assert "layernorm_q.hip" in re.search(r"^SRCS\s*=\s*(.+)$", make, re.M).group(1).split()


PTR = 1 << 20  # an aligned address that is never dereferenced: every case below is refused, or done, before a launch


def _entry(x=PTR, weight=PTR, bias=PTR, out_scale=PTR, yq=PTR, rows=5, n=768, row_stride=None, dtype=BF16, out_dtype=I8):
    fn = quanto_hip.cdll.quanto_hip_layer_norm_q
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64] * 3 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return fn(x, weight, bias, out_scale, yq, rows, n, n if row_stride is None else row_stride, 1e-5, dtype, out_dtype, None)


# (what, arguments, status).  A served problem is shown as served by the status of its null output: the last check before the launch.
STATUSES = [
    ("rows == 0", dict(rows=0), OK),
    ("rows == 0, null pointers", dict(rows=0, x=None, out_scale=None, yq=None), OK),
    ("n == 0", dict(n=0), OK),
    ("negative rows", dict(rows=-1), EINVAL),
    ("negative n", dict(n=-1), EINVAL),
    ("negative row stride", dict(row_stride=-768), EINVAL),
    ("a negative size ahead of an unsupported dtype", dict(rows=-1, dtype=I8), EINVAL),
    ("rows that overlap", dict(row_stride=767), EINVAL),
    ("one row has no stride", dict(rows=1, row_stride=0, yq=None), EINVAL),
    ("int8 input", dict(dtype=I8), ENOTSUP),
    ("a dtype that is no dtype", dict(dtype=99), ENOTSUP),
    ("uint8 codes", dict(out_dtype=U8), ENOTSUP),
    ("float codes", dict(out_dtype=BF16), ENOTSUP),
    ("n = limit + 1", dict(n=C.LIMIT + 1), ENOTSUP),
    ("n = limit + 1, even when empty", dict(n=C.LIMIT + 1, rows=0), ENOTSUP),
    ("n = limit is served", dict(n=C.LIMIT, yq=None), EINVAL),
    ("2^31 rows", dict(rows=1 << 31), ENOTSUP),
    ("2^31 - 1 rows are served", dict(rows=(1 << 31) - 1, yq=None), EINVAL),
    ("null x", dict(x=None), EINVAL),
    ("null output scale", dict(out_scale=None), EINVAL),
    ("null output", dict(yq=None), EINVAL),
    ("no weight, no bias: served", dict(weight=None, bias=None, yq=None), EINVAL),
    ("fp16 to e4m3, a wider row stride: served", dict(dtype=F16, out_dtype=F8_E4M3FN, row_stride=777, yq=None), EINVAL),
    ("fp32: served", dict(dtype=F32, yq=None), EINVAL),
]


def test_the_entry_validates_its_arguments_before_any_hip_call():
    for what, args, status in STATUSES:
        assert _entry(**args) == status, what


def test_the_python_mirror_of_the_rule_agrees_with_the_c_query():
    lib = quanto_hip.lib
    query = quanto_hip.cdll.quanto_hip_layer_norm_q_supported
    for rows in (0, 1, 65, (1 << 31) - 1, 1 << 31):
        for n in (0, 1, 1024, 1025, C.LIMIT, C.LIMIT + 1):
            for t in (torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int8):
                for code in (torch.int8, torch.float8_e4m3fn, torch.float8_e5m2, torch.float8_e4m3fnuz, torch.uint8):
                    tdt, cdt = hip_mod._DTYPES.get(t, 99), hip_mod._DTYPES.get(code, 99)
                    assert lib.layer_norm_q_supported(rows, n, t, code) == (query(rows, n, tdt, cdt) == OK), (rows, n, t, code)
    assert lib.layer_norm_q_supported(5, C.LIMIT, torch.bfloat16, torch.int8) and not lib.layer_norm_q_supported(5, C.LIMIT + 1, torch.bfloat16, torch.int8)


def test_the_cpu_route_of_what_the_kernel_would_refuse_is_the_sequence():
    x = torch.randn(3, 16, dtype=torch.float64)
    scale = torch.tensor(0.03, dtype=torch.float64)
    got = torch.ops.quanto.layer_norm_q(x, [16], None, None, 1e-5, scale, torch.int8)
    assert torch.equal(got, torch.ops.quanto.quantize_symmetric(torch.nn.functional.layer_norm(x, (16,)), torch.int8, None, scale))

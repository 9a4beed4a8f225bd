"""Fused output quantization, the parts that need no device: the op ``quanto::qbytes_mm_q`` and its default implementation, the opt-in
``fuse_output_quantization`` on a small frozen model, the new C entries and every clause of their argument check (null data pointers: the check
answers before it looks at them, as in tests/test_size_limits_cpu.py)."""
import ctypes

import pytest
import torch

from optimum_quanto_amd import (ActivationQBytesTensor, QLinear, freeze, fuse_output_quantization, qfloat8_e4m3fn, qfloat8_e5m2, qint4, qint8,
                                quantize)
from optimum_quanto_amd.library.hip import quanto_hip

from helpers import BF16, E4M3, E4M3FNUZ, E5M2, EINVAL, ENOTSUP, F16, F32, I8, OK
from helpers import full_range_codes as _codes

AUTO, NAIVE, GEMV, MFMA, MFMA_LARGE, SKINNY, NATIVE8 = range(7)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("mid", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("dtype", [torch.int8, torch.float8_e4m3fn, torch.float8_e5m2])
def test_op_default_is_the_two_op_sequence(dtype, mid, with_bias):
    gen = torch.Generator().manual_seed(11)
    M, N, K = 7, 24, 64
    a, b = _codes(dtype, (M, K), gen), _codes(dtype, (N, K), gen)
    if dtype != torch.int8:  # keep the fp16 product finite: e5m2 codes reach 57344
        a, b = (a.to(torch.float32) / 512).to(dtype), (b.to(torch.float32) / 512).to(dtype)
    scales = ((torch.rand((N, 1), generator=gen) + 0.5) * 1e-3).to(mid)
    bias = torch.randn(N, generator=gen).to(mid) if with_bias else None
    y = torch.ops.quanto.qbytes_mm_bias(a, b, scales, bias)
    out_scale = (y.abs().max().to(torch.float32) / (127 if dtype == torch.int8 else torch.finfo(dtype).max) * 0.7).to(mid)
    want = torch.ops.quanto.quantize_symmetric(y, dtype, None, out_scale)
    got = torch.ops.quanto.qbytes_mm_q(a, b, scales, bias, out_scale)
    assert got.dtype == dtype and got.shape == (M, N)
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    # a leading batch dimension is carried through, a one-element scale tensor is taken as the scalar
    got3 = torch.ops.quanto.qbytes_mm_q(a.reshape(1, M, K), b, scales, bias, out_scale.reshape(1))
    assert got3.shape == (1, M, N) and torch.equal(got3.view(torch.uint8).reshape(M, N), want.view(torch.uint8))


def _two_layer_model(weights, activations, dtype=torch.bfloat16):
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(64, 48), torch.nn.Linear(48, 32, bias=False)).to(dtype)
    quantize(model, weights=weights, activations=activations)
    freeze(model)
    for layer, (si, so) in zip(model, [(0.03, 0.02), (0.02, 0.01)]):
        if isinstance(layer, QLinear):
            layer.input_scale.fill_(si)
            layer.output_scale.fill_(so)
    return model


@pytest.mark.parametrize("qt", [qint8, qfloat8_e4m3fn, qfloat8_e5m2], ids=lambda q: q.name)
def test_fuse_output_quantization_marks_and_keeps_the_bits(qt):
    model = _two_layer_model(qt, qt)
    x = torch.randn(2, 5, 64, dtype=torch.bfloat16)
    keys = set(model.state_dict().keys())
    with torch.no_grad():
        ref = model(x)
        assert fuse_output_quantization(model) == ["0", "1"]
        assert all(m._fuse_output_quantization for m in model)
        fused = model(x)
        assert isinstance(fused, ActivationQBytesTensor) and fused.qtype == qt and fused.shape == ref.shape
        assert torch.equal(fused._data.view(torch.uint8), ref._data.view(torch.uint8))
        assert torch.equal(fused._scale, ref._scale)
        assert set(model.state_dict().keys()) == keys  # the mark is not serialised
        # with a gradient wanted the marked module runs the existing forward
        with torch.enable_grad():
            again = model(x)
        assert torch.equal(again._data.view(torch.uint8), ref._data.view(torch.uint8))
        assert fuse_output_quantization(model, enable=False) == ["0", "1"]
        assert not any(m._fuse_output_quantization for m in model)
        assert fuse_output_quantization(model, enable=False) == []


def test_marked_forward_calls_the_fused_op(monkeypatch):
    """The first layer gets a float input (its input hook quantizes it), the second the first's codes: both reach quanto::qbytes_mm_q once marked, and neither
    runs the separate output quantization."""
    import optimum_quanto_amd.nn.module as module_mod

    model = _two_layer_model(qint8, qint8)
    fuse_output_quantization(model)
    x = torch.randn(3, 64, dtype=torch.bfloat16)
    seen = []
    real = module_mod.quantize_activation
    monkeypatch.setattr(module_mod, "quantize_activation", lambda t, qtype, scale: (seen.append(tuple(t.shape)), real(t, qtype=qtype, scale=scale))[1])
    with torch.no_grad():
        out = model(x)
    assert isinstance(out, ActivationQBytesTensor)
    assert seen == [(3, 64)]  # the input hook of the first layer only: no float output was quantized in a second pass


def test_disable_output_quantization_unmarks():
    model = _two_layer_model(qint8, qint8)
    assert fuse_output_quantization(model) == ["0", "1"]
    model[1].disable_output_quantization()
    assert not model[1]._fuse_output_quantization
    with torch.no_grad():
        out = model(torch.randn(3, 64, dtype=torch.bfloat16))
    assert type(out) is torch.Tensor and out.dtype == torch.bfloat16  # the last layer returns its float output again
    assert fuse_output_quantization(model) == ["0"]  # a module without its output hook is not marked


@pytest.mark.parametrize("weights,activations,dtype", [(qint4, qint8, torch.bfloat16), (qint8, None, torch.bfloat16), (qint8, qfloat8_e4m3fn, torch.bfloat16),
                                                      (qint8, qint8, torch.float32)],
                         ids=["int4-weights", "no-activations", "mixed-families", "fp32-module"])
def test_models_outside_the_served_pairs_stay_unmarked(weights, activations, dtype):
    model = _two_layer_model(weights, activations, dtype)
    assert fuse_output_quantization(model) == []
    assert not any(m._fuse_output_quantization for m in model)


def test_unfrozen_modules_stay_unmarked():
    model = torch.nn.Sequential(torch.nn.Linear(64, 48)).to(torch.bfloat16)
    quantize(model, weights=qint8, activations=qint8)
    assert fuse_output_quantization(model) == []


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------
_c = quanto_hip.cdll
_vp, _i64, _ci, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t


def _entries():
    ws, plan = _c.quanto_hip_qbytes_mm_q_ws, _c.quanto_hip_qbytes_mm_q_plan
    ws.restype, ws.argtypes = _ci, [_vp] * 6 + [_i64] * 3 + [_ci] * 4 + [_vp, _sz, _vp]
    plan.restype, plan.argtypes = _ci, [_i64] * 3 + [_ci] * 4 + [ctypes.POINTER(_ci), ctypes.POINTER(_i64)]
    unfused = _c.quanto_hip_qbytes_mm_plan
    unfused.restype, unfused.argtypes = _ci, [_i64] * 3 + [_ci] * 4 + [ctypes.POINTER(_ci), ctypes.POINTER(_i64)]
    return ws, plan, unfused


def _q_ws(M, N, K, a=I8, b=I8, mid=BF16, kernel=AUTO):
    return _entries()[0](None, None, None, None, None, None, M, N, K, a, b, mid, kernel, None, 0, None)


def _plan(entry, M, N, K, a=I8, b=I8, mid=BF16, kernel=AUTO):
    k, ws = _ci(-7), _i64(-7)
    st = entry(M, N, K, a, b, mid, kernel, ctypes.byref(k), ctypes.byref(ws))
    return (k.value, ws.value) if st == 0 else st


def test_new_c_symbols_are_exported_and_the_abi_version_stays():
    _entries()
    _c.quanto_hip_abi_version.restype = _ci
    assert _c.quanto_hip_abi_version() == 1
    assert "quanto_hip_qbytes_mm_q_ws" in __import__("optimum_quanto_amd.library.hip", fromlist=["_PROTOTYPES"])._PROTOTYPES


NOT_SERVED = {
    "fp32 mid dtype": dict(mid=F32),
    "mid dtype not a float": dict(mid=I8),
    "int8 x e4m3": dict(a=I8, b=E4M3),
    "e4m3 x e5m2": dict(a=E4M3, b=E5M2),
    "float activations": dict(a=BF16, b=I8),
    "e4m3fnuz pair": dict(a=E4M3FNUZ, b=E4M3FNUZ),
    "K not a multiple of 64": dict(K=96),
    "K below 64": dict(K=32),
    "M * K at 2^31": dict(M=1 << 19, K=1 << 12),
    "N * K at 2^31": dict(N=1 << 19, K=1 << 12),
    "a kernel that stores no codes": dict(kernel=MFMA_LARGE),
    "the naive kernel": dict(kernel=NAIVE),
}


@pytest.mark.parametrize("why", sorted(NOT_SERVED))
def test_every_clause_of_the_argument_check_answers_enotsup(why):
    shape = dict(M=300, N=512, K=4096)
    kw = dict(NOT_SERVED[why])
    for d in "MNK":
        shape[d] = kw.pop(d, shape[d])
    assert _q_ws(shape["M"], shape["N"], shape["K"], **kw) == ENOTSUP, why
    assert _plan(_entries()[1], shape["M"], shape["N"], shape["K"], **kw) == ENOTSUP, why


def test_argument_check_einval_and_served_cases():
    assert _q_ws(-1, 512, 4096) == EINVAL and _q_ws(300, 0, 4096) == EINVAL and _q_ws(300, 512, 0) == EINVAL
    assert _q_ws(300, 512, 4096, kernel=42) == EINVAL  # no such kernel
    assert _entries()[1](300, 512, 4096, I8, I8, BF16, AUTO, None, None) == EINVAL
    # served: the check passes and only then are the (null) data pointers looked at; an empty product is done
    for pair in (I8, E4M3, E5M2):
        for mid in (BF16, F16):
            assert _q_ws(300, 512, 4096, a=pair, b=pair, mid=mid) == EINVAL
            assert _q_ws(300, 512, 4096, a=pair, b=pair, mid=mid, kernel=NATIVE8) == EINVAL
            assert _q_ws(0, 512, 4096, a=pair, b=pair, mid=mid) == OK
    assert _q_ws((1 << 19) - 1, 512, 4096) == EINVAL  # the largest M this K admits


@pytest.mark.parametrize("M,N,K", [(300, 512, 4096), (512, 4096, 14336), (128, 4096, 4096), (32, 4096, 14336), (256, 8192, 8192), (4096, 4096, 4096), (17, 100, 192)])
def test_plan_is_the_unfused_plan(M, N, K):
    """Same kernel, same split, same scratch for the fused and the unfused entry (the planner does not look at the output)."""
    _, fused, unfused = _entries()
    for pair in (I8, E4M3, E5M2):
        for mid in (BF16, F16):
            want = _plan(unfused, M, N, K, a=pair, b=pair, mid=mid)
            assert want[0] == NATIVE8
            assert _plan(fused, M, N, K, a=pair, b=pair, mid=mid) == want
            assert _plan(fused, M, N, K, a=pair, b=pair, mid=mid, kernel=NATIVE8) == want

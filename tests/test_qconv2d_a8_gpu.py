"""QConv2d with quantized activations on the 8-bit matrix instructions (csrc/qconv_a8.hip, quanto::qbytes_conv2d_a8) on the MI355X."""
import numpy as np
import pytest
import torch

import optimum_quanto_amd as Q
from optimum_quanto_amd.library.hip import quanto_hip

from oracle import quanto_oracle as O

from helpers import TORCH_DT, assert_close_to_exact, assert_close_with_bias, assert_similar, observed_activation_scales, to_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = {"e4m3fn": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def _kernel_name(xdt, wdt):
    if xdt == torch.int8:
        return "conv2d_a8_int8"
    return "conv2d_a8_fp8_w8" if wdt == torch.int8 else "conv2d_a8_fp8"


def _codes(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int8:
        return torch.randint(-128, 128, shape, generator=g, dtype=torch.int8)
    return (torch.randn(shape, generator=g) * 4).to(dtype)


def _scales(OC, dt, seed):
    g = torch.Generator().manual_seed(seed)
    xs = torch.tensor([0.0173], dtype=TORCH_DT[dt])
    ws = (torch.rand(OC, 1, 1, 1, generator=g) * 0.004 + 0.0005).to(TORCH_DT[dt])
    return xs, ws


def _im2col(x, KH, KW, s, p, d):
    """float64 im2col of the codes (exact for int8 / fp8 values): [B*OH*OW, C*KH*KW] in the weight's (c, i, j) order."""
    cols = torch.nn.functional.unfold(x, (KH, KW), dilation=d, padding=p, stride=s)  # [B, K, L]
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def _values(t):
    return t.to(torch.float64) if t.dtype == torch.int8 else t.to(torch.float32).to(torch.float64)


def _run(x, xs, w, ws, bias, s, p, d, workspace=True):
    """The binding (workspace when the K split wants one) or the C entry with no workspace at all (unsplit)."""
    lib = quanto_hip.lib
    if workspace:
        return lib.qbytes_conv2d_a8(x, xs, w, ws, bias, s, p, d)
    B, C, H, W = x.shape
    OC, _, KH, KW = w.shape
    OH, OW = lib.conv2d_out_size(H, KH, s[0], p[0], d[0]), lib.conv2d_out_size(W, KW, s[1], p[1], d[1])
    odt = ws.dtype
    y = torch.empty((B, OC, OH, OW), dtype=odt, device=x.device)
    xs1, ws1 = xs.reshape(1).to(odt).contiguous(), ws.reshape(-1).contiguous()
    b1 = None if bias is None else bias.to(odt).contiguous()
    from optimum_quanto_amd.library.hip import _DTYPES

    st = lib._c.quanto_hip_qbytes_conv2d_a8(x.data_ptr(), xs1.data_ptr(), w.data_ptr(), ws1.data_ptr(), 0 if b1 is None else b1.data_ptr(), y.data_ptr(),
                                            B, C, H, W, OC, KH, KW, OH, OW, s[0], s[1], p[0], p[1], d[0], d[1], _DTYPES[x.dtype], _DTYPES[w.dtype],
                                            _DTYPES[odt], 0, 0, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    return y


def _int_reference(x, xs, w, ws, bias, s, p, d, dt):
    """oracle.qbytes_int_mm_ref on the im2col of the integer codes, sc = round_dt(a_scale * w_scale), bias added to the rounded product."""
    B = x.shape[0]
    OC, _, KH, KW = w.shape
    a = _im2col(x.to(torch.float64), KH, KW, s, p, d).numpy().astype(np.int64)
    sc = to_numpy(xs.to(TORCH_DT[dt]) * ws.reshape(-1).to(TORCH_DT[dt]))  # torch's product in the dtype
    v = O.qbytes_int_mm_ref(a, w.reshape(OC, -1).numpy().astype(np.int64), sc, dt)
    if bias is not None:
        v = O.round_to(v.astype(np.float32) + to_numpy(bias.to(TORCH_DT[dt])).reshape(1, -1), dt)
    L = v.shape[0] // B
    return v.reshape(B, L, OC).transpose(0, 2, 1)


# (B, cin, H, W, OC, KH, KW, stride, padding, dilation): every window, strides 1 / 2, dilations 1 / 2, padding 0..3, ragged K, odd sizes
INT_GRID = [
    (2, 64, 13, 11, 96, 3, 3, (1, 1), (1, 1), (1, 1)),
    (1, 3, 31, 29, 10, 7, 7, (2, 2), (3, 3), (1, 1)),
    (8, 5, 9, 15, 200, 5, 5, (1, 2), (2, 0), (2, 1)),
    (2, 128, 7, 7, 128, 1, 1, (1, 1), (0, 0), (1, 1)),
    (1, 128, 15, 9, 200, 3, 3, (2, 1), (0, 3), (2, 2)),
    (8, 64, 5, 7, 10, 1, 1, (2, 2), (1, 0), (1, 1)),
    (1, 5, 17, 13, 96, 3, 5, (1, 1), (2, 1), (1, 2)),
    (2, 3, 21, 23, 128, 5, 3, (2, 1), (3, 2), (1, 1)),
    (1, 128, 9, 9, 96, 7, 7, (1, 1), (3, 3), (1, 1)),   # 49 taps: two mask words; K = 6272 gets split
]


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("geo", INT_GRID, ids=lambda g: "x".join(str(v) for v in g[:7]) + f"-s{g[7][0]}{g[7][1]}p{g[8][0]}{g[8][1]}d{g[9][0]}{g[9][1]}")
def test_int8_x_int8_bit_exact_split_and_unsplit(geo, bias, dt):
    B, C, H, W, OC, KH, KW, s, p, d = geo
    x, w = _codes((B, C, H, W), torch.int8, 1), _codes((OC, C, KH, KW), torch.int8, 2)
    xs, ws = _scales(OC, dt, 3)
    b = (torch.randn(OC, generator=torch.Generator().manual_seed(10)) * 0.5).to(TORCH_DT[dt]) if bias else None
    want = _int_reference(x, xs, w, ws, b, s, p, d, dt)
    xd, wd, xsd, wsd, bd = x.to(DEV), w.to(DEV), xs.to(DEV), ws.to(DEV), None if b is None else b.to(DEV)
    y_ws = _run(xd, xsd, wd, wsd, bd, s, p, d, workspace=True)
    assert quanto_hip.lib.last_kernel() == "conv2d_a8_int8"
    y_no = _run(xd, xsd, wd, wsd, bd, s, p, d, workspace=False)
    assert quanto_hip.lib.last_kernel() == "conv2d_a8_int8"
    torch.cuda.synchronize()
    assert torch.equal(y_ws, y_no), "split and unsplit results differ"
    got = to_numpy(y_ws).reshape(want.shape)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} elements differ from the integer reference"


def test_int8_forced_split_is_bit_identical(monkeypatch):
    B, C, H, W, OC = 2, 128, 14, 14, 128
    x, w = _codes((B, C, H, W), torch.int8, 4).to(DEV), _codes((OC, C, 3, 3), torch.int8, 5).to(DEV)
    xs, ws = (t.to(DEV) for t in _scales(OC, "bf16", 6))
    y1 = _run(x, xs, w, ws, None, (1, 1), (1, 1), (1, 1), workspace=False)
    for split in ("2", "3", "9"):
        monkeypatch.setenv("QUANTO_HIP_CONV_SPLIT", split)
        y = _run(x, xs, w, ws, None, (1, 1), (1, 1), (1, 1), workspace=True)
        torch.cuda.synchronize()
        assert torch.equal(y, y1), f"split {split}"


FP_PAIRS = [(torch.float8_e4m3fn, torch.float8_e4m3fn), (torch.float8_e4m3fn, torch.float8_e5m2), (torch.float8_e5m2, torch.float8_e4m3fn),
            (torch.float8_e5m2, torch.float8_e5m2), (torch.float8_e4m3fn, torch.int8), (torch.float8_e5m2, torch.int8)]
FP_GRID = [INT_GRID[0], INT_GRID[1], INT_GRID[2], INT_GRID[4], INT_GRID[8]]


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("geo", FP_GRID, ids=lambda g: "x".join(str(v) for v in g[:7]))
@pytest.mark.parametrize("xdt,wdt", FP_PAIRS, ids=lambda t: str(t).replace("torch.", ""))
def test_fp8_pairs_within_exact_math_gate(xdt, wdt, geo, bias, dt):
    B, C, H, W, OC, KH, KW, s, p, d = geo
    x, w = _codes((B, C, H, W), xdt, 7), _codes((OC, C, KH, KW), wdt, 8)
    xs, ws = _scales(OC, dt, 9)
    b = (torch.randn(OC, generator=torch.Generator().manual_seed(10)) * 0.5).to(TORCH_DT[dt]) if bias else None
    y = _run(x.to(DEV), xs.to(DEV), w.to(DEV), ws.to(DEV), None if b is None else b.to(DEV), s, p, d)
    assert quanto_hip.lib.last_kernel() == _kernel_name(xdt, wdt)
    a = _im2col(_values(x), KH, KW, s, p, d).numpy()
    sc = to_numpy(xs.to(TORCH_DT[dt]) * ws.reshape(-1).to(TORCH_DT[dt])).astype(np.float64)
    prod = np.matmul(a, _values(w).reshape(OC, -1).numpy().T) * sc.reshape(1, -1)
    got = to_numpy(y).reshape(B, OC, -1).transpose(0, 2, 1).reshape(-1, OC)
    what = f"{xdt} x {wdt} {geo} {dt}"
    if b is None:
        assert_close_to_exact(got, prod, dt, what)
    elif dt == "fp32":  # an fp32 sum of K products is not within one fp32 ulp of the exact one: the fp32 gate on product + bias
        assert_close_to_exact(got, prod + to_numpy(b).astype(np.float64).reshape(1, -1), dt, what)
    else:
        assert_close_with_bias(got, prod, to_numpy(b.to(TORCH_DT[dt])).astype(np.float64).reshape(1, -1), dt, what)


def _all_codes(dtype):
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    if dtype == torch.int8:
        return codes.view(torch.int8)
    codes[~torch.isfinite(codes.view(dtype).to(torch.float32))] = 0  # non-finite codes -> 0
    return codes.view(dtype)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("xdt,wdt", [(torch.int8, torch.int8)] + FP_PAIRS, ids=lambda t: str(t).replace("torch.", ""))
def test_every_code_against_every_code(xdt, wdt, dt):
    """K = 1: one product per output - every finite activation code times every weight code, bit-exact after the one rounding."""
    x = _all_codes(xdt).reshape(1, 1, 16, 16)
    w = _all_codes(wdt).reshape(256, 1, 1, 1)
    xs = torch.ones(1, dtype=TORCH_DT[dt])
    ws = torch.ones(256, 1, 1, 1, dtype=TORCH_DT[dt])
    y = _run(x.to(DEV), xs.to(DEV), w.to(DEV), ws.to(DEV), None, (1, 1), (0, 0), (1, 1))
    prod = np.outer(_values(w).reshape(-1).numpy(), _values(x).reshape(-1).numpy()).astype(np.float32)  # exact: [OC, pixels]
    with np.errstate(over="ignore"):
        want = O.round_to(prod, dt)
    got = to_numpy(y).reshape(256, 256)
    assert np.array_equal(got, want), f"{int((got != want).sum())} products differ"


# ---- module level (the reference's tests/nn/test_qconv2d.py:31-103) ----------------------------------------------------------------------------
ACTS = {"a-qint8": Q.qint8, "a-qfloat8-e4m3": Q.qfloat8_e4m3fn, "a-qfloat8-e5m2": Q.qfloat8_e5m2}
WEIGHTS = {"w-qint8": Q.qint8, "w-qfloat8-e4m3": Q.qfloat8_e4m3fn}


def _qconv(cin, cout, k, dtype, weights, activations, stride=1, padding=0, groups=1, seed=0):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, k, stride=stride, padding=padding, groups=groups, bias=True).to(dtype).to(DEV)
    return Q.QConv2d.from_module(conv, weights=weights, activations=activations)


def _qinput(shape, qtype, dtype, seed=0):
    torch.manual_seed(seed)
    t = (torch.rand(shape, dtype=torch.float32) * 2 - 1).to(dtype).to(DEV)
    return Q.quantize_activation(t, qtype=qtype, scale=Q.absmax_scale(t, qtype=qtype))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("aname", list(ACTS))
@pytest.mark.parametrize("batch,img", [(1, 28), (10, 32)])
def test_qconv2d_quantized_activations_module(batch, img, aname, wname, dtype):
    weights, activations = WEIGHTS[wname], ACTS[aname]
    if weights is not Q.qint8 and activations is Q.qint8:
        pytest.skip("int8 activations x fp8 weights keep the dequantizing route (not served)")
    qconv = _qconv(3, 10, 3, dtype, weights, activations)
    qin = _qinput((batch, 3, img, img), activations, dtype)
    with torch.no_grad(), observed_activation_scales():
        qconv(qin)
    Q.freeze(qconv)
    with torch.no_grad():
        qout = qconv(qin)
    if activations is Q.qfloat8_e5m2 and dtype == torch.float16:  # the fp16 scale product of an e5m2 scale underflows: dequantizing route kept
        assert not quanto_hip.lib.last_kernel().startswith("conv2d_a8")
    else:
        assert quanto_hip.lib.last_kernel() == _kernel_name(qin._data.dtype, qconv.qweight._data.dtype)
    with torch.no_grad():
        ref = torch.nn.functional.conv2d(qin.dequantize(), qconv.qweight.dequantize(), qconv.bias)
    atol = {torch.float16: 1e-3, torch.float32: 1e-4}[dtype]
    if activations is not Q.qint8:
        atol = 5e-3
    assert_similar(qout.dequantize() if isinstance(qout, Q.QTensor) else qout, ref, atol=atol)


@pytest.mark.parametrize("activations", [Q.qint8, Q.qfloat8_e4m3fn], ids=["a-qint8", "a-qfloat8-e4m3"])
def test_w8a8_conv_net_runs_on_the_new_kernel(activations, monkeypatch):
    """conv -> ReLU -> conv on a quantized input: int8 activations stay quantized through the ReLU, so both convolutions take the new kernel; an fp8
    output is dequantized by the ReLU, so there only the first one does."""
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(16, 64, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(64, 32, 3, stride=2, padding=1)).to(torch.bfloat16).to(DEV)
    x = torch.randn(4, 16, 23, 23, dtype=torch.bfloat16, device=DEV)
    qx = Q.quantize_activation(x, qtype=activations, scale=Q.absmax_scale(x, qtype=activations))
    with torch.no_grad():
        ref = model(qx.dequantize())
    Q.quantize(model, weights=Q.qint8, activations=activations)
    with torch.no_grad(), observed_activation_scales():
        model(qx)
    Q.freeze(model)
    names = []
    monkeypatch.setattr(quanto_hip.lib, "qbytes_conv2d_a8", _recording(quanto_hip.lib.qbytes_conv2d_a8, names))
    with torch.no_grad():
        out = model(qx)
    out = out.dequantize() if isinstance(out, Q.QTensor) else out
    want = _kernel_name(activations.dtype, torch.int8)
    assert names == ([want, want] if activations is Q.qint8 else [want]), names
    assert_similar(out, ref, atol=2e-2)


def _recording(fn, names):
    def wrapped(*args, **kwargs):
        y = fn(*args, **kwargs)
        names.append(quanto_hip.lib.last_kernel())
        return y

    return wrapped


# ---- routes that must not move --------------------------------------------------------------------------------------------------------------------
def _mark_last_kernel():
    """Run a small plain product so that last_kernel() names something other than a conv2d_a8 kernel."""
    a = torch.ones(4, 64, dtype=torch.bfloat16, device=DEV)
    torch.ops.quanto.qbytes_mm(a, torch.ones(64, 64, dtype=torch.int8, device=DEV), torch.ones(64, 1, dtype=torch.bfloat16, device=DEV))
    assert not quanto_hip.lib.last_kernel().startswith("conv2d_a8")


def _op_default(qin, qconv, stride=1, padding=0):
    from optimum_quanto_amd.library.ops import qbytes_conv2d_a8_default

    s, p = [stride] * 2, [padding] * 2
    return qbytes_conv2d_a8_default(qin._data, qin._scale, qconv.qweight._data, qconv.qweight._scale, qconv.bias, s, p, [1, 1])


def test_route_with_gradient_wanted_is_unchanged():
    qconv = _qconv(8, 16, 3, torch.float32, Q.qint8, Q.qint8)  # not frozen: the weight is quantized per call and wants a gradient
    qin = _qinput((2, 8, 12, 12), Q.qint8, torch.float32)
    with torch.no_grad(), observed_activation_scales():
        qconv(qin)
    _mark_last_kernel()
    with torch.enable_grad():
        out = torch.nn.functional.conv2d(qin, qconv.qweight, qconv.bias)
    assert out.requires_grad
    assert not quanto_hip.lib.last_kernel().startswith("conv2d_a8")
    torch.testing.assert_close(out.detach(), _op_default(qin, qconv), rtol=1e-5, atol=1e-5)


def test_route_grouped_conv_is_unchanged():
    qconv = _qconv(16, 32, 3, torch.bfloat16, Q.qint8, Q.qint8, padding=1, groups=4)
    qin = _qinput((2, 16, 10, 10), Q.qint8, torch.bfloat16)
    with torch.no_grad(), observed_activation_scales():
        qconv(qin)
    Q.freeze(qconv)
    _mark_last_kernel()
    with torch.no_grad():
        out = torch.nn.functional.conv2d(qin, qconv.qweight, qconv.bias, 1, 1, 1, 4)
    assert not quanto_hip.lib.last_kernel().startswith("conv2d_a8")
    x = qin.dequantize()
    want = torch.nn.functional.conv2d(x, qconv.qweight.dequantize(), qconv.bias, 1, 1, 1, 4)
    torch.testing.assert_close(out, want, rtol=1.6e-2, atol=1e-2)


def test_route_int4_weights_with_quantized_activations_is_unchanged():
    qconv = _qconv(32, 64, 3, torch.bfloat16, Q.qint4, Q.qint8, padding=1)
    qin = _qinput((2, 32, 10, 10), Q.qint8, torch.bfloat16)
    with torch.no_grad(), observed_activation_scales():
        qconv(qin)
    Q.freeze(qconv)
    _mark_last_kernel()
    with torch.no_grad():
        out = torch.nn.functional.conv2d(qin, qconv.qweight, qconv.bias, 1, 1)
    assert not quanto_hip.lib.last_kernel().startswith("conv2d_a8")
    want = torch.nn.functional.conv2d(qin.dequantize(), qconv.qweight.dequantize(), qconv.bias, 1, 1)
    assert_similar(out, want, atol=1e-2)


def test_route_e4m3fnuz_activations_is_unchanged():
    qconv = _qconv(32, 64, 3, torch.bfloat16, Q.qint8, Q.qfloat8_e4m3fnuz, padding=1)
    qin = _qinput((2, 32, 10, 10), Q.qfloat8_e4m3fnuz, torch.bfloat16)
    with torch.no_grad(), observed_activation_scales():
        qconv(qin)
    Q.freeze(qconv)
    _mark_last_kernel()
    with torch.no_grad():
        out = torch.nn.functional.conv2d(qin, qconv.qweight, qconv.bias, 1, 1)
    assert not quanto_hip.lib.last_kernel().startswith("conv2d_a8")
    assert_similar(out, _op_default(qin, qconv, padding=1), atol=1e-2)


def test_route_plain_bf16_input_keeps_the_16bit_kernel():
    qconv = _qconv(64, 96, 3, torch.bfloat16, Q.qint8, None, padding=1)
    Q.freeze(qconv)
    x = torch.randn(2, 64, 14, 14, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        qconv(x)
    assert quanto_hip.lib.last_kernel().startswith("conv2d_mfma")


# ---- empty batch and graph capture ------------------------------------------------------------------------------------------------------------------
def test_empty_batch_returns_empty():
    x = torch.zeros(0, 8, 9, 9, dtype=torch.int8, device=DEV)
    w = _codes((16, 8, 3, 3), torch.int8, 1).to(DEV)
    xs, ws = (t.to(DEV) for t in _scales(16, "bf16", 2))
    y = quanto_hip.lib.qbytes_conv2d_a8(x, xs, w, ws, None, (1, 1), (1, 1), (1, 1))
    assert y.shape == (0, 16, 9, 9) and y.dtype == torch.bfloat16
    y = torch.ops.quanto.qbytes_conv2d_a8(x, xs, w, ws, None, [1, 1], [1, 1], [1, 1])
    assert y.shape == (0, 16, 9, 9)


@pytest.mark.parametrize("xdt,wdt,C", [(torch.int8, torch.int8, 64), (torch.float8_e4m3fn, torch.int8, 512), (torch.float8_e5m2, torch.float8_e4m3fn, 64)])
def test_graph_capture_matches_eager(xdt, wdt, C):
    x, w = _codes((1, C, 7, 7), xdt, 3).to(DEV), _codes((128, C, 3, 3), wdt, 4).to(DEV)
    xs, ws = (t.to(DEV) for t in _scales(128, "bf16", 5))
    args = (x, xs, w, ws, None, [1, 1], [1, 1], [1, 1])
    eager = torch.ops.quanto.qbytes_conv2d_a8(*args)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.ops.quanto.qbytes_conv2d_a8(*args)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = torch.ops.quanto.qbytes_conv2d_a8(*args)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)

"""Fused output quantization of QConv2d with quantized activations on the device: ``quanto::qbytes_conv2d_a8_q`` (csrc/qconv_a8.hip with QOUT, store_codes)
against the two existing ops.

Criterion everywhere: the fused codes equal ``quantize_symmetric(lib.qbytes_conv2d_a8(...), dtype, None, out_scale)`` computed by the existing kernels on
the same device tensors under the same knobs, bit for bit, every element; ``last_kernel()`` is the unfused name plus ``_q``.

``out_scale`` is the 0.9-quantile of the unfused |y| divided by the code type's maximum (127 / 448 / 57344), rounded to the mid dtype: the sequence
itself then clamps about a tenth of the elements.  Asserted: 2-25 % of the sequence's codes sit at the extreme values, so no case passes on all-zero or
all-clamped codes.  All shapes are small: a case takes milliseconds.
"""
import pytest
import torch

import optimum_quanto_amd as Q
from optimum_quanto_amd.library.hip import _DTYPES, quanto_hip

from helpers import CODE_QMAX as QMAX
from helpers import assert_nothing_outside, quantile_out_scale, sentinel_buffer

pytestmark = pytest.mark.gpu
DEV = "cuda"
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


def _kernel_name(xdt, wdt):
    if xdt == torch.int8:
        return "conv2d_a8_int8"
    return "conv2d_a8_fp8_w8" if wdt == torch.int8 else "conv2d_a8_fp8"


def _codes(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int8:
        return torch.randint(-128, 128, shape, generator=g, dtype=torch.int8)
    return (torch.randn(shape, generator=g) * 4).to(dtype)


RMS = {torch.int8: 74.0, E4M3: 4.0, E5M2: 4.0}  # of _codes


def _scales(OC, K, xdt, wdt, dt, seed):
    """Scales that keep the output of order one whatever the formats and K, so that out_scale is far from the bottom of fp16 for every code type."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.tensor([1.0 / (RMS[xdt] * K ** 0.5)], dtype=TDT[dt])
    ws = ((torch.rand(OC, 1, 1, 1, generator=g) + 0.5) / RMS[wdt]).to(TDT[dt])
    return xs, ws


def problem(geo, xdt, wdt, dt, bias, seed=1):
    B, C, H, W, OC, KH, KW, s, p, d = geo
    x, w = _codes((B, C, H, W), xdt, seed), _codes((OC, C, KH, KW), wdt, seed + 1)
    xs, ws = _scales(OC, C * KH * KW, xdt, wdt, dt, seed + 2)
    b = (torch.randn(OC, generator=torch.Generator().manual_seed(seed + 3)) * 0.5).to(TDT[dt]) if bias else None
    return dict(x=x.to(DEV), xs=xs.to(DEV), w=w.to(DEV), ws=ws.to(DEV), b=None if b is None else b.to(DEV), s=s, p=p, d=d)


def operands(p):
    return p["x"], p["xs"], p["w"], p["ws"], p["b"]


def geometry(p):
    return p["s"], p["p"], p["d"]


def extreme_share(codes):
    """Share of the codes at the two extreme values of their type (int8: -128 / 127; float8: +-max, the clamp's targets)."""
    if codes.dtype == torch.int8:
        return ((codes == 127) | (codes == -128)).to(torch.float32).mean().item()
    return (codes.to(torch.float32).abs() == QMAX[codes.dtype]).to(torch.float32).mean().item()


def sequence(p):
    """(codes of the existing quantizer on the existing kernel's output, out_scale) - with the route and the share of extreme codes asserted."""
    lib = quanto_hip.lib
    y = lib.qbytes_conv2d_a8(*operands(p), *geometry(p))
    assert lib.last_kernel() == _kernel_name(p["x"].dtype, p["w"].dtype)
    assert bool(torch.isfinite(y).all())
    dtype = p["x"].dtype
    out_scale = quantile_out_scale(y, dtype)
    want = torch.ops.quanto.quantize_symmetric(y, dtype, None, out_scale)
    share = extreme_share(want)
    print(f"{tuple(y.shape)} {dtype} {y.dtype}: out_scale {out_scale.item():.6g}, extreme codes {share:.4f}")
    assert 0.02 <= share <= 0.25, f"{share:.4f} of the sequence's codes sit at the extreme values at this output scale"
    return want, out_scale


def c_entry(p, out_scale=None, scratch=False, yq=None):
    """The C entry itself - unfused (``out_scale`` None) or fused - with no workspace at all (unsplit) or with a scratch buffer sized by the workspace
    query under the current environment; the binding keeps its plan per shape, this does not."""
    lib = quanto_hip.lib
    x, xs, w, ws, b = operands(p)
    s, pad, d = geometry(p)
    B, C, H, W = x.shape
    OC, _, KH, KW = w.shape
    OH, OW = lib.conv2d_out_size(H, KH, s[0], pad[0], d[0]), lib.conv2d_out_size(W, KW, s[1], pad[1], d[1])
    odt = ws.dtype
    geo = (B, C, H, W, OC, KH, KW, OH, OW, s[0], s[1], pad[0], pad[1], d[0], d[1], _DTYPES[x.dtype], _DTYPES[w.dtype], _DTYPES[odt])
    nbytes = int(lib._c.quanto_hip_qbytes_conv2d_a8_workspace_size(*geo)) if scratch else 0
    assert nbytes >= 0
    buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
    xs1, ws1 = xs.reshape(1).to(odt).contiguous(), ws.reshape(-1).contiguous()
    head = (x.data_ptr(), xs1.data_ptr(), w.data_ptr(), ws1.data_ptr(), 0 if b is None else b.data_ptr())
    tail = (0 if buf is None else buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    if out_scale is None:
        out = torch.empty((B, OC, OH, OW), dtype=odt, device=DEV)
        st = lib._c.quanto_hip_qbytes_conv2d_a8(*head, out.data_ptr(), *geo, *tail)
    else:
        out = torch.empty((B, OC, OH, OW), dtype=x.dtype, device=DEV) if yq is None else yq
        assert tuple(out.shape) == (B, OC, OH, OW) and out.is_contiguous()
        os1 = out_scale.reshape(1).to(odt).contiguous()
        st = lib._c.quanto_hip_qbytes_conv2d_a8_q(*head, os1.data_ptr(), out.data_ptr(), *geo, *tail)
    assert st == 0
    torch.cuda.synchronize()  # the temporaries stay alive until the kernels have read them
    assert lib.last_kernel() == _kernel_name(x.dtype, w.dtype) + ("" if out_scale is None else "_q")
    return out, nbytes


def fused(p, out_scale, workspace=True, yq=None):
    """The binding (workspace when the K split wants one), or the C entry with no workspace at all (unsplit) and, if given, the caller's ``yq``."""
    lib = quanto_hip.lib
    if workspace and yq is None:
        got = lib.qbytes_conv2d_a8_q(*operands(p), out_scale, *geometry(p))
        assert lib.last_kernel() == _kernel_name(p["x"].dtype, p["w"].dtype) + "_q"
        return got
    return c_entry(p, out_scale, yq=yq)[0]


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape
    g, w = got.view(torch.uint8), want.view(torch.uint8)
    assert torch.equal(g, w), f"{int((g != w).sum())} of {g.numel()} codes differ from the two-op sequence {what}"


def check_fused(p):
    """Fused codes through the binding (split when the plan splits, as the sequence's convolution); for int8 x int8 - whose accumulators are exact,
    split or not - also through the C entry without a workspace."""
    want, out_scale = sequence(p)
    got = fused(p, out_scale, workspace=True)
    same(got, want, "(with workspace)")
    if p["x"].dtype == torch.int8:
        got_no = fused(p, out_scale, workspace=False)
        same(got_no, want, "(without workspace)")
        same(got_no, got, "(with against without workspace)")
    return got, out_scale


# (B, cin, H, W, OC, KH, KW, stride, padding, dilation): the grid of tests/test_qconv2d_a8_gpu.py - windows 1x1 to 7x7, strides and dilations 1 / 2,
# ragged K, OC in {10, 96, 128, 200}, the wide tap mask, one natural K split
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
FP_PAIRS = [(E4M3, E4M3), (E4M3, E5M2), (E5M2, E4M3), (E5M2, E5M2), (E4M3, torch.int8), (E5M2, torch.int8)]
FP_GRID = [INT_GRID[0], INT_GRID[1], INT_GRID[2], INT_GRID[4], INT_GRID[8]]
_geo_id = lambda g: "x".join(str(v) for v in g[:7]) + f"-s{g[7][0]}{g[7][1]}p{g[8][0]}{g[8][1]}d{g[9][0]}{g[9][1]}"  # noqa: E731
_dt_id = lambda t: str(t).replace("torch.", "")  # noqa: E731


def test_the_natural_split_case_is_split():
    B, C, H, W, OC, KH, KW, s, p, d = INT_GRID[8]
    assert quanto_hip.lib._conv2d_a8_workspace((B, C, H, W), (OC, C, KH, KW), torch.int8, torch.int8, torch.bfloat16, s, p, d) > 0


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("geo", INT_GRID, ids=_geo_id)
def test_int8_codes_equal_the_sequence_with_and_without_workspace(geo, bias, dt):
    check_fused(problem(geo, torch.int8, torch.int8, dt, bias))


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("geo", FP_GRID, ids=_geo_id)
@pytest.mark.parametrize("xdt,wdt", FP_PAIRS, ids=_dt_id)
def test_fp8_pairs_codes_equal_the_sequence(xdt, wdt, geo, bias, dt):
    check_fused(problem(geo, xdt, wdt, dt, bias, seed=7))


# ---- geometries aimed at the code store ----------------------------------------------------------------------------------------------------------------
STORE_GRID = [
    (5, 16, 3, 3, 24, 3, 3, (1, 1), (0, 0), (1, 1)),     # plane of 1 pixel: every lane's four pixels are four images
    (7, 16, 4, 3, 24, 3, 3, (1, 1), (0, 0), (1, 1)),     # plane of 2 pixels
    (6, 16, 3, 5, 24, 3, 3, (1, 1), (0, 0), (1, 1)),     # plane of 3 pixels
    (3, 8, 6, 6, 40, 3, 3, (1, 1), (1, 1), (1, 1)),      # L = 36 (L % 4 == 0), M = 108: a ragged last pixel tile on the dword path
    (1, 16, 1, 129, 24, 1, 1, (1, 1), (0, 0), (1, 1)),   # M = 129: one pixel in the second tile
]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("geo", STORE_GRID, ids=_geo_id)
@pytest.mark.parametrize("xdt", [torch.int8, E4M3], ids=_dt_id)
def test_store_paths(xdt, geo, bias, dt):
    B, C, H, W, OC, KH, KW, s, p, d = geo
    L = ((H + 2 * p[0] - KH) // s[0] + 1) * ((W + 2 * p[1] - KW) // s[1] + 1)
    assert (L, B * L) in ((1, 5), (2, 14), (3, 18), (36, 108), (129, 129))
    check_fused(problem(geo, xdt, xdt, dt, bias, seed=11))


@pytest.mark.parametrize("offset", [0, 1, 2, 4, 16])
@pytest.mark.parametrize("geo", [STORE_GRID[3], STORE_GRID[2]], ids=["L36", "L3"])
@pytest.mark.parametrize("xdt", [torch.int8, E4M3], ids=_dt_id)
def test_no_byte_outside_a_misaligned_output(xdt, geo, offset):
    p = problem(geo, xdt, xdt, "bf16", True, seed=13)
    want, out_scale = sequence(p)
    n = want.numel()
    buf, lead = sentinel_buffer(n, offset, DEV)
    yq = buf[lead:lead + n].view(xdt).reshape(want.shape)
    assert yq.data_ptr() % 256 == offset
    fused(p, out_scale, yq=yq)
    assert torch.equal(buf[lead:lead + n], want.view(torch.uint8).reshape(-1)), "codes differ from the two-op sequence"
    assert_nothing_outside(buf, lead, n, "the output")


# ---- forced split: the reduce kernel runs the code epilogue on the summed accumulators ------------------------------------------------------------------
SPLIT_GEO = (2, 128, 14, 14, 128, 3, 3, (1, 1), (1, 1), (1, 1))


@pytest.mark.parametrize("xdt,wdt", [(torch.int8, torch.int8), (E4M3, E4M3), (E4M3, torch.int8)], ids=_dt_id)
def test_forced_split(monkeypatch, xdt, wdt):
    p = problem(SPLIT_GEO, xdt, wdt, "bf16", True, seed=17)
    _, out_scale = sequence(p)
    y1, _ = c_entry(p)  # no workspace: unsplit
    unsplit, _ = c_entry(p, out_scale)
    same(unsplit, torch.ops.quanto.quantize_symmetric(y1, xdt, None, out_scale), "(unsplit)")
    for split in (2, 3, 9):
        monkeypatch.setenv("QUANTO_HIP_CONV_SPLIT", str(split))
        y, nbytes = c_entry(p, scratch=True)
        assert nbytes == split * 4 * 128 * 128 * 4, "the plan did not split as forced"  # 4 pixel tiles x 1 channel tile
        want = torch.ops.quanto.quantize_symmetric(y, xdt, None, out_scale)
        assert 0.02 <= extreme_share(want) <= 0.25
        got, _ = c_entry(p, out_scale, scratch=True)
        same(got, want, f"(split {split})")
        if xdt == torch.int8:
            same(got, unsplit, f"(split {split} against unsplit)")


# ---- the op: the fused kernel exactly when quanto::qbytes_conv2d_a8 runs its kernel, the sequence on the existing ops otherwise -------------------------
def _mark_last_kernel():
    """Run a small plain product so that last_kernel() names something other than a conv2d_a8 kernel: the sequence's float route launches no kernel
    of the library's that sets a name, and the name of an earlier test's launch would otherwise be read."""
    a = torch.ones(4, 64, dtype=torch.bfloat16, device=DEV)
    torch.ops.quanto.qbytes_mm(a, torch.ones(64, 64, dtype=torch.int8, device=DEV), torch.ones(64, 1, dtype=torch.bfloat16, device=DEV))
    assert not quanto_hip.lib.last_kernel().startswith("conv2d_a8")


def check_op(p, expect_fused, xs=None):
    lib = quanto_hip.lib
    x, xs0, w, ws, b = operands(p)
    xs = xs0 if xs is None else xs
    geo = [list(v) for v in geometry(p)]
    y = torch.ops.quanto.qbytes_conv2d_a8(x, xs, w, ws, b, *geo)
    out_scale = quantile_out_scale(y, x.dtype)
    want = torch.ops.quanto.quantize_symmetric(y, x.dtype, None, out_scale)
    assert 0.02 <= extreme_share(want) <= 0.25
    from optimum_quanto_amd.library.ops import qbytes_conv2d_a8_q_default

    default = qbytes_conv2d_a8_q_default(x, xs, w, ws, b, out_scale, *geo)
    _mark_last_kernel()
    got = torch.ops.quanto.qbytes_conv2d_a8_q(x, xs, w, ws, b, out_scale, *geo)
    route = lib.last_kernel()
    same(got, want)
    same(got, default, "(the default op)")
    if expect_fused:
        assert route == _kernel_name(x.dtype, w.dtype) + "_q"
    else:
        assert not route.endswith("_q")


def test_op_takes_the_fused_kernel_when_served():
    check_op(problem(INT_GRID[0], torch.int8, torch.int8, "bf16", True), True)
    check_op(problem(INT_GRID[0], E5M2, torch.int8, "fp32", False), True)


def test_op_runs_the_sequence_for_int8_activations_with_fp8_weights():
    check_op(problem((2, 16, 9, 9, 24, 3, 3, (1, 1), (1, 1), (1, 1)), torch.int8, E4M3, "bf16", True), False)


def test_op_runs_the_sequence_for_a_per_channel_input_scale():
    p = problem((2, 16, 9, 9, 24, 3, 3, (1, 1), (1, 1), (1, 1)), torch.int8, torch.int8, "bf16", True)
    xs = (torch.rand(1, 16, 1, 1, generator=torch.Generator().manual_seed(5)) * 0.01 + 0.01).to(torch.bfloat16).to(DEV)
    check_op(p, False, xs=xs)


def test_op_runs_the_sequence_beyond_the_tap_masks():
    # 12 x 11 = 132 taps: beyond conv2d_geometry_ok's 127 - cheap to build with one channel
    check_op(problem((1, 1, 14, 13, 8, 12, 11, (1, 1), (5, 5), (1, 1)), torch.int8, torch.int8, "bf16", False), False)


# ---- module level ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("qt", [Q.qint8, Q.qfloat8_e4m3fn], ids=lambda q: q.name)
def test_qconv2d_chain_with_and_without_fusion(monkeypatch, qt, dtype):
    import optimum_quanto_amd.nn.module as module_mod

    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.Conv2d(16, 24, 3, stride=2, padding=1, bias=False)).to(dtype).to(DEV)
    Q.quantize(model, weights=qt, activations=qt)
    Q.freeze(model)
    x = torch.randn(3, 8, 11, 13, dtype=dtype, device=DEV)
    qmax = QMAX[qt.dtype]
    quantized = []
    real_quantize = module_mod.quantize_activation
    monkeypatch.setattr(module_mod, "quantize_activation", lambda t, qtype, scale: (quantized.append(tuple(t.shape)), real_quantize(t, qtype=qtype, scale=scale))[1])
    with torch.no_grad():
        h = torch.nn.functional.conv2d(x, model[0].weight.dequantize(), model[0].bias, 1, 1)
        model[0].output_scale = (torch.quantile(h.abs().float().reshape(-1), 0.9) / qmax).to(dtype)
        model[1].input_scale = model[0].output_scale.clone()
        o = torch.nn.functional.conv2d(model[0](x).dequantize(), model[1].weight.dequantize(), None, 2, 1)  # from the codes the second layer gets
        model[1].output_scale = (torch.quantile(o.abs().float().reshape(-1), 0.9) / qmax).to(dtype)
        del quantized[:]
        ref = model(x)
        assert quanto_hip.lib.last_kernel() == _kernel_name(qt.dtype, qt.dtype)
        assert quantized == [(3, 16, 11, 13), (3, 24, 6, 7)]  # the float output of either layer
        assert Q.fuse_output_quantization(model) == ["0", "1"]
        del quantized[:]
        out = model(x)
        assert quanto_hip.lib.last_kernel() == _kernel_name(qt.dtype, qt.dtype) + "_q"
        assert quantized == [(3, 16, 11, 13)]  # the first layer's input is a float tensor; no second pass for the second layer
    assert isinstance(out, Q.ActivationQBytesTensor) and type(out) is type(ref) and out.shape == ref.shape == (3, 24, 6, 7)
    assert 0.02 <= extreme_share(ref._data) <= 0.25
    assert torch.equal(out._data.view(torch.uint8), ref._data.view(torch.uint8))
    assert torch.equal(out._scale, ref._scale)

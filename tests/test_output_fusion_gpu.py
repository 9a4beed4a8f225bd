"""Fused output quantization on the device: ``quanto::qbytes_mm_q`` (csrc/qmm_native8.hip, the epilogue that stores codes) against the two existing ops.

Criterion everywhere: the fused codes equal ``quantize_symmetric(qbytes_mm_bias(...))`` computed by the existing ops on the same tensors under the same
knobs, bit for bit, every element; and the route is the fused kernel wherever it is served.

Inputs (``problem``): seeded codes over the full range of the 8-bit type with a shared rank-one component - row r of an operand is 0.75 amp_r c + 0.25 noise, c_k = +-1,
the noise uniform in (-1, 1); amp is +-(0.8 .. 1) on the operand with fewer rows and +-u^2 (u uniform) on the other - so that the outputs are spread like a peaked
distribution with a long shoulder instead of a narrow Gaussian: with the output scale at 0.7 x absmax / qmax the sequence itself then clamps a few percent of the
elements (asserted: between 1 % and 25 %; iid codes would clamp 0.2 % of a 300 x 264 output), and the clamp, the rounding (int8: exact .5 ties, the quotient has
8 significant bits) and the float8 conversion are all exercised.  Per-feature scales in (0.8, 1.2) x 8192 / max|accumulator|: the float output fits fp16 as well.
"""
import ctypes

import pytest
import torch

from optimum_quanto_amd import QLinear, freeze, fuse_output_quantization, qfloat8_e4m3fn, qint8, quantize
from optimum_quanto_amd.library.hip import quanto_hip

from helpers import CODE_DTYPES as KINDS
from helpers import CODE_QMAX as QMAX
from helpers import assert_nothing_outside, sentinel_buffer

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED = "mfma_native8_q"
MIDS = {"bf16": torch.bfloat16, "fp16": torch.float16}
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.int8: 3, torch.float8_e4m3fn: 5, torch.float8_e5m2: 6}


# one row of 8 or 16 outputs: the clamped share moves in steps of 1 / 8, 1 / 16 - streams in which only the one or two largest outputs exceed 0.7 x the largest
TINY_SALT = {(1, 8): 100017, (1, 16): 100042}


def _operand(rows, K, direction, dtype, gen, amplitude, flat):
    u = torch.rand((rows, 1), generator=gen)
    amp = torch.where(torch.rand((rows, 1), generator=gen) < 0.5, -1.0, 1.0) * (0.8 + 0.2 * u if flat else u * u)
    v = 0.75 * amp * direction + 0.25 * (torch.rand((rows, K), generator=gen) * 2 - 1)  # in (-1, 1)
    if dtype == torch.int8:
        return torch.clamp(torch.round(v * 128), -128, 127).to(torch.int8)
    return (v * amplitude).to(dtype)  # float8: round to nearest, magnitudes from the subnormals up to the largest finite value


def problem(M, N, K, kind, mid, with_bias, seed=0):
    dtype, mdt = KINDS[kind], MIDS[mid]
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * N + K + TINY_SALT.get((M, N), 0))
    direction = torch.where(torch.rand((1, K), generator=gen) < 0.5, -1.0, 1.0)
    # e5m2 x e5m2 into fp16: full-range activations against full-range weights need a per-feature scale below fp16's smallest subnormal; the weights stay below 2
    w_amplitude = 2.0 if (kind, mid) == ("e5m2", "fp16") else QMAX[dtype]
    a, b = _operand(M, K, direction, dtype, gen, QMAX[dtype], M < N), _operand(N, K, direction, dtype, gen, w_amplitude, M >= N)
    acc_max = (a.to(torch.float64) @ b.to(torch.float64).t()).abs().max().clamp_min(1.0)
    scales = ((0.8 + 0.4 * torch.rand((N, 1), generator=gen)).to(torch.float64) * 8192.0 / acc_max).to(mdt)
    bias = ((torch.rand(N, generator=gen) * 2 - 1) * 256).to(mdt) if with_bias else None
    return a.to(DEV), b.to(DEV), scales.to(DEV), None if bias is None else bias.to(DEV)


def sequence(a, b, scales, bias):
    """(float output of the existing product op, out_scale = 0.7 x absmax / qmax in the float dtype, codes of the existing quantizer, share of clamped elements)."""
    y = torch.ops.quanto.qbytes_mm_bias(a, b, scales, bias)
    qmax = QMAX[a.dtype]
    out_scale = (y.abs().max().to(torch.float32) / qmax * 0.7).to(y.dtype)
    want = torch.ops.quanto.quantize_symmetric(y, a.dtype, None, out_scale)
    share = ((y / out_scale).abs().to(torch.float32) > qmax).to(torch.float32).mean().item()
    return y, out_scale, want, share


def check_fused(a, b, scales, bias, expect_route=True):
    y, out_scale, want, share = sequence(a, b, scales, bias)
    unfused_route = quanto_hip.lib.last_kernel()
    got = torch.ops.quanto.qbytes_mm_q(a, b, scales, bias, out_scale)
    route = quanto_hip.lib.last_kernel()
    print(f"shape {tuple(a.shape)} x {tuple(b.shape)} {a.dtype} {scales.dtype} bias {bias is not None}: clamped share {share:.4f}, route {route}")
    assert 0.01 <= share <= 0.25, f"the sequence clamps {share:.4f} of the elements at this output scale"
    assert got.dtype == a.dtype and got.shape == want.shape
    g, w = got.view(torch.uint8), want.view(torch.uint8)
    assert torch.equal(g, w), f"{int((g != w).sum())} of {g.numel()} codes differ from the two-op sequence"
    if expect_route:
        assert route == FUSED
    else:
        assert route != FUSED and unfused_route != FUSED
    return got


# ---- shapes: every M, N, K with both tile sizes; the format / dtype / bias combination cycles through the twelve ------------------------------------
MS, NS = (1, 17, 128, 129, 300), (8, 16, 100, 136, 256, 264)
KS = (64, 192, 128, 512)  # 64-byte rows: K = 64 (mod 128); 128-byte rows: K a multiple of 128
COMBOS = [(k, m, bi) for k in KINDS for m in MIDS for bi in (False, True)]


def _shape_cases():
    cases = []
    for small in (0, 1):
        for i, (M, N) in enumerate((M, N) for M in MS for N in NS):
            K = KS[(i + i // 6 + small) % 4]
            kind, mid, with_bias = COMBOS[(i + 5 * small) % 12]
            cases.append(pytest.param(small, M, N, K, kind, mid, with_bias, id=f"small{small}-{M}x{N}x{K}-{kind}-{mid}-{'bias' if with_bias else 'nobias'}"))
    return cases


def test_shape_cases_cover_every_size_with_both_tiles():
    for small in (0, 1):
        mine = [c.values for c in _shape_cases() if c.values[0] == small]
        assert {c[1] for c in mine} == set(MS) and {c[2] for c in mine} == set(NS) and {c[3] for c in mine} == set(KS)
    assert {c.values[4:] for c in _shape_cases()} == set(COMBOS)


@pytest.mark.parametrize("small,M,N,K,kind,mid,with_bias", _shape_cases())
def test_fused_codes_equal_the_sequence(monkeypatch, small, M, N, K, kind, mid, with_bias):
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_SMALL", str(small))
    check_fused(*problem(M, N, K, kind, mid, with_bias))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("mid", list(MIDS))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("K", [192, 512])
def test_every_format_and_dtype(kind, mid, with_bias, K):
    """The twelve combinations on both kernels under the planner's own tile choice (e5m2 with fp16 included: the existing op serves it)."""
    check_fused(*problem(129, 136, K, kind, mid, with_bias, seed=1))


# ---- split-K: the slice path runs the same epilogue on 8 / S token fragments ------------------------------------------------------------------------
def _q_plan(M, N, K, a, mid):
    k, ws = ctypes.c_int(0), ctypes.c_int64(0)
    st = quanto_hip.lib._c.quanto_hip_qbytes_mm_q_plan(M, N, K, DT[a], DT[a], DT[mid], 0, ctypes.byref(k), ctypes.byref(ws))
    assert st == 0
    return k.value, ws.value


@pytest.mark.parametrize("kind,mid,with_bias", [("int8", "bf16", True), ("e4m3", "fp16", False), ("e5m2", "bf16", True)])
@pytest.mark.parametrize("M,N", [(128, 128), (129, 136)])
@pytest.mark.parametrize("split", [2, 4, 8])
@pytest.mark.parametrize("small", [0, 1])
def test_split_k_slices(monkeypatch, small, split, M, N, kind, mid, with_bias):
    K = 2048
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_SMALL", str(small))
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_SPLIT", str(split))
    tile = 128 if small else 256
    tiles = -(-M // tile) * -(-N // tile)
    kernel, ws = _q_plan(M, N, K, KINDS[kind], MIDS[mid])
    assert kernel == 6 and ws == 4096 + tiles * split * tile * tile * 4, "the plan did not split as forced"
    check_fused(*problem(M, N, K, kind, mid, with_bias, seed=2))


def test_split_k_abandoned_slices(monkeypatch):
    """Poll limit 0: nobody waits, the last arriver of a tile stores the codes of every slice it finds abandoned."""
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_SMALL", "1")
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_SPLIT", "4")
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_POLL_TICKS", "0")
    assert _q_plan(129, 136, 2048, torch.int8, torch.bfloat16)[1] > 0
    args = problem(129, 136, 2048, "int8", "bf16", True, seed=3)
    first = check_fused(*args)
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_POLL_TICKS", "20000")
    assert torch.equal(first, check_fused(*args))  # the state words were left zero


# ---- bounds: nothing outside [M, N] is written ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("M,N,K,kind", [(17, 100, 64, "int8"), (129, 136, 128, "e4m3"), (301, 264, 192, "int8"), (1, 8, 512, "e5m2")])
def test_no_byte_outside_the_output(monkeypatch, small, offset, M, N, K, kind):
    assert (M * N) % 16 != 0
    monkeypatch.setenv("QUANTO_HIP_NATIVE8_SMALL", str(small))
    a, b, scales, bias = problem(M, N, K, kind, "bf16", True, seed=4)
    _, out_scale, want, _ = sequence(a, b, scales, bias)
    buf, lead = sentinel_buffer(M * N, offset, DEV)
    yq = buf[lead:lead + M * N]
    s = scales.reshape(-1).contiguous()
    st = quanto_hip.lib._c.quanto_hip_qbytes_mm_q_ws(a.data_ptr(), b.data_ptr(), s.data_ptr(), bias.data_ptr(), out_scale.data_ptr(), yq.data_ptr(), M, N, K,
                                                     DT[a.dtype], DT[a.dtype], DT[s.dtype], 0, 0, 0, torch.cuda.current_stream().cuda_stream)
    assert st == 0 and quanto_hip.lib.last_kernel() == FUSED
    torch.cuda.synchronize()
    assert torch.equal(yq, want.view(torch.uint8).reshape(-1))
    assert_nothing_outside(buf, lead, M * N, "[M, N]")


# ---- what the library does not serve still returns the sequence's codes ----------------------------------------------------------------------------
def test_fallback_k_not_a_multiple_of_64():
    check_fused(*problem(129, 136, 96, "int8", "bf16", True, seed=5), expect_route=False)


def test_fallback_fp32_scales():
    a, b, scales, bias = problem(129, 136, 128, "int8", "bf16", True, seed=6)
    check_fused(a, b, scales.to(torch.float32), bias.to(torch.float32), expect_route=False)


def test_fallback_misaligned_view():
    a, b, scales, bias = problem(129, 136, 128, "e4m3", "bf16", False, seed=7)
    shifted = torch.empty(a.numel() + 16, dtype=torch.uint8, device=DEV)[1:1 + a.numel()]
    shifted.copy_(a.view(torch.uint8).reshape(-1))
    a1 = shifted.view(a.dtype).reshape(a.shape)
    assert a1.data_ptr() % 16 == 1 and a1.is_contiguous()
    check_fused(a1, b, scales, bias, expect_route=False)


# ---- module level ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", [qint8, qfloat8_e4m3fn], ids=lambda q: q.name)
def test_qlinear_chain_with_and_without_fusion(qt):
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Linear(128, 192), torch.nn.Linear(192, 136, bias=False)).to(torch.bfloat16).to(DEV)
    quantize(model, weights=qt, activations=qt)
    freeze(model)
    x = torch.randn(3, 43, 128, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        model[0].input_scale = (x.abs().max() / QMAX[qt.dtype]).to(torch.bfloat16)
        h = torch.nn.functional.linear(x, model[0].weight.dequantize(), model[0].bias)
        model[0].output_scale = (h.abs().max() / QMAX[qt.dtype] * 0.7).to(torch.bfloat16)
        model[1].input_scale = model[0].output_scale.clone()
        o = torch.nn.functional.linear(h, model[1].weight.dequantize())
        model[1].output_scale = (o.abs().max() / QMAX[qt.dtype] * 0.7).to(torch.bfloat16)
        ref = model(x)
        assert quanto_hip.lib.last_kernel() != FUSED
        assert fuse_output_quantization(model) == ["0", "1"]
        mid = model[0](x)
        assert quanto_hip.lib.last_kernel() == FUSED
        assert mid.shape == (3, 43, 192) and mid._data.dtype == qt.dtype
        fused = model(x)
        assert quanto_hip.lib.last_kernel() == FUSED
    assert isinstance(model[0], QLinear) and type(fused) is type(ref) and fused.shape == ref.shape == (3, 43, 136)
    assert torch.equal(fused._data.view(torch.uint8), ref._data.view(torch.uint8))
    assert torch.equal(fused._scale, ref._scale)

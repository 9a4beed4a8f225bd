"""Fused output quantization of W4A8 / W2A8 layers on the device: ``quanto::qbits_mm_a8_q`` (csrc/qbits_a8_fused.hip with QOUT, gf::epilogue_codes in
csrc/qh_group_fused.h) against the two existing ops.

Criterion everywhere: the fused codes equal ``quantize_symmetric(lib.qbits_mm_a8(...), dtype, None, out_scale)`` computed by the existing kernels on the same
tensors under the same knobs, bit for bit, every element.  The bindings ``lib.qbits_mm_a8`` / ``lib.qbits_mm_a8_q`` are called directly, which puts both
sides on the a8 kernel at any M; the op's routing and the modules have their own tests at the end.

Inputs: a weight of ``helpers.make_qbits_problem``, activation codes drawn uniformly over the full range of the 8-bit type (float8: every finite bit
pattern), a per-tensor activation scale that keeps the output within a few units (fp16 included).  ``out_scale`` is the 0.9-quantile of the unfused |y|
divided by qmax, rounded to the output dtype: the sequence itself then clamps about a tenth of the elements (asserted: between 2 % and 25 %; a one-row
output of 8 / 16 features moves in steps of 1 / 8, 1 / 16), so the clamp, the rounding and the float8 conversion are all exercised.
"""
import numpy as np
import pytest
import torch

from optimum_quanto_amd import QLinear, freeze, fuse_output_quantization, qfloat8_e5m2, qint2, qint4, qint8, quantize
from optimum_quanto_amd.library.hip import quanto_hip

from helpers import CODE_DTYPES as KINDS
from helpers import CODE_QMAX as QMAX
from helpers import assert_nothing_outside, clamped_share, full_range_codes, make_qbits_problem, quantile_out_scale, sentinel_buffer, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
A_SCALE = {"int8": 0.02, "e4m3": 0.01, "e5m2": 1e-4}  # |codes| reach 128 / 448 / 57344: outputs of a few units whatever the kind
ROUTE = {"int8": "a8_fused_int8", "e4m3": "a8_fused_fp8", "e5m2": "a8_fused_bf8"}
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
INT8_EXTREMES = set()  # the smallest and largest int8 code every int8 case of this file produced


def route(kind, bits, fused):
    return ROUTE[kind] + ("_w2" if bits == 2 else "") + ("_q" if fused else "")


def problem(M, N, K, kind, dt, bits, with_bias, zp, seed=0, group_size=128):
    p = make_qbits_problem(1, N, K, dt, bits=bits, group_size=group_size, zeropoint=zp, seed=seed + M + N + K)
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * N + K)
    a = full_range_codes(KINDS[kind], (M, K), gen)
    shift = torch.from_numpy(p["shift"]) if p["shift"].dtype == np.uint8 else to_torch(p["shift"], dt)
    bias = (torch.randn(N, generator=gen) * 0.5).to(TDT[dt]) if with_bias else None
    return dict(a=a.to(DEV), a_scale=torch.tensor([A_SCALE[kind]], dtype=TDT[dt], device=DEV), packed=torch.from_numpy(p["packed"]).to(DEV),
                scale=to_torch(p["scale"], dt, DEV), shift=shift.to(DEV), bias=None if bias is None else bias.to(DEV), bits=bits, group_size=group_size,
                N=N, K=K, kind=kind)


def weight_args(p):
    return p["packed"], p["scale"], p["shift"], p["bias"]


def sequence(p):
    """(codes of the existing quantizer on the existing kernel's output, out_scale) - with the route and the clamped share asserted."""
    lib = quanto_hip.lib
    y = lib.qbits_mm_a8(p["a"], p["a_scale"], *weight_args(p), p["bits"], p["group_size"], p["N"], p["K"])
    assert lib.last_kernel() == route(p["kind"], p["bits"], False)
    assert bool(torch.isfinite(y).all())
    out_scale = quantile_out_scale(y, p["a"].dtype)
    share = clamped_share(y, out_scale, p["a"].dtype)
    want = torch.ops.quanto.quantize_symmetric(y, p["a"].dtype, None, out_scale)
    print(f"{tuple(y.shape)} {p['kind']} {y.dtype} int{p['bits']}: out_scale {out_scale.item():.6g}, clamped share {share:.4f}")
    assert 0.02 <= share <= 0.25, f"the sequence clamps {share:.4f} of the elements at this output scale"
    return want, out_scale


def fused(p, out_scale, out=None):
    lib = quanto_hip.lib
    got = lib.qbits_mm_a8_q(p["a"], p["a_scale"], *weight_args(p), out_scale, p["bits"], p["group_size"], p["N"], p["K"], _out=out)
    assert lib.last_kernel() == route(p["kind"], p["bits"], True)
    return got


def check_fused(p):
    want, out_scale = sequence(p)
    got = fused(p, out_scale)
    assert got.dtype == p["a"].dtype and got.shape == want.shape
    g, w = got.view(torch.uint8), want.view(torch.uint8)
    assert torch.equal(g, w), f"{int((g != w).sum())} of {g.numel()} codes differ from the two-op sequence"
    if p["kind"] == "int8":
        INT8_EXTREMES.update((int(got.min()), int(got.max())))
    return got, out_scale


# ---- shapes: every M, N, K with both token tiles; the activation kind / dtype / bias / shift combination cycles through the twenty-four ---------------
MS = (1, 17, 65, 128, 129, 200)
NS = {4: (8, 16, 104, 136, 256, 264), 2: (16, 48, 144, 256, 272)}
KS = (128, 256, 384)  # 1, 2, 3 groups: both parities of the loop driver's last accumulator set
COMBOS = [(k, d, bi, zp) for k in KINDS for d in TDT for bi in (False, True) for zp in (False, True)]


def _shape_cases():
    cases = []
    for t, bm in enumerate((64, 128)):
        i = 0
        for bits in (4, 2):
            for M in MS:
                for N in NS[bits]:
                    K = KS[(i + i // 3 + t) % 3]
                    kind, dt, with_bias, zp = COMBOS[(i + 7 * t) % 24]
                    cases.append(pytest.param(bm, M, N, K, bits, kind, dt, with_bias, zp,
                                              id=f"bm{bm}-{M}x{N}x{K}-int{bits}-{kind}-{dt}-{'bias' if with_bias else 'nobias'}-{'zp' if zp else 'shift'}"))
                    i += 1
    return cases


def test_shape_cases_cover_every_size_with_both_tiles():
    for bm in (64, 128):
        mine = [c.values for c in _shape_cases() if c.values[0] == bm]
        for bits in (4, 2):
            sub = [c for c in mine if c[4] == bits]
            assert {c[1] for c in sub} == set(MS) and {c[2] for c in sub} == set(NS[bits]) and {c[3] for c in sub} == set(KS)
            assert {(c[1], c[2]) for c in sub} == {(M, N) for M in MS for N in NS[bits]}
        assert {c[5:] for c in mine} == set(COMBOS)


@pytest.mark.parametrize("bm,M,N,K,bits,kind,dt,with_bias,zp", _shape_cases())
def test_fused_codes_equal_the_sequence(monkeypatch, bm, M, N, K, bits, kind, dt, with_bias, zp):
    monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", "1")
    monkeypatch.setenv("QUANTO_HIP_A8_BM", str(bm))
    check_fused(problem(M, N, K, kind, dt, bits, with_bias, zp))


# ---- split-K: the tile's last arriver runs the code epilogue on the summed accumulators -------------------------------------------------------------
@pytest.mark.parametrize("kind,dt,with_bias,zp,bits", [("int8", "bf16", True, False, 4), ("e4m3", "fp16", False, False, 4), ("e5m2", "bf16", False, True, 4),
                                                      ("e4m3", "fp16", False, False, 2)])
@pytest.mark.parametrize("M,N", [(128, 128), (129, 136)])
@pytest.mark.parametrize("split", [2, 4, 8])
@pytest.mark.parametrize("bm", [64, 128])
def test_split_k(monkeypatch, bm, split, M, N, kind, dt, with_bias, zp, bits):
    K = 1024  # 4, 2, 1 tiles per slice
    if bits == 2 and N % 16:
        N += 8  # int2 is served for N % 16 == 0: the ragged shape is (129, 144) there
    monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", str(split))
    monkeypatch.setenv("QUANTO_HIP_A8_BM", str(bm))
    ws = quanto_hip.lib.qbits_mm_a8_workspace(M, N, K, bits, 128, KINDS[kind], TDT[dt])
    assert ws == 4096 + -(-N // 128) * -(-M // bm) * split * 512 * bm, "the plan did not split as forced"
    p = problem(M, N, K, kind, dt, bits, with_bias, zp, seed=2)
    got, out_scale = check_fused(p)
    again = fused(p, out_scale)  # the arrival counters came back zeroed
    assert torch.equal(again.view(torch.uint8), got.view(torch.uint8))


# ---- bounds: nothing outside [M, N] is written ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("bm", [64, 128])
@pytest.mark.parametrize("M,N,K,bits,kind", [(17, 104, 128, 4, "int8"), (129, 136, 256, 4, "e4m3"), (200, 272, 384, 2, "e5m2"), (1, 16, 128, 2, "int8")])
def test_no_byte_outside_the_output(monkeypatch, bm, offset, M, N, K, bits, kind):
    monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", "1")
    monkeypatch.setenv("QUANTO_HIP_A8_BM", str(bm))
    p = problem(M, N, K, kind, "bf16", bits, True, False, seed=4)
    want, out_scale = sequence(p)
    buf, lead = sentinel_buffer(M * N, offset, DEV)
    yq = buf[lead:lead + M * N].view(p["a"].dtype).reshape(M, N)
    fused(p, out_scale, out=yq)
    torch.cuda.synchronize()
    assert torch.equal(buf[lead:lead + M * N], want.view(torch.uint8).reshape(-1))
    assert_nothing_outside(buf, lead, M * N, "[M, N]")


def test_int8_codes_reach_both_ends(monkeypatch):
    """Over the int8 cases of this file both -128 and 127 occur among the codes (run alone, this test runs one int8 case itself)."""
    if not INT8_EXTREMES:
        monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", "1")
        check_fused(problem(129, 136, 256, "int8", "bf16", 4, True, False))
    assert {-128, 127} <= INT8_EXTREMES


# ---- the op: the fused kernel exactly when quanto::qbits_mm_a8 would run the a8 kernel, the sequence on the existing ops otherwise -------------------
def check_op(p, expect_fused, a=None):
    a = p["a"] if a is None else a
    lib = quanto_hip.lib
    args = (p["a_scale"], *weight_args(p))
    y = torch.ops.quanto.qbits_mm_a8(p["a"], *args, p["bits"], p["group_size"], p["N"], p["K"])
    unfused_route = lib.last_kernel()
    out_scale = quantile_out_scale(y, a.dtype)
    assert 0.02 <= clamped_share(y, out_scale, a.dtype) <= 0.25
    want = torch.ops.quanto.quantize_symmetric(y, a.dtype, None, out_scale)
    got = torch.ops.quanto.qbits_mm_a8_q(a, *args, out_scale, p["bits"], p["group_size"], p["N"], p["K"])
    fused_route = lib.last_kernel()
    assert got.dtype == a.dtype and torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    if expect_fused:
        assert unfused_route == route(p["kind"], p["bits"], False) and fused_route == route(p["kind"], p["bits"], True)
    else:
        assert not fused_route.endswith("_q")
    return got


def test_op_takes_the_fused_kernel_above_64_rows():
    p = problem(300, 136, 256, "int8", "bf16", 4, True, False, seed=5)
    got = check_op(p, True)
    p3 = dict(p, a=p["a"].reshape(3, 100, 256))  # leading batch dimensions are carried through
    out_scale = quantile_out_scale(quanto_hip.lib.qbits_mm_a8(p["a"], p["a_scale"], *weight_args(p), 4, 128, 136, 256), torch.int8)
    got3 = torch.ops.quanto.qbits_mm_a8_q(p3["a"], p["a_scale"], *weight_args(p), out_scale, 4, 128, 136, 256)
    assert got3.shape == (3, 100, 136) and torch.equal(got3.reshape(300, 136), got)


def test_op_runs_the_sequence_up_to_64_rows():
    check_op(problem(64, 136, 256, "int8", "bf16", 4, True, False, seed=6), False)


def test_op_runs_the_sequence_beyond_the_tile_cap(monkeypatch):
    monkeypatch.setenv("QUANTO_HIP_A8_MAX_TILES", "1")
    check_op(problem(300, 136, 256, "e4m3", "bf16", 4, False, False, seed=7), False)


def test_op_runs_the_sequence_for_group_size_64():
    check_op(problem(300, 136, 256, "int8", "fp16", 4, True, False, seed=8, group_size=64), False)


def test_op_runs_the_sequence_when_n_is_not_a_multiple_of_8():
    check_op(problem(300, 100, 256, "e5m2", "bf16", 4, False, True, seed=9), False)


def test_op_runs_the_sequence_on_a_misaligned_view():
    p = problem(300, 136, 256, "int8", "bf16", 4, True, False, seed=10)
    a = p["a"]
    shifted = torch.empty(a.numel() + 16, dtype=torch.uint8, device=DEV)[1:1 + a.numel()]
    shifted.copy_(a.view(torch.uint8).reshape(-1))
    a1 = shifted.view(a.dtype).reshape(a.shape)
    assert a1.data_ptr() % 16 == 1 and a1.is_contiguous()
    check_op(p, False, a=a1)


# ---- module level ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wq,aq,kind,bits", [(qint4, qint8, "int8", 4), (qint2, qfloat8_e5m2, "e5m2", 2)], ids=["qint4-qint8", "qint2-qfloat8_e5m2"])
def test_qlinear_chain_with_and_without_fusion(wq, aq, kind, bits):
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Linear(256, 256), torch.nn.Linear(256, 128, bias=False)).to(torch.bfloat16).to(DEV)
    quantize(model, weights=wq, activations=aq)
    freeze(model)
    x = torch.randn(96, 256, dtype=torch.bfloat16, device=DEV)
    qmax = QMAX[aq.dtype]
    with torch.no_grad():
        model[0].input_scale = (x.abs().max() / qmax).to(torch.bfloat16)
        h = torch.nn.functional.linear(x, model[0].weight.dequantize(), model[0].bias)
        model[0].output_scale = (h.abs().max() / qmax * 0.7).to(torch.bfloat16)
        model[1].input_scale = model[0].output_scale.clone()
        o = torch.nn.functional.linear(h, model[1].weight.dequantize())
        model[1].output_scale = (o.abs().max() / qmax * 0.7).to(torch.bfloat16)
        ref = model(x)
        assert not quanto_hip.lib.last_kernel().endswith("_q")
        assert fuse_output_quantization(model) == ["0", "1"]
        mid = model[0](x)
        assert quanto_hip.lib.last_kernel() == route(kind, bits, True)
        assert mid.shape == (96, 256) and mid._data.dtype == aq.dtype
        out = model(x)
        assert quanto_hip.lib.last_kernel() == route(kind, bits, True)
    assert isinstance(model[0], QLinear) and type(out) is type(ref) and out.shape == ref.shape == (96, 128)
    assert torch.equal(out._data.view(torch.uint8), ref._data.view(torch.uint8))
    assert torch.equal(out._scale, ref._scale)

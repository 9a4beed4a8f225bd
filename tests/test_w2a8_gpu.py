"""W2A8 and e5m2 activations on the 8-bit matrix kernel (csrc/qbits_a8_fused.hip): int2 weights x int8 / e4m3 / e5m2 activations and int4 weights x
e5m2 activations - the rest of the quantized-activation x weight grid of the reference's tests/tensor/ops/test_linear_dispatch.py:22-42 and
tests/nn/test_qlinear.py:97-113.

Gates as in tests/test_w4a8_gpu.py: int8 activations, unsplit form: BIT-EXACT against oracle.qbits_mm_a8_chain (generic in the weight width); split-K and
fp8 activations: the exact-math gate against the float64 product of the stored values; every weight code against every finite e5m2 code: exact products;
module level: the reference's own tolerance against the dequantize-first product.
"""
import numpy as np
import pytest
import torch

import optimum_quanto_amd as Q
from optimum_quanto_amd.library.hip import quanto_hip
from oracle import quanto_oracle as O

from helpers import assert_close_to_exact, assert_similar, fp8_tensor, make_qbits_problem, observed_activation_scales, to_numpy, to_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _act_int8(M, K, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-128, 128, size=(M, K), dtype=np.int8)
    sx = O.round_to(np.array([0.0173 + 0.001 * (seed % 7)], np.float32), "bf16")
    return a, sx


def _act_fp8(M, K, kind, seed):
    rng = np.random.default_rng(seed)
    return O.fp8_encode((rng.standard_normal((M, K)) * 40).astype(np.float32), kind)


def _run(p, a_t, sx, dt, bits, bias=None):
    shift = torch.from_numpy(p["shift"]).to(DEV) if p["shift"].dtype == np.uint8 else to_torch(p["shift"], dt, DEV)
    y = quanto_hip.lib.qbits_mm_a8(a_t, to_torch(sx, dt, DEV), torch.from_numpy(p["packed"]).to(DEV), to_torch(p["scale"], dt, DEV), shift,
                                   None if bias is None else to_torch(bias, dt, DEV), bits, 128, p["N"], p["K"])
    return to_numpy(y)


@pytest.mark.parametrize("bm", ["64", "128"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("zp", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,N,K", [(65, 128, 256), (200, 272, 1024), (1, 16, 128), (300, 528, 384), (128, 4096, 4096)])
def test_w2a8_int8_bit_exact(monkeypatch, bm, dt, zp, with_bias, M, N, K):
    """int2 weights (four planes per packed byte): both token tiles, ragged M and N, 1 .. 32 groups, float shifts and integer zero-points, with and
    without a bias: every output element identical to the fp32 fma chain over the exact integer group sums."""
    monkeypatch.setenv("QUANTO_HIP_A8_BM", bm)
    monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", "1")
    p = make_qbits_problem(2, N, K, dt, bits=2, zeropoint=zp, seed=M + N + K)
    a, sx = _act_int8(M, K, seed=M + K)
    sx = O.round_to(sx, dt)
    bias = O.round_to(np.random.default_rng(3).standard_normal(N).astype(np.float32), dt) if with_bias else None
    y = _run(p, torch.from_numpy(a).to(DEV), sx, dt, 2, bias)
    assert quanto_hip.lib.last_kernel() == "a8_fused_int8_w2"
    want = O.qbits_mm_a8_chain(a, sx, p["packed"], 2, p["scale"], p["shift"], 128, N, K, dt, bias)
    np.testing.assert_array_equal(y, want)


def test_w2a8_4096_cubed_bit_exact():
    """The bench shape, whole output, int2 x int8: bit-exact (1024 tiles: the plan does not split K)."""
    M = N = K = 4096
    p = make_qbits_problem(2, N, K, "bf16", bits=2, seed=7)
    a, sx = _act_int8(M, K, seed=11)
    y = _run(p, torch.from_numpy(a).to(DEV), sx, "bf16", 2)
    np.testing.assert_array_equal(y, O.qbits_mm_a8_chain(a, sx, p["packed"], 2, p["scale"], p["shift"], 128, N, K, "bf16"))


@pytest.mark.parametrize("act", ["int8", "e5m2"])
@pytest.mark.parametrize("split", ["2", "4"])
@pytest.mark.parametrize("M,N,K", [(96, 256, 2048), (130, 1024, 4096), (512, 4096, 4096)])
def test_w2a8_split_k_exact_math_and_deterministic(monkeypatch, act, split, M, N, K):
    """The K split with int2 weights (partial tiles through the workspace, last arriver adds in split order): exact-math gate, and two runs give the
    same bits."""
    monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", split)
    p = make_qbits_problem(2, N, K, "bf16", bits=2, seed=N + K)
    if act == "int8":
        a, sx = _act_int8(M, K, seed=M)
        ta, av = torch.from_numpy(a).to(DEV), a
    else:
        codes = _act_fp8(M, K, "e5m2", seed=M)
        sx = O.round_to(np.array([0.021], np.float32), "bf16")
        ta, av = fp8_tensor(codes, "e5m2", DEV), O.fp8_decode(codes, "e5m2")
    y = _run(p, ta, sx, "bf16", 2)
    assert_close_to_exact(y, O.qbits_mm_a8_exact(av, sx, p["packed"], 2, p["scale"], p["shift"], 128, N, K), "bf16",
                          f"w2a8 {act} split {split} {M}x{K}x{N}")
    np.testing.assert_array_equal(_run(p, ta, sx, "bf16", 2), y)


def test_w2a8_split_k_three_tiles_per_split(monkeypatch):
    """int2 weights, an odd tile count above 1 behind a split, 64-token tiles forced: 6 groups over 2 workgroups = 3 tiles each (the two-stage loop of
    csrc/qh_group_fused.h runs its pair once and its odd tail); ragged M, N = 144 (the second feature block holds 16 of its 128 features); int8 activations."""
    M, N, K = 130, 144, 768
    monkeypatch.setenv("QUANTO_HIP_A8_SPLIT", "2")
    monkeypatch.setenv("QUANTO_HIP_A8_BM", "64")
    p = make_qbits_problem(2, N, K, "bf16", bits=2, seed=N + K)
    a, sx = _act_int8(M, K, seed=M)
    ta = torch.from_numpy(a).to(DEV)
    assert quanto_hip.lib.qbits_mm_a8_workspace(M, N, K, 2, 128, ta.dtype, torch.bfloat16) == 4096 + 2 * 3 * 2 * 512 * 64  # the knobs took effect
    y = _run(p, ta, sx, "bf16", 2)
    assert quanto_hip.lib.last_kernel() == "a8_fused_int8_w2"
    assert_close_to_exact(y, O.qbits_mm_a8_exact(a, sx, p["packed"], 2, p["scale"], p["shift"], 128, N, K), "bf16", "w2a8 int8 split 2, 3 tiles, bm 64")
    np.testing.assert_array_equal(_run(p, ta, sx, "bf16", 2), y)


@pytest.mark.parametrize("bits,kind", [(2, "e4m3fn"), (2, "e5m2"), (4, "e5m2")])
@pytest.mark.parametrize("bm", ["64", "128"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("zp", [False, True])
@pytest.mark.parametrize("M,N,K", [(65, 128, 256), (200, 272, 1024), (300, 528, 384), (512, 1024, 4096)])
def test_fp8_activations_new_formats(monkeypatch, bits, kind, bm, dt, zp, M, N, K):
    """int2 x e4m3 (a 4-entry code table), int2 x e5m2 and int4 x e5m2 (bf8 B operand) on the K = 128 MX-format matrix instruction: every product of
    an fp8 value and a weight code is exact - float64 gate on the stored values."""
    monkeypatch.setenv("QUANTO_HIP_A8_BM", bm)
    p = make_qbits_problem(2, N, K, dt, bits=bits, zeropoint=zp, seed=M + N)
    codes = _act_fp8(M, K, kind, seed=M + K)
    sx = O.round_to(np.array([0.021], np.float32), dt)
    y = _run(p, fp8_tensor(codes, kind, DEV), sx, dt, bits)
    assert quanto_hip.lib.last_kernel() == {(2, "e4m3fn"): "a8_fused_fp8_w2", (2, "e5m2"): "a8_fused_bf8_w2", (4, "e5m2"): "a8_fused_bf8"}[(bits, kind)]
    want = O.qbits_mm_a8_exact(O.fp8_decode(codes, kind), sx, p["packed"], bits, p["scale"], p["shift"], 128, N, K)
    assert_close_to_exact(y, want, dt, f"w{bits} {kind} {M}x{K}x{N}")


@pytest.mark.parametrize("bits,kind", [(4, "e5m2"), (2, "e5m2"), (2, "e4m3fn")])
def test_every_weight_code_against_every_finite_fp8_code(bits, kind):
    """One group: activation row m holds one finite fp8 code c_m in all 128 positions, feature n holds the weight code n mod 2^bits in all positions, so
    y[m, n] = c_m * 128 * (scale * q_n - shift) - one output element per (activation code, weight code) pair, exact in fp32 (c_m has at most 3 mantissa
    bits, 128 q_n below 2^11), rounded once to bf16.  A wrong entry of the weight code table or a wrong decode of the activation format (bf8 read as
    fp8: off by powers of two) fails the element."""
    N, K = 16, 128
    q = np.repeat((np.arange(N) % (1 << bits)).astype(np.uint8)[:, None], K, axis=1)
    packed = O.pack_weights(O.group(q, 0, 128), bits)
    scale = O.round_to(np.full((N, 1), 2.0**-6, np.float32), "bf16")
    shift = O.round_to(np.full((N, 1), 2.0**-7, np.float32), "bf16")
    exp_mask = 0x7C if kind == "e5m2" else 0x7F
    codes = np.array([c for c in range(256) if (c & exp_mask) != exp_mask], dtype=np.uint8)  # e5m2: 248 finite codes, e4m3fn: 254
    a = np.repeat(codes[:, None], K, axis=1)
    sx = np.array([1.0], np.float32)
    y = quanto_hip.lib.qbits_mm_a8(fp8_tensor(a, kind, DEV), to_torch(sx, "bf16", DEV), torch.from_numpy(packed).to(DEV), to_torch(scale, "bf16", DEV),
                                   to_torch(shift, "bf16", DEV), None, bits, 128, N, K)
    assert quanto_hip.lib.last_kernel().startswith("a8_fused")
    want = O.qbits_mm_a8_exact(O.fp8_decode(a, kind), sx, packed, bits, scale, shift, 128, N, K)
    y = to_numpy(y).astype(np.float64)
    np.testing.assert_array_equal(y, O.round_to(want.astype(np.float32), "bf16").astype(np.float64))


@pytest.mark.parametrize("bits,kind,name", [(4, "int8", "a8_fused_int8"), (4, "e4m3fn", "a8_fused_fp8"), (4, "e5m2", "a8_fused_bf8"),
                                            (2, "int8", "a8_fused_int8_w2"), (2, "e4m3fn", "a8_fused_fp8_w2"), (2, "e5m2", "a8_fused_bf8_w2")])
def test_last_kernel_names(bits, kind, name):
    p = make_qbits_problem(2, 256, 512, "bf16", bits=bits, seed=5)
    if kind == "int8":
        a, sx = _act_int8(100, 512, seed=5)
        ta = torch.from_numpy(a).to(DEV)
    else:
        ta, sx = fp8_tensor(_act_fp8(100, 512, kind, seed=5), kind, DEV), np.array([0.02], np.float32)
    _run(p, ta, sx, "bf16", bits)
    assert quanto_hip.lib.last_kernel() == name


@pytest.mark.parametrize("weights,activations,how", [("qint2", "qint8", "qlinear"), ("qint4", "qfloat8_e5m2", "quantize"),
                                                     ("qint2", "qfloat8_e5m2", "quantize")])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_module_level_new_formats_use_the_fused_kernel(weights, activations, how, dtype):
    """QLinear(weights=qint2, activations=qint8) and quantize(model, weights=qint4 | qint2, activations=qfloat8_e5m2) at 300 tokens: the layer's
    F.linear lands on the fused kernel (WeightQBitsLinearFunction passes the weight width and the per-tensor activation through unchanged) and agrees
    with the dequantize-first product of the same quantized operands within the reference's tolerance."""
    torch.manual_seed(0)
    wq, aq = getattr(Q, weights), getattr(Q, activations)
    lin = torch.nn.Linear(1024, 512).to(dtype).to(DEV)
    if how == "qlinear":
        model = torch.nn.Sequential(Q.QLinear.from_module(lin, weights=wq, activations=aq))
    else:
        model = torch.nn.Sequential(lin)
        Q.quantize(model, weights=wq, activations=aq)
    qlin = model[0]
    x = torch.randn(300, 1024, device=DEV, dtype=dtype)
    with torch.no_grad(), observed_activation_scales():
        model(x)
    Q.freeze(model)
    with torch.no_grad():
        y = model(x)
        assert quanto_hip.lib.last_kernel().startswith("a8_fused")
        xq = Q.quantize_activation(x, qtype=aq, scale=qlin.input_scale)
        want = torch.nn.functional.linear(xq.dequantize().float(), qlin.qweight.dequantize().float(), qlin.bias.float()).to(dtype)
    assert isinstance(y, Q.ActivationQBytesTensor) and y.qtype == aq
    assert_similar(y.dequantize(), want)


@pytest.mark.parametrize("bits,kind,M,N,fused", [(2, "int8", 300, 1024, True), (2, "int8", 8, 1024, False), (2, "e5m2", 8, 1024, False),
                                                 (2, "int8", 512, 14336, True), (2, "int8", 2048, 4096, False),
                                                 (2, "e5m2", 2048, 4096, True), (4, "e5m2", 2048, 4096, True), (2, "e5m2", 4096, 4096, False)])
def test_op_routing_of_the_new_formats(bits, kind, M, N, fused):
    """quanto::qbits_mm_a8 takes the fused kernel from 64 rows on while it is measured faster than the dequantize-first sequence
    (profiles/r07_w2a8_crossover.jsonl): int2 x int8 up to 448 output tiles, int2 x e5m2 and int4 x e5m2 up to 512 like int4 x int8 / e4m3."""
    K = 4096
    packed = torch.randint(0, 256, (N * bits // 8, K), dtype=torch.uint8, device=DEV)
    scale = torch.full((N * K // 128, 1), 0.01, device=DEV, dtype=torch.bfloat16)
    shift = torch.full((N * K // 128, 1), 0.02, device=DEV, dtype=torch.bfloat16)
    if kind == "int8":
        a = torch.randint(-100, 100, (M, K), device=DEV, dtype=torch.int8)
    else:
        a = torch.randn(M, K, device=DEV).to(torch.float8_e5m2)
    sx = torch.tensor([0.02], device=DEV, dtype=torch.bfloat16)
    torch.ops.quanto.qbits_mm_a8(a, sx, packed, scale, shift, None, bits, 128, N, K)
    assert quanto_hip.lib.last_kernel().startswith("a8_fused") == fused, quanto_hip.lib.last_kernel()

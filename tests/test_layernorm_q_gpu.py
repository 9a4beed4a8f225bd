"""``quanto::layer_norm_q`` on the device (csrc/layernorm_q.hip).  Every case asks the condition of layernorm_q_cases.py against the float64 oracle
built there - each code the oracle's or its neighbour, at most max(2, 1e-4 numel) differing - and that the kernel took the call wherever the op's
predicate says so.  The CPU file proves on the same inputs that an fp32 two-pass sequence stays inside the condition."""
import pytest
import torch

from optimum_quanto_amd import ActivationQBytesTensor, QLayerNorm, QLinear, freeze, fuse_output_quantization, qint8, quantize
from optimum_quanto_amd.library import ops as ops_mod
from optimum_quanto_amd.library.hip import quanto_hip

import layernorm_q_cases as C
from helpers import assert_nothing_outside, observed_activation_scales, sentinel_buffer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "layer_norm_q"


def _other_kernel():
    """Leaves another name in ``last_kernel()``: what a later ``== NAME`` / ``!= NAME`` then says is about the call in between."""
    lib = quanto_hip.lib
    lib.qbytes_mm(torch.ones((1, 64), dtype=torch.bfloat16, device=DEV), torch.ones((64, 64), dtype=torch.int8, device=DEV),
                  torch.ones((64,), dtype=torch.bfloat16, device=DEV))
    assert lib.last_kernel() != NAME


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(p, x=None, expect_kernel=True):
    """The op on device tensors (``x``: another view of the problem's input, already on the device)."""
    x = _dev(p.x) if x is None else x
    w, b, scale = _dev(p.weight), _dev(p.bias), _dev(p.scale)
    assert ops_mod._layer_norm_q_kernel_takes(x, list(p.norm), w, b, scale, p.dtype) == expect_kernel
    _other_kernel()
    got = torch.ops.quanto.layer_norm_q(x, list(p.norm), w, b, C.EPS, scale, p.dtype)
    assert (quanto_hip.lib.last_kernel() == NAME) == expect_kernel
    assert got.dtype == p.dtype and got.shape == p.x.shape and got.is_contiguous()
    return got


@pytest.mark.parametrize("case", C.SHAPE_CASES + C.PAIR_CASES + C.PARAM_CASES + C.ND_CASES + C.STAT_CASES, ids=lambda c: c.id)
def test_codes_meet_the_condition(case):
    p = C.problem(case)
    C.assert_condition(_run(p), p.want, case.id)


def test_constant_rows_give_the_codes_of_the_bias_alone():
    for case in (c for c in C.STAT_CASES if c.kind == "constant"):
        p = C.problem(case)
        bias_codes = ops_mod.quantize_symmetric(p.bias.expand(p.x.shape), p.dtype, None, p.scale)
        assert torch.equal(_run(p).cpu().view(torch.uint8), bias_codes.view(torch.uint8))


@pytest.mark.parametrize("layout", ["offset1", "stride_n_plus_1", "stride_n_plus_8", "offset1_stride_n_plus_3", "transposed_lead"])
@pytest.mark.parametrize("case", C.VIEW_CASES, ids=lambda c: c.id)
def test_views(case, layout):
    """The same problem through other views of its input: a buffer offset by one element (loads per element), rows n + 1 apart (per element), n + 8 apart
    (16-byte loads stay), both, and leading dimensions that do not collapse to one row stride (the binding copies)."""
    p = C.problem(case)
    rows = p.x.numel() // p.norm[-1]
    n = p.norm[-1]
    x2 = p.x.reshape(rows, n)
    if layout == "transposed_lead":
        lead = case.lead if len(case.lead) == 2 else (2, rows // 2)
        # [b, a, n] storage viewed as [a, b, n]: rows contiguous inside, two row strides
        x = _dev(p.x.reshape(lead + (n,)).transpose(0, 1).contiguous()).transpose(0, 1)
        assert not x.is_contiguous() and x.stride(-1) == 1
        got = _run(p._replace(x=p.x.reshape(lead + (n,)), want=p.want.reshape(lead + (n,))), x=x)
        C.assert_condition(got, p.want.reshape(lead + (n,)), f"{case.id} {layout}")
        return
    offset, pitch = {"offset1": (1, n), "stride_n_plus_1": (0, n + 1), "stride_n_plus_8": (0, n + 8), "offset1_stride_n_plus_3": (1, n + 3)}[layout]
    buf = torch.full((offset + rows * pitch + 8,), float("nan"), dtype=p.x.dtype, device=DEV)  # what lies between the rows must not be read into them
    x = buf[offset:offset + rows * pitch].view(rows, pitch)[:, :n]
    x.copy_(x2)
    assert x.data_ptr() == buf.data_ptr() + offset * buf.element_size() and x.stride() == (pitch, 1)
    got = _run(p._replace(x=x2, want=p.want.reshape(rows, n)), x=x)
    C.assert_condition(got, p.want.reshape(rows, n), f"{case.id} {layout}")


@pytest.mark.parametrize("offset", [0, 1, 4, 5])
@pytest.mark.parametrize("case", [C.Case("random", (3,), (197,)), C.Case("random", (3,), (1025,)), C.Case("random", (1,), (7,)), C.Case("random", (5,), (1000,))],
                         ids=lambda c: c.id)
def test_the_entry_stores_inside_its_output_only(case, offset):
    """The C entry on an output that starts ``offset`` bytes into a sentinel buffer (8-, 4- and 1-byte stores; rows whose length is no multiple of 4
    start at odd addresses from the second on): the codes meet the condition and no byte outside [rows, n] changes."""
    p = C.problem(case)
    x, w, b, scale = _dev(p.x), _dev(p.weight), _dev(p.bias), _dev(p.scale)
    rows, n = p.x.shape
    buf, lead = sentinel_buffer(rows * n, offset, DEV)
    yq = buf[lead:lead + rows * n]
    dt = {torch.bfloat16: 2}[p.x.dtype]
    st = quanto_hip.lib._c.quanto_hip_layer_norm_q(x.data_ptr(), w.data_ptr(), b.data_ptr(), scale.data_ptr(), yq.data_ptr(), rows, n, n, C.EPS, dt, 3,
                                                   torch.cuda.current_stream().cuda_stream)
    assert st == 0 and quanto_hip.lib.last_kernel() == NAME
    torch.cuda.synchronize()
    assert_nothing_outside(buf, lead, rows * n, f"{case.id} at output offset {offset}")
    C.assert_condition(yq.view(torch.int8).reshape(rows, n), p.want, f"{case.id} output offset {offset}")


def test_beyond_the_limit_and_fp64_run_the_sequence():
    for case in C.BEYOND_CASES:
        p = C.problem(case)
        got = _run(p, expect_kernel=False)
        x, w, b, scale = _dev(p.x), _dev(p.weight), _dev(p.bias), _dev(p.scale)
        assert torch.equal(got, ops_mod.layer_norm_q_default(x, list(p.norm), w, b, C.EPS, scale, p.dtype))
        C.assert_condition(got, p.want, case.id)
    p = C.problem(C.Case("random", (5,), (197,)))
    x, w, b, scale = (t.to(torch.float64).to(DEV) for t in (p.x, p.weight, p.bias, p.scale))
    _other_kernel()
    got = torch.ops.quanto.layer_norm_q(x, [197], w, b, C.EPS, scale, torch.int8)
    assert quanto_hip.lib.last_kernel() != NAME
    assert torch.equal(got, ops_mod.layer_norm_q_default(x, [197], w, b, C.EPS, scale, torch.int8))
    # rows that are not contiguous inside: the sequence as well
    xs = _dev(p.x)[:, ::2]
    _other_kernel()
    got = torch.ops.quanto.layer_norm_q(xs, [99], None, None, C.EPS, _dev(p.scale), torch.int8)
    assert quanto_hip.lib.last_kernel() != NAME
    assert torch.equal(got, ops_mod.layer_norm_q_default(xs, [99], None, None, C.EPS, _dev(p.scale), torch.int8))


def test_a_block_with_a_fused_qlayernorm_feeds_its_linear_with_codes():
    """LayerNorm(64) -> Linear(64, 128) -> ReLU -> Linear(128, 64) on (2, 5, 64) bf16, W8A8 with ``layernorm=True``: the marked QLayerNorm returns an
    ActivationQBytesTensor from one ``layer_norm_q`` launch, the first Linear multiplies its codes on the 8-bit matrix units, the block stays within
    5 % of the float block's peak, and the marked module's codes meet the condition against the unmarked module's."""
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.LayerNorm(64), torch.nn.Linear(64, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64)).to(torch.bfloat16).to(DEV)
    x = torch.randn(2, 5, 64, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        ref = model(x)
        quantize(model, weights=qint8, activations=qint8, layernorm=True)
        assert [type(m) for m in model] == [QLayerNorm, QLinear, torch.nn.ReLU, QLinear]
        with observed_activation_scales():
            model(x)
        assert float(model[0].output_scale) != 1.0 and float(model[1].input_scale) != 1.0
        freeze(model)
        _other_kernel()
        unmarked = model[0](x)
        assert quanto_hip.lib.last_kernel() != NAME and isinstance(unmarked, ActivationQBytesTensor)
        assert fuse_output_quantization(model) == ["0", "1", "3"]
        _other_kernel()
        marked = model[0](x)
        assert quanto_hip.lib.last_kernel() == NAME
        assert isinstance(marked, ActivationQBytesTensor) and marked.qtype == qint8 and marked.shape == x.shape
        assert marked._data.dtype == torch.int8 and torch.equal(marked._scale, model[0].output_scale)
        C.assert_condition(marked._data, unmarked._data, "marked against unmarked QLayerNorm")
        hidden = model[1](marked)
        assert quanto_hip.lib.last_kernel() == "mfma_native8_q"  # int8 x int8, the epilogue that stores codes (test_output_fusion_gpu.py)
        assert isinstance(hidden, ActivationQBytesTensor)
        out = model(x)
        out = out.dequantize() if isinstance(out, ActivationQBytesTensor) else out
        assert (out.float() - ref.float()).abs().max() < 0.05 * ref.float().abs().max()

"""``quanto::qbytes_bmm`` on the device (csrc/qbytes_bmm.hip): every comparison is ``torch.equal`` against a numpy oracle computed here - the sum as
an int64 matmul, ``.astype(np.float32)`` (one round-to-nearest-even), ``* np.float32(scale)``, rounded once to the output dtype - plus the handler's
attention patterns against the same calls on the CPU."""
import functools

import numpy as np
import pytest
import torch

from optimum_quanto_amd.library.hip import quanto_hip
from optimum_quanto_amd.tensor import absmax_scale, qfloat8, qint8, quantize_activation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SCALE = 0.0123  # (its fp32 value: no power of two, so the multiply rounds)


def _round_to(v: np.ndarray, dtype) -> torch.Tensor:
    """fp32 values rounded once, to nearest even, to ``dtype`` - as a torch tensor on the host."""
    assert v.dtype == np.float32
    if dtype == torch.float32:
        return torch.from_numpy(v.copy())
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return torch.from_numpy(v.astype(np.float16))
    u = v.view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)  # (finite inputs only)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def _oracle(a: np.ndarray, w: np.ndarray, scale, dtype) -> torch.Tensor:
    acc = np.matmul(a.astype(np.int64), w.astype(np.int64))
    return _round_to(acc.astype(np.float32) * np.float32(scale), dtype)


def _run(a, w, dtype, scale=SCALE):
    """The op on device tensors; the kernel must have taken the call."""
    _other_kernel()
    y = torch.ops.quanto.qbytes_bmm(a, w, torch.tensor(scale, dtype=torch.float32, device=DEV), dtype)
    assert quanto_hip.lib.last_kernel() == "bmm_i8"
    return y.cpu()


def _other_kernel():
    """Leaves another name in ``last_kernel()``: what a later ``== "bmm_i8"`` / ``!= "bmm_i8"`` then says is about the call in between."""
    lib = quanto_hip.lib
    lib.qbytes_mm(torch.ones((1, 64), dtype=torch.bfloat16, device=DEV), torch.ones((64, 64), dtype=torch.int8, device=DEV),
                  torch.ones((64,), dtype=torch.bfloat16, device=DEV))
    assert lib.last_kernel() != "bmm_i8"


SHAPES = [(1, 1, 1, 1), (2, 64, 64, 64), (3, 70, 90, 80), (8, 24, 24, 32), (2, 65, 63, 197), (2, 130, 24, 200), (1, 33, 257, 16), (65537, 1, 1, 16)]


@functools.lru_cache(maxsize=None)
def _problem(shape):
    """Full-range random codes (-128 included) of one shape, on the host and on the device in both layouts of w, and the three oracles."""
    B, M, N, K = shape
    rng = np.random.default_rng(B * 1000003 + M * 10007 + N * 101 + K)
    a = rng.integers(-128, 128, size=(B, M, K), dtype=np.int8)
    w = rng.integers(-128, 128, size=(B, K, N), dtype=np.int8)
    a.flat[0], w.flat[0] = -128, -128
    ad, wd = torch.from_numpy(a).to(DEV), torch.from_numpy(w).to(DEV)
    layouts = {"NN": wd, "NT": wd.transpose(1, 2).contiguous().transpose(1, 2)}
    assert layouts["NN"].is_contiguous() and (layouts["NT"].stride(1) == 1 or K == 1)
    return ad, layouts, {dt: _oracle(a, w, SCALE, dt) for dt in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("layout", ["NN", "NT"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_in_both_layouts_of_w(shape, layout, dtype):
    a, layouts, want = _problem(shape)
    got = _run(a, layouts[layout], dtype)
    assert got.dtype == dtype and tuple(got.shape) == (shape[0], shape[1], shape[2])
    assert torch.equal(got, want[dtype])


@pytest.mark.parametrize("layout", ["NN", "NT"])
def test_identity_times_an_asymmetric_w_returns_w(layout):
    """A swapped row / column map of either operand or of the output would return the transpose of a batch member, or another member."""
    B, n = 3, 64
    a = torch.eye(n, dtype=torch.int8).expand(B, n, n).contiguous()
    k, j, b = np.meshgrid(np.arange(n), np.arange(n), np.arange(B), indexing="ij")
    w = np.ascontiguousarray(((3 * k + 7 * j * j + 11 * b) % 251 - 125).astype(np.int8).transpose(2, 0, 1))  # [B, k, j]
    assert not np.array_equal(w[0], w[0].T) and not np.array_equal(w[0], w[1])
    wd = torch.from_numpy(w).to(DEV)
    if layout == "NT":
        wd = wd.transpose(1, 2).contiguous().transpose(1, 2)
    for dtype in (torch.float32, torch.bfloat16):
        got = _run(a.to(DEV), wd, dtype, scale=0.5)
        assert torch.equal(got, _round_to(w.astype(np.float32) * np.float32(0.5), dtype))


@pytest.mark.parametrize("layout", ["NN", "NT"])
@pytest.mark.parametrize("av,wv,K,total", [(127, -128, 4112, -66844672), (-128, -128, 65536, 1 << 30)], ids=["above_2^24", "2^30"])
def test_sums_beyond_the_fp32_integers(av, wv, K, total, layout):
    """|sum| > 2^24: the int32 -> fp32 conversion rounds (to nearest even, once); 2^30: the accumulator's upper range."""
    B, M, N = 2, 5, 3
    a = np.full((B, M, K), av, dtype=np.int8)
    w = np.full((B, K, N), wv, dtype=np.int8)
    assert int(a[0, 0].astype(np.int64) @ w[0, :, 0].astype(np.int64)) == total and abs(total) > 1 << 24
    wd = torch.from_numpy(w).to(DEV)
    if layout == "NT":
        wd = wd.transpose(1, 2).contiguous().transpose(1, 2)
    for dtype in DTYPES:
        assert torch.equal(_run(torch.from_numpy(a).to(DEV), wd, dtype, scale=1e-5), _oracle(a, w, 1e-5, dtype))


def test_a_sum_that_the_conversion_must_round():
    """66 844 672 and 2^30 are fp32 values themselves; 127 * 127 * 1041 = 16 790 289 is not: it lies halfway between two fp32 neighbours, so the
    conversion must round, and to the even one."""
    K = 1041
    a = np.full((1, 1, K), 127, dtype=np.int8)
    w = np.full((1, K, 1), 127, dtype=np.int8)
    total = 127 * 127 * K
    assert total > 1 << 24 and total % 2 == 1 and float(np.float32(total)) == total - 1 and ((total - 1) >> 1) % 2 == 0
    got = _run(torch.from_numpy(a).to(DEV), torch.from_numpy(w).to(DEV), torch.float32, scale=1.0)
    assert got.item() == float(np.float32(total))


def _rand(rng, *shape):
    return rng.integers(-128, 128, size=shape, dtype=np.int8)


def test_a_that_starts_one_byte_into_its_storage():
    rng = np.random.default_rng(5)
    B, M, N, K = 2, 37, 40, 48
    a, w = _rand(rng, B, M, K), _rand(rng, B, K, N)
    buf = torch.full((B * M * K + 1,), 127, dtype=torch.int8, device=DEV)
    buf[1:] = torch.from_numpy(a).to(DEV).reshape(-1)
    ad = buf[1:].view(B, M, K)
    assert ad.data_ptr() % 2 == 1
    for dtype in DTYPES:
        assert torch.equal(_run(ad, torch.from_numpy(w).to(DEV), dtype), _oracle(a, w, SCALE, dtype))


# (offset of the slice inside its row, row length of the wider tensor): 16-byte, 4-byte and byte loads, each with a row tail (K, N = 70)
@pytest.mark.parametrize("off,stride", [(16, 96), (4, 84), (3, 77)], ids=["16B", "4B", "1B"])
@pytest.mark.parametrize("layout", ["NN", "NT"])
def test_inner_slices_of_wider_tensors_read_nothing_around_their_rows(off, stride, layout):
    """Row stride > row length, everything around each row filled with 127: a read past a row's end (or ahead of its start) changes the sums."""
    rng = np.random.default_rng(off)
    B, M, N, K = 2, 66, 70, 70
    a = _rand(rng, B, M, K)
    big_a = torch.full((B, M + 2, stride), 127, dtype=torch.int8, device=DEV)
    big_a[:, 1:M + 1, off:off + K] = torch.from_numpy(a).to(DEV)
    ad = big_a[:, 1:M + 1, off:off + K]
    if layout == "NN":
        w = _rand(rng, B, K, N)
        big_w = torch.full((B, K + 2, stride), 127, dtype=torch.int8, device=DEV)
        big_w[:, 1:K + 1, off:off + N] = torch.from_numpy(w).to(DEV)
        wd = big_w[:, 1:K + 1, off:off + N]
        assert wd.stride() == ((K + 2) * stride, stride, 1)
    else:
        wt = _rand(rng, B, N, K)
        big_w = torch.full((B, N + 2, stride), 127, dtype=torch.int8, device=DEV)
        big_w[:, 1:N + 1, off:off + K] = torch.from_numpy(wt).to(DEV)
        wd = big_w[:, 1:N + 1, off:off + K].transpose(1, 2)
        assert wd.stride() == ((N + 2) * stride, 1, stride)
        w = np.ascontiguousarray(wt.transpose(0, 2, 1))
    assert ad.stride() == ((M + 2) * stride, stride, 1) and not ad.is_contiguous()
    for dtype in (torch.float32, torch.bfloat16):
        assert torch.equal(_run(ad, wd, dtype), _oracle(a, w, SCALE, dtype))


@pytest.mark.parametrize("layout", ["NN", "NT"])
def test_w_expanded_over_the_batch(layout):
    rng = np.random.default_rng(7)
    B, M, N, K = 5, 20, 30, 100
    a, w1 = _rand(rng, B, M, K), _rand(rng, 1, K, N)
    wd = torch.from_numpy(w1).to(DEV)
    if layout == "NT":
        wd = wd.transpose(1, 2).contiguous().transpose(1, 2)
    wd = wd.expand(B, K, N)
    assert wd.stride(0) == 0
    for dtype in (torch.float32, torch.float16):
        assert torch.equal(_run(torch.from_numpy(a).to(DEV), wd, dtype), _oracle(a, np.broadcast_to(w1, (B, K, N)), SCALE, dtype))
    # a expanded as well
    a1 = torch.from_numpy(a[:1]).to(DEV).expand(B, M, K)
    assert torch.equal(_run(a1, wd, torch.float32), _oracle(np.broadcast_to(a[:1], (B, M, K)), np.broadcast_to(w1, (B, K, N)), SCALE, torch.float32))


def test_a_view_with_no_unit_stride_dimension_is_copied():
    rng = np.random.default_rng(8)
    B, M, N, K = 2, 9, 11, 40
    a, w2 = _rand(rng, B, M, 2 * K), _rand(rng, B, K, 2 * N)
    ad, wd = torch.from_numpy(a).to(DEV)[..., ::2], torch.from_numpy(w2).to(DEV)[..., ::2]
    assert wd.stride() == (2 * K * N, 2 * N, 2) and ad.stride(2) == 2
    assert torch.equal(_run(ad, wd, torch.bfloat16), _oracle(a[..., ::2], w2[..., ::2], SCALE, torch.bfloat16))


def test_an_empty_sum_stores_zeros_and_an_empty_output_launches_nothing():
    z = lambda *shape: torch.zeros(shape, dtype=torch.int8, device=DEV)  # noqa: E731
    got = _run(z(2, 3, 0), z(2, 0, 5), torch.float16)
    assert tuple(got.shape) == (2, 3, 5) and torch.equal(got, torch.zeros((2, 3, 5), dtype=torch.float16))
    one = torch.ones((), dtype=torch.float32, device=DEV)
    for a, w in ((z(0, 3, 4), z(0, 4, 5)), (z(2, 0, 4), z(2, 4, 5)), (z(2, 3, 4), z(2, 4, 0))):
        y = torch.ops.quanto.qbytes_bmm(a, w, one, torch.float32)
        assert tuple(y.shape) == (a.shape[0], a.shape[1], w.shape[2]) and y.numel() == 0


# ---- the handler: torch.matmul / torch.bmm on ActivationQBytesTensors -----------------------------------------------------------------------------
def _quantized(gen, shape, dtype, qtype=qint8):
    t = torch.randn(shape, generator=gen).to(dtype)
    return quantize_activation(t, qtype=qtype, scale=absmax_scale(t, qtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_attention_patterns_through_the_handler_equal_the_cpu(dtype):
    """q k^T and p v of an eager attention block (q / k / v by view + transpose, p quantized codes) and the 3-D transposed-view product: all K <= 1024,
    where the kernel is bit-identical to the fp32 sequence the CPU runs."""
    gen = torch.Generator().manual_seed(11)
    bsz, s, h, d = 2, 24, 4, 32  # bmm shapes (8, 24, 24, 32) and (8, 24, 32, 24)
    lib = quanto_hip.lib

    def attention(q, k, v, p):
        q, k, v = (t.view(bsz, s, h, d).transpose(1, 2) for t in (q, k, v))
        _other_kernel() if q.is_cuda else None
        scores = torch.matmul(q, k.transpose(2, 3))
        if q.is_cuda:
            assert lib.last_kernel() == "bmm_i8"
            _other_kernel()
        out = torch.matmul(p, v)
        if q.is_cuda:
            assert lib.last_kernel() == "bmm_i8"
        return scores, out

    q, k, v = (_quantized(gen, (bsz, s, h * d), dtype) for _ in range(3))
    p = _quantized(gen, (bsz, h, s, s), dtype)
    host = attention(q, k, v, p)
    device = attention(*(t.to(DEV) for t in (q, k, v, p)))
    for got, want in zip(device, host):
        assert type(got) is torch.Tensor and got.dtype == dtype and got.is_cuda
        assert torch.equal(got.cpu(), want)

    a, b = _quantized(gen, (3, 70, 197), dtype), _quantized(gen, (3, 90, 197), dtype)
    want = torch.matmul(a, b.transpose(1, 2))
    _other_kernel()
    got = torch.matmul(a.to(DEV), b.to(DEV).transpose(1, 2))
    assert lib.last_kernel() == "bmm_i8"
    assert torch.equal(got.cpu(), want)


def test_fp8_pairs_and_float_operands_keep_their_routes():
    gen = torch.Generator().manual_seed(12)
    lib = quanto_hip.lib
    a8, b8 = (_quantized(gen, shape, torch.bfloat16, qfloat8).to(DEV) for shape in ((2, 5, 16), (2, 16, 7)))
    a, b = (_quantized(gen, shape, torch.bfloat16).to(DEV) for shape in ((2, 5, 16), (2, 16, 7)))
    x = torch.randn((2, 5, 16), generator=gen).to(torch.bfloat16).to(DEV)
    _other_kernel()
    assert torch.equal(torch.bmm(a8, b8), torch.bmm(a8.dequantize(), b8.dequantize()))  # qfallback
    assert torch.equal(torch.bmm(a, b8), torch.bmm(a.dequantize(), b8.dequantize()))
    assert torch.equal(torch.bmm(x, b), torch.bmm(x, b.dequantize()))  # float x quantized
    assert torch.equal(torch.bmm(a, b.dequantize()), torch.bmm(a.dequantize(), b.dequantize()))  # quantized x float
    assert lib.last_kernel() != "bmm_i8"
    torch.bmm(a, b)
    assert lib.last_kernel() == "bmm_i8"


def test_graph_capture_and_replay():
    """One graph, one stream, no parallel branches; two replays equal the eager result, two eager runs are bit-identical."""
    a, layouts, want = _problem((3, 70, 90, 80))
    w = layouts["NN"]
    scale = torch.tensor(SCALE, dtype=torch.float32, device=DEV)
    eager = torch.ops.quanto.qbytes_bmm(a, w, scale, torch.bfloat16)
    assert torch.equal(eager, torch.ops.quanto.qbytes_bmm(a, w, scale, torch.bfloat16))
    assert torch.equal(eager.cpu(), want[torch.bfloat16])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        torch.ops.quanto.qbytes_bmm(a, w, scale, torch.bfloat16)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        y = torch.ops.quanto.qbytes_bmm(a, w, scale, torch.bfloat16)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)

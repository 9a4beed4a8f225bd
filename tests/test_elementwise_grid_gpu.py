"""The elementwise kernels (csrc/quantize.hip, csrc/unpack.hip) past their grid caps: the second grid-stride iteration and the ragged end.

Every launcher caps its grid and the kernel loops with a grid stride; real weights (4096 x 11008) and real activations run in that regime.  Each case here is
the smallest tensor of its kind at which at least one thread takes a second iteration, with an end that fills no whole vector or plane, on seeded random data.
Criterion: the device bytes equal the reference library's torch sequence run on CPU tensors (the ``default=`` implementations of library/ops.py,
``tensor.packing.pack_weights``, ``scale * data.to(dtype)``), bit for bit.

Before a case builds its tensors it recomputes the launcher's block count from the formula in the .hip file (``blocks``) and asserts that the work exceeds what
the capped grid covers in one pass: a raised cap makes the case fail instead of testing nothing.
"""
import pytest
import torch

from optimum_quanto_amd.library import ops
from optimum_quanto_amd.library.hip import quanto_hip
from optimum_quanto_amd.tensor.packing import pack_weights

from helpers import TORCH_DT

pytestmark = pytest.mark.gpu
DEV = "cuda"
THREADS = 256  # every launcher here: dim3(256)


def blocks(work: int, cap: int) -> int:
    """ceil(work / 256) clamped to [1, cap]: the block count every launcher below computes from its work items."""
    return max(1, min(-(-work // THREADS), cap))


def assert_second_pass(work: int, cap: int):
    """The capped grid's threads cover fewer than ``work`` items in one pass."""
    assert blocks(work, cap) == cap and work > cap * THREADS, f"{work} work items fit one pass of {cap} blocks: the cap was raised, enlarge the case"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def assert_bytes_equal(got: torch.Tensor, want: torch.Tensor, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    g, w = got.cpu().reshape(-1), want.reshape(-1)
    g, w = g.view(torch.uint8), w.view(torch.uint8)
    bad = g != w
    if bad.any():
        i = bad.nonzero()[:, 0]
        raise AssertionError(f"{what}: {i.numel()} of {w.numel()} bytes differ from the CPU sequence, the first at byte {int(i[0])}, the last at {int(i[-1])}")


# ---- quantize_symmetric: 8 elements per thread and iteration ----------------------------------------------------------------------------------------
QS_CAP = 256 * 16  # quantize.hip launch_mode: `if (blocks > 256 * 16) blocks = 256 * 16;` over nvec = numel >> 3


@pytest.mark.parametrize("dt,target,scale", [("bf16", torch.int8, 0.05), ("fp32", torch.float8_e4m3fn, 0.01)], ids=["bf16-int8", "fp32-e4m3fn"])
def test_quantize_symmetric_per_tensor(dt, target, scale):
    numel = 8_388_608 + 2_405
    assert_second_pass(numel >> 3, QS_CAP)
    assert numel % 8, "ragged tail"
    x = (torch.randn(numel, generator=gen(1)) * 3).to(TORCH_DT[dt])
    s = torch.tensor(scale, dtype=TORCH_DT[dt])
    want = ops.quantize_symmetric(x, target, None, s)
    assert_bytes_equal(torch.ops.quanto.quantize_symmetric(x.to(DEV), target, None, s.to(DEV)), want, f"per-tensor {dt}")


@pytest.mark.parametrize("axis", [0, -1])
def test_quantize_symmetric_per_axis(axis):
    shape = (4099, 2053)
    numel = shape[0] * shape[1]
    assert_second_pass(numel >> 3, QS_CAP)
    assert numel % 8 and shape[1] % 8
    x = (torch.randn(shape, generator=gen(2)) * 3).to(torch.bfloat16)
    s = (0.02 + 0.06 * torch.rand((shape[0], 1) if axis == 0 else (1, shape[1]), generator=gen(3))).to(torch.bfloat16)
    want = ops.quantize_symmetric(x, torch.int8, axis, s)
    assert_bytes_equal(torch.ops.quanto.quantize_symmetric(x.to(DEV), torch.int8, axis, s.to(DEV)), want, f"axis {axis}")


# ---- dequantize_symmetric: 16 elements per thread and iteration -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dt,scale", [(torch.int8, "bf16", 0.0173), (torch.float8_e4m3fn, "fp16", 0.01)], ids=["int8-bf16", "e4m3fn-fp16"])
def test_dequantize_symmetric(kind, dt, scale):
    numel = 16_777_216 + 4_811
    assert_second_pass(numel >> 4, 4096)  # quantize.hip launch_dequantize: `(nvec + 255) / 256 > 4096 ? 4096 : ...` over nvec = numel >> 4
    assert numel % 16
    codes = torch.randint(0, 256, (numel,), dtype=torch.int16, generator=gen(4)).to(torch.uint8)
    if kind != torch.int8:
        codes[(codes & 0x7F) == 0x7F] = 0  # the two NaN codes of e4m3fn (test_elementwise_values_gpu.py has them)
    data = codes.view(kind)
    s = torch.tensor(scale, dtype=TORCH_DT[dt])
    got = quanto_hip.lib.dequantize_symmetric(data.to(DEV), s.to(DEV))
    assert got is not None
    assert_bytes_equal(got, s * data.to(TORCH_DT[dt]), f"dequantize {kind} -> {dt}")


# ---- quantize_affine: 4 elements per thread and iteration -------------------------------------------------------------------------------------------
def affine_problem(shape, dt, bits, group_size, int_shift, seed):
    """Seeded weight with max-type scale / shift per grouped row, so that the codes spread over [0, 2^bits)."""
    w = (torch.randn(shape, generator=gen(seed)) * 0.05).to(TORCH_DT[dt])
    rows = w.reshape(-1, group_size or shape[1])
    lo, hi = rows.amin(dim=1, keepdim=True), rows.amax(dim=1, keepdim=True)
    scale = ((hi - lo) / (2 ** bits - 1)).to(w.dtype)
    shift = torch.clamp(torch.round(-lo / scale), 0, 2 ** bits - 1).to(torch.uint8) if int_shift else -lo
    return w, scale, shift


@pytest.mark.parametrize("shape,group_size,dt,int_shift", [((2051, 2051), None, "bf16", False), ((2056, 2048), 128, "fp16", True)],
                         ids=["per-channel-bf16-shift", "group128-fp16-zp"])
def test_quantize_affine(shape, group_size, dt, int_shift):
    numel = shape[0] * shape[1]
    assert_second_pass(numel // 4, 256 * 16)  # quantize.hip quantize_affine: `blocks = (numel / 4 + 255) / 256; ... if (blocks > 256 * 16) blocks = 256 * 16;`
    w, scale, shift = affine_problem(shape, dt, 4, group_size, int_shift, 5)
    want = ops.quantize_affine(w, 4, 0, group_size, scale, shift)
    assert want.unique().numel() == 16
    got = torch.ops.quanto.quantize_affine(w.to(DEV), 4, 0, group_size, scale.to(DEV), shift.to(DEV))
    assert_bytes_equal(got, want, f"quantize_affine {shape}")


# ---- quantize_affine_packed, pack: one packed byte per thread and iteration -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bits,dt,int_shift", [((2051, 2051), 4, "bf16", True), ((4101, 2051), 2, "fp16", False)], ids=["int4-bf16-zp", "int2-fp16-shift"])
def test_quantize_affine_packed_and_pack(shape, bits, dt, int_shift):
    vpi = 8 // bits
    row_dim = -(-shape[0] // vpi)
    cap = 256 * 32  # quantize.hip quantize_affine_packed and pack_weights: `blocks = (row_dim * C + 255) / 256; ... if (blocks > 256 * 32) blocks = 256 * 32;`
    assert_second_pass(row_dim * shape[1], cap)
    assert shape[0] % vpi, "the last plane is ragged"
    lib = quanto_hip.lib
    w, scale, shift = affine_problem(shape, dt, bits, None, int_shift, 6)
    want = ops.quantize_affine(w, bits, 0, None, scale, shift)
    assert want.unique().numel() == 1 << bits
    want_packed = pack_weights(want, bits)
    assert_bytes_equal(lib.quantize_affine_packed(w.to(DEV), bits, None, scale.to(DEV), shift.to(DEV)), want_packed, f"quantize_affine_packed int{bits}")
    assert_bytes_equal(lib.pack(want.to(DEV), bits), want_packed, f"pack int{bits}")


# ---- unpack, dequantize_qbits ------------------------------------------------------------------------------------------------------------------------
UNPACK_CAP = 256 * 8  # unpack.hip grid_for: `const int64_t cap = 256 * 8;`


@pytest.mark.parametrize("bits", [4, 2])
@pytest.mark.parametrize("n,vector", [(8_388_608 + 1_600, True), (524_288 + 37, False)], ids=["vector", "scalar"])
def test_unpack(n, vector, bits):
    assert (n % 16 == 0) == vector  # unpack.hip unpack_dispatch: the 16-byte kernel when n % 16 == 0 (and the pointers are aligned)
    assert_second_pass(n // 16 if vector else n, UNPACK_CAP)
    packed = torch.randint(0, 256, (n,), dtype=torch.int16, generator=gen(7)).to(torch.uint8)
    assert_bytes_equal(torch.ops.quanto.unpack(packed.to(DEV), bits), ops.unpack_default(packed, bits), f"unpack int{bits}")


@pytest.mark.parametrize("N,K,group_size,dt,int_shift", [(4128, 4096, 128, "bf16", False), (1100, 1000, None, "fp16", True)], ids=["vector", "scalar"])
def test_dequantize_qbits(N, K, group_size, dt, int_shift):
    C = group_size or K
    rows = N * K // C
    row_dim = -(-rows // 2)
    vector = C % 16 == 0  # unpack.hip dequantize_launch: 16 packed bytes per thread when C % 16 == 0, one otherwise
    assert vector == (group_size is not None)
    assert_second_pass(row_dim * (C // 16) if vector else row_dim * C, UNPACK_CAP)
    packed = torch.randint(0, 256, (row_dim, C), dtype=torch.int16, generator=gen(8)).to(torch.uint8)
    scale = (0.005 + 0.01 * torch.rand((rows, 1), generator=gen(9))).to(TORCH_DT[dt])
    shift = torch.randint(0, 16, (rows, 1), dtype=torch.uint8, generator=gen(10)) if int_shift else (scale.to(torch.float32) * 7.5).to(scale.dtype)
    want = ops.dequantize_qbits_default(packed, scale, shift, 4, group_size, N, K)
    got = torch.ops.quanto.dequantize_qbits(packed.to(DEV), scale.to(DEV), shift.to(DEV), 4, group_size, N, K)
    assert_bytes_equal(got, want, f"dequantize_qbits {N}x{K}")

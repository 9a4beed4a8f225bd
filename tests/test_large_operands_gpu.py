"""Every matmul route at the operand sizes and grid limits its support rule admits.

The parity suite builds operands of at most ~2^26 elements; the support rules allow 16 to 64 times more (M*K < 2^30 / 2^31 / 2^32,
N*K < 2^31, grid.y <= 65535).  Each case here runs ONE call straight through the C ABI, just below a limit its route's rule states,
into an output buffer filled with NaN, and checks that call three ways:

* every element written and finite;
* sampled rows (the first and last ones, the rows whose operand byte offset crosses 2^31 and 2^32, the last tile row) - or, for the
  short lm_head calls, the whole output - against float64 math through the parity gate (helpers.assert_close_to_exact);
* a Freivalds projection y.v == x.(W^T v) in float64 for random +-1 vectors v, with the per-element gate summed over the projection
  as the bound: a wrong tile anywhere in the output moves it.

The operands are built on the device from a seeded generator in the oracle's formats (generic packed int4 / int2 with scale and shift,
int8 / fp8 with a per-row scale); their float64 images are rebuilt on the device for the rows a check needs.  Each case stays under
~8 GiB of device memory and frees it before the next one.
"""
import ctypes
import gc

import numpy as np
import pytest
import torch

from helpers import assert_close_to_exact, projection_bound, to_numpy
from optimum_quanto_amd.library.hip import quanto_hip

pytestmark = pytest.mark.gpu

BF16, I8, E4M3 = 2, 3, 5
AUTO, NAIVE, GEMV, MFMA, MFMA_LARGE, SKINNY, NATIVE8 = 0, 1, 2, 3, 4, 5, 6
NAMES = {NAIVE: "naive", GEMV: "gemv", MFMA: "mfma", MFMA_LARGE: "mfma_large", SKINNY: "skinny", NATIVE8: "mfma_native8"}
DEV = "cuda"
CHUNK = 1 << 26  # elements per float64 chunk of the reference math (512 MiB)


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _bf16_normal(rows, cols, gen, scale=1.0):
    """bf16 [rows, cols], filled in row chunks (no float32 copy of the whole operand)."""
    t = torch.empty((rows, cols), dtype=torch.bfloat16, device=DEV)
    step = max(1, CHUNK // cols)
    for r in range(0, rows, step):
        r1 = min(rows, r + step)
        t[r:r1] = (torch.randn((r1 - r, cols), generator=gen, device=DEV) * scale).to(torch.bfloat16)
    return t


def _bytes(n, gen):
    return torch.randint(0, 256, (n,), generator=gen, device=DEV, dtype=torch.int32).to(torch.uint8)


def _int8(rows, cols, gen):
    t = torch.empty((rows, cols), dtype=torch.int8, device=DEV)
    step = max(1, CHUNK // cols)
    for r in range(0, rows, step):
        r1 = min(rows, r + step)
        t[r:r1] = torch.randint(-127, 128, (r1 - r, cols), generator=gen, device=DEV, dtype=torch.int32).to(torch.int8)
    return t


def _e4m3(rows, cols, gen):
    """float8_e4m3fn [rows, cols] of random finite codes (the two NaN codes replaced by zero)."""
    t = torch.empty((rows, cols), dtype=torch.uint8, device=DEV)
    step = max(1, CHUNK // cols)
    for r in range(0, rows, step):
        r1 = min(rows, r + step)
        b = _bytes((r1 - r) * cols, gen).view(r1 - r, cols)
        t[r:r1] = torch.where((b & 0x7F) == 0x7F, torch.zeros_like(b), b)
    return t.view(torch.float8_e4m3fn)


class QBitsWeight:
    """A generic packed int4 / int2 weight (group size 128, float shift) and the float64 image scale * q - shift of any of its rows."""

    def __init__(self, N, K, bits, gen):
        self.N, self.K, self.bits, self.G = N, K, bits, K // 128
        R = N * self.G
        self.planes = 8 // bits
        self.packed = _bytes(R // self.planes * 128, gen).view(R // self.planes, 128)
        self.scale = (torch.rand((R,), generator=gen, device=DEV) * 0.015 + 0.005).to(torch.bfloat16)
        self.shift = (self.scale.float() * (torch.rand((R,), generator=gen, device=DEV) * 2 + (2 ** bits / 2 - 1))).to(torch.bfloat16)

    def rows64(self, n0, n1):
        """float64 [n1 - n0, K]: the exact dequantized features n0 .. n1 - 1."""
        G, bits, rp = self.G, self.bits, self.N * self.G // self.planes
        r = torch.arange(n0 * G, n1 * G, device=DEV)
        plane, row = r // rp, r % rp
        q = (self.packed[row].to(torch.int32) >> (bits * plane[:, None].to(torch.int32))) & ((1 << bits) - 1)
        w = q.double() * self.scale[r].double()[:, None] - self.shift[r].double()[:, None]
        return w.view(n1 - n0, self.K)

    def pointers(self):
        return self.packed.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr()


class QBytesWeight:
    """An int8 / e4m3 weight [N, K] with a per-row bf16 scale."""

    def __init__(self, N, K, b_dtype, gen):
        self.N, self.K, self.b_dtype = N, K, b_dtype
        self.data = _int8(N, K, gen) if b_dtype == I8 else _e4m3(N, K, gen)
        self.scale = (torch.rand((N,), generator=gen, device=DEV) * 0.015 + 0.005).to(torch.bfloat16)

    def rows64(self, n0, n1):
        return self.data[n0:n1].float().double() * self.scale[n0:n1].double()[:, None]


def _weight_rows(w, rows_per_chunk=None):
    step = rows_per_chunk or max(1, CHUNK // w.K)
    for n0 in range(0, w.N, step):
        n1 = min(w.N, n0 + step)
        yield n0, n1, w.rows64(n0, n1)


def _act64(x, rows):
    x = x[rows]
    return x.float().double()


def _plan_qbits(M, N, K, bits, kernel):
    c = quanto_hip.lib._c
    k, ws = ctypes.c_int(0), ctypes.c_int64(0)
    assert c.quanto_hip_qbits_mm_plan(M, N, K, bits, 128, BF16, kernel, ctypes.byref(k), ctypes.byref(ws)) == 0
    return k.value, ws.value


def _plan_qbytes(M, N, K, a_dtype, b_dtype, kernel):
    c = quanto_hip.lib._c
    k, ws = ctypes.c_int(0), ctypes.c_int64(0)
    assert c.quanto_hip_qbytes_mm_plan(M, N, K, a_dtype, b_dtype, BF16, kernel, ctypes.byref(k), ctypes.byref(ws)) == 0
    return k.value, ws.value


def _workspace(nbytes):
    return torch.zeros((max(nbytes, 16),), dtype=torch.uint8, device=DEV)  # counter region zero on entry


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_output(M, N):
    return torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)


def _check_written(y, what):
    bad = int((~torch.isfinite(y)).sum())
    assert bad == 0, f"{what}: {bad} output elements not written (or not finite)"


def _check_full(y, x, w, what, out_scale=1.0):
    """Short calls: the whole output against float64 math (weight rows in chunks)."""
    x64 = x.float().double()
    exact = torch.empty((y.shape[0], w.N), dtype=torch.float64, device=DEV)
    for n0, n1, w64 in _weight_rows(w):
        exact[:, n0:n1] = (x64 @ w64.T) * out_scale
    assert_close_to_exact(to_numpy(y), exact.cpu().numpy(), "bf16", what)


def _sample_rows(M, K, esize, tile):
    """First and last rows, the rows whose activation byte offset crosses 2^31 and 2^32, the first and last row of the last tile."""
    rows = {0, 1, M - 1, (M - 1) // tile * tile}
    for lim in (1 << 31, 1 << 32):
        m = lim // (K * esize)
        rows.update(r for r in (m - 1, m, m + 1) if 0 <= r < M)
    return sorted(rows)


def _check_rows(y, x, w, rows, what, out_scale=1.0):
    x64 = _act64(x, torch.tensor(rows, device=DEV))
    exact = torch.cat([x64 @ w64.T for _, _, w64 in _weight_rows(w)], dim=1) * out_scale
    assert_close_to_exact(to_numpy(y[rows]), exact.cpu().numpy(), "bf16", f"{what} rows {rows}")


def _check_freivalds(y, x, w, what, out_scale=1.0, nvec=3, seed=0):
    """y.v against x.(W^T v) in float64 for `nvec` random +-1 vectors v.  Bound per row: the parity gate's per-element error (2 bf16 ulp of
    the output plus 1e-2 of the largest output for cancelled elements, DESIGN.md "Parity") summed over the projection, with the fp32
    accumulation's own slack."""
    M, N = y.shape
    v = (torch.randint(0, 2, (N, nvec), generator=_gen(seed), device=DEV, dtype=torch.int32) * 2 - 1).double()
    wv = torch.zeros((w.K, nvec), dtype=torch.float64, device=DEV)
    for n0, n1, w64 in _weight_rows(w):
        wv += w64.T @ v[n0:n1]
    ymax = float(y.float().abs().max())
    assert ymax > 0, f"{what}: all-zero output"
    step = max(1, CHUNK // max(w.K, N))
    worst = 0.0
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        yc = y[m0:m1].float().double()
        got = yc @ v
        want = (x[m0:m1].float().double() @ wv) * out_scale
        bound = projection_bound(yc.abs().sum(dim=1, keepdim=True), N, ymax)
        ratio = float(((got - want).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what}: Freivalds projection off in rows {m0}..{m1 - 1} ({ratio:.2f} x the bound)"
    return worst


def _run_qbits(x, w, M, kernel, ws_bytes):
    c = quanto_hip.lib._c
    y = _nan_output(M, w.N)
    ws = _workspace(ws_bytes) if ws_bytes > 0 else None
    pk, sc, sh = w.pointers()
    st = c.quanto_hip_qbits_mm(x.data_ptr(), pk, sc, sh, None, y.data_ptr(), M, w.N, w.K, w.bits, 128, BF16, BF16, kernel,
                               None if ws is None else ws.data_ptr(), ws_bytes if ws is not None else 0, _stream())
    assert st == 0, quanto_hip.lib._c.quanto_hip_status_string(st)
    torch.cuda.synchronize()
    return y


def _run_qbytes(x, w, M, a_dtype, kernel, ws_bytes):
    c = quanto_hip.lib._c
    y = _nan_output(M, w.N)
    ws = _workspace(ws_bytes) if ws_bytes > 0 else None
    st = c.quanto_hip_qbytes_mm_ws(x.data_ptr(), w.data.data_ptr(), w.scale.data_ptr(), None, y.data_ptr(), M, w.N, w.K, a_dtype, w.b_dtype,
                                   BF16, kernel, None if ws is None else ws.data_ptr(), ws_bytes if ws is not None else 0, _stream())
    assert st == 0, quanto_hip.lib._c.quanto_hip_status_string(st)
    torch.cuda.synchronize()
    return y


# ---- lm_head decode / short prefill: N*K close to 2^31 elements, M small: the whole output against float64 math ----------------------
LM_QBITS = [  # (M, N, K, bits, expected AUTO kernel)
    (1, 256000, 8192, 4, GEMV),      # N*K = 1.95 x 2^30: int4 GEMV streams a 1 GiB packed weight
    (8, 128256, 16384, 4, SKINNY),   # N*K = 1.96 x 2^30
    (65, 152064, 8192, 4, SKINNY),   # first M above the batched-decode range
    (8, 152064, 8192, 2, SKINNY),    # int2 lm_head
]


@pytest.mark.parametrize("M,N,K,bits,route", LM_QBITS, ids=[f"{m}x{n}x{k}-int{b}" for m, n, k, b, _ in LM_QBITS])
def test_qbits_lm_head(M, N, K, bits, route):
    kernel, ws = _plan_qbits(M, N, K, bits, AUTO)
    assert kernel == route
    gen = _gen(M + N + bits)
    w = QBitsWeight(N, K, bits, gen)
    x = _bf16_normal(M, K, gen)
    y = _run_qbits(x, w, M, AUTO, ws)
    assert quanto_hip.lib.last_kernel() == NAMES[route]
    _check_written(y, "lm_head qbits")
    _check_full(y, x, w, f"qbits lm_head {M}x{N}x{K} int{bits}")


LM_QBYTES = [  # (M, N, K, weight dtype, expected AUTO kernel)
    (1, 256000, 8192, I8, GEMV),             # 2 GiB int8 weight through the GEMV
    (64, 128256, 16384, E4M3, SKINNY),       # N*K = 1.96 x 2^30, 2 GiB e4m3
    (65, 256000, 8192, I8, MFMA_LARGE),      # lm_head prefill: the large-tile kernel
    (65, 262143, 8192, E4M3, MFMA_LARGE),    # N*K = 2^31 - 8192: the last N its N*K < 2^31 rule admits at this K
]


@pytest.mark.parametrize("M,N,K,bdt,route", LM_QBYTES, ids=[f"{m}x{n}x{k}-{'i8' if b == I8 else 'e4m3'}" for m, n, k, b, _ in LM_QBYTES])
def test_qbytes_lm_head(M, N, K, bdt, route):
    kernel, ws = _plan_qbytes(M, N, K, BF16, bdt, AUTO)
    assert kernel == route
    gen = _gen(M + N + bdt)
    w = QBytesWeight(N, K, bdt, gen)
    x = _bf16_normal(M, K, gen)
    y = _run_qbytes(x, w, M, BF16, AUTO, ws)
    assert quanto_hip.lib.last_kernel() == NAMES[route]
    _check_written(y, "lm_head qbytes")
    _check_full(y, x, w, f"qbytes lm_head {M}x{N}x{K} {bdt}")


# ---- long prefill: M*K at the rule's limit, N small: sampled rows + Freivalds over the whole output --------------------------------------
def test_qbits_mfma_long_prefill_beyond_dequant_limit():
    """int4 at M*K = 2^30 (long prefill, where dequantize + dense stops): the register-staged 128x128 kernel with its group-sum scratch."""
    M, N, K = 131072, 128, 8192
    kernel, ws = _plan_qbits(M, N, K, 4, MFMA)
    gen = _gen(11)
    w = QBitsWeight(N, K, 4, gen)
    x = _bf16_normal(M, K, gen)
    y = _run_qbits(x, w, M, kernel, ws)
    assert quanto_hip.lib.last_kernel() == "mfma"
    _check_written(y, "qbits mfma")
    _check_rows(y, x, w, _sample_rows(M, K, 2, 128), "qbits mfma M*K = 2^30")
    _check_freivalds(y, x, w, "qbits mfma M*K = 2^30")


def test_qbits_mfma_at_its_grid_limit():
    """The 128x128 kernel puts its M tiles in grid.y: the last M its rule admits is 65535 tiles of 128 rows (K = 128, N = 64)."""
    M, N, K = 65535 * 128, 64, 128
    kernel, ws = _plan_qbits(M, N, K, 4, MFMA)
    assert kernel == MFMA
    c = quanto_hip.lib._c
    assert c.quanto_hip_qbits_mm_workspace_size(M + 1, N, K, 4, 128, BF16, MFMA) == -2  # one row more: a 65536th tile, refused
    gen = _gen(12)
    w = QBitsWeight(N, K, 4, gen)
    x = _bf16_normal(M, K, gen)
    y = _run_qbits(x, w, M, kernel, ws)
    assert quanto_hip.lib.last_kernel() == "mfma"
    _check_written(y, "qbits mfma grid limit")
    _check_rows(y, x, w, _sample_rows(M, K, 2, 128), "qbits mfma grid.y = 65535")
    _check_freivalds(y, x, w, "qbits mfma grid.y = 65535")


@pytest.mark.parametrize("bdt,kernel,M", [(I8, MFMA, 131072), (E4M3, MFMA_LARGE, 131071)], ids=["i8-mfma", "e4m3-mfma_large"])
def test_qbytes_long_prefill(bdt, kernel, M):
    """bf16 x int8 / e4m3 at K = 8192: the 128x128 kernel at M*K = 2^30 (beyond the large-tile rule) and the large-tile kernel at
    M*K = 2^30 - 8192, the last M its M*K < 2^30 rule admits."""
    N, K = 128, 8192
    if kernel == MFMA_LARGE:
        c = quanto_hip.lib._c
        assert c.quanto_hip_qbytes_mm_workspace_size(M + 1, N, K, BF16, bdt, BF16, MFMA_LARGE) == -2
    k, ws = _plan_qbytes(M, N, K, BF16, bdt, kernel)
    assert k == kernel
    gen = _gen(20 + kernel)
    w = QBytesWeight(N, K, bdt, gen)
    x = _bf16_normal(M, K, gen)
    y = _run_qbytes(x, w, M, BF16, kernel, ws)
    assert quanto_hip.lib.last_kernel() == NAMES[kernel]
    _check_written(y, "qbytes long prefill")
    _check_rows(y, x, w, _sample_rows(M, K, 2, 256), f"qbytes {NAMES[kernel]}")
    _check_freivalds(y, x, w, f"qbytes {NAMES[kernel]}")


@pytest.mark.parametrize("M,route", [(262143, NATIVE8), (524289, NAIVE)], ids=["native8-below-2^31", "naive-beyond-2^32-bytes"])
def test_int8_activations_at_the_native8_limit(M, route):
    """int8 x int8 at K = 8192: native8 at M*K = 2^31 - 8192 (the last M its rule admits), and beyond it the one-thread-per-output
    kernel AUTO falls to, with activations of 4 GiB + one row (tiny N: the naive kernel is slow at real widths)."""
    N, K = 64 if route == NATIVE8 else 16, 8192
    kernel, ws = _plan_qbytes(M, N, K, I8, I8, AUTO)
    assert kernel == route
    gen = _gen(30 + route)
    w = QBytesWeight(N, K, I8, gen)
    x = _int8(M, K, gen)
    y = _run_qbytes(x, w, M, I8, AUTO, ws)
    assert quanto_hip.lib.last_kernel() == NAMES[route]
    _check_written(y, "int8 x int8")
    _check_rows(y, x, w, _sample_rows(M, K, 1, 256), f"int8 x int8 {NAMES[route]}")
    _check_freivalds(y, x, w, f"int8 x int8 {NAMES[route]}")


def test_a8_int8_at_its_last_m():
    """W4A8 at the last M the corrected rule admits (65535 tiles of 64 tokens in grid.y) with M*K just below 2^32: int8 activations of
    ~4 GiB, whose byte offsets cross 2^31 and 2^32 inside the LDS-DMA loads.  Unsplit int8: the output is a function of the integers."""
    M, N, K = 65535 * 64, 128, 1024
    c = quanto_hip.lib._c
    assert c.quanto_hip_qbits_mm_a8_workspace_size(M, N, K, 4, 128, I8, BF16) == 0
    assert c.quanto_hip_qbits_mm_a8_workspace_size(M + 1, N, K, 4, 128, I8, BF16) == -2
    gen = _gen(40)
    w = QBitsWeight(N, K, 4, gen)
    a = _int8(M, K, gen)
    a_scale = torch.tensor([0.0078125], dtype=torch.bfloat16, device=DEV)
    y = _nan_output(M, N)
    pk, sc, sh = w.pointers()
    st = c.quanto_hip_qbits_mm_a8(a.data_ptr(), a_scale.data_ptr(), pk, sc, sh, None, y.data_ptr(), M, N, K, 4, 128, I8, BF16, BF16, None, 0,
                                  _stream())
    assert st == 0, c.quanto_hip_status_string(st)
    torch.cuda.synchronize()
    assert quanto_hip.lib.last_kernel() == "a8_fused_int8"
    _check_written(y, "a8")
    s = float(a_scale)
    _check_rows(y, a, w, _sample_rows(M, K, 1, 64), "a8 int8 last M", out_scale=s)
    _check_freivalds(y, a, w, "a8 int8 last M", out_scale=s)

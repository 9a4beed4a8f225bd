"""The size limits of the matmul routes, from the host-only plan / workspace-size entries (no GPU needed).

* Planner pins: which (kernel, workspace bytes) the planner picks at real lm_head and long-prefill shapes and at (limit - 1, limit) of every
  product limit a support rule states - a routing change shows up here as a test diff, not only as a slowdown on long prompts.
* Launch grids: every kernel that puts an M-tile count in grid.y takes at most hipDeviceProp_t::maxGridSize[1] tiles at the largest M its
  rule admits (found by bisection on the rule itself).
* Rejection: a forced kernel asked for a shape beyond its rule gets QUANTO_HIP_ENOTSUP from the size / plan entries, never a size.
tests/test_large_operands_gpu.py runs each route just below these limits on the device.
"""
import ctypes

import pytest

from optimum_quanto_amd.library.hip import quanto_hip

ENOTSUP = -2
F32, BF16, I8, E4M3 = 0, 2, 3, 5
AUTO, NAIVE, GEMV, MFMA, MFMA_LARGE, SKINNY, NATIVE8, DEQUANT_MFMA, MFMA_FUSED4, MMV, MFMA_LARGE4 = range(11)
# hipDeviceProp_t::maxGridSize on the MI355X (gfx950, ROCm 7): [2147483647, 65536, 65536].  The kernels' rules keep grid.y <= 65535.
MAX_GRID_Y = 65536

_c = quanto_hip.cdll
_i64, _ci = ctypes.c_int64, ctypes.c_int
_c.quanto_hip_qbits_mm_plan.restype = _ci
_c.quanto_hip_qbits_mm_plan.argtypes = [_i64] * 3 + [_ci] * 4 + [ctypes.POINTER(_ci), ctypes.POINTER(_i64)]
_c.quanto_hip_qbytes_mm_plan.restype = _ci
_c.quanto_hip_qbytes_mm_plan.argtypes = [_i64] * 3 + [_ci] * 4 + [ctypes.POINTER(_ci), ctypes.POINTER(_i64)]
_c.quanto_hip_qbits_mm_workspace_size.restype = _i64
_c.quanto_hip_qbits_mm_workspace_size.argtypes = [_i64] * 3 + [_ci] * 4
_c.quanto_hip_qbytes_mm_workspace_size.restype = _i64
_c.quanto_hip_qbytes_mm_workspace_size.argtypes = [_i64] * 3 + [_ci] * 4
_c.quanto_hip_qbits_mm_a8_workspace_size.restype = _i64
_c.quanto_hip_qbits_mm_a8_workspace_size.argtypes = [_i64] * 3 + [_ci] * 4
_c.quanto_hip_qbytes_conv2d_a8_workspace_size.restype = _i64
_c.quanto_hip_qbytes_conv2d_a8_workspace_size.argtypes = [_i64] * 9 + [_ci] * 9


def qbits_plan(M, N, K, bits=4, gs=128, dt=BF16, kernel=AUTO):
    k, ws = _ci(0), _i64(0)
    st = _c.quanto_hip_qbits_mm_plan(M, N, K, bits, gs, dt, kernel, ctypes.byref(k), ctypes.byref(ws))
    return (k.value, ws.value) if st == 0 else st


def qbytes_plan(M, N, K, a=BF16, b=I8, out=BF16, kernel=AUTO):
    k, ws = _ci(0), _i64(0)
    st = _c.quanto_hip_qbytes_mm_plan(M, N, K, a, b, out, kernel, ctypes.byref(k), ctypes.byref(ws))
    return (k.value, ws.value) if st == 0 else st


def a8_ws(M, N, K, bits=4, a=I8):
    return _c.quanto_hip_qbits_mm_a8_workspace_size(M, N, K, bits, 128, a, BF16)


LM_HEADS = [(152064, 8192), (256000, 8192), (128256, 16384)]  # Qwen2 72B, Gemma, Llama 3 405B-style: N*K = 1.16 / 1.95 / 1.96 x 2^30


@pytest.mark.parametrize("N,K", LM_HEADS)
def test_lm_head_routes(N, K):
    """Decode (M <= 64) streams the weight (GEMV / skinny); prefill goes to the large-tile 8-bit kernel, and for int4 to the skinny kernel
    at 65 and the register-staged 128x128 kernel (group-sum scratch: fp32 [K/128][roundup(M, 128)]) from 512 rows on; int2 prefill
    falls to the naive kernel; 8-bit activations always run native8 (N*K < 2^31)."""
    G = K // 128
    for M in (1, 8, 64, 65, 512, 32768):
        mpad = -(-M // 128) * 128
        int4 = {1: (GEMV, 0), 65: (SKINNY, 0), 512: (MFMA, G * mpad * 4), 32768: (MFMA, G * mpad * 4)}.get(M, (SKINNY, 0))
        int2 = (GEMV, 0) if M == 1 else (SKINNY, 0) if M <= 65 else (NAIVE, 0)
        q8 = (GEMV, 0) if M == 1 else (SKINNY, 0) if M <= 64 else (MFMA_LARGE, 0)
        assert qbits_plan(M, N, K) == int4, (M, N, K)
        assert qbits_plan(M, N, K, bits=2) == int2, (M, N, K)
        assert qbytes_plan(M, N, K, b=I8) == q8, (M, N, K)
        assert qbytes_plan(M, N, K, b=E4M3) == q8, (M, N, K)
        assert qbytes_plan(M, N, K, a=I8, b=I8) == (NATIVE8, 0), (M, N, K)
        assert qbytes_plan(M, N, K, a=E4M3, b=E4M3) == (NATIVE8, 0), (M, N, K)


PREFILL = [  # (M, N, K): int4 / int8 / e4m3 weights with bf16 activations all fall to the 128x128 kernel (M*K >= 2^30)
    (131072, 4096, 14336), (65536, 8192, 28672), (32768, 16384, 53248),
    (65536, 16384, 53248), (131072, 8192, 28672), (131072, 128256, 16384),
]


@pytest.mark.parametrize("M,N,K", PREFILL)
def test_long_prefill_routes(M, N, K):
    mpad = -(-M // 128) * 128
    assert qbits_plan(M, N, K) == (MFMA, K // 128 * mpad * 4)
    assert qbits_plan(M, N, K, bits=2) == (NAIVE, 0)  # not met: int2 long prefill has no tiled kernel
    assert qbytes_plan(M, N, K, b=I8) == (MFMA, 0)
    assert qbytes_plan(M, N, K, b=E4M3) == (MFMA, 0)
    native8 = M * K < 1 << 31
    for a in (I8, E4M3):
        assert qbytes_plan(M, N, K, a=a, b=a) == ((NATIVE8, 0) if native8 else (NAIVE, 0))  # not met: the naive cliff at M*K >= 2^31
    # W4A8 (M*K < 2^32, at most 65535 tiles of 64 tokens): unsplit; K = 53248 is refused (its 416-group scale tables fill no LDS plan)
    assert a8_ws(M, N, K) == (ENOTSUP if K == 53248 else 0)


def _at(limit, K):
    """(limit - 1) // K, the last row count with rows * K < limit, and the first one beyond it."""
    return (limit - 1) // K, (limit - 1) // K + 1


@pytest.mark.parametrize("K", [4096, 8192])
def test_product_limits(K):
    """Each product limit of a support rule at (limit - 1, limit): the forced kernel is planned just below and refused at the limit."""
    # M*K < 2^30: the large-tile 8-bit kernel, dequantize + dense, the large-tile int4 kernel
    lo, hi = _at(1 << 30, K)
    assert qbytes_plan(lo, 4096, K, kernel=MFMA_LARGE)[0] == MFMA_LARGE
    assert qbytes_plan(hi, 4096, K, kernel=MFMA_LARGE) == ENOTSUP
    assert qbits_plan(lo, 4096, K, kernel=DEQUANT_MFMA) == (DEQUANT_MFMA, 4096 * K * 2)
    assert qbits_plan(hi, 4096, K, kernel=DEQUANT_MFMA) == ENOTSUP
    assert qbits_plan(lo, 4096, K, kernel=MFMA_LARGE4) == (MFMA_LARGE4, 0)
    assert qbits_plan(hi, 4096, K, kernel=MFMA_LARGE4) == ENOTSUP
    # N*K < 2^30: dequantize + dense (the dense weight); N*K < 2^31: the large-tile 8-bit kernel and native8
    lo, hi = _at(1 << 30, K)
    assert qbits_plan(4096, lo, K, kernel=DEQUANT_MFMA)[0] == DEQUANT_MFMA
    assert qbits_plan(4096, hi, K, kernel=DEQUANT_MFMA) == ENOTSUP
    lo, hi = _at(1 << 31, K)
    assert qbytes_plan(65, lo, K, kernel=MFMA_LARGE)[0] == MFMA_LARGE
    assert qbytes_plan(65, hi, K, kernel=MFMA_LARGE) == ENOTSUP
    assert qbytes_plan(65, lo, K, a=I8, b=I8) == (NATIVE8, 0)
    assert qbytes_plan(65, hi, K, a=I8, b=I8) == (NAIVE, 0)
    # M*K < 2^31: native8, the fused int4 GEMM
    assert qbytes_plan(lo, 64, K, a=I8, b=I8) == (NATIVE8, 0)
    assert qbytes_plan(hi, 64, K, a=I8, b=I8) == (NAIVE, 0)
    assert qbytes_plan(lo, 64, K, a=E4M3, b=E4M3, kernel=NATIVE8)[0] == NATIVE8
    assert qbytes_plan(hi, 64, K, a=E4M3, b=E4M3, kernel=NATIVE8) == ENOTSUP
    assert qbits_plan(lo, 4096, K, kernel=MFMA_FUSED4)[0] == MFMA_FUSED4
    assert qbits_plan(hi, 4096, K, kernel=MFMA_FUSED4) == ENOTSUP
    # M*K < 2^32: W4A8 / W2A8 (here the grid bound of 65535 x 64 tokens is the tighter one only for K < 1024)
    lo, hi = _at(1 << 32, K)
    for bits, adt in ((4, I8), (2, E4M3)):
        assert a8_ws(lo, 128, K, bits, adt) == 0
        assert a8_ws(hi, 128, K, bits, adt) == ENOTSUP


def _largest(accepts, hi=1 << 31):
    """The largest M in [1, hi] that `accepts` (a rule that holds up to some M and fails beyond it)."""
    assert accepts(1)
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if accepts(mid) else (lo, mid - 1)
    return lo


# kernels that put their M tiles in grid.y: (name, smallest token tile the kernel may take (its own constants), rule as a function of M)
GRID_Y = [
    ("qmm_mfma qbits (BM 128)", 128, lambda M: qbits_plan(M, 64, 128, kernel=MFMA) != ENOTSUP),
    ("qmm_mfma qbytes (BM 128)", 128, lambda M: qbytes_plan(M, 64, 128, kernel=MFMA) != ENOTSUP),
    ("qmm_f32 qbits (BM 128)", 128, lambda M: qbits_plan(M, 64, 128, dt=F32, kernel=MFMA) != ENOTSUP),
    ("qmm_f32 qbytes (BM 128)", 128, lambda M: qbytes_plan(M, 64, 128, a=F32, out=F32, kernel=MFMA) != ENOTSUP),
    ("qbits_mfma_fused (bm 64 / 128)", 64, lambda M: qbits_plan(M, 64, 128, kernel=MFMA_FUSED4) != ENOTSUP),
    ("qbits_a8_fused int4 (bm 64 / 128)", 64, lambda M: a8_ws(M, 64, 128) >= 0),
    ("qbits_a8_fused int2 (bm 64 / 128)", 64, lambda M: a8_ws(M, 64, 128, 2, E4M3) >= 0),
    ("qconv_a8 (BM 128 pixels)", 128,
     lambda M: _c.quanto_hip_qbytes_conv2d_a8_workspace_size(1, 8, 1, M, 64, 1, 1, 1, M, 1, 1, 0, 0, 1, 1, I8, I8, BF16) >= 0),
]


@pytest.mark.parametrize("name,tile,accepts", GRID_Y, ids=[g[0] for g in GRID_Y])
def test_grid_y_fits_at_the_largest_admitted_m(name, tile, accepts):
    """At the largest M its rule admits, the kernel's M-tile count fits grid.y (hipDeviceProp_t::maxGridSize[1]).  Without this bound the
    C ABI took e.g. quanto_hip_qbits_mm_a8(M = 30,000,000, N = K = 128) - 469 k workgroups in y - as supported, unsplit."""
    M = _largest(accepts)
    tiles = -(-M // tile)
    assert tiles <= MAX_GRID_Y, f"{name}: M = {M} admitted, {tiles} tiles in grid.y"
    assert tiles == 65535, f"{name}: the grid bound is not the binding limit here (M = {M})"
    assert a8_ws(30_000_000, 128, 128) == ENOTSUP


def test_forced_kernels_beyond_their_rule_are_refused():
    """A forced kernel outside its rule: ENOTSUP from both the plan and the workspace-size entries, not a size (AUTO never is)."""
    refused = [
        (qbits_plan, (300, 4096, 4096), dict(kernel=GEMV)),                   # GEMV: M <= 64 rows
        (qbits_plan, (300, 4096, 4096), dict(kernel=SKINNY)),                 # streaming kernel: M <= 256
        (qbits_plan, (64, 4096, 4096), dict(kernel=MMV)),                     # register-streaming kernel: M <= 32
        (qbits_plan, (300, 4096, 4096), dict(bits=2, kernel=MFMA_LARGE4)),    # int4 only
        (qbits_plan, (300, 4096, 4096), dict(gs=32, kernel=MFMA)),            # group sizes 64 / 128
        (qbytes_plan, (300, 4096, 4096), dict(kernel=GEMV)),                  # M <= 8
        (qbytes_plan, (300, 4096, 4096), dict(kernel=NATIVE8)),               # float activations
        (qbytes_plan, (300, 4096, 4096), dict(a=I8, b=I8, kernel=MFMA_LARGE)),  # 16-bit activations only
    ]
    for plan, shape, kw in refused:
        assert plan(*shape, **kw) == ENOTSUP, (plan.__name__, shape, kw)
    assert _c.quanto_hip_qbits_mm_workspace_size(300, 4096, 4096, 4, 128, BF16, SKINNY) == ENOTSUP
    assert _c.quanto_hip_qbytes_mm_workspace_size(300, 4096, 4096, BF16, I8, BF16, GEMV) == ENOTSUP
    assert _c.quanto_hip_qbits_mm_workspace_size(300, 4096, 4096, 4, 128, BF16, 42) == -1  # no such kernel
    # the same shapes under AUTO, and a forced kernel inside its rule, still plan
    assert qbits_plan(300, 4096, 4096)[0] in (MFMA_FUSED4, DEQUANT_MFMA)
    assert qbits_plan(300, 4096, 4096, kernel=NAIVE) == (NAIVE, 0)
    assert qbytes_plan(300, 4096, 4096, a=I8, b=I8) == (NATIVE8, qbytes_plan(300, 4096, 4096, a=I8, b=I8, kernel=NATIVE8)[1])

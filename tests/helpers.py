"""Shared helpers for the parity tests: oracle-built inputs and numpy <-> torch conversions."""
import numpy as np
import torch

from oracle import quanto_oracle as O

TORCH_DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
FP8_TORCH = {"e4m3fn": torch.float8_e4m3fn, "e4m3fnuz": torch.float8_e4m3fnuz, "e5m2": torch.float8_e5m2}


def to_torch(a: np.ndarray, dt: str, device="cpu") -> torch.Tensor:
    """float32 array holding dt-representable values -> torch tensor of that dtype (exact)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH_DT[dt]).to(device)


def to_numpy(t: torch.Tensor) -> np.ndarray:
    if t.dtype in FP8_TORCH.values():
        return t.view(torch.uint8).cpu().numpy()
    if t.dtype.is_floating_point:
        return t.detach().to(torch.float32).cpu().numpy()
    return t.detach().cpu().numpy()


def fp8_tensor(codes: np.ndarray, kind: str, device="cpu") -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(FP8_TORCH[kind]).to(device)


_WEIGHT_CACHE = {}  # weight_seed given: the quantized weight of a (shape, format, seed) is built once per session and shared by every M


def _activations(M, K, dt, rng):
    return O.round_to(rng.standard_normal((M, K)).astype(np.float32), dt)


def make_qbits_problem(M, N, K, dt, bits=4, group_size=128, zeropoint=False, seed=0, wscale=0.02, weight_seed=None):
    """Seeded activations + a weight quantized by the (reference-pinned) oracle, generic PackedTensor layout.
    ``weight_seed``: draw the weight from its own stream and cache the quantized result (suites that sweep M over one weight)."""

    def weight(rng):
        w = O.round_to((rng.standard_normal((N, K)) * wscale).astype(np.float32), dt)
        scale, shift = O.max_scale_shift(w, bits, 0, group_size, dt)
        if zeropoint:
            shift = np.clip(np.rint(O.round_to(shift / scale, dt)), 0, 2**bits - 1).astype(np.uint8)
        q = O.quantize_affine(w, bits, 0, group_size, scale, shift, dt)
        return dict(packed=O.pack_weights(q, bits), scale=scale, shift=shift)

    rng = np.random.default_rng(seed)
    if weight_seed is None:
        wq = weight(rng)  # historical stream order: weight first, then activations
    else:
        key = ("qbits", N, K, dt, bits, group_size, zeropoint, weight_seed, wscale)
        if key not in _WEIGHT_CACHE:
            _WEIGHT_CACHE[key] = weight(np.random.default_rng(weight_seed))
        wq = _WEIGHT_CACHE[key]
    x = _activations(M, K, dt, rng)
    return dict(x=x, packed=wq["packed"], scale=wq["scale"], shift=wq["shift"], bits=bits, group_size=group_size, N=N, K=K, dt=dt,
                wkey=None if weight_seed is None else key)


_EXACT_W = {}  # float64 dequantized weights of cached problems, the last six: an M sweep alternates dtype x zero-point (x members of a multi launch)


def qbits_exact(p, x=None, bias=None):
    """O.qbits_mm_exact on a problem of make_qbits_problem (``x``: another activation, e.g. the shared input of a multi launch); the float64
    weight of a cached problem (``weight_seed``) is kept between the Ms of a sweep instead of being dequantized again for every M."""
    x = p["x"] if x is None else x
    key = p.get("wkey")
    if key is None:
        return O.qbits_mm_exact(x, p["packed"], p["bits"], p["scale"], p["shift"], p["group_size"], p["N"], p["K"], bias)
    if key not in _EXACT_W:
        while len(_EXACT_W) >= 6:
            _EXACT_W.pop(next(iter(_EXACT_W)))
        _EXACT_W[key] = O.dequantize_qbits_exact(p["packed"], p["bits"], p["scale"], p["shift"], 0, p["group_size"], (p["N"], p["K"]))
    y = np.matmul(np.asarray(x, np.float64), _EXACT_W[key].T)
    return y if bias is None else y + np.asarray(bias, np.float64)


def make_qbytes_problem(M, N, K, dt, kind=None, seed=0, wscale=0.02, weight_seed=None):
    """int8 (kind None) or fp8 weight with per-row absmax scale, built by the oracle (``weight_seed``: as make_qbits_problem)."""

    def weight(rng):
        w = O.round_to((rng.standard_normal((N, K)) * wscale).astype(np.float32), dt)
        if kind is None:
            scale = O.absmax_scale(w, 127.0, 0, dt)
            data = O.quantize_symmetric_int8(w, scale, dt)
        else:
            scale = O.absmax_scale(w, O.FP8_MAX[kind], 0, dt)
            data = O.quantize_symmetric_fp8(w, scale, kind, dt)
        return dict(data=data, scale=scale)

    rng = np.random.default_rng(seed)
    if weight_seed is None:
        wq = weight(rng)
    else:
        key = ("qbytes", N, K, dt, kind, weight_seed, wscale)
        if key not in _WEIGHT_CACHE:
            _WEIGHT_CACHE[key] = weight(np.random.default_rng(weight_seed))
        wq = _WEIGHT_CACHE[key]
    x = _activations(M, K, dt, rng)
    return dict(x=x, data=wq["data"], scale=wq["scale"], kind=kind, N=N, K=K, dt=dt, wkey=None if weight_seed is None else key)


def qbytes_exact(p, x=None):
    """O.qbytes_mm_exact on a problem of make_qbytes_problem; the float64 image of a cached weight is kept between the Ms of a sweep."""
    x = p["x"] if x is None else x
    key = p.get("wkey")
    if key is None:
        return O.qbytes_mm_exact(x, p["data"], p["scale"], p["kind"])
    if key not in _EXACT_W:
        while len(_EXACT_W) >= 6:
            _EXACT_W.pop(next(iter(_EXACT_W)))
        w = O.fp8_decode(p["data"], p["kind"]).astype(np.float64) if p["kind"] else np.asarray(p["data"]).astype(np.float64)
        _EXACT_W[key] = np.ascontiguousarray(w.T)
    return np.matmul(np.asarray(x, np.float64), _EXACT_W[key]) * np.asarray(p["scale"], np.float64).reshape(1, -1)


def assert_close_to_exact(y: np.ndarray, y_exact: np.ndarray, dt: str, what=""):
    """The parity gate (DESIGN.md "Parity"):

    * fp32 / fp16 outputs: relative Frobenius AND relative max error vs exact math <= 1e-3 (north-star tolerance);
      expected ~1e-6 (fp32) and ~3e-4 (fp16, pure output rounding).
    * bf16 outputs: one bf16 ulp is 3.9e-3, so the gate is "within 1 ulp of the correctly rounded exact result on
      >= 99.5 % of the elements, never more than 2 ulp, and <= 1e-3 Frobenius against that rounded result".
    """
    y = np.asarray(y, np.float64)
    if dt in ("fp32", "fp16"):
        fro, mx = O.rel_fro(y, y_exact), O.rel_max(y, y_exact)
        assert fro <= 1e-3 and mx <= 1e-3, f"{what}: rel_fro={fro:.3e} rel_max={mx:.3e}"
    else:
        target = O.round_to(np.asarray(y_exact, np.float32), dt)
        ulps = O.ulp_distance(y, target, dt)
        frac = float((ulps <= 1).mean())
        fro = O.rel_fro(y, target)
        # tiny outputs (cancellation) can sit many bf16 ulps away while being accurate in absolute terms
        scale_abs = np.abs(y_exact).max()
        big = np.abs(y_exact) > 1e-2 * scale_abs
        assert frac >= 0.995 and ulps[big].max(initial=0) <= 2 and fro <= 1e-3, \
            f"{what}: frac<=1ulp={frac:.4f} max_ulp={ulps[big].max(initial=0)} rel_fro={fro:.3e}"


def assert_close_with_bias(y: np.ndarray, prod_exact: np.ndarray, bias: np.ndarray, dt: str, what=""):
    """Reference order of operations: round the product to ``dt``, add the bias, round again
    (tensor/function.py:45-46, tensor/weights/qbytes.py:79-81).  A 1-ulp difference of the rounded product is
    legitimate (accumulation order), so the bound is one ulp of the product plus one ulp of the result."""
    y = np.asarray(y, np.float64)
    prod = O.round_to(np.asarray(prod_exact, np.float32), dt).astype(np.float64)
    want = O.round_to((prod + bias).astype(np.float32), dt).astype(np.float64)
    eps = {"fp32": 2.0**-23, "fp16": 2.0**-10, "bf16": 2.0**-7}[dt]
    bound = eps * (np.abs(prod) + np.abs(want)) * 1.01 + 1e-30
    bad = np.abs(y - want) > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond 1 ulp(product)+1 ulp(result); max err {np.abs(y - want).max():.3e}"
    assert (y == want).mean() > 0.97, f"{what}: only {(y == want).mean():.4f} identical to the reference sequence"


def projection_bound(abs_sum, n: int, ymax: float):
    """Bound on |sum_j v_j y_j - exact| for a +-1 projection over ``n`` bf16 outputs whose absolute values sum to ``abs_sum`` (a tensor, one
    entry per projected row / pixel): the parity gate's per-element error (2 bf16 ulp of the output plus 1e-2 of the largest output ``ymax``
    for cancelled elements, DESIGN.md "Parity") summed over the projection, with the fp32 accumulation's own slack.  The one formula of the
    Freivalds checks in test_large_operands_gpu.py and test_large_convs_gpu.py."""
    return (2.0 ** -6) * abs_sum + n * (2.0 ** -7) * 1e-2 * ymax + 1e-6 * n * ymax


def assert_similar(a: torch.Tensor, b: torch.Tensor, atol=None, rtol=None):
    """The reference's own similarity check (tests/helpers.py:85-99): cosine similarity ~ 1."""
    assert a.dtype == b.dtype and a.shape == b.shape
    if atol is None:
        atol = torch.finfo(a.dtype).resolution
    if rtol is None:
        rtol = {torch.float32: 1e-5, torch.float16: 1e-3, torch.bfloat16: 1e-1}[a.dtype]
    sim = torch.nn.functional.cosine_similarity(a.flatten().float(), b.flatten().float(), dim=0)
    assert torch.allclose(sim, torch.tensor(1.0, dtype=sim.dtype, device=sim.device), atol=atol, rtol=rtol), \
        f"alignment {float(sim):.8f} deviates from 1"


class observed_activation_scales:
    """Test stand-in for a calibration pass (the reference's ``Calibration`` is host code outside this backend's scope; plug-in mode
    uses the reference's own).  While active, every quantized module with quantized activations takes ``input_scale`` /
    ``output_scale`` = the absmax scale of the tensor it just saw (last batch wins, no running average)."""

    def __enter__(self):
        from torch.nn.modules.module import register_module_forward_hook, register_module_forward_pre_hook

        import optimum_quanto_amd as Q

        def wanted(m):
            return isinstance(m, Q.QModuleMixin) and m.activation_qtype is not None

        def before(m, args):  # global hooks run before the module's own quantize_input / quantize_output hooks
            if wanted(m):
                x = args[0]
                m.input_scale = (torch.max(x._scale) if isinstance(x, Q.ActivationQBytesTensor) else Q.absmax_scale(x, m.activation_qtype)).to(m.input_scale.dtype)

        def after(m, args, out):
            if wanted(m):
                m.output_scale = Q.absmax_scale(out, m.activation_qtype).to(m.output_scale.dtype)

        self.handles = [register_module_forward_pre_hook(before), register_module_forward_hook(after)]
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()


# ---- designed input sets of the elementwise quantize / dequantize tests (test_elementwise_values_cpu.py, test_elementwise_values_gpu.py) ------------------
TARGETS = {"int8": torch.int8, "e4m3fn": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
FINITE_CODES = {"int8": 256, "e4m3fn": 254, "e5m2": 248}  # distinct finite codes of each 8-bit target
# per-tensor scales of the 16-bit sets, each rounded to the dtype: six shared ones, one that makes fp16 quotients overflow / bf16 quotients leave fp32's
# range and one at the other end (a subnormal fp16 scale)
SCALES_16 = {"fp16": (1.0, 0.5, 3.0, 0.0123, 1e-4, 700.0, 6e-8, 60000.0), "bf16": (1.0, 0.5, 3.0, 0.0123, 1e-4, 700.0, 1e-30, 1e30)}
SCALES_32 = (1.0, 2.0 ** -7, 3.0, 0.0123, 1e-4)
AFFINE_SCALES = (1.0, 0.5, 3.0, 0.0123, 0.37)
AFFINE_ROTATIONS = 20  # rotation r gives group g the scale (g + r) % 5 and the shift (g + r) % 4: every group meets the twenty pairs


def scale_tensor(values, dt: str) -> torch.Tensor:
    """The listed scales, rounded to ``dt``."""
    return torch.tensor(values, dtype=torch.float64).to(TORCH_DT[dt])


def finite_values_16(dt: str, limit=None) -> torch.Tensor:
    """Every finite bit pattern of a 16-bit float dtype in bit order (both zeros, every subnormal): 63488 fp16 / 65280 bf16 values; ``limit``: only
    those with |x| <= limit."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(TORCH_DT[dt])
    keep = torch.isfinite(v) if limit is None else v.to(torch.float32).abs() <= limit
    return v[keep].clone()


def value_vector_16(dt: str) -> torch.Tensor:
    """finite_values_16 plus its first three values again: both counts are multiples of 8, and with three more an 8-wide vector straddles two rows of
    the repeated vector, the columns of seven rotations do not fill a vector and the per-tensor launch has a ragged tail."""
    v = finite_values_16(dt)
    return torch.cat([v, v[:3]])


def fp8_boundaries(kind: str) -> np.ndarray:
    """float64: every finite value of the float8 kind (both zeros) and every midpoint between adjacent ones - the points where the code changes."""
    vals = O.fp8_decode(np.arange(256, dtype=np.uint8), kind).astype(np.float64)
    vals = vals[np.isfinite(vals)]
    u = np.unique(vals)
    return np.concatenate([vals, (u[:-1] + u[1:]) / 2])


def symmetric_boundaries(target: str) -> np.ndarray:
    if target == "int8":
        return np.arange(-130, 130, dtype=np.float64) + 0.5
    return fp8_boundaries(target)


def tie_inputs(boundaries: np.ndarray, scale: float, dt: str = "fp32") -> torch.Tensor:
    """fl32(b * s) for every boundary b and its three fp32 neighbours on each side, in one fp32 tensor; for a 16-bit ``dt`` those values rounded to it,
    the ones that leave its finite range dropped (s is then the scale rounded to ``dt``)."""
    s = np.float32(scale_tensor([scale], dt).to(torch.float32).item())
    b = boundaries.astype(np.float32)
    assert (b.astype(np.float64) == boundaries).all(), "boundaries are exact in fp32"
    centre = b * s
    cols = [centre]
    for direction in (-np.inf, np.inf):
        x = centre
        for _ in range(3):
            x = np.nextafter(x, np.float32(direction), dtype=np.float32)
            cols.append(x)
    x = torch.from_numpy(np.stack(cols, axis=1).reshape(-1)).to(TORCH_DT[dt])
    return x[torch.isfinite(x)].clone()


def axis_first_case(dt: str):
    """([8, n] base whose rows are the value vector, [8, 1] scales): n is no multiple of 8, vectors straddle rows."""
    return value_vector_16(dt).repeat(8, 1), scale_tensor(SCALES_16[dt], dt).reshape(8, 1)


def axis_last_case(dt: str):
    """([n, 7] base whose column c is the value vector rotated by 9001 c, [1, 7] scales): 7 does not divide the 8-wide vector."""
    v = value_vector_16(dt)
    return torch.stack([torch.roll(v, 9001 * c) for c in range(7)], dim=1).contiguous(), scale_tensor(SCALES_16[dt][:7], dt).reshape(1, 7)


def affine_case_16(dt: str, bits: int, int_shift: bool, rotation: int = 0):
    """(base [N, 256], scale [2N, 1], shift [2N, 1]) for groups of 128: every finite value with |x| <= 64 in bit order, padded with zeros; group g has
    scale AFFINE_SCALES[(g + r) % 5] and the float shift (0, 0.5 s, 7.5 s, 1.25)[(g + r) % 4] or the zero-point (g + r) % 2^bits."""
    v = finite_values_16(dt, limit=64.0)
    K = 256
    N = -(-v.numel() // K)
    base = torch.zeros(N * K, dtype=v.dtype)
    base[: v.numel()] = v
    g = torch.arange(N * K // 128) + rotation
    s64 = torch.tensor(AFFINE_SCALES, dtype=torch.float64)[g % 5]
    scale = s64.to(v.dtype).reshape(-1, 1)
    if int_shift:
        shift = (g % (1 << bits)).to(torch.uint8).reshape(-1, 1)
    else:
        s = scale.reshape(-1).to(torch.float64)
        table = torch.stack([torch.zeros_like(s), 0.5 * s, 7.5 * s, torch.full_like(s, 1.25)])
        shift = table[g % 4, torch.arange(g.numel())].to(v.dtype).reshape(-1, 1)
    return base.reshape(N, K), scale, shift


def affine_case_32(bits: int, int_shift: bool):
    """fp32 ties of the affine quantizer: for each scale of SCALES_32 two groups of 128 holding fl32((k + 0.5) s), k = -2 .. 2^bits, with three fp32
    neighbours on each side, padded with zeros; group g has the float shift (g % 3) s (the tie moves up by whole codes) or the zero-point g % 2^bits."""
    rows, scales = [], []
    for s in SCALES_32:
        x = tie_inputs(np.arange(-2, (1 << bits) + 1, dtype=np.float64) + 0.5, s)
        assert x.numel() <= 256
        row = torch.zeros(256, dtype=torch.float32)
        row[: x.numel()] = x
        rows.append(row)
        scales += [s, s]
    scale = torch.tensor(scales, dtype=torch.float64).to(torch.float32).reshape(-1, 1)
    g = torch.arange(scale.numel())
    shift = (g % (1 << bits)).to(torch.uint8).reshape(-1, 1) if int_shift else ((g % 3).to(torch.float32).reshape(-1, 1) * scale)
    return torch.stack(rows), scale, shift


def dequantize_codes(numel: int) -> torch.Tensor:
    """uint8: the 256 byte values, tiled to ``numel``."""
    return (torch.arange(numel, dtype=torch.int32) % 256).to(torch.uint8)


def dequantize_scales(dt: str) -> torch.Tensor:
    """Every scale of the 16-bit lists that ``dt`` can hold (fp32: all ten), rounded to it."""
    values = SCALES_16[dt] if dt in SCALES_16 else tuple(dict.fromkeys(SCALES_16["fp16"] + SCALES_16["bf16"]))
    return scale_tensor(values, dt)


# ---- fused output quantization (tests/test_*output_fusion_*.py): what the files of the three products share ---------------------------------------------
OK, EINVAL, ENOTSUP, EALIGN = 0, -1, -2, -4  # QUANTO_HIP_* statuses (include/quanto_hip.h)
F32, F16, BF16, I8, U8, E4M3, E5M2, E4M3FNUZ = range(8)  # quanto_hip_dtype
CODE_DTYPES = {"int8": torch.int8, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
CODE_QMAX = {torch.int8: 127.0, torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}
SENTINEL = 0xA5


def full_range_codes(dtype, shape, gen):
    """Codes over the full range of ``dtype`` (float8: every finite bit pattern, the non-finite ones replaced by zero)."""
    if dtype == torch.int8:
        return torch.randint(-128, 128, shape, dtype=torch.int8, generator=gen)
    bits = torch.randint(0, 256, shape, dtype=torch.int16, generator=gen).to(torch.uint8)
    finite = torch.isfinite(bits.view(dtype).to(torch.float32))
    return torch.where(finite, bits, torch.zeros_like(bits)).view(dtype)


def quantile_out_scale(y, dtype):
    """The 0.9-quantile of |y| over the largest code of ``dtype``, in y's dtype: an output scale at which the sequence itself clamps."""
    return (torch.quantile(y.abs().to(torch.float32).reshape(-1), 0.9) / CODE_QMAX[dtype]).to(y.dtype)


def clamped_share(y, out_scale, dtype):
    """Share of the elements of ``y`` the sequence clamps at ``out_scale``."""
    return ((y / out_scale).to(torch.float32).abs() > CODE_QMAX[dtype]).to(torch.float32).mean().item()


def sentinel_buffer(nbytes, offset, device):
    """(buffer, lead): ``nbytes`` of output at byte ``lead`` = 256 + offset of a 256-byte aligned buffer filled with SENTINEL, 4096 bytes behind it."""
    lead = 256 + offset
    buf = torch.full((lead + nbytes + 4096,), SENTINEL, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 256 == 0
    return buf, lead


def assert_nothing_outside(buf, lead, nbytes, what):
    assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + nbytes:] == SENTINEL).all()), f"bytes outside {what} were written"

"""Designed problems for the exact-route tests (tests/test_exact_routes_cpu.py, tests/test_exact_routes_gpu.py): every matmul and convolution row of
tests/containment_cases.py on inputs whose arithmetic is exact in fp32 whatever the order of accumulation, so that every route - split or unsplit,
folded or dequantize-first - must return the bits of float64 math rounded once to the output type.

Two designs per row and variant (``variants``: the row's own formats, the other 16-bit type, every 8-bit weight type of the header the plan accepts):

* pass "A", decode: one-hot activations (a single 1.0, or the code of 1 at activation scale 1) select one weight column per activation row; the
  launches of a row sweep the selection over every column.  The weight codes rotate so that the selected columns show every code (8-bit types: every
  finite byte value, int8 -128 included; int4 / int2: every value at every position inside a packed byte).  The expected output is the oracle's decode
  of that element times its scale.
* pass "B", dense: integer activations with a mean (0..3, some rows negated; int8 codes over the full range for the 8-bit activation routes), all weight
  codes (fp8: the window of codes that keeps the bound; float8 x float8: also ``PIPE_SPAN``), run once without and once with an integer-valued bias.

Scales are powers of two that differ between neighbouring rows and groups (2^-((n + 2 g) mod 5)); float shifts are zero-points times the scale, the
zero-points rotating over 0, 2^bits - 1 and interior values.

The exactness bound (``Bound``, asserted on the host): with u[n] the smallest power of two every product x w[n, k] is a multiple of,
sum_k |x_k| |w_nk| < 2^24 u[n] for every output, and the same for the two terms of the folded form (sum |x| scale q and sum |x| shift) on their own.
Every fp32 partial sum of such a problem is an integer multiple of u below 2^24 u: exact, in any order.
"""
import contextlib
import os
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

import containment_cases as C
from helpers import TORCH_DT, to_torch
from oracle import quanto_oracle as O

MAX_LAUNCHES = 512
ENTRIES = ("qbits_mm", "qbytes_mm_ws", "qbits_mm_multi_ws", "qbytes_mm_multi_ws", "qbits_mm_a8", "qbytes_bmm", "qbytes_conv2d",
           "qbytes_conv2d_depthwise", "qbits_conv2d", "qbytes_conv2d_a8")
GROUPS = {e: C.GROUPS[e] for e in ENTRIES}
ROWS = [r for e in ENTRIES for r in GROUPS[e]]
# the 8-bit weight types include/quanto_hip.h defines for each entry whose rows are run at every weight type (the convolution entries have no plan entry
# that looks at the type: the header's list is the rule there)
WEIGHT_TYPES = {"qbytes_mm_ws": ("int8", "e4m3fn", "e5m2", "e4m3fnuz"), "qbytes_mm_multi_ws": ("int8", "e4m3fn", "e5m2", "e4m3fnuz"),
                "qbytes_conv2d": ("int8", "e4m3fn", "e5m2"), "qbytes_conv2d_depthwise": ("int8", "e4m3fn", "e5m2")}
ZERO_POINTS = {4: (0, 15, 8, 3, 11, 7, 1), 2: (0, 3, 1, 2, 3, 0, 2)}  # seven each: the rotation (n + 3 g) mod 7 shares no period with tiles or scales
SCALE_STEPS = 5                                                        # scales 2^0 .. 2^-4

# What a route rounds by design before its last rounding, and therefore where pass B does not expect "float64 rounded once".  One entry, no route of
# its own: with power-of-two scales no route rounds a weight, a partial sum or a scaled product to a non-representable value (DESIGN.md "Parity").
ROUNDS_BY_DESIGN = [
    dict(what="bias on a 16-bit output",
         applies=lambda dt, bias: bias and dt != "fp32",
         expected="round(round(product) + bias): the product is rounded to the output type, the bias is added in fp32, the sum is rounded again",
         # round_add_round, the copy of the rule every product epilogue calls - and the one epilogue that keeps the statements inline, for the
         # measurement its comment records (n8::epilogue).  tests/test_exact_routes_cpu.py: no other file under csrc/ holds the expression.
         cites=("csrc/qh_common.h:60", "csrc/qmm_native8.hip:216"),
         why="the two-op order of the reference (a product in the output dtype, then `out + bias`: tensor/function.py:45-46, tensor/weights/qbytes.py:79-81), "
             "which include/quanto_hip.h promises bit for bit ('rounded product plus bias, rounded again') and the registered default ops compute; the fp32 "
             "entries add the bias to the fp32 product, which is exact here.  The bias launch is still compared bit for bit, against this order."),
]


# Routes exempted from the bit comparison of pass B (they still run pass A, and pass B under the gate they have elsewhere in the suite,
# helpers.assert_close_to_exact / assert_close_with_bias).  Each entry is a finding (DESIGN.md "Parity") with the keys entry, name (the kernel of the
# row), cite ("csrc/file.hip:line", the line where the route rounds an intermediate by design), why and measured.  None: with power-of-two scales no
# route rounds an intermediate on these problems.
EXEMPT: List[dict] = []

# The bound below speaks of fp32 additions.  float8 x float8 routes (mfma_native8, conv2d_a8_fp8) hand 128 products at a time to ONE MX-format matrix
# instruction (csrc/qconv_a8.hip:290, include/quanto_hip.h: "the fp32 matrix-pipe sum of exact products"), and that sum is not a chain of fp32 additions:
# the instruction keeps fewer bits below its largest product than an fp32 would, so a problem that meets the bound can still lose low bits of far-apart
# products inside the instruction.  That is a property of the instruction, not of a kernel: with pass B's window at the full width the bound allows for
# K = 45 .. 360 (codes spanning up to 2^17), 0.7 - 2 % of a convolution's bf16 outputs were one ulp off on an MI355X, fewer at a span of 2^14, none at
# 2^12 and below - and the matmul rows, whose K >= 512 keeps the window of the bound itself narrow, were bit-exact throughout.  So that the arithmetic of
# these routes is exact as well, their pass B takes float8 codes no further than PIPE_SPAN apart (largest value over smallest unit); with |x| <= 3 every
# product of an output then lies within PIPE_WINDOW of the unit u: the products span what the codes alone spanned where no bit was lost.  Asserted per row on
# the host next to the bound (``Bound`` "matrix-pipe window").  Pass A is not concerned: one product per output.
FP8_KINDS = ("e4m3fn", "e5m2", "e4m3fnuz")
PIPE_SPAN = 2.0 ** 10
PIPE_WINDOW = 2.0 ** 12


def pipe_span(akind, wkind):
    """PIPE_SPAN where activations and weights are both float8 codes (the products are summed by the MX-format matrix instruction), no limit elsewhere."""
    return PIPE_SPAN if akind in FP8_KINDS and wkind in FP8_KINDS else np.inf


def exempted(row):
    """The EXEMPT entry of a row (or variant), None for all others."""
    for e in EXEMPT:
        if (row.entry, row.name) == (e["entry"], e["name"]):
            return e
    return None


class Bound(NamedTuple):
    what: str
    worst: float   # max over the outputs of sum |x| |w| / (2^24 u): below 1


class Design(NamedTuple):
    launches: int
    static: Dict[str, torch.Tensor]                              # regions uploaded once
    acts: Callable[[int, int], Dict[str, torch.Tensor]]          # the activation regions of launches [l0, l1): name -> [l1 - l0, ...]
    sets: Dict[str, torch.Tensor]                                # regions that exist once per weight set: name -> [sets, ...]
    set_of: Callable[[int], int]                                 # launch -> weight set
    bias_on: Callable[[int], bool]                               # launch -> the bias pointers are passed
    outputs: Dict[str, Tuple[torch.dtype, tuple]]
    want: Callable[[int, int], Dict[str, np.ndarray]]            # launches [l0, l1) -> name -> float32 [l1 - l0, *shape]
    bounds: List[Bound]
    facts: dict                                                  # what the host file asserts about the design (coverage)
    default_op: Optional[Callable[[int], Dict[str, torch.Tensor]]]  # launch -> the registered op's outputs on the host
    exact: Optional[Callable[[int], Dict[str, tuple]]] = None    # pass B: launch -> name -> (the float64 product, the bias or None)


# ---- variants ------------------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def knobs(row):
    """The row's QUANTO_HIP_* knobs in the environment (containment_cases.knobs_env for code that has no monkeypatch at hand)."""
    old = {k: os.environ.get(k) for k, _ in row.knobs}
    try:
        for k, v in row.knobs:
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _with(row, tag, **changes):
    f = row.f
    f.update(changes)
    return row._replace(id=f"{row.id}~{tag}", fmt=tuple(sorted(f.items())))


def _same_route(row, v):
    fam = C.family(row)
    a, b = fam.plan(row), fam.plan(v)
    if b.status != C.OK or a.kernel != b.kernel:
        return False
    if hasattr(fam, "member_kernels") and a.kernel == C.AUTO:
        return fam.member_kernels(row) == fam.member_kernels(v)
    return True


def variants(row) -> list:
    """The row, the row at the other 16-bit type (rows with 16-bit activations) and each of them at every other 8-bit weight type of the header - where the
    plan entry answers OK and the same kernel.  Call under the row's knobs."""
    f, out = row.f, [row]
    if row.entry != "qbytes_bmm" and f.get("a", f["dt"]) in ("bf16", "fp16"):
        other = "fp16" if f["dt"] == "bf16" else "bf16"
        out.append(_with(row, other, dt=other, **({"a": other} if "a" in f else {})))
    for v in list(out):
        out += [_with(v, b, b=b) for b in WEIGHT_TYPES.get(row.entry, ()) if b != f["b"]]
    return [v for v in out if v is row or _same_route(row, v)]


# ---- numbers -------------------------------------------------------------------------------------------------------------------------------------------------
def lowbit(v):
    """The value of the lowest set bit of each float64 (inf for 0)."""
    m, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    i = (m * 2.0 ** 53).astype(np.int64)
    return np.where(i == 0, np.inf, (i & -i).astype(np.float64) * 2.0 ** (e.astype(np.float64) - 53))


def _rd(v64, dt):
    v32 = np.asarray(v64, np.float64).astype(np.float32)
    assert (v32.astype(np.float64) == v64).all(), "the exact value has more than 24 bits: the design is not exact in fp32"
    assert np.abs(v32).max(initial=0) <= {"fp16": 65504.0}.get(dt, 3e38), "the exact value leaves the output type's range"
    return O.round_to(v32, dt)


def expect(product64, dt, bias=None):
    """float64 math rounded once to ``dt``; with a bias on a 16-bit output the order of ROUNDS_BY_DESIGN."""
    if bias is None:
        return _rd(product64, dt)
    if not ROUNDS_BY_DESIGN[0]["applies"](dt, True):
        return _rd(product64 + bias, dt)
    return _rd(_rd(product64, dt).astype(np.float64) + bias, dt)


def byte_values(kind):
    """Every byte of an 8-bit type that is a number: all 256 for int8, the finite codes of a float8 type."""
    b = np.arange(256, dtype=np.uint8)
    return b if kind == "int8" else b[np.isfinite(O.fp8_decode(b, kind))]


def decode(byte, kind):
    return byte.view(np.int8).astype(np.float64) if kind == "int8" else O.fp8_decode(byte, kind).astype(np.float64)


def bounded_bytes(kind, abs_x_sum, dt, span=np.inf):
    """Pass B: the largest set of float8 codes {lowbit >= u, |v| abs_x_sum < 2^24 u} - every sum of abs_x_sum worth of |x| over them stays exact - that
    also keeps such a sum inside the range of an fp16 output and, where ``span`` is given, no value above span * u (PIPE_SPAN)."""
    b = byte_values(kind)
    if kind == "int8":
        return b
    v = np.abs(decode(b, kind))
    low = lowbit(v)
    fits = v * abs_x_sum < (65504.0 if dt == "fp16" else np.inf)
    keep = lambda u: fits & (low >= u) & (v * abs_x_sum < 2.0 ** 24 * u) & (v <= span * u)  # noqa: E731
    return b[keep(max(np.unique(low[np.isfinite(low)]), key=lambda u: int(keep(u).sum())))]


class Weight(NamedTuple):
    regions: Dict[str, torch.Tensor]   # packed / scale / shift, or data / scales
    w64: np.ndarray                    # [N, K]: the dequantized weight, exact
    parts: List[np.ndarray]            # [N, K] each: |terms| whose sums over |x| must stay below 2^24 u
    u: np.ndarray                      # [N]
    codes: np.ndarray                  # [N, K]: the stored code of each element
    pos: np.ndarray                    # [N, K]: its position inside a packed byte (0 for 8-bit types)
    zp: Optional[np.ndarray]           # [N, K]: the zero-point of its group
    ncodes: int
    scale64: Optional[np.ndarray] = None  # [N, K]: the scale of each element (packed weights)


def _pot(n, g=0):
    return 2.0 ** -((n + 2 * g) % SCALE_STEPS)


def qbytes_weight(N, K, kind, dt, off=0, allowed=None) -> Weight:
    ids = byte_values(kind) if allowed is None else allowed
    n, k = np.ogrid[:N, :K]
    byte = np.ascontiguousarray(ids[(off + n + (N | 1) * k) % len(ids)], dtype=np.uint8)  # an odd stride: a row does not cycle through a few codes
    dec, s = decode(byte, kind), _pot(np.arange(N))
    u = s * lowbit(dec).min(axis=1)
    data = byte.view(np.int8) if kind == "int8" else byte
    return Weight({"data": torch.from_numpy(data), "scales": to_torch(s.reshape(N, 1), dt)}, dec * s[:, None], [np.abs(dec) * s[:, None]], u, byte,
                  np.zeros((N, K), np.int64), None, len(byte_values(kind)))


# Routes that multiply the reference's dequantized weight, rounded to the activation type (include/quanto_hip.h: DEQUANT_MFMA, MFMA_LARGE4 and
# quanto_hip_qbits_conv2d).  With zero-points below 2^bits that rounding never rounds; pass "C" gives these routes float shifts of 384 (bf16) / 3072
# (fp16) scales and more, so that scale * (q - shift / scale) needs one bit more than the type has and every odd code is a TIE of the rounding - the
# expected output is the exact product with the weight rounded to nearest even, as the header promises, rounded once.
ROUNDED_WEIGHT_ROUTES = ("mfma_large4", "dequant_mfma", "conv2d_mfma_int4", "conv2d_mfma_int2", "conv2d_rows_dequant_int4", "conv2d_rows_dequant_int2")
BIG_SHIFTS = {"bf16": (384, 320, 448), "fp16": (3072, 2560, 3584)}


def passes(row):
    return ("A", "B", "C") if row.name in ROUNDED_WEIGHT_ROUTES and "multi" not in row.entry else ("A", "B")


def qbits_weight(N, K, bits, gs, dt, off=0, rounded=False) -> Weight:
    cols = gs or K
    G, vpi = K // cols, 8 // bits
    R = N * G
    n, k = np.ogrid[:N, :K]
    g = k // cols
    q = ((off + n + 5 * k) % (1 << bits)).astype(np.uint8)
    s = _pot(n, g) * (2.0 ** -6 if rounded and dt == "fp16" else 1.0)  # (pass C at fp16: sums of 3072-scale weights stay inside the type)
    zp = np.asarray(BIG_SHIFTS[dt] if rounded else ZERO_POINTS[bits], np.int64)[(n + 3 * g) % (3 if rounded else 7)]
    sg, zg = s[:, ::cols], zp[:, ::cols]  # [N, G]
    row_dim = -(-R // vpi)
    pos = (n * G + g) // row_dim
    regions = {"packed": torch.from_numpy(O.pack_weights(q.reshape(R, cols), bits)), "scale": to_torch(sg.reshape(R, 1), dt),
               "shift": to_torch((sg * zg).reshape(R, 1), dt)}
    w64 = s * (q.astype(np.float64) - zp)
    if rounded:  # the weight these routes multiply: round(round(scale q) - shift) in dt (tensor/qbits.py:27-49), half of it ties
        w64 = O.round_to(w64.astype(np.float32), dt).astype(np.float64)
        assert (w64 != s * (q.astype(np.float64) - zp)).mean() > 0.4
        return Weight(regions, w64, [np.abs(w64)], lowbit(w64).min(axis=1), q, pos, None, 1 << bits)
    return Weight(regions, w64, [np.abs(w64), s * q, s * zp], sg.min(axis=1), q, pos, zp, 1 << bits, s * np.ones((N, K)))


def dense_values(shape, rng, signed_axis):
    """Integers 0..3 with every eighth slice along ``signed_axis`` (from the fourth on) negated: a mean of about 1.1, never a -0."""
    x = rng.integers(0, 4, size=shape).astype(np.float64)
    idx = [slice(None)] * len(shape)
    idx[signed_axis] = slice(3, None, 8)
    x[tuple(idx)] *= -1
    return x + 0.0


def dense_int8(shape, rng):
    x = rng.integers(-128, 128, size=shape, dtype=np.int8)
    x.reshape(-1)[[0, -1]] = -128
    x.reshape(-1)[1] = 127
    return x


def act_tensor(values, kind):
    """Host tensor of the activation type ``kind`` holding ``values`` (exact): float type, int8 codes or float8 codes."""
    if kind in TORCH_DT:
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(TORCH_DT[kind])
    if kind == "int8":
        return torch.from_numpy(np.ascontiguousarray(values).astype(np.int8))
    codes = O.fp8_encode(np.asarray(values, np.float32), kind)
    assert (O.fp8_decode(codes, kind).astype(np.float64) == values).all()
    return torch.from_numpy(codes)


def _bias(N):
    return ((np.arange(N) * 7) % 23 - 11).astype(np.float64)


def _pipe_bound(xv, w):
    """max |x| max_k |w[n, k]| against PIPE_WINDOW u[n]: every product of an output within the window the matrix instruction adds exactly."""
    return Bound("matrix-pipe window", float((np.abs(xv).max() * np.abs(w.w64).max(axis=1) / (PIPE_WINDOW * w.u)).max()))


def _bound(what, abs_sums, u):
    """abs_sums [..., N] (N last) against 2^24 u[N]."""
    return Bound(what, float((abs_sums / (2.0 ** 24 * u)).max()))


# ---- matmul entries ------------------------------------------------------------------------------------------------------------------------------------------
def _mm_design(row, pas) -> Design:
    f, e = row.f, row.entry
    multi, qbits = "multi" in e, e.startswith("qbits")
    M, Ns, K = row.shape
    Ns = list(Ns) if multi else [Ns]
    dt = f["dt"]
    akind = f.get("a", dt)
    xname = "x" if e in ("qbits_mm", "qbits_mm_multi_ws") else "a"
    sfx = [str(i) for i in range(len(Ns))] if multi else [""]
    a8 = e == "qbits_mm_a8"
    rng = np.random.default_rng(C._seed(row))
    if pas != "A":
        xv = dense_int8((M, K), rng).astype(np.float64) if akind == "int8" else dense_values((M, K), rng, 0)
    abs_x_sum = K * (128 if akind == "int8" else 3)
    ws = []
    for i, N in enumerate(Ns):
        if qbits:
            ws.append(qbits_weight(N, K, f["bits"], 128 if a8 else f["gs"], dt, off=3 * i, rounded=pas == "C"))
        else:
            ws.append(qbytes_weight(N, K, f["b"], dt, off=41 * i, allowed=bounded_bytes(f["b"], abs_x_sum, dt, pipe_span(akind, f["b"])) if pas == "B" else None))
    int_rule = not qbits and akind == "int8" and f["b"] == "int8"  # oracle.qbytes_int_mm_ref: the int32 sum, one rounding to fp32, times the scale
    a_scale = (1.0 if pas == "A" else 0.125) if a8 else 1.0
    static = {}
    for w, s in zip(ws, sfx):
        names = {"packed": "packed", "scale": "scale", "shift": "shift", "data": "b", "scales": "scales"}
        static.update({names[k] + s: v for k, v in w.regions.items()})
        if pas != "A":
            static["bias" + s] = to_torch(_bias(w.w64.shape[0]), dt)
    if a8:
        static["a_scale"] = to_torch(np.array([a_scale]), dt)
    outputs = {"y" + s: (TORCH_DT[dt], (M, N)) for s, N in zip(sfx, Ns)}

    if pas == "A":
        L = min(MAX_LAUNCHES, -(-K // M))
        ks = (np.arange(L)[:, None] * M + np.arange(M)[None, :]) % K  # [L, M]

        def acts(l0, l1):
            x = np.zeros((l1 - l0, M, K), np.float32)
            x[np.arange(l1 - l0)[:, None], np.arange(M)[None, :], ks[l0:l1]] = 1.0
            return {xname: act_tensor(x, akind)}

        def want(l0, l1):
            return {"y" + s: expect(w.w64.T[ks[l0:l1]] * a_scale, dt) for w, s in zip(ws, sfx)}

        sel = np.unique(ks)
        facts = dict(columns=sel, K=K, weights=[(w, [sel]) for w in ws])
        bounds = []
    else:
        L = 2

        def acts(l0, l1):
            return {xname: act_tensor(np.broadcast_to(xv, (l1 - l0, M, K)), akind)}

        def product(w):
            acc = xv @ w.w64.T
            if int_rule:  # w64 = code * 2^-j: the integer sum, rounded to fp32, then scaled
                s = _pot(np.arange(w.w64.shape[0]))
                assert np.abs(acc / s).max() < 2 ** 31
                acc = (acc / s).astype(np.float32).astype(np.float64) * s
            return acc * a_scale

        def want(l0, l1):
            return {"y" + s: np.stack([expect(product(w), dt, _bias(w.w64.shape[0]) if l == 1 else None) for l in range(l0, l1)])
                    for w, s in zip(ws, sfx)}

        facts = dict(weights=[(w, [np.arange(K)]) for w in ws], x=xv)
        bounds = [] if int_rule else [_bound(f"member {i} term {t}", np.abs(xv) @ part.T, w.u) for i, w in enumerate(ws) for t, part in enumerate(w.parts)]
        if not qbits and np.isfinite(pipe_span(akind, f["b"])):
            bounds += [_pipe_bound(xv, w) for w in ws]
        if row.name == "mfma_fused4":  # its matrix operand is OFFSET + q (csrc/qbits_mfma_fused.hip: 128 in bf16, 1024 in fp16), the shift term takes it back
            o, w = {"bf16": 128.0, "fp16": 1024.0}[dt], ws[0]
            bounds += [_bound(f"offset term {t}", np.abs(xv) @ part.T, w.u) for t, part in enumerate([w.scale64 * (w.codes + o), w.scale64 * (w.zp + o)])]

    def default_op(l):
        x = acts(l, l + 1)[xname][0]
        outs = {}
        for w, s in zip(ws, sfx):
            bias = static["bias" + s] if pas != "A" and l == 1 else None
            if qbits:
                args = (static["packed" + s], static["scale" + s], static["shift" + s], bias, f["bits"], (128 if a8 else f["gs"]) or None, w.w64.shape[0], K)
                xa = x.view(C_FP8[akind]) if akind in C_FP8 else x
                outs["y" + s] = torch.ops.quanto.qbits_mm_a8(xa, static["a_scale"], *args) if a8 else torch.ops.quanto.qbits_mm(xa, *args)
            else:
                b = static["b" + s] if f["b"] == "int8" else static["b" + s].view(C_FP8[f["b"]])
                xa = x.view(C_FP8[akind]) if akind in C_FP8 else x
                outs["y" + s] = torch.ops.quanto.qbytes_mm_bias(xa, b, static["scales" + s], bias)
        return outs

    exact = None if pas == "A" else lambda l: {"y" + s: (product(w), _bias(w.w64.shape[0]) if l == 1 else None) for w, s in zip(ws, sfx)}
    return Design(L, static, acts, {}, lambda l: 0, lambda l: pas != "A" and l == 1, outputs, want, bounds, facts, default_op, exact)


C_FP8 = {"e4m3fn": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2, "e4m3fnuz": torch.float8_e4m3fnuz}


# ---- qbytes_bmm ----------------------------------------------------------------------------------------------------------------------------------------------
BMM_SCALE = 2.0 ** -6


def _bmm_design(row, pas) -> Design:
    (B, M, N, K), f = row.shape, row.f
    dt = f["dt"]
    rng = np.random.default_rng(C._seed(row))
    ids = byte_values("int8")
    b_, n, k = np.ogrid[:B, :N, :K]
    wb = np.ascontiguousarray(ids[(b_ * 97 + n + N * k) % 256], dtype=np.uint8)  # [B, N, K] bytes
    w = wb.view(np.int8)
    stored = np.ascontiguousarray(w.transpose(0, 2, 1)) if f["layout"] == "NN" else w  # NN: [B, K, N], N contiguous; NT: [B, N, K]
    static = {"w": torch.from_numpy(stored), "scale": torch.tensor([BMM_SCALE], dtype=torch.float32)}
    outputs = {"y": (TORCH_DT[dt], (B, M, N))}
    w64 = w.astype(np.float64)

    def rule(acc):
        assert np.abs(acc).max() < 2 ** 31
        return expect(acc.astype(np.float32).astype(np.float64) * BMM_SCALE, dt)

    if pas == "A":
        L = min(MAX_LAUNCHES, -(-K // M))
        ks = (np.arange(L)[:, None, None] * M + np.arange(M)[None, None, :] + 7 * np.arange(B)[None, :, None]) % K  # [L, B, M]

        def acts(l0, l1):
            a = np.zeros((l1 - l0, B, M, K), np.int8)
            a[np.arange(l1 - l0)[:, None, None], np.arange(B)[None, :, None], np.arange(M)[None, None, :], ks[l0:l1]] = 1
            return {"a": torch.from_numpy(a)}

        def want(l0, l1):
            return {"y": rule(np.stack([np.stack([w64[b].T[ks[l, b]] for b in range(B)]) for l in range(l0, l1)]))}

        facts = dict(columns=np.unique(ks), K=K, weights=[(_codes_only(wb[b], 256), [np.unique(ks[:, b])]) for b in range(B)])
    else:
        L = 1
        av = dense_int8((B, M, K), rng)

        def acts(l0, l1):
            return {"a": torch.from_numpy(np.broadcast_to(av, (l1 - l0, B, M, K)).copy())}

        def want(l0, l1):
            return {"y": np.stack([rule(np.matmul(av.astype(np.float64), w64.transpose(0, 2, 1)))] * (l1 - l0))}

        facts = dict(weights=[(_codes_only(wb[b], 256), [np.arange(K)]) for b in range(B)], x=av)

    def default_op(l):
        wt = torch.from_numpy(w).transpose(1, 2)  # [B, K, N]
        return {"y": torch.ops.quanto.qbytes_bmm(acts(l, l + 1)["a"][0], wt, static["scale"], TORCH_DT[dt])}

    exact = None if pas == "A" else lambda l: {"y": (np.matmul(av.astype(np.float64), w64.transpose(0, 2, 1)) * BMM_SCALE, None)}
    return Design(L, static, acts, {}, lambda l: 0, lambda l: False, outputs, want, [], facts, default_op, exact)


def _codes_only(codes, ncodes):
    z = np.zeros(codes.shape, np.int64)
    return Weight({}, None, [], None, codes, z, None, ncodes)


# ---- convolution entries -------------------------------------------------------------------------------------------------------------------------------------
def _positions(g):
    """Input pixels of the one-hot sweep: one per stride phase around the centre (between them every tap of the window meets an output pixel) and two
    corners (windows that hang into the padding)."""
    h0, w0 = g.H // 2, g.W // 2
    return [(h0 + i, w0 + j) for i in range(g.s[0]) for j in range(g.s[1])] + [(0, 0), (g.H - 1, g.W - 1)]


def _unfold(x64, g):
    """im2col of [B, C, H, W]: [B, C, KH * KW, OH * OW]."""
    cols = torch.nn.functional.unfold(torch.from_numpy(x64), (g.KH, g.KW), g.d, g.p, g.s)
    return cols.reshape(x64.shape[0], x64.shape[1], g.KH * g.KW, -1).numpy()


def _conv_design(row, pas) -> Design:
    g, f, e = row.shape, row.f, row.entry
    dw, qbits, a8 = e == "qbytes_conv2d_depthwise", e == "qbits_conv2d", e == "qbytes_conv2d_a8"
    dt = f["dt"]
    akind = f["a"] if a8 else dt
    taps = g.KH * g.KW
    Kw = taps if dw else g.K                      # columns of the weight matrix [OC, Kw]
    groups, mult = (g.cin, g.OC // g.cin) if dw else (1, 1)
    wshape = (g.OC, 1 if dw else g.cin, g.KH, g.KW)
    rng = np.random.default_rng(C._seed(row))
    abs_x_sum = Kw * (128 if akind == "int8" else 3)
    a_scale = (1.0 if pas == "A" else 0.125) if a8 else 1.0
    int_rule = a8 and akind == "int8"
    allowed = None if qbits else bounded_bytes(f["b"], abs_x_sum, dt, pipe_span(akind, f["b"])) if pas == "B" else byte_values(f["b"])
    nsets = 1 if qbits else -(-len(allowed) // (g.OC * Kw))  # a depthwise weight is smaller than the set of codes: several weights, one per launch

    def weight(i):
        if qbits:
            return qbits_weight(g.OC, Kw, f["bits"], f["gs"], dt, off=3 * i, rounded=pas == "C")
        return qbytes_weight(g.OC, Kw, f["b"], dt, off=i * g.OC * Kw, allowed=allowed)

    ws = [weight(i) for i in range(nsets)]
    names = {"packed": "packed", "scale": "scale", "shift": "shift", "data": "w", "scales": "w_scale" if a8 else "scales"}
    static = {names[k]: v for k, v in ws[0].regions.items() if k != "data" or nsets == 1}
    sets = {"w": torch.stack([w.regions["data"] for w in ws])} if nsets > 1 else {}
    if a8:
        static["a_scale"] = to_torch(np.array([a_scale]), dt)
    if pas != "A":
        static["bias"] = to_torch(_bias(g.OC), dt)
    outputs = {"y": (TORCH_DT[dt], (g.B, g.OC, g.OH, g.OW))}
    chan = lambda v: np.asarray(v).reshape(1, -1, 1, 1)  # noqa: E731
    set_of = (lambda l: l % nsets) if pas == "A" else (lambda l: l // 2)  # noqa: E731
    bias_on = lambda l: pas != "A" and l % 2 == 1  # noqa: E731

    def product(x64, w):
        """[b, OC, OH, OW], exact: integer (or float8) values in float64; then the rule of the entry."""
        acc = C._conv64(x64, w.w64.reshape(wshape), g, groups)
        if int_rule:  # sc[n] = a_scale * w_scale[n], a power of two; the int32 sum rounded to fp32 first (oracle.qbytes_int_mm_ref on the im2col)
            s = chan(_pot(np.arange(g.OC)))
            assert np.abs(acc / s).max() < 2 ** 31
            acc = (acc / s).astype(np.float32).astype(np.float64) * s
        return acc * a_scale

    def x_tensor(values):
        return act_tensor(values, akind)

    if pas == "A":
        pos = _positions(g)
        per_set = -(-g.cin * len(pos) // g.B)
        L = nsets * per_set
        assert L <= MAX_LAUNCHES

        def pixel(l, b):
            t = (l // nsets) * g.B + b
            return t % g.cin, pos[(t // g.cin) % len(pos)]

        def values(l0, l1):
            x = np.zeros((l1 - l0, g.B, g.cin, g.H, g.W), np.float64)
            for l in range(l0, l1):
                for b in range(g.B):
                    c, (h, w_) = pixel(l, b)
                    x[l - l0, b, c, h, w_] = 1.0
            return x

        def acts(l0, l1):
            return {"x": x_tensor(values(l0, l1))}

        def want(l0, l1):
            x = values(l0, l1)
            return {"y": np.stack([expect(product(x[l - l0], ws[l % nsets]), dt) for l in range(l0, l1)])}

        # the weight columns each set's launches select: (channel, tap) pairs whose im2col column is not empty
        selected = []
        for i in range(nsets):
            ls = [l for l in range(L) if l % nsets == i]
            hit = np.zeros((g.cin, taps), bool)
            for l in ls:
                hit |= (_unfold(values(l, l + 1)[0], g) != 0).any(axis=(0, 3))
            if dw:  # weight row oc reads channel oc // mult: its columns are the taps that channel selected
                selected.append([np.flatnonzero(hit[oc // mult]) for oc in range(g.OC)])
            else:
                selected.append([np.flatnonzero(hit.reshape(-1))])
        facts = dict(columns=np.flatnonzero(np.logical_or.reduce([hit_all(s, Kw) for s in selected])), K=Kw,
                     weights=[(w, s) for w, s in zip(ws, selected)])
        bounds = []
    else:
        L = 2 * nsets  # each weight set without and with the bias
        xv = dense_int8((g.B, g.cin, g.H, g.W), rng).astype(np.float64) if akind == "int8" else dense_values((g.B, g.cin, g.H, g.W), rng, 3)

        def acts(l0, l1):
            return {"x": x_tensor(np.broadcast_to(xv, (l1 - l0,) + xv.shape))}

        def want(l0, l1):
            return {"y": np.stack([expect(product(xv, ws[l // 2]), dt, chan(_bias(g.OC)) if l % 2 else None) for l in range(l0, l1)])}

        facts = dict(weights=[(w, [np.arange(Kw)]) for w in ws], x=xv)
        sums = lambda part: C._conv64(np.abs(xv), part.reshape(wshape), g, groups).transpose(0, 2, 3, 1)  # noqa: E731
        bounds = [] if int_rule else [_bound(f"set {i} term {t}", sums(part), w.u) for i, w in enumerate(ws) for t, part in enumerate(w.parts)]
        if not qbits and np.isfinite(pipe_span(akind, f["b"])):
            bounds += [_pipe_bound(xv, w) for w in ws]

    def default_op(l):
        """The registered op without its bias, the bias added to its output: F.conv2d, which the default ops hand the bias to, adds it before its one
        rounding on some host backends and after it on others - the two-op order is the one the kernels and the header promise."""
        x = acts(l, l + 1)["x"][0]
        geo = (list(g.s), list(g.p), list(g.d))
        if qbits:
            y = torch.ops.quanto.qbits_conv2d(x, static["packed"], static["scale"], static["shift"], None, f["bits"], f["gs"] or None, list(wshape), *geo)
        else:
            w = ws[set_of(l)].regions["data"].reshape(wshape)
            w = w if f["b"] == "int8" else w.view(C_FP8[f["b"]])
            if a8:
                xa = x.view(C_FP8[akind]) if akind in C_FP8 else x
                y = torch.ops.quanto.qbytes_conv2d_a8(xa, static["a_scale"], w, static["w_scale"], None, *geo)
            else:
                y = torch.ops.quanto.qbytes_conv2d(x, w, static["scales"], None, *geo)
        return {"y": y + static["bias"].reshape(1, -1, 1, 1) if bias_on(l) else y}

    exact = None if pas == "A" else lambda l: {"y": (product(xv, ws[l // 2]), chan(_bias(g.OC)) if l % 2 else None)}
    return Design(L, static, acts, sets, set_of, bias_on, outputs, want, bounds, facts, default_op, exact)


def hit_all(selected, K):
    m = np.zeros(K, bool)
    for s in selected:
        m[s] = True
    return m


# ---- the table -----------------------------------------------------------------------------------------------------------------------------------------------
def design(row, pas) -> Design:
    """The designed problem of a row (or variant) for pass "A" or "B"."""
    assert pas in ("A", "B", "C")
    if row.entry == "qbytes_bmm":
        return _bmm_design(row, pas)
    if "conv2d" in row.entry:
        return _conv_design(row, pas)
    return _mm_design(row, pas)


def coverage(d: Design, pas: str) -> List[str]:
    """What the design fails to show, as sentences (empty: complete).  Pass A: every weight column selected, every code at every position of a packed
    byte, both zero-point extremes and an interior one, among the selected elements.  Pass B: the same over the whole weight of the integer types."""
    missing = []
    if pas == "A":
        if len(d.facts["columns"]) != d.facts["K"]:
            missing.append(f"{d.facts['K'] - len(d.facts['columns'])} of {d.facts['K']} weight columns are never selected")
    seen, zps, ncodes, positions = set(), set(), None, set()
    for w, selected in d.facts["weights"]:
        ncodes = w.ncodes
        rows = range(w.codes.shape[0]) if len(selected) > 1 else [slice(None)]
        for r, cols in zip(rows, selected):
            codes, pos = np.atleast_2d(w.codes[r])[:, cols], np.atleast_2d(w.pos[r])[:, cols]
            seen |= set(zip(pos.reshape(-1).tolist(), codes.reshape(-1).tolist()))
            positions |= set(np.unique(w.pos).tolist())
            if w.zp is not None:
                zps |= set(np.unique(np.atleast_2d(w.zp[r])[:, cols]).tolist())
    want = ncodes * len(positions)
    if pas == "A" or ncodes <= 16 or ncodes == 256:
        if len(seen) != want:
            missing.append(f"{want - len(seen)} of {want} (position, code) pairs are never shown")
    if zps:
        top = max(ZERO_POINTS[4] if ncodes == 16 else ZERO_POINTS[2])
        if not ({0, top} <= zps and len(zps) > 2):
            missing.append(f"zero-points shown: {sorted(zps)}")
    return missing

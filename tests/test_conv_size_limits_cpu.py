"""The size limits of the convolution routes, from host code only (no GPU needed).

* The index arithmetic the tap gather relies on: a numpy model of ``conv_div_small`` over its whole documented range.
* ``conv_geometry_ok`` (csrc/qh_conv.h), probed through the one host-only entry that evaluates it
  (``quanto_hip_qbytes_conv2d_a8_workspace_size``: >= 0 accepted, ENOTSUP refused), against its Python mirror
  ``_Bindings.conv2d_geometry_ok``: every clause at (limit - 1, limit) with a geometry in which only that clause binds.
* The route-specific clauses.  The row form's rule (``conv2d_rows_eligible``) is visible on the host through
  ``quanto_hip_qbits_conv2d_workspace_size_geom`` (it counts the dense weight exactly when the rule holds) and has no Python mirror.  The
  packed-weight clause OC*G < 2^31 and the depthwise rule have no host-only C entry: their Python mirrors are pinned here against a
  transcription of the C rule, and tests/test_large_convs_gpu.py calls the C entries themselves at the same points on the device.
tests/test_large_convs_gpu.py runs each route just inside these limits.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from optimum_quanto_amd.library.hip import _Bindings, quanto_hip

ENOTSUP = -2
BF16, I8 = 2, 3

_c = quanto_hip.cdll
_i64, _ci = ctypes.c_int64, ctypes.c_int
_c.quanto_hip_qbytes_conv2d_a8_workspace_size.restype = _i64
_c.quanto_hip_qbytes_conv2d_a8_workspace_size.argtypes = [_i64] * 9 + [_ci] * 9
_c.quanto_hip_conv2d_workspace_size.restype = _i64
_c.quanto_hip_conv2d_workspace_size.argtypes = [_i64] * 5
_c.quanto_hip_qbits_conv2d_workspace_size_geom.restype = _i64
_c.quanto_hip_qbits_conv2d_workspace_size_geom.argtypes = [_i64] * 8 + [_ci] * 2


# ---- conv_div_small -------------------------------------------------------------------------------------------------------------------------
def _div_magic(d):
    """div_magic of csrc/qh_conv.h: ceil(2^32 / d), 0 when the divisor is 1."""
    return 0 if d <= 1 else ((1 << 32) + d - 1) // d


def _conv_div_small(n, d):
    """Model of the device function conv_div_small of csrc/qh_conv.h (the way scripts/models/conv_rows_model.py models the row form's
    indices): q = __umulhi(n, ceil(2^32 / d)) - the high 32 bits of a 32 x 32-bit product, here in uint64 - or n itself when the magic
    number is 0 (d = 1); the remainder is n - q d."""
    magic = _div_magic(d)
    n = np.asarray(n, np.uint64)
    q = (n * np.uint64(magic)) >> np.uint64(32) if magic else n.copy()
    return q, n - q * np.uint64(d)


@pytest.mark.parametrize("d", range(1, 128))
def test_conv_div_small_is_exact_over_its_documented_range(d):
    """Model of conv_div_small (csrc/qh_conv.h), documented as exact for n < 2^24 and d <= 127: every window size d = KH KW (and KW, KH)
    the rule admits, over n = 0 .. 4 d, every stride-th multiple of d with its two neighbours up to 2^24 - 1, the last multiple, and the
    top 4096 values below 2^24 - where k = cin KH KW - 1 lands when K is at its limit."""
    top = (1 << 24) - 1
    assert _div_magic(d) < 1 << 32 and (_div_magic(d) == 0) == (d == 1)
    mult = np.arange(0, top // d + 1, 61, dtype=np.int64) * d
    mult = np.concatenate([mult, [top // d * d]])
    n = np.concatenate([np.arange(0, 4 * d + 1), mult - 1, mult, mult + 1, np.arange(top - 4095, top + 1)])
    n = np.unique(n[(n >= 0) & (n <= top)])
    q, rem = _conv_div_small(n, d)
    assert np.array_equal(q.astype(np.int64), n // d), f"d = {d}: first wrong n = {n[np.argmax(q.astype(np.int64) != n // d)]}"
    assert np.array_equal(rem.astype(np.int64), n % d)


def test_conv_div_small_model_notices_a_range_it_is_not_valid_for():
    """The check has teeth: just beyond the documented range the same formula is wrong (so the sweep above would notice a wider rule)."""
    n = np.arange(1 << 24, 1 << 32, 4093, dtype=np.int64)
    wrong = 0
    for d in (3, 7, 127):
        q, _ = _conv_div_small(n, d)
        wrong += int((q.astype(np.int64) != n // d).sum())
    assert wrong > 0


# ---- conv_geometry_ok: the C rule and its Python mirror -------------------------------------------------------------------------------------
def _out(size, k, s, p, d):
    return (size + 2 * p - d * (k - 1) - 1) // s + 1


def _geom(B, cin, H, W, OC, KH, KW, s=(1, 1), p=(0, 0), d=(1, 1)):
    return dict(B=B, cin=cin, H=H, W=W, OC=OC, KH=KH, KW=KW, s=s, p=p, d=d, OH=_out(H, KH, s[0], p[0], d[0]), OW=_out(W, KW, s[1], p[1], d[1]))


def c_rule(g):
    """conv_geometry_ok as the C library evaluates it."""
    r = _c.quanto_hip_qbytes_conv2d_a8_workspace_size(g["B"], g["cin"], g["H"], g["W"], g["OC"], g["KH"], g["KW"], g["OH"], g["OW"], g["s"][0], g["s"][1],
                                                      g["p"][0], g["p"][1], g["d"][0], g["d"][1], I8, I8, BF16)
    assert r >= 0 or r == ENOTSUP, f"status {r} for {g}"
    return r >= 0


def py_rule(g):
    return _Bindings.conv2d_geometry_ok((g["B"], g["cin"], g["H"], g["W"]), (g["OC"], g["cin"], g["KH"], g["KW"]), g["s"], g["p"], g["d"])


def clauses(g):
    """The clauses of conv_geometry_ok by name -> holds?  (The test's own arithmetic: which clause binds at a probe.)"""
    K, M = g["cin"] * g["KH"] * g["KW"], g["B"] * g["OH"] * g["OW"]
    return {"K": K < 1 << 24, "taps": g["KH"] * g["KW"] <= 127, "x elements": g["B"] * g["cin"] * g["H"] * g["W"] < 1 << 30,
            "y elements": M * g["OC"] < 1 << 31, "OC K": g["OC"] * K < 1 << 31, "pixel tiles": -(-M // 128) <= 65535}


def failing(g):
    return sorted(k for k, v in clauses(g).items() if not v)


BIG = (1 << 20, 1 << 20)  # a stride beyond every image here: one output pixel per image, whatever H and W are
# (clause, last accepted geometry, first refused geometry, the value the clause bounds at each)
PROBES = [
    ("K", _geom(1, (1 << 24) - 1, 1, 1, 1, 1, 1), _geom(1, 1 << 24, 1, 1, 1, 1, 1), lambda g: g["cin"] * g["KH"] * g["KW"], 1 << 24),
    ("K", _geom(1, 132104, 1, 127, 64, 1, 127), _geom(1, 132105, 1, 127, 64, 1, 127), lambda g: g["cin"] * g["KH"] * g["KW"], None),
    ("taps", _geom(1, 1, 1, 128, 1, 1, 127), _geom(1, 1, 1, 128, 1, 1, 128), lambda g: g["KH"] * g["KW"], 128),
    ("taps", _geom(1, 8, 32, 32, 8, 11, 11), _geom(1, 8, 32, 32, 8, 8, 16), lambda g: g["KH"] * g["KW"], 128),
    # 2^30 - 1 = 231 * 4681 * 331
    ("x elements", _geom(1, 231, 4681, 331, 1, 1, 1, s=BIG), _geom(1, 1024, 1024, 1024, 1, 1, 1, s=BIG), lambda g: g["B"] * g["cin"] * g["H"] * g["W"], 1 << 30),
    ("x elements", _geom(4095, 64, 64, 64, 8, 3, 3, s=(2, 2), p=(1, 1)), _geom(4096, 64, 64, 64, 8, 3, 3, s=(2, 2), p=(1, 1)),
     lambda g: g["B"] * g["cin"] * g["H"] * g["W"], 1 << 30),
    # 2^31 - 1 is prime: one pixel of 2^31 - 1 channels (K = 1, so OC K is below its own limit too)
    ("y elements", _geom(1, 1, 1, 1, (1 << 31) - 1, 1, 1), _geom(1, 1, 256, 128, 1 << 16, 1, 1), lambda g: g["B"] * g["OC"] * g["OH"] * g["OW"], 1 << 31),
    ("y elements", _geom(3, 16, 1100, 1271, 512, 1, 1), _geom(3, 16, 1100, 1271, 513, 1, 1), lambda g: g["B"] * g["OC"] * g["OH"] * g["OW"], None),
    ("OC K", _geom(1, 1, 1, 1, (1 << 31) - 1, 1, 1), _geom(1, 1 << 15, 1, 1, 1 << 16, 1, 1), lambda g: g["OC"] * g["cin"] * g["KH"] * g["KW"], 1 << 31),
    ("OC K", _geom(1, 1 << 15, 1, 1, (1 << 16) - 1, 1, 1), _geom(1, 1 << 15, 1, 1, 1 << 16, 1, 1), lambda g: g["OC"] * g["cin"] * g["KH"] * g["KW"], 1 << 31),
    ("pixel tiles", _geom(1, 1, 1, 65535 * 128, 1, 1, 1), _geom(1, 1, 1, 65535 * 128 + 1, 1, 1, 1), lambda g: -(-g["B"] * g["OH"] * g["OW"] // 128), 65536),
    # 65535 * 128 pixels as 15 images of 544 x 1028; a segmentation batch: 32 images with 512 x 512 outputs = 2^23 pixels = 65536 tiles
    ("pixel tiles", _geom(15, 8, 544, 1028, 64, 3, 3, p=(1, 1)), _geom(32, 8, 512, 512, 64, 3, 3, p=(1, 1)), lambda g: -(-g["B"] * g["OH"] * g["OW"] // 128), 65536),
]


@pytest.mark.parametrize("clause,lo,hi,value,limit", PROBES, ids=[f"{p[0].replace(' ', '_')}-{i}" for i, p in enumerate(PROBES)])
def test_each_clause_of_conv_geometry_ok_at_its_limit(clause, lo, hi, value, limit):
    """(limit - 1, limit) of one clause: the C rule and the mirror take the first and refuse the second, and the named clause is the only
    one the refused geometry breaks."""
    assert failing(lo) == [], f"{clause}: the accepted probe breaks {failing(lo)}"
    assert failing(hi) == [clause], f"{clause}: the refused probe breaks {failing(hi)}"
    if limit is not None:
        assert value(hi) == limit and value(lo) < limit
    assert c_rule(lo) and py_rule(lo), (clause, lo)
    assert not c_rule(hi) and not py_rule(hi), (clause, hi)


def test_the_segmentation_batch_on_the_tile_bound():
    """32 images with 512 x 512 outputs are 2^23 pixels = 65536 tiles of 128: refused; 65535 * 128 pixels are accepted."""
    seg = _geom(32, 8, 512, 512, 64, 3, 3, p=(1, 1))
    assert seg["B"] * seg["OH"] * seg["OW"] == 1 << 23 and failing(seg) == ["pixel tiles"]
    assert not c_rule(seg) and not py_rule(seg)
    last = _geom(15, 8, 544, 1028, 64, 3, 3, p=(1, 1))
    assert last["B"] * last["OH"] * last["OW"] == 65535 * 128
    assert c_rule(last) and py_rule(last)


def _largest(accepts, hi=1 << 31):
    """The largest B in [1, hi] that `accepts` (a rule that holds up to some B and fails beyond it)."""
    assert accepts(1)
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if accepts(mid) else (lo, mid - 1)
    return lo


BISECT = [  # (what, geometry as a function of B, the clause that stops B, the largest B)
    ("planes of one tile", lambda B: _geom(B, 1, 8, 16, 1, 1, 1), "pixel tiles", 65535),
    ("512 x 512 segmentation maps", lambda B: _geom(B, 8, 512, 512, 64, 3, 3, p=(1, 1)), "pixel tiles", 31),
    ("(64, 56, 56) feature maps, stride 2", lambda B: _geom(B, 64, 56, 56, 64, 3, 3, s=(2, 2), p=(1, 1)), "x elements", ((1 << 30) - 1) // (64 * 56 * 56)),
    ("1 x 1 to 4096 channels on 7 x 7", lambda B: _geom(B, 64, 7, 7, 4096, 1, 1), "y elements", ((1 << 31) - 1) // (4096 * 49)),
]


@pytest.mark.parametrize("what,geom,clause,want", BISECT, ids=[b[0] for b in BISECT])
def test_largest_batch_of_a_fixed_geometry(what, geom, clause, want):
    """Bisection on B over the C rule itself: the largest batch is the one the named clause allows, and the mirror turns at the same B."""
    B = _largest(lambda b: c_rule(geom(b)), hi=1 << 24)
    assert B == want, f"{what}: the C rule admits B = {B}"
    assert failing(geom(B)) == [] and failing(geom(B + 1)) == [clause]
    assert B == _largest(lambda b: py_rule(geom(b)), hi=1 << 24)
    assert -(-geom(B)["B"] * geom(B)["OH"] * geom(B)["OW"] // 128) <= 65535


def test_mirror_equals_the_c_rule_on_random_geometries():
    """Seeded geometries with log-uniform sizes (most near one limit or another): the mirror and the C rule always agree, and agree with the
    clause table of this file."""
    rng = np.random.default_rng(0)
    seen = {True: 0, False: 0}

    def draw(hi_log2):
        return int(2 ** rng.uniform(0, hi_log2))

    for _ in range(4000):
        KH, KW = draw(4.5), draw(4.5)
        d = (int(rng.integers(1, 3)), int(rng.integers(1, 3)))
        p = (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        s = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
        H, W = d[0] * (KH - 1) + 1 + draw(12) - 1, d[1] * (KW - 1) + 1 + draw(12) - 1  # the window fits
        g = _geom(draw(14), draw(16), H, W, draw(18), KH, KW, s, p, d)
        want = failing(g) == []
        assert c_rule(g) == want and py_rule(g) == want, g
        seen[want] += 1
    assert min(seen.values()) > 400, seen


# ---- row form: conv2d_rows_eligible through the geometry-aware workspace size ---------------------------------------------------------------
def _rows_taken(B, cin, W, OC, KH, KW, OH, OW, sw=1, dw=1):
    """Whether quanto_hip_qbits_conv2d would take the row form (given the workspace): the size entry counts the dense weight exactly then."""
    K = cin * KH * KW
    with_geom = _c.quanto_hip_qbits_conv2d_workspace_size_geom(B, cin, W, OC, KH, KW, OH, OW, sw, dw)
    split = _c.quanto_hip_conv2d_workspace_size(B, OH, OW, OC, K)
    assert with_geom >= 0 and split >= 0
    dense = -(-OC * K * 2 // 256) * 256
    assert with_geom - split in (0, dense), (with_geom, split, dense)
    return with_geom - split == dense


def test_row_form_rule_at_its_limits():
    """conv2d_rows_eligible (csrc/qconv_mfma.hip): three taps wide at dilation 1, W >= 4, cin KH a multiple of 8, KH KW <= 31, and
    OC K < 2^30 - the dense weight's byte offsets in 31 bits; from 8 pixel tiles on."""
    assert _rows_taken(8, 128, 56, 128, 3, 3, 56, 56)
    # KH KW <= 31: 10 x 3 is the last window (cin KH = 80)
    assert _rows_taken(8, 8, 56, 128, 10, 3, 47, 54) and not _rows_taken(8, 8, 56, 128, 11, 3, 46, 54)
    assert not _rows_taken(8, 128, 56, 128, 3, 3, 56, 56, dw=2) and not _rows_taken(8, 128, 56, 128, 3, 5, 56, 52)
    assert not _rows_taken(8, 4, 56, 128, 3, 3, 56, 56)          # cin KH = 12
    assert _rows_taken(512, 8, 4, 128, 1, 3, 4, 2) and not _rows_taken(512, 8, 3, 128, 1, 3, 4, 1)  # W >= 4
    # OC K < 2^30 with K = 24 (K has a factor 3: the product never equals 2^30): the last OC and the first one beyond it
    oc = ((1 << 30) - 1) // 24
    assert oc * 24 < 1 << 30 <= (oc + 1) * 24
    assert _rows_taken(8, 8, 128, oc, 1, 3, 1, 126) and not _rows_taken(8, 8, 128, oc + 1, 1, 3, 1, 126)
    # K = 1152 (cin 128, 3 x 3): OC = 932067 is the last one
    oc = ((1 << 30) - 1) // 1152
    assert _rows_taken(8, 128, 56, oc, 3, 3, 56, 56) and not _rows_taken(8, 128, 56, oc + 1, 3, 3, 56, 56)
    # fewer than 8 pixel tiles keep the tap kernel
    assert _rows_taken(8, 128, 16, 128, 3, 3, 8, 16) and not _rows_taken(7, 128, 16, 128, 3, 3, 8, 16)


# ---- mirrors of the rules with no host-only C entry -----------------------------------------------------------------------------------------
class _Shape:
    """What the mirrors read of a device tensor: shape, dtype, dim(), is_cuda (no memory behind it)."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

    def dim(self):
        return len(self.shape)


_mirror = types.SimpleNamespace(conv2d_out_size=_Bindings.conv2d_out_size, conv2d_geometry_ok=_Bindings.conv2d_geometry_ok,
                                _qbytes_conv2d_dtypes_ok=_Bindings._qbytes_conv2d_dtypes_ok)


def py_depthwise(B, C, H, W, OC, KH, KW, s=(1, 1), p=(0, 0), d=(1, 1)):
    return _Bindings.qbytes_conv2d_depthwise_supported(_mirror, _Shape((B, C, H, W), torch.bfloat16), _Shape((OC, 1, KH, KW), torch.int8), s, p, d)


def c_depthwise_rule(B, C, H, W, OC, KH, KW, s=(1, 1), p=(0, 0), d=(1, 1)):
    """Transcription of the size clauses of qbytes_conv2d_depthwise_supported (csrc/qconv_depthwise.hip), by name -> holds?"""
    OH, OW = _out(H, KH, s[0], p[0], d[0]), _out(W, KW, s[1], p[1], d[1])
    return {"x elements": B * C * H * W < 1 << 31, "y elements": B * OC * OH * OW < 1 << 31, "taps": KH * KW <= 4096, "H": H < 1 << 20, "W": W < 1 << 20}


DW_PROBES = [  # (clause, last accepted, first refused)
    # 2^30 - 1 = 7161 * 49981: two channels of it are 2^31 - 2 elements
    ("x elements", (1, 2, 7161, 49981, 2, 1, 1, BIG), (1, 2, 1 << 15, 1 << 15, 2, 1, 1, BIG)),
    ("x elements", (1, 512, 2047, 2049, 512, 7, 7, (1 << 20, 1 << 20), (6, 6), (2, 2)), (1, 512, 2048, 2048, 512, 7, 7, (1 << 20, 1 << 20), (6, 6), (2, 2))),
    ("y elements", (1, 2, 1, 1, (1 << 31) - 2, 1, 1), (1, 2, 1, 1, 1 << 31, 1, 1)),
    ("y elements", (1, 512, 1024, 2047, 1024, 3, 3, (1, 1), (1, 1)), (1, 512, 1024, 2048, 1024, 3, 3, (1, 1), (1, 1))),
    ("taps", (1, 2, 64, 64, 2, 64, 64), (1, 2, 64, 65, 2, 64, 65)),
    ("H", (1, 2, (1 << 20) - 1, 1, 2, 3, 1, (1, 1), (1, 0)), (1, 2, 1 << 20, 1, 2, 3, 1, (1, 1), (1, 0))),
    ("W", (1, 2, 1, (1 << 20) - 1, 2, 1, 3, (1, 1), (0, 1)), (1, 2, 1, 1 << 20, 2, 1, 3, (1, 1), (0, 1))),
]


@pytest.mark.parametrize("clause,lo,hi", DW_PROBES, ids=[f"{p[0].replace(' ', '_')}-{i}" for i, p in enumerate(DW_PROBES)])
def test_depthwise_mirror_equals_the_c_rule(clause, lo, hi):
    """Every size clause of the depthwise rule at (limit - 1, limit), H and W < 2^20 included: a caller that asks the mirror first keeps the
    reference path exactly where the C entry would answer ENOTSUP (test_large_convs_gpu.py calls the C entry at the same points)."""
    assert all(c_depthwise_rule(*lo).values()), c_depthwise_rule(*lo)
    assert sorted(k for k, v in c_depthwise_rule(*hi).items() if not v) == [clause]
    assert py_depthwise(*lo), lo
    assert not py_depthwise(*hi), hi


def py_qbits(x_shape, w_shape, bits, gs, s=(1, 1), p=(0, 0), d=(1, 1)):
    return _Bindings.qbits_conv2d_supported(_mirror, _Shape(x_shape, torch.bfloat16), w_shape, bits, gs, s, p, d)


def test_packed_weight_mirror_and_the_oc_g_clause():
    """qbits_conv2d_supported: OC a multiple of the values per byte, groups of a multiple of 8 (or one per channel), OC G < 2^31 and
    conv_geometry_ok.  With the smallest admitted group (8) G = K / 8, so OC G <= OC K / 8 < 2^28 wherever OC K < 2^31 holds: the OC G clause
    is implied by the geometry rule and never the binding one - pinned here so that a smaller admitted group size would show up."""
    x, w = (1, 1 << 15, 1, 1), ((1 << 16) - 2, 1 << 15, 1, 1)          # OC K = 2^31 - 2^16: the last even OC at this K
    assert py_qbits(x, w, 4, 8) and py_qbits(x, w, 4, None) and py_qbits(x, w, 4, 128)
    assert w[0] * (w[1] // 8) < 1 << 28
    assert not py_qbits(x, (1 << 16, 1 << 15, 1, 1), 4, 8)             # OC K = 2^31
    assert not py_qbits(x, w, 4, 4) and not py_qbits(x, w, 4, 12)      # groups of a multiple of 8
    assert not py_qbits(x, ((1 << 16) - 1, 1 << 15, 1, 1), 4, 8)       # odd OC
    assert py_qbits(x, ((1 << 16) - 4, 1 << 15, 1, 1), 2, 8) and not py_qbits(x, w, 2, 8)  # int2: OC a multiple of 4
    assert not py_qbits(x, w, 3, 8) and not py_qbits(x, w, 8, 8)
    for oc, k in (((1 << 16) - 2, 1 << 15), ((1 << 27) - 2, 16), (1 << 20, 2040)):
        assert oc * k < 1 << 31 and oc * (k // 8) < 1 << 31

"""Every convolution route at the image sizes and grid limits its support rule admits.

tests/test_qconv2d.py and tests/test_qconv2d_a8_gpu.py stop at ~25 000 output pixels; conv_geometry_ok (csrc/qh_conv.h) and the depthwise
rule admit 2^23 pixels, 2^30 / 2^31 input elements, 2^31 output elements and K up to 2^24.  Each accepted case here runs ONE call straight
through the C ABI just inside a limit, with the workspace the library's own size entry asks for, into an output filled with NaN, and checks
that call three ways:

* written: no NaN is left in the output;
* sampled pixels (first / last, the last pixel tile, both sides of image boundaries that fall inside a 4-pixel lane group or a 128-pixel
  tile, the corners of the first and last image, the pixels whose input and output byte offsets cross 2^31 and 2^32), all OC channels of
  each, against float64 math written here in plain torch (an index gather of the window, zeros over the padding, times the float64 image
  of the quantized weight) through the parity gate (helpers.assert_close_to_exact / assert_close_with_bias); int8 x int8 outputs must
  equal the integer result exactly;
* projection: for 3 random +-1 vectors v over the output channels, sum_oc v[oc] y[b, oc, oh, ow] of EVERY pixel against the float64
  convolution of x with the one combined filter sum_oc v[oc] W64[oc] (tap by tap, in chunks of images), within helpers.projection_bound
  with N = OC - a wrong tile anywhere in the output moves it.

A category of sampled pixels that does not exist for a geometry (no image boundary inside a lane group, no offset reaching 2^31) is
asserted not to exist.  Where a geometry has more than 48 image boundaries inside tiles (millions of tiny images) the first and last eight
and 32 seeded ones are sampled; the projection covers all of them.  Refused cases pass operands of the full stated size, so a call the
rule wrongly admitted would still stay inside its buffers.  The operands are built on the device from a seeded generator; every case
stays under ~8 GiB of device memory and frees it before the next one.
"""
import ctypes
import gc

import numpy as np
import pytest
import torch

from helpers import assert_close_to_exact, assert_close_with_bias, projection_bound, to_numpy
from optimum_quanto_amd.library.hip import quanto_hip

pytestmark = pytest.mark.gpu

ENOTSUP = -2
BF16, I8, E4M3 = 2, 3, 5
DEV = "cuda"
CHUNK = 1 << 26  # elements per float64 chunk of the reference math (512 MiB)


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _gen(seed, dev=None):
    return torch.Generator(device=dev or DEV).manual_seed(seed)


class Geom:
    """One conv2d call: x [B, cin, H, W], weight [OC, cin (depthwise: 1), KH, KW], y [B, OC, OH, OW]."""

    def __init__(self, B, cin, H, W, OC, KH, KW, s=(1, 1), p=(0, 0), d=(1, 1), depthwise=False):
        self.B, self.cin, self.H, self.W, self.OC, self.KH, self.KW, self.s, self.p, self.d, self.depthwise = B, cin, H, W, OC, KH, KW, s, p, d, depthwise
        self.OH = (H + 2 * p[0] - d[0] * (KH - 1) - 1) // s[0] + 1
        self.OW = (W + 2 * p[1] - d[1] * (KW - 1) - 1) // s[1] + 1
        self.L, self.M = self.OH * self.OW, B * self.OH * self.OW
        self.K = (1 if depthwise else cin) * KH * KW
        self.mult = OC // cin if depthwise else None

    @property
    def ints(self):
        return (self.B, self.cin, self.H, self.W, self.OC, self.KH, self.KW, self.OH, self.OW, self.s[0], self.s[1], self.p[0], self.p[1], self.d[0], self.d[1])

    @property
    def x_elems(self):
        return self.B * self.cin * self.H * self.W

    @property
    def y_elems(self):
        return self.B * self.OC * self.L

    @property
    def tiles(self):
        return -(-self.M // 128)

    def __repr__(self):
        return f"({self.B},{self.cin},{self.H},{self.W})->{self.OC} {self.KH}x{self.KW} s{self.s} p{self.p} d{self.d}"


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
def _fill(n, dtype, draw, dev=None):
    t = torch.empty((n,), dtype=dtype, device=dev or DEV)
    for i in range(0, n, CHUNK):
        j = min(n, i + CHUNK)
        t[i:j] = draw(j - i)
    return t


def _bf16_normal(n, gen, scale=1.0, dev=None):
    return _fill(n, torch.bfloat16, lambda k: (torch.randn((k,), generator=gen, device=dev or DEV) * scale).to(torch.bfloat16), dev)


def _int8(n, gen, dev=None):
    return _fill(n, torch.int8, lambda k: torch.randint(-127, 128, (k,), generator=gen, device=dev or DEV, dtype=torch.int32).to(torch.int8), dev)


def _bytes(n, gen, dev=None):
    return _fill(n, torch.uint8, lambda k: torch.randint(0, 256, (k,), generator=gen, device=dev or DEV, dtype=torch.int32).to(torch.uint8), dev)


def _e4m3(n, gen, dev=None):
    """float8_e4m3fn of random finite codes (the two NaN codes replaced by zero)."""
    b = _bytes(n, gen, dev)
    return torch.where((b & 0x7F) == 0x7F, torch.zeros_like(b), b).view(torch.float8_e4m3fn)


def _values64(t):
    """The float64 values of activations / codes (bf16, int8 and fp8 are all exact in float32)."""
    return t.to(torch.float32).to(torch.float64)


def _scales(n, gen, dev=None):
    return (torch.rand((n,), generator=gen, device=dev or DEV) * 0.015 + 0.005).to(torch.bfloat16)


class BytesWeight:
    """An int8 / e4m3 weight [N, K] with a per-channel bf16 scale; ``factor``: what the kernel multiplies a channel's sum by (the scale, or for
    quantized activations round_bf16(a_scale * scale))."""

    def __init__(self, N, K, kind, gen, dev=None):
        self.N, self.K, self.kind = N, K, kind
        self.data = (_int8(N * K, gen, dev) if kind == I8 else _e4m3(N * K, gen, dev)).view(N, K)
        self.scale = _scales(N, gen, dev)
        self.factor = self.scale

    def codes64(self, n0, n1):
        return _values64(self.data[n0:n1])

    def rows64(self, n0, n1):
        return self.codes64(n0, n1) * self.factor[n0:n1].double()[:, None]


class BitsWeight:
    """A generic packed int4 / int2 weight [N, K] (groups of ``gs`` along K, None: one per channel; float shift) and the float64 image of the
    dense weight the reference materialises for it: T(T(scale q) - shift) in bf16 (tensor/qbits.py:27-49), rounding by rounding."""

    def __init__(self, N, K, bits, gs, gen, dev=None):
        self.N, self.K, self.bits, self.gs = N, K, bits, gs or K
        self.G = K // self.gs
        assert self.G * self.gs == K
        self.planes = 8 // bits
        assert N % self.planes == 0
        R = N * self.G
        self.packed = _bytes(N // self.planes * K, gen, dev)
        self.scale = _scales(R, gen, dev)
        self.shift = _fill(R, torch.bfloat16, lambda k: torch.rand((k,), generator=gen, device=dev or DEV).to(torch.bfloat16) * 2 + (2 ** bits / 2 - 1), dev)
        self.shift = (self.scale.float() * self.shift.float()).to(torch.bfloat16)

    def rows64(self, n0, n1):
        P, dev = self.N // self.planes, self.packed.device
        n = torch.arange(n0, n1, device=dev)
        plane, p = n // P, n % P
        q = (self.packed.view(P, self.K)[p].to(torch.int32) >> (self.bits * plane[:, None].to(torch.int32))) & ((1 << self.bits) - 1)
        r = (n[:, None] * self.G + torch.arange(self.G, device=dev)[None, :])
        sc = self.scale[r].float().repeat_interleave(self.gs, dim=1)
        sh = self.shift[r].float().repeat_interleave(self.gs, dim=1)
        return ((sc * q.float()).to(torch.bfloat16).float() - sh).to(torch.bfloat16).double()


def _weight_rows(w):
    step = max(1, CHUNK // w.K)
    for n0 in range(0, w.N, step):
        n1 = min(w.N, n0 + step)
        yield n0, n1, w.rows64(n0, n1)


# ---- the three checks -------------------------------------------------------------------------------------------------------------------------
def _check_written(y, what):
    bad = 0
    flat = y.view(-1)
    for i in range(0, flat.numel(), 1 << 28):
        bad += int((~torch.isfinite(flat[i:i + (1 << 28)])).sum())
    assert bad == 0, f"{what}: {bad} output elements not written (or not finite)"


def _px_off(g, m, es):
    b, l = divmod(m, g.L)
    oh, ow = divmod(l, g.OW)
    return es * (b * g.cin * g.H * g.W + oh * g.s[0] * g.W + ow * g.s[1])


def sample_pixels(g, es_in, es_out=2, seed=0):
    """Flat pixel indices m = b L + l to compare, and the categories that do not exist for this geometry (asserted here)."""
    L, M, B, OW = g.L, g.M, g.B, g.OW
    ms = {0, min(1, M - 1), M - 1, (M - 1) // 128 * 128}
    # image boundaries inside a 128-pixel tile (those inside a 4-pixel lane group among them): the pixels on either side
    if B == 1 or L % 128 == 0:
        inside = []  # one image, or every image a whole number of tiles: no image ends inside a pixel tile
    else:
        per = 128 // np.gcd(L, 128)  # every per-th boundary is tile-aligned
        inside = [b for b in range(1, B)] if B <= 4096 else None
        if inside is None:
            rng = np.random.default_rng(seed)
            inside = sorted(set(range(1, 9)) | set(range(B - 8, B)) | set(int(v) for v in rng.integers(1, B, 64)))
        inside = [b for b in inside if (b * L) % 128 != 0]
        assert inside, (B, L, per)
        if len(inside) > 48:
            rng = np.random.default_rng(seed + 1)
            inside = sorted(set(inside[:8]) | set(inside[-8:]) | set(inside[int(i)] for i in rng.integers(0, len(inside), 32)))
    in_group = [b for b in inside if (b * L) % 4 != 0]
    if L % 4 == 0 or B == 1:
        assert not in_group, "no image ends inside a lane's four pixels"
    else:
        assert in_group, "an image ends inside a lane's four pixels"
    for b in inside:
        ms.update((b * L - 1, b * L))
    # the four corners of the first and last image
    for b in (0, B - 1):
        ms.update(b * L + l for l in (0, OW - 1, L - OW, L - 1))
    # input byte offsets (px_off) crossing 2^31 / 2^32
    img = g.cin * g.H * g.W
    for lim in (1 << 31, 1 << 32):
        if g.x_elems * es_in <= lim:
            assert _px_off(g, M - 1, es_in) < lim  # the category does not exist: every input offset is below the limit
            continue
        b, rem = divmod(lim // es_in, img)
        if rem > (g.OH - 1) * g.s[0] * g.W + (OW - 1) * g.s[1]:
            cand = [b * L + L - 2, b * L + L - 1, (b + 1) * L, (b + 1) * L + 1]  # crossed between two images
        else:
            oh = min(rem // (g.s[0] * g.W), g.OH - 1)
            ow = min((rem - oh * g.s[0] * g.W) // g.s[1], OW - 1)
            m = b * L + oh * OW + ow
            cand = [m - 1, m, m + 1]
        ms.update(m for m in cand if 0 <= m < M)
    # output byte offsets crossing 2^31 / 2^32: the pixel whose channel planes hold that byte, and its neighbours
    for lim in (1 << 31, 1 << 32):
        if g.y_elems * es_out <= lim:
            continue  # (asserted by the caller against y.numel())
        b, rem = divmod(lim // es_out, g.OC * L)
        l = rem % L
        ms.update(m for m in (b * L + l - 1, b * L + l, b * L + l + 1) if 0 <= m < M)
    return sorted(ms)


def _gather_windows(x4, g, ms):
    """float64 [P, cin, KH, KW]: the windows of the pixels ``ms`` by index gather, zeros over the padding."""
    dev = x4.device
    m = torch.tensor(ms, device=dev, dtype=torch.int64)
    b, l = m // g.L, m % g.L
    oh, ow = l // g.OW, l % g.OW
    ih = oh[:, None] * g.s[0] - g.p[0] + torch.arange(g.KH, device=dev)[None, :] * g.d[0]
    iw = ow[:, None] * g.s[1] - g.p[1] + torch.arange(g.KW, device=dev)[None, :] * g.d[1]
    ok = ((ih >= 0) & (ih < g.H))[:, :, None] & ((iw >= 0) & (iw < g.W))[:, None, :]
    xg = x4[b[:, None, None, None], torch.arange(g.cin, device=dev)[None, :, None, None], ih.clamp(0, g.H - 1)[:, None, :, None],
            iw.clamp(0, g.W - 1)[:, None, None, :]]
    return _values64(xg) * ok[:, None].double(), b, l


def pixels_exact(x4, g, w, ms, rows=None):
    """float64 [P, OC]: all output channels of the pixels ``ms`` (``rows``: w.rows64 or another row function, e.g. the integer codes)."""
    xg, b, l = _gather_windows(x4, g, ms)
    rows = rows or w.rows64
    if g.depthwise:
        w64 = rows(0, w.N).view(g.cin, g.mult, g.KH * g.KW)
        out = torch.einsum("pct,cmt->pcm", xg.reshape(len(ms), g.cin, -1), w64).reshape(len(ms), g.OC)
    else:
        xg = xg.reshape(len(ms), g.K)
        step = max(1, CHUNK // g.K)
        out = torch.cat([xg @ rows(n0, min(w.N, n0 + step)).T for n0 in range(0, w.N, step)], dim=1)
    return out, b, l


def _y_pixels(y4, g, b, l):
    return y4.view(g.B, g.OC, g.L)[b, :, l]  # [P, OC]


def check_pixels(y4, x4, g, w, ms, bias, what):
    exact, b, l = pixels_exact(x4, g, w, ms)
    got = to_numpy(_y_pixels(y4, g, b, l))
    if bias is None:
        assert_close_to_exact(got, exact.cpu().numpy(), "bf16", f"{what}: {len(ms)} sampled pixels")
    else:
        assert_close_with_bias(got, exact.cpu().numpy(), np.broadcast_to(to_numpy(bias).astype(np.float64), got.shape), "bf16", f"{what}: {len(ms)} sampled pixels")


def check_pixels_int8(y4, x4, g, w, ms, bias, what):
    """int8 x int8: the integer sums are exact, so the output is a function of the integers - bf16(fp32(acc) * sc) (+ bias, rounded again)."""
    acc, b, l = pixels_exact(x4, g, w, ms, rows=w.codes64)
    assert float(acc.abs().max()) < 2 ** 31
    want = (acc.to(torch.int64).to(torch.float32) * w.factor.float()[None, :]).to(torch.bfloat16)
    if bias is not None:
        want = (want.float() + bias.float()[None, :]).to(torch.bfloat16)
    got = _y_pixels(y4, g, b, l)
    diff = int((got.float() != want.float()).sum())
    assert diff == 0, f"{what}: {diff} of {got.numel()} sampled outputs differ from the integer result"


def combined_filters(g, w, v):
    """float64 [nvec, cin, KH, KW]: sum_oc v[oc] W64[oc] (depthwise: over the channel's multiplier)."""
    nvec = v.shape[1]
    if g.depthwise:
        w64 = w.rows64(0, w.N).view(g.cin, g.mult, g.KH, g.KW)
        return torch.einsum("cmij,cmv->vcij", w64, v.view(g.cin, g.mult, nvec))
    wv = torch.zeros((nvec, g.K), dtype=torch.float64, device=v.device)
    for n0, n1, w64 in _weight_rows(w):
        wv += v[n0:n1].T @ w64
    return wv.view(nvec, g.cin, g.KH, g.KW)


def project_reference(x4, g, wv, b0, b1):
    """float64 [b1 - b0, nvec, OH, OW]: the convolution of images b0 .. b1 - 1 with the filters wv, tap by tap on the zero-padded images."""
    xp = torch.nn.functional.pad(_values64(x4[b0:b1]), (g.p[1], g.p[1], g.p[0], g.p[0]))
    out = torch.zeros((b1 - b0, wv.shape[0], g.OH, g.OW), dtype=torch.float64, device=x4.device)
    for i in range(g.KH):
        for j in range(g.KW):
            win = xp[:, :, i * g.d[0]: i * g.d[0] + (g.OH - 1) * g.s[0] + 1: g.s[0], j * g.d[1]: j * g.d[1] + (g.OW - 1) * g.s[1] + 1: g.s[1]]
            out += torch.einsum("bchw,vc->bvhw", win, wv[:, :, i, j])
    return out


def check_projection(y4, x4, g, w, bias, what, nvec=3, seed=0):
    """sum_oc v[oc] y[b, oc, oh, ow] of every pixel against the float64 convolution with the combined filter; bound: helpers.projection_bound
    (the one of test_large_operands_gpu._check_freivalds) with N = OC."""
    dev = y4.device
    v = (torch.randint(0, 2, (g.OC, nvec), generator=_gen(seed, dev), device=dev, dtype=torch.int32) * 2 - 1).double()
    wv = combined_filters(g, w, v)
    bv = None if bias is None else bias.double() @ v  # [nvec]
    ymax = 0.0
    flat = y4.view(-1)
    for i in range(0, flat.numel(), 1 << 28):
        ymax = max(ymax, float(flat[i:i + (1 << 28)].float().abs().max()))
    assert ymax > 0, f"{what}: all-zero output"
    img_x, img_y = g.cin * g.H * g.W, g.OC * g.L
    assert img_x <= CHUNK and g.L <= CHUNK, "one image per reference chunk at least"
    nb = max(1, min(CHUNK // img_x, CHUNK // img_y))
    ocs = max(1, CHUNK // (nb * g.L))
    worst = 0.0
    for b0 in range(0, g.B, nb):
        b1 = min(g.B, b0 + nb)
        got = torch.zeros((b1 - b0, nvec, g.OH, g.OW), dtype=torch.float64, device=dev)
        asum = torch.zeros((b1 - b0, 1, g.OH, g.OW), dtype=torch.float64, device=dev)
        for c0 in range(0, g.OC, ocs):
            yc = y4[b0:b1, c0:c0 + ocs].float().double()
            got += torch.einsum("bchw,cv->bvhw", yc, v[c0:c0 + ocs])
            asum += yc.abs().sum(dim=1, keepdim=True)
        want = project_reference(x4, g, wv, b0, b1)
        if bv is not None:
            want += bv[None, :, None, None]
        ratio = float(((got - want).abs() / projection_bound(asum, g.OC, ymax)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{what}: projection over the channels off in images {b0}..{b1 - 1} ({ratio:.2f} x the bound)"
    return worst


# ---- calls ------------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_output(g):
    return torch.full((g.B, g.OC, g.OH, g.OW), float("nan"), dtype=torch.bfloat16, device=DEV)


def _workspace(nbytes):
    assert nbytes >= 0, nbytes
    return (torch.empty((nbytes,), dtype=torch.uint8, device=DEV), nbytes) if nbytes > 0 else (None, 0)


def _ptr(t):
    return None if t is None else t.data_ptr()


def call_qbytes(g, x, w, bias, y, a_dt=BF16):
    c = quanto_hip.lib._c
    ws, n = _workspace(int(c.quanto_hip_conv2d_workspace_size(g.B, g.OH, g.OW, g.OC, g.K)))
    st = c.quanto_hip_qbytes_conv2d(x.data_ptr(), w.data.data_ptr(), w.scale.data_ptr(), _ptr(bias), y.data_ptr(), *g.ints, a_dt, w.kind, BF16, _ptr(ws), n, _stream())
    torch.cuda.synchronize()
    return st


def call_qbits(g, x, w, bias, y):
    c = quanto_hip.lib._c
    ws, n = _workspace(int(c.quanto_hip_qbits_conv2d_workspace_size_geom(g.B, g.cin, g.W, g.OC, g.KH, g.KW, g.OH, g.OW, g.s[1], g.d[1])))
    st = c.quanto_hip_qbits_conv2d(x.data_ptr(), w.packed.data_ptr(), w.scale.data_ptr(), w.shift.data_ptr(), _ptr(bias), y.data_ptr(), *g.ints, w.bits,
                                   0 if w.G == 1 else w.gs, BF16, BF16, _ptr(ws), n, _stream())
    torch.cuda.synchronize()
    return st


def call_depthwise(g, x, w, bias, y):
    st = quanto_hip.lib._c.quanto_hip_qbytes_conv2d_depthwise(x.data_ptr(), w.data.data_ptr(), w.scale.data_ptr(), _ptr(bias), y.data_ptr(), *g.ints, BF16, w.kind,
                                                              BF16, _stream())
    torch.cuda.synchronize()
    return st


def a8_workspace_size(g, a_dt, b_dt):
    return int(quanto_hip.lib._c.quanto_hip_qbytes_conv2d_a8_workspace_size(*g.ints, a_dt, b_dt, BF16))


def call_a8(g, x, a_scale, w, bias, y, a_dt, ws_bytes):
    ws, n = _workspace(ws_bytes)
    st = quanto_hip.lib._c.quanto_hip_qbytes_conv2d_a8(x.data_ptr(), a_scale.data_ptr(), w.data.data_ptr(), w.scale.data_ptr(), _ptr(bias), y.data_ptr(), *g.ints,
                                                       a_dt, w.kind, BF16, _ptr(ws), n, _stream())
    torch.cuda.synchronize()
    return st


def _bias(g, on, gen):
    return (torch.randn((g.OC,), generator=gen, device=DEV) * 0.5).to(torch.bfloat16) if on else None


def _status(st):
    return quanto_hip.lib._c.quanto_hip_status_string(st)


def _binding(g):
    """The clauses of conv_geometry_ok this geometry breaks."""
    c = {"K": g.K < 1 << 24, "taps": g.KH * g.KW <= 127, "x elements": g.x_elems < 1 << 30, "y elements": g.y_elems < 1 << 31, "OC K": g.OC * g.K < 1 << 31,
         "pixel tiles": g.tiles <= 65535}
    return sorted(k for k, ok in c.items() if not ok)


# geometries shared by several routes
G_X30 = dict(B=1024, cin=63, H=129, W=129, OC=64, KH=3, KW=3, s=(2, 2), p=(1, 1))    # B cin H W = 2^30 - 163 840; L = 65 x 65: odd
G_TILES = dict(B=128, cin=8, H=255, W=257, OC=64, KH=3, KW=3, p=(1, 1))              # M = 65535 x 128, L = 255 x 257: odd

# ---- accepted: dense convolutions with float activations ------------------------------------------------------------------------------------------
DENSE = [
    # (id, geometry, weight (kind, bits, group size), bias, route, what it pins -> (value, limit))
    ("1-tap-int8-x-elements", G_X30, (I8, 8, None), True, "conv2d_mfma", lambda g: (g.x_elems, 1 << 30)),
    ("2-rows-int8-65535-tiles", G_TILES, (I8, 8, None), False, "conv2d_mfma_rows", lambda g: (g.tiles, 65536)),
    # B OC OH OW = 2^31 - 2048; L = 1100 x 1271 = 4 x odd: the 8-byte vector stores of the register epilogue; output bytes pass 2^32
    ("3-tap-e4m3-y-elements", dict(B=3, cin=16, H=1100, W=1271, OC=512, KH=1, KW=1), (E4M3, 8, None), True, "conv2d_mfma", lambda g: (g.y_elems, 1 << 31)),
    # K = 16 777 081: conv_div_small at the top of its range, 64 splits over 262 142 K-tiles, the reduce kernel; one output pixel
    ("4-tap-int8-K", dict(B=1, cin=132103, H=1, W=127, OC=64, KH=1, KW=127), (I8, 8, None), False, "conv2d_mfma", lambda g: (g.K, 1 << 24)),
    # planes of 1, 2 and 3 pixels, 65535 tiles: the fp32-reciprocal m / L and lanes whose four pixels span up to four images
    ("5-tap-int8-planes-of-1", dict(B=65535 * 128, cin=8, H=1, W=1, OC=16, KH=3, KW=3, p=(1, 1)), (I8, 8, None), True, "conv2d_mfma", lambda g: (g.tiles, 65536)),
    ("5-tap-int8-planes-of-2", dict(B=65535 * 64, cin=8, H=1, W=2, OC=16, KH=3, KW=3, p=(1, 1)), (I8, 8, None), False, "conv2d_mfma", lambda g: (g.tiles, 65536)),
    ("5-tap-int8-planes-of-3", dict(B=65535 * 128 // 3, cin=8, H=1, W=3, OC=16, KH=3, KW=3, p=(1, 1)), (I8, 8, None), True, "conv2d_mfma", lambda g: (g.tiles, 65536)),
    # one plane of 2896 x 2896 = 8 386 816 pixels: the oh = l / OW decomposition at its largest
    ("6-one-image-2896x2896", dict(B=1, cin=8, H=2896, W=2896, OC=32, KH=3, KW=3, p=(1, 1)), (I8, 8, None), False, "conv2d_mfma_rows", lambda g: (g.tiles, 65536)),
    # OC K = 2^31 - 16 508 (cin odd: the tap form)
    ("7-tap-int8-OC-K", dict(B=1, cin=4095, H=16, W=16, OC=58268, KH=3, KW=3, p=(1, 1)), (I8, 8, None), True, "conv2d_mfma", lambda g: (g.OC * g.K, 1 << 31)),
    # int4, groups of 8: OC G < 2^31 cannot be reached (G = K / 8 and OC K < 2^31): the largest packed weight the rule admits, 1 GiB with
    # OC K = 2^31 - 8192 and OC G = 2^28 - 1024 scales and shifts (two pixel tiles: the tap form)
    ("8-tap-int4-g8-OC-K", dict(B=1, cin=4096, H=16, W=16, OC=58254, KH=3, KW=3, p=(1, 1)), (None, 4, 8), False, "conv2d_mfma_int4", lambda g: (g.OC * g.K, 1 << 31)),
    ("9-tap-int2-x-elements", G_X30, (None, 2, None), True, "conv2d_mfma_int2", lambda g: (g.x_elems, 1 << 30)),
    # the row form on the dequantized weight: OC K = 2^30 - 40 960 (a 2 GiB dense weight in the scratch) on 8 tiles, and 65535 tiles
    ("10-rows-dequant-int4-OC-K", dict(B=1, cin=4096, H=32, W=32, OC=29126, KH=3, KW=3, p=(1, 1)), (None, 4, 128), True, "conv2d_rows_dequant_int4",
     lambda g: (g.OC * g.K, 1 << 30)),
    ("10-rows-dequant-int4-65535-tiles", G_TILES, (None, 4, 8), False, "conv2d_rows_dequant_int4", lambda g: (g.tiles, 65536)),
]


@pytest.mark.parametrize("cid,geo,wfmt,bias_on,route,pins", DENSE, ids=[c[0] for c in DENSE])
def test_dense_route_just_inside_its_limit(cid, geo, wfmt, bias_on, route, pins):
    g = Geom(**geo)
    value, limit = pins(g)
    assert value < limit and limit - value <= max(1, limit // 4096), f"{cid}: {value} is not just below {limit}"
    assert _binding(g) == []
    kind, bits, gs = wfmt
    gen = _gen(sum(map(ord, cid)))
    x = _bf16_normal(g.x_elems, gen, scale=g.K ** -0.5 if g.K > 1 << 20 else 1.0).view(g.B, g.cin, g.H, g.W)
    w = BytesWeight(g.OC, g.K, kind, gen) if bits == 8 else BitsWeight(g.OC, g.K, bits, gs, gen)
    bias = _bias(g, bias_on, gen)
    y = _nan_output(g)
    st = (call_qbytes if bits == 8 else call_qbits)(g, x, w, bias, y)
    assert st == 0, _status(st)
    assert quanto_hip.lib.last_kernel() == route
    what = f"{route} {g}"
    _check_written(y, what)
    ms = sample_pixels(g, 2)
    assert (y.numel() * 2 > 1 << 32) == (g.y_elems * 2 > 1 << 32)
    check_pixels(y, x, g, w, ms, bias, what)
    check_projection(y, x, g, w, bias, what)


# ---- accepted: quantized activations --------------------------------------------------------------------------------------------------------------
A8 = [
    ("11-a8-int8-x-elements", G_X30, I8, I8, True, "conv2d_a8_int8"),
    ("11-a8-int8-65535-tiles", G_TILES, I8, I8, False, "conv2d_a8_int8"),
    ("12-a8-fp8-65535-tiles", G_TILES, E4M3, E4M3, True, "conv2d_a8_fp8"),
    ("12-a8-fp8-x-elements", G_X30, E4M3, E4M3, False, "conv2d_a8_fp8"),
]


@pytest.mark.parametrize("cid,geo,adt,bdt,bias_on,route", A8, ids=[c[0] for c in A8])
def test_a8_route_just_inside_its_limit(cid, geo, adt, bdt, bias_on, route):
    g = Geom(**geo)
    assert _binding(g) == []
    gen = _gen(sum(map(ord, cid)))
    x = (_int8(g.x_elems, gen) if adt == I8 else _e4m3(g.x_elems, gen)).view(g.B, g.cin, g.H, g.W)
    w = BytesWeight(g.OC, g.K, bdt, gen)
    a_scale = torch.tensor([0.0078125 if adt == I8 else 0.001953125], dtype=torch.bfloat16, device=DEV)
    if bdt != I8:
        w.scale = (w.scale.float() / 32).to(torch.bfloat16)  # fp8 codes reach 448
    w.factor = (a_scale.float() * w.scale.float()).to(torch.bfloat16)  # sc[n] = round_dtype(fp32(a_scale) * fp32(w_scale[n]))
    bias = _bias(g, bias_on, gen)
    y = _nan_output(g)
    ws_bytes = a8_workspace_size(g, adt, bdt)
    st = call_a8(g, x, a_scale, w, bias, y, adt, ws_bytes)
    assert st == 0, _status(st)
    assert quanto_hip.lib.last_kernel() == route
    what = f"{route} {g}"
    _check_written(y, what)
    ms = sample_pixels(g, 1)
    if adt == I8:
        check_pixels_int8(y, x, g, w, ms, bias, what)
    check_pixels(y, x, g, w, ms, bias, what)
    check_projection(y, x, g, w, bias, what)


# ---- accepted: depthwise ------------------------------------------------------------------------------------------------------------------------------
DEPTHWISE = [
    # B C H W = 2^31 - 2^21 (4 GiB of bf16): size_t plane offsets past 2^32; dilation 2: the quad form
    ("13-quad-7x7-dil2-x-elements", dict(B=128, cin=16, H=1024, W=1023, OC=16, KH=7, KW=7, s=(2, 2), p=(6, 6), d=(2, 2)), I8, True, "conv2d_depthwise",
     lambda g: (g.x_elems, 1 << 31)),
    # B OC OH OW = 2^31 - 2^21 with multiplier 2; and 2^31 - 2^22 at stride 2 (multiplier 8: a stride-2 output is a quarter of its input)
    ("14-strip-3x3-s1-y-elements", dict(B=128, cin=8, H=1023, W=1024, OC=16, KH=3, KW=3, p=(1, 1)), E4M3, False, "conv2d_depthwise_strip", lambda g: (g.y_elems, 1 << 31)),
    ("14-strip-5x5-s2-y-elements", dict(B=128, cin=8, H=1022, W=1024, OC=64, KH=5, KW=5, s=(2, 2), p=(2, 2)), I8, True, "conv2d_depthwise_strip",
     lambda g: (g.y_elems, 1 << 31)),
    # the generic tap loop: a window of 4096 taps; columns and rows of 2^20 - 1 elements
    ("15-generic-64x64-window", dict(B=2, cin=4, H=80, W=72, OC=8, KH=64, KW=64, p=(3, 5)), I8, True, "conv2d_depthwise", lambda g: (g.KH * g.KW, 4097)),
    ("15-generic-H-2^20-1", dict(B=2, cin=4, H=(1 << 20) - 1, W=1, OC=4, KH=3, KW=1, p=(1, 0)), I8, False, "conv2d_depthwise", lambda g: (g.H, 1 << 20)),
    ("15-generic-W-2^20-1", dict(B=2, cin=4, H=1, W=(1 << 20) - 1, OC=8, KH=1, KW=3, p=(0, 1)), E4M3, True, "conv2d_depthwise", lambda g: (g.W, 1 << 20)),
]


@pytest.mark.parametrize("cid,geo,kind,bias_on,route,pins", DEPTHWISE, ids=[c[0] for c in DEPTHWISE])
def test_depthwise_route_just_inside_its_limit(cid, geo, kind, bias_on, route, pins):
    g = Geom(depthwise=True, **geo)
    value, limit = pins(g)
    assert value < limit and limit - value <= max(1, limit // 256), f"{cid}: {value} is not just below {limit}"
    assert g.x_elems < 1 << 31 and g.y_elems < 1 << 31 and g.KH * g.KW <= 4096 and g.H < 1 << 20 and g.W < 1 << 20
    gen = _gen(sum(map(ord, cid)))
    x = _bf16_normal(g.x_elems, gen).view(g.B, g.cin, g.H, g.W)
    w = BytesWeight(g.OC, g.K, kind, gen)
    if kind != I8:
        w.scale = (w.scale.float() / 32).to(torch.bfloat16)
        w.factor = w.scale
    bias = _bias(g, bias_on, gen)
    y = _nan_output(g)
    st = call_depthwise(g, x, w, bias, y)
    assert st == 0, _status(st)
    assert quanto_hip.lib.last_kernel() == route
    what = f"{route} {g}"
    _check_written(y, what)
    check_pixels(y, x, g, w, sample_pixels(g, 2), bias, what)
    check_projection(y, x, g, w, bias, what)


# ---- refused: the first geometry beyond each clause, with operands of the full stated size -------------------------------------------------------
def _zeros(n, dtype):
    return torch.zeros((n,), dtype=dtype, device=DEV)


def _untouched(y):
    flat = y.view(-1)
    return all(bool(torch.isnan(flat[i:i + (1 << 28)]).all()) for i in range(0, flat.numel(), 1 << 28))


class _Operand:
    pass


def _full_size_weight(g, kind=I8, bits=8, gs=None):
    w = _Operand()
    w.kind, w.bits = kind, bits
    if bits == 8:
        w.data, w.scale = _zeros(g.OC * g.K, torch.int8), _zeros(g.OC, torch.bfloat16)
    else:
        w.gs = gs or g.K
        w.G = g.K // w.gs
        w.packed = _zeros(g.OC * g.K * bits // 8, torch.uint8)
        w.scale, w.shift = _zeros(g.OC * w.G, torch.bfloat16), _zeros(g.OC * w.G, torch.bfloat16)
    return w


REFUSED_DENSE = [  # (clause, geometry): one step beyond the accepted neighbour above
    ("pixel tiles", dict(B=32, cin=8, H=512, W=512, OC=8, KH=3, KW=3, p=(1, 1))),                     # the segmentation batch: 65536 tiles
    ("pixel tiles", dict(B=1, cin=8, H=1, W=65535 * 128 + 1, OC=8, KH=1, KW=1)),                      # one pixel more than 65535 tiles
    ("x elements", dict(B=1024, cin=64, H=128, W=128, OC=64, KH=3, KW=3, s=(2, 2), p=(1, 1))),        # 2^30 input elements (2 GiB)
    ("y elements", dict(B=4, cin=16, H=1024, W=1024, OC=512, KH=1, KW=1)),                            # 2^31 output elements (4 GiB)
    ("K", dict(B=1, cin=132105, H=1, W=127, OC=64, KH=1, KW=127)),                                    # K = 16 777 335
    ("K", dict(B=1, cin=1 << 24, H=1, W=1, OC=2, KH=1, KW=1)),                                        # K = 2^24
    ("OC K", dict(B=1, cin=4096, H=16, W=16, OC=58256, KH=3, KW=3, p=(1, 1))),                        # OC K = 2^31 + 65 536 (2 GiB of weight)
    ("taps", dict(B=1, cin=8, H=32, W=32, OC=8, KH=8, KW=16)),                                        # 128 taps
]


@pytest.mark.parametrize("route", ["qbytes", "qbits", "a8"])
@pytest.mark.parametrize("clause,geo", REFUSED_DENSE, ids=[f"{c.replace(' ', '_')}-{i}" for i, (c, _) in enumerate(REFUSED_DENSE)])
def test_first_geometry_beyond_a_clause_is_refused(clause, geo, route):
    g = Geom(**geo)
    assert _binding(g) == [clause], _binding(g)
    y = _nan_output(g)
    if route == "a8":
        assert a8_workspace_size(g, I8, I8) == ENOTSUP
        x, w = _zeros(g.x_elems, torch.int8), _full_size_weight(g)
        st = call_a8(g, x, torch.ones((1,), dtype=torch.bfloat16, device=DEV), w, None, y, I8, 0)
    elif route == "qbytes":
        x, w = _zeros(g.x_elems, torch.bfloat16), _full_size_weight(g)
        st = call_qbytes(g, x, w, None, y)
    else:
        x, w = _zeros(g.x_elems, torch.bfloat16), _full_size_weight(g, None, 4, 8 if g.K % 8 == 0 else None)
        st = call_qbits(g, x, w, None, y)
    assert st == ENOTSUP, _status(st)
    assert _untouched(y), "a refused call wrote to its output"


REFUSED_DW = [  # (clause, geometry): the depthwise rule's clauses - the probes of test_conv_size_limits_cpu.DW_PROBES that are affordable
    ("x elements", dict(B=128, cin=16, H=1024, W=1024, OC=16, KH=7, KW=7, s=(2, 2), p=(6, 6), d=(2, 2))),   # 2^31 input elements (4 GiB)
    ("y elements", dict(B=128, cin=8, H=1024, W=1024, OC=16, KH=3, KW=3, p=(1, 1))),                        # 2^31 output elements (4 GiB)
    ("taps", dict(B=2, cin=4, H=80, W=72, OC=8, KH=64, KW=65, p=(3, 5))),                                   # 4160 taps
    ("H", dict(B=2, cin=4, H=1 << 20, W=1, OC=4, KH=3, KW=1, p=(1, 0))),
    ("W", dict(B=2, cin=4, H=1, W=1 << 20, OC=8, KH=1, KW=3, p=(0, 1))),
]


@pytest.mark.parametrize("clause,geo", REFUSED_DW, ids=[f"{c.replace(' ', '_')}" for c, _ in REFUSED_DW])
def test_depthwise_first_geometry_beyond_a_clause_is_refused(clause, geo):
    """The C rule at the points where test_conv_size_limits_cpu.py pins the Python mirror: the two agree, H and W < 2^20 included."""
    g = Geom(depthwise=True, **geo)
    broken = {"x elements": g.x_elems >= 1 << 31, "y elements": g.y_elems >= 1 << 31, "taps": g.KH * g.KW > 4096, "H": g.H >= 1 << 20, "W": g.W >= 1 << 20}
    assert sorted(k for k, v in broken.items() if v) == [clause]
    x, w, y = _zeros(g.x_elems, torch.bfloat16), _full_size_weight(g), _nan_output(g)
    assert not quanto_hip.lib.qbytes_conv2d_depthwise_supported(x.view(g.B, g.cin, g.H, g.W), w.data.view(g.OC, 1, g.KH, g.KW), g.s, g.p, g.d)
    st = call_depthwise(g, x, w, None, y)
    assert st == ENOTSUP, _status(st)
    assert _untouched(y), "a refused call wrote to its output"


# ---- module level: beyond the rules a QConv2d leaves the convolution kernels and still matches the reference --------------------------------------
def _reference_conv(q, x, groups=1):
    """The reference path: dequantize the weight, float convolution (nn/qconv2d.py:54-55)."""
    return torch.nn.functional.conv2d(x, q.weight.dequantize(), q.bias, q.stride, q.padding, q.dilation, groups)


def test_qconv2d_beyond_the_tile_bound_leaves_the_convolution_kernels():
    """32 images with 512 x 512 outputs (65536 pixel tiles): conv2d_geometry_ok refuses, the QConv2d does not raise ENOTSUP and no convolution
    kernel runs - the dispatch (tensor/weights.py: qconv2d) lowers a dense convolution it cannot run implicitly to im2col + quanto::qbytes_mm,
    so last_kernel() names a matmul route, never a conv2d_* one - and the result is the reference path's (dequantize + float convolution)
    within the reference's own tolerance."""
    import optimum_quanto_amd as Q
    from helpers import assert_similar

    torch.manual_seed(0)
    conv = torch.nn.Conv2d(4, 8, 3, padding=1, bias=True).to(torch.bfloat16)
    q = Q.QConv2d.from_module(conv, weights=Q.qint8).to(DEV)
    Q.freeze(q)
    x = _bf16_normal(32 * 4 * 512 * 512, _gen(5)).view(32, 4, 512, 512)
    assert not quanto_hip.lib.conv2d_geometry_ok(tuple(x.shape), tuple(q.weight.shape), (1, 1), (1, 1), (1, 1))
    small = x[:1].contiguous()
    with torch.no_grad():
        q(small)
        assert quanto_hip.lib.last_kernel().startswith("conv2d_mfma")  # inside the rule: the implicit GEMM
        y = q(x)
        torch.cuda.synchronize()
        assert not quanto_hip.lib.last_kernel().startswith("conv2d"), quanto_hip.lib.last_kernel()
        for b0 in range(0, 32, 8):
            assert_similar(y[b0:b0 + 8], _reference_conv(q, x[b0:b0 + 8]))
            torch.testing.assert_close(y[b0:b0 + 8].float(), _reference_conv(q, x[b0:b0 + 8]).float(), rtol=2 ** -6, atol=2 ** -6)


def test_depthwise_qconv2d_with_2_to_the_20_rows_takes_the_reference_path():
    """H = 2^20: the C rule refuses (qconv_depthwise.hip) and, with the mirror's clause, the dispatch no longer asks the kernel - the layer
    keeps dequantize + float convolution, bit for bit, and last_kernel() is unchanged by the call."""
    import optimum_quanto_amd as Q

    torch.manual_seed(1)
    conv = torch.nn.Conv2d(4, 4, (3, 1), padding=(1, 0), groups=4, bias=True).to(torch.bfloat16)
    q = Q.QConv2d.from_module(conv, weights=Q.qint8).to(DEV)
    Q.freeze(q)
    with torch.no_grad():
        inside = _bf16_normal(4 * ((1 << 20) - 1), _gen(6)).view(1, 4, (1 << 20) - 1, 1)
        y_in = q(inside)
        assert quanto_hip.lib.last_kernel() == "conv2d_depthwise"
        torch.testing.assert_close(y_in.float(), _reference_conv(q, inside, 4).float(), rtol=2 ** -6, atol=2 ** -6)
        quanto_hip.lib.qbytes_mm(torch.ones((1, 64), dtype=torch.bfloat16, device=DEV), torch.ones((8, 64), dtype=torch.int8, device=DEV),
                                 torch.ones((8,), dtype=torch.bfloat16, device=DEV))
        before = quanto_hip.lib.last_kernel()
        assert not before.startswith("conv2d")
        x = _bf16_normal(4 << 20, _gen(7)).view(1, 4, 1 << 20, 1)
        y = q(x)
        torch.cuda.synchronize()
        assert quanto_hip.lib.last_kernel() == before
        assert torch.equal(y, _reference_conv(q, x, 4))

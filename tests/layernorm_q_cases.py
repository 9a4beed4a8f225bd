"""Inputs, oracle and accuracy condition shared by test_layernorm_q_cpu.py and test_layernorm_q_gpu.py (``quanto::layer_norm_q``).

Oracle for the codes: ``layer_norm`` in float64 on the CPU, cast to the tensor dtype T, then the Python ``quantize_symmetric`` of library/ops.py.

Condition, the same for every case: every code equals the oracle's or is its neighbouring representable code (int8 +-1, the adjacent float8 value),
and at most ``max(2, 1e-4 * numel)`` elements differ.  Where the figures come from: a sequence that computes its statistics in fp32 differs from the
float64 oracle only where the float element lands on the other side of a rounding boundary of T and that step crosses a code boundary; three fp32
roundings (about 2e-7 relative) against T's spacing and the code step give a share of 1e-5 or below for the three dtypes - torch's own CPU sequence and
an fp32 two-pass emulation measured <= 8e-6 over 512 rows of n in {33 .. 4096} - so the cap leaves ten times room and wrong statistics cannot pass it.
The CPU file proves the condition for the emulation on every input below and for torch's own CPU sequence on every input but the ``mean1000`` rows;
the GPU file asks it of the kernel.  On the ``mean1000`` rows torch's CPU layer_norm does not stay inside the cap, through no fault of its statistics:
it evaluates x * rstd - mean * rstd in fp32, two products of about 1000 * rstd whose roundings (half a unit of 2^-24 x 1000 x rstd each) are not small
against the difference.  ``torch_cpu_cap`` is the cap that formula can meet, from that error; measured there: 0 .. 20 differing codes in 3840 .. 20480,
all one step.

Input kinds (``Case.kind``):
 - ``random``: rows of N(offset_r, spread_r), weight 1 + 0.25 N(0, 1) (both signs occur), bias 0.5 N(0, 1); the output scale is 0.7 x absmax / qmax
   of the float64 output: the largest few percent clamp.
 - ``mean1000``: rows 1000 + 4 m_r + g k with k integers in [-3, 3] that sum to zero over the row and g the spacing of T at 1000 (bf16: 4, fp16: 0.5;
   fp32: 0.25 - the finest spacing at which an fp32 sum of a row of 4096 such values is still exact, fp32's own 2^-14 cannot be summed in fp32 at
   all).  Mean and squared deviations are exact in fp32 for a two-pass kernel; E[x^2] - mean^2 in fp32 loses the variance entirely (1e6 against
   at most 144): ``one_pass=True`` of the emulation fails the condition on these rows, asserted in the CPU file.
 - ``constant``: every row one value (3, -2, 1024, 0): var = 0, the codes are those of the bias alone.
 - ``outlier``: ``random`` with one element of every row at 1000.
 - ``saturate``: ``random`` with the output scale at 0.05 x absmax / qmax: most elements clamp, on both sides.
"""
import functools
from typing import NamedTuple, Optional, Tuple

import torch

from optimum_quanto_amd.library import ops as ops_mod

T_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
CODE_DTYPES = {"int8": torch.int8, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
CODE_QMAX = {"int8": 127.0, "e4m3": 448.0, "e5m2": 57344.0}
EPS = 1e-5
LIMIT = 8192  # LAYER_NORM_Q_MAX_N
WAVE_ROW_MAX_N = 1024  # up to here one wave holds a row, beyond a workgroup (csrc/layernorm_q.hip)


class Case(NamedTuple):
    kind: str
    lead: Tuple[int, ...]  # leading dimensions: their product is the row count
    norm: Tuple[int, ...]  # normalized_shape
    t: str = "bf16"
    code: str = "int8"
    affine: str = "wb"  # "wb": weight and bias, "w": no bias, "none": neither

    @property
    def id(self) -> str:
        return f"{self.kind}-{'x'.join(map(str, self.lead))}-{'x'.join(map(str, self.norm))}-{self.t}-{self.code}-{self.affine}"


class Problem(NamedTuple):
    x: torch.Tensor
    weight: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]
    scale: torch.Tensor  # 0-dim, T
    dtype: torch.dtype   # the code type
    norm: Tuple[int, ...]
    want: torch.Tensor   # the oracle's codes


# every edge of a load, store and reduction form: single elements, the dword and the unit of 8, one short of / exactly / one past a wave's 64 lanes x 8
# and x 16 (the wave-per-row form's two units, its last row length 1024), the workgroup form from 1025 on, a ragged unit in its last pass, the limit
ROW_LENGTHS = (1, 3, 4, 7, 8, 33, 63, 64, 65, 197, 255, 256, 257, 511, 512, 513, 768, 1000, 1024, 1025, 2047, 2049, 4096, 8191, LIMIT)
ROW_COUNTS = (1, 3, 5, 65)  # one row, fewer than a workgroup's four waves, one more than four, more than one workgroup in both forms

SHAPE_CASES = [Case("random", (rows,), (n,)) for n in ROW_LENGTHS for rows in ROW_COUNTS]
PAIR_CASES = [Case("random", (5,), (n,), t, code) for t in T_DTYPES for code in CODE_DTYPES for n in (197, 4096) if (t, code) != ("bf16", "int8")]
PARAM_CASES = [Case("random", (3,), (n,), t, "int8", affine) for affine in ("w", "none") for n, t in ((65, "bf16"), (2047, "bf16"), (257, "fp32"))]
ND_CASES = [Case("random", (2, 3), (8, 24)), Case("random", (2, 2), (48, 64)), Case("random", (2, 3), (6, 5, 7), "fp16", "e4m3")]
STAT_CASES = ([Case("mean1000", (5,), (n,), t) for t in T_DTYPES for n in (768, 4096)]
              + [Case("mean1000", (3,), (197,), "bf16", "e4m3"), Case("constant", (4,), (1000,)), Case("constant", (4,), (2048,), "fp16", "e5m2"),
                 Case("outlier", (5,), (768,)), Case("outlier", (5,), (4096,), "fp16"), Case("outlier", (3,), (1025,), "fp32", "e4m3"),
                 Case("saturate", (5,), (257,)), Case("saturate", (5,), (4096,), "fp16", "e4m3"), Case("saturate", (3,), (1024,), "fp32", "e5m2")])
# the inputs whose views the GPU file lays out differently (offset by one element, row strides n + 1 and n + 8, leading dimensions that do not collapse)
VIEW_CASES = [Case("random", (6,), (768,)), Case("random", (6,), (4096,)), Case("random", (6,), (200,), "fp32", "e4m3"), Case("random", (2, 3), (1032,), "fp16")]
# not served by the kernel: the sequence runs
BEYOND_CASES = [Case("random", (3,), (LIMIT + 1,))]
ALL_CASES = SHAPE_CASES + PAIR_CASES + PARAM_CASES + ND_CASES + STAT_CASES + VIEW_CASES + BEYOND_CASES
assert len({c.id for c in ALL_CASES}) == len(ALL_CASES)


def _seed(case: Case) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % (1 << 31)


def float64_layer_norm(x, norm, weight, bias, eps=EPS):
    d = torch.float64
    return torch.nn.functional.layer_norm(x.to(d), norm, None if weight is None else weight.to(d), None if bias is None else bias.to(d), eps)


def oracle_codes(x, norm, weight, bias, scale, dtype, eps=EPS):
    """float64 layer norm, cast to T, the Python quantize_symmetric."""
    return ops_mod.quantize_symmetric(float64_layer_norm(x, norm, weight, bias, eps).to(x.dtype), dtype, None, scale)


@functools.lru_cache(maxsize=None)
def problem(case: Case) -> Problem:
    """The case's tensors on the CPU and the oracle's codes: built once, shared, never modified."""
    T, dtype = T_DTYPES[case.t], CODE_DTYPES[case.code]
    gen = torch.Generator().manual_seed(_seed(case))
    rows, n = 1, 1
    for d in case.lead:
        rows *= d
    for d in case.norm:
        n *= d
    f64 = dict(generator=gen, dtype=torch.float64)
    if case.kind == "mean1000":
        g = {"bf16": 4.0, "fp16": 0.5, "fp32": 0.25}[case.t]
        half = torch.randint(-3, 4, (rows, n // 2), generator=gen).to(torch.float64)
        k = torch.cat([half, -half] + ([torch.zeros(rows, 1, dtype=torch.float64)] if n % 2 else []), dim=1)
        k = torch.stack([k[r, torch.randperm(n, generator=gen)] for r in range(rows)])
        centre = 1000.0 + 4.0 * torch.randint(-2, 3, (rows, 1), generator=gen).to(torch.float64)
        x = centre + g * k
    elif case.kind == "constant":
        x = torch.tensor([3.0, -2.0, 1024.0, 0.0])[:rows].to(torch.float64).reshape(rows, 1).expand(rows, n).clone()
    else:
        offset, spread = torch.randn((rows, 1), **f64) * 2, 0.25 + 2 * torch.rand((rows, 1), **f64)
        x = offset + spread * torch.randn((rows, n), **f64)
        if case.kind == "outlier":
            x[torch.arange(rows), torch.randint(0, n, (rows,), generator=gen)] = 1000.0
    x = x.to(T).reshape(case.lead + case.norm)
    assert case.kind != "mean1000" or torch.equal(x.to(torch.float64).reshape(rows, n).mean(1), centre.reshape(rows))  # every value is exact in T
    weight = (1 + 0.25 * torch.randn(case.norm, **f64)).to(T) if case.affine in ("wb", "w") else None
    bias = (0.5 * torch.randn(case.norm, **f64)).to(T) if case.affine == "wb" else None
    peak = float64_layer_norm(x, case.norm, weight, bias).abs().max().clamp_min(1e-3)
    scale = (peak * (0.05 if case.kind == "saturate" else 0.7) / CODE_QMAX[case.code]).to(T)
    assert scale.ndim == 0 and float(scale) > 0
    return Problem(x, weight, bias, scale, dtype, case.norm, oracle_codes(x, case.norm, weight, bias, scale, dtype))


def ordinal(codes: torch.Tensor) -> torch.Tensor:
    """The position of every code among the representable values of its type, as int32: neighbouring values differ by one (both float8 zeros are 0)."""
    if codes.dtype == torch.int8:
        return codes.to(torch.int32)
    bits = codes.view(torch.uint8).to(torch.int32)
    magnitude = bits & 0x7F
    return torch.where(bits >= 0x80, -magnitude, magnitude)


def difference(got: torch.Tensor, want: torch.Tensor):
    """(number of differing elements, largest distance in code steps, cap on the number) of two code tensors."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    got, want = got.cpu(), want.cpu()
    differing = int((got.view(torch.uint8) != want.view(torch.uint8)).sum())
    steps = int((ordinal(got) - ordinal(want)).abs().max()) if got.numel() else 0
    return differing, steps, max(2, int(1e-4 * got.numel()))


def assert_condition(got: torch.Tensor, want: torch.Tensor, what: str):
    differing, steps, cap = difference(got, want)
    print(f"{what}: {differing} of {got.numel()} codes differ (cap {cap}), largest distance {steps} code step(s)")
    assert steps <= 1, f"{what}: a code {steps} steps from the oracle's"
    assert differing <= cap, f"{what}: {differing} codes differ, the cap is {cap}"


def torch_cpu_cap(p: Problem) -> int:
    """The number of differing codes torch's CPU sequence may show on a ``mean1000`` input: its x * rstd - mean * rstd carries an absolute error of up
    to 2 x 2^-24 x max|x| x rstd (two products rounded to fp32, a third rounding in the difference is smaller), which moves the float element across
    a code boundary for a share of 2 x error / code step of the elements - the code step of int8 is the scale - times |weight| <= 2; a factor 2 on top
    for the rounding to T in between."""
    assert p.dtype == torch.int8
    n = p.want.shape[-1]
    x = p.x.reshape(-1, n).to(torch.float64)
    rstd = 1 / torch.sqrt(x.var(1, unbiased=False) + EPS)
    error = 2 * 2.0 ** -24 * float((x.abs().amax(1) * rstd).max())
    return max(2, int(p.want.numel() * 2 * 2 * 2 * error / float(p.scale)))


def emulated_codes(p: Problem, one_pass: bool = False) -> torch.Tensor:
    """What csrc/layernorm_q.hip computes, in torch on the CPU: fp32 statistics in two passes (``one_pass``: the E[x^2] - mean^2 form the kernel must
    not use), rstd = 1 / sqrt(var + eps), the affine step in fp32 rounded once to T, the Python quantize_symmetric on that.  Only the order of the
    sums differs from the kernel's."""
    n = 1
    for d in p.norm:
        n *= d
    x = p.x.reshape(-1, n).to(torch.float32)
    mean = x.sum(1, keepdim=True) / n
    d = x - mean
    var = ((x * x).sum(1, keepdim=True) / n - mean * mean).clamp_min(0) if one_pass else (d * d).sum(1, keepdim=True) / n
    y = d * (1 / torch.sqrt(var + EPS))
    if p.weight is not None:
        y = y * p.weight.reshape(1, n).to(torch.float32)
    if p.bias is not None:
        y = y + p.bias.reshape(1, n).to(torch.float32)
    return ops_mod.quantize_symmetric(y.to(p.x.dtype).reshape(p.x.shape), p.dtype, None, p.scale)

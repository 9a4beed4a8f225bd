"""Every matmul and convolution route bit-exact on problems whose arithmetic is exact.

Each row of tests/containment_cases.py for the ten product entries, at its own type, at the other 16-bit type and at every 8-bit weight type the plan
accepts (tests/exact_cases.py ``variants``), runs the two designed problems of tests/exact_cases.py straight through the C ABI, its buffers in a
``containment.Arena``:

* pass A: one-hot activations sweep every weight column (up to 512 launches of one row into one output region each); the output must be the oracle's
  decode of the selected element times its scale - every code of the weight type, every position inside a packed byte, every scale and zero-point by its
  own row and group;
* pass B: dense integer activations with a mean, all weight codes, without and with an integer bias; the output must be the float64 product rounded
  once to the output type (the bias launch: in the order of ``exact_cases.ROUNDS_BY_DESIGN``).  A route listed in ``exact_cases.EXEMPT`` - there is
  none - would keep the tolerance gate it has elsewhere in the suite on this data.  The float8 x float8 routes take float8 codes no further apart than
  ``exact_cases.PIPE_SPAN``, so that the sum inside their K = 128 matrix instruction is exact as well;
* pass C, the routes that multiply the dequantized weight rounded to the activation type (``exact_cases.ROUNDED_WEIGHT_ROUTES``) only: pass B with
  float shifts large enough that this rounding rounds, half of the weights at a tie.

Both are compared with ``==`` on every element (the sign of a zero is not asserted).  The host file (tests/test_exact_routes_cpu.py) asserts that the
designs cover what they claim and satisfy the bound under which no fp32 partial sum rounds.  One test per entry; a failing row does not hide the others,
and its message gives the first wrong element, the value got and the value wanted.
"""
import numpy as np
import pytest
import torch

import containment_cases as C
import exact_cases as E
from containment import Arena
from helpers import assert_close_to_exact, assert_close_with_bias, to_numpy
from optimum_quanto_amd.library.hip import quanto_hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK_BYTES = 32 << 20  # activation bytes of the launches that share one arena
ALIGN = 256


def _stacked(t):
    """[n, ...] -> (uint8 [n * stride], stride, bytes per slice): every slice starts on a 256-byte boundary."""
    raw = t.contiguous().reshape(t.shape[0], -1).view(torch.uint8)
    nb = raw.shape[1]
    stride = -(-nb // ALIGN) * ALIGN
    buf = torch.zeros((t.shape[0], stride), dtype=torch.uint8)
    buf[:, :nb] = raw
    return buf.reshape(-1), stride, nb


class Launch:
    """The arena as one launch sees it: stacked regions at the launch's slice, the bias regions only where the launch passes a bias."""

    def __init__(self, arena, offsets, with_bias):
        self.arena, self.offsets, self.with_bias = arena, offsets, with_bias

    def ptr(self, name):
        if name.startswith("bias") and not self.with_bias:
            return 0
        p = self.arena.ptr(name)
        return p + self.offsets.get(name, 0) if p else 0


def _first_wrong(got, want):
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {want.size} elements wrong, first at launch {i[0]}, index {i[1:]}: got {got[i]!r}, want {want[i]!r}"


def _run(row, v, pas):
    """One variant of a row through one pass; raises AssertionError naming the first wrong element."""
    fam, d = C.family(row), E.design(v, pas)
    plan = fam.plan(v)
    assert plan.status == C.OK, f"plan status {plan.status}"
    per_launch = sum(t[0].numel() * t.element_size() for t in d.acts(0, 1).values())
    chunk = max(1, min(d.launches, CHUNK_BYTES // per_launch))
    sets = {name: _stacked(t) for name, t in d.sets.items()}
    for l0 in range(0, d.launches, chunk):
        l1 = min(d.launches, l0 + chunk)
        a = Arena(0xFF, DEV)
        for name, t in d.static.items():
            a.add_input(name, t)
        strides = {}
        for name, t in d.acts(l0, l1).items():
            buf, strides[name], _ = _stacked(t)
            a.add_input(name, buf)
        for name, (buf, _, _) in sets.items():
            a.add_input(name, buf)
        out_bytes = {}
        for name, (dtype, shape) in d.outputs.items():
            nb = C.nbytes(dtype, shape)
            strides[name], out_bytes[name] = -(-nb // ALIGN) * ALIGN, nb
            a.add_output(name, (l1 - l0) * strides[name])
        if plan.ws_bytes > 0:
            a.add_workspace("ws", plan.ws_bytes, counters=row.counters)
        a.build()
        for l in range(l0, l1):
            offsets = {name: (l - l0) * s for name, s in strides.items()}
            offsets.update({name: d.set_of(l) * s for name, (_, s, _) in sets.items()})
            st = fam.call(v, Launch(a, offsets, d.bias_on(l)), a.ptr("ws"), plan.ws_bytes)
            assert st == C.OK, f"pass {pas} launch {l}: status {st}"
            if row.name is not None and l in (l0, l1 - 1):
                assert quanto_hip.lib.last_kernel() == row.name, f"pass {pas}: ran {quanto_hip.lib.last_kernel()}, the row says {row.name}"
        torch.cuda.synchronize()
        a.check(f"pass {pas} launches {l0}..{l1 - 1}")
        want = d.want(l0, l1)
        for name, (dtype, shape) in d.outputs.items():
            raw = a.bytes(name).cpu().reshape(l1 - l0, strides[name])[:, :out_bytes[name]].contiguous()
            got = to_numpy(raw.view(dtype).reshape((l1 - l0,) + tuple(shape)))
            if pas != "A" and E.exempted(row):  # the gate the route has elsewhere in the suite, on the same data
                for l in range(l0, l1):
                    product, bias = d.exact(l)[name]
                    if bias is None:
                        assert_close_to_exact(got[l - l0], product, v.f["dt"], f"pass B launch {l} (exempted: {E.exempted(row)['cite']})")
                    else:
                        assert_close_with_bias(got[l - l0], product, bias, v.f["dt"], f"pass B launch {l} (exempted: {E.exempted(row)['cite']})")
                continue
            wrong = _first_wrong(got, want[name])
            assert wrong is None, f"pass {pas} launches {l0}..{l1 - 1} output '{name}': {wrong}"


def _rows(monkeypatch, rows, wanted):
    """Every variant of ``rows`` through the passes ``wanted(row, pas)`` selects; every failure is reported, by row and variant."""
    failures, runs = [], 0
    for row in rows:
        with monkeypatch.context() as m:
            C.knobs_env(row, m)
            for v in E.variants(row):
                for pas in E.passes(row):
                    if not wanted(row, pas):
                        continue
                    runs += 1
                    try:
                        _run(row, v, pas)
                    except AssertionError as e:
                        failures.append(f"[{v.id}] {e}")
    assert runs and not failures, f"{len(failures)} of {runs} runs failed:\n" + "\n".join(failures)


@pytest.mark.parametrize("entry", E.ENTRIES)
def test_every_route_returns_the_exact_bits(monkeypatch, entry):
    """No row and no pass is skipped; a route of exact_cases.EXEMPT (none today) is held to its tolerance gate in the dense passes (``_run``)."""
    _rows(monkeypatch, E.GROUPS[entry], lambda row, pas: True)

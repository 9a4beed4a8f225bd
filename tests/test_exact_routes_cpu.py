"""Host part of the exact-route tests: the designed problems of tests/exact_cases.py show what they claim, satisfy the bound under which fp32
accumulation is exact in any order, are planned onto the route their row names - and the registered torch-expression ops, run on them on the host, give
the expected bits (an independent check of the oracle rule the device file, tests/test_exact_routes_gpu.py, compares against)."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import containment_cases as C
import exact_cases as E
from helpers import to_numpy
from test_containment_cpu import expected_name


def test_the_ten_product_entries_are_the_scope():
    products = {e for e, fam in C.FAMILIES.items() if fam is not C.Elementwise}
    assert set(E.ENTRIES) == products and len(E.ENTRIES) == 10
    assert len(E.ROWS) == sum(1 for r in C.ROWS if r.entry in products), "the table is not shrunk"


def test_numbers():
    assert E.lowbit(np.array([0.0, 1.0, 6.0, 0.375, -448.0, 2.0 ** -16])).tolist() == [np.inf, 1.0, 2.0, 0.125, 64.0, 2.0 ** -16]
    assert E.expect(np.array([257.0]), "bf16").tolist() == [256.0] and E.expect(np.array([259.0]), "bf16").tolist() == [260.0]  # ties to even
    # the bias on a 16-bit output (ROUNDS_BY_DESIGN): 257 -> 256, + 1 = 257 -> 256; rounded once 258 would stay 258
    assert E.expect(np.array([257.0]), "bf16", np.array([1.0])).tolist() == [256.0] and E.expect(np.array([257.0]), "fp32", np.array([1.0])).tolist() == [258.0]
    with pytest.raises(AssertionError, match="24 bits"):
        E.expect(np.array([2.0 ** 24 + 1]), "fp32")
    assert len(E.byte_values("int8")) == 256 and len(E.byte_values("e4m3fn")) == 254 and len(E.byte_values("e5m2")) == 248 and len(E.byte_values("e4m3fnuz")) == 255
    for kind in ("e4m3fn", "e5m2", "e4m3fnuz"):  # the window of pass B: both signs, a zero, and a real share of the codes even at the largest K of the table
        v = E.decode(E.bounded_bytes(kind, 3 * 1536, "fp16"), kind)
        assert len(v) >= 60 and (v > 0).any() and (v < 0).any() and (v == 0).any(), (kind, len(v))
        assert np.abs(v).max() * 3 * 1536 < 2.0 ** 24 * E.lowbit(v).min()


def test_what_is_rounded_by_design_is_cited():
    assert [r["what"] for r in E.ROUNDS_BY_DESIGN] == ["bias on a 16-bit output"], "a new entry is a finding: DESIGN.md 'Parity' lists each"
    for r in E.ROUNDS_BY_DESIGN:
        assert r["why"] and r["expected"]
        for cite in r["cites"]:
            path, line = cite.split(":")
            with open(os.path.join(C.ROOT, "optimum_quanto_amd", path)) as fh:
                assert "bias" in fh.read().splitlines()[int(line) - 1], cite
    # the rule is written once, in the helper's header: no file under csrc/ but the cited ones holds the round-add-round expression (a cite beyond
    # the header's is a unit whose measurement kept its statements inline - a finding, recorded in that unit's comment)
    rule = re.compile(r"to_f32\(E::from_f32\([^()]*(\([^()]*\)[^()]*)*\)\)\s*\+")  # T(v) + ..., v any expression
    holders = []
    for path in sorted(glob.glob(os.path.join(C.ROOT, "optimum_quanto_amd", "csrc", "*.h*"))):  # *.h, *.hip
        with open(path) as fh:
            if rule.search(fh.read()):
                holders.append(os.path.basename(path))
    cited = sorted({os.path.relpath(cite.split(":")[0], "csrc") for cite in E.ROUNDS_BY_DESIGN[0]["cites"]})
    assert cited == ["qh_common.h", "qmm_native8.hip"] and holders == cited, holders


def test_every_exemption_names_a_route_and_a_line():
    assert [(e["entry"], e["name"]) for e in E.EXEMPT] == [], "a new entry is a finding: DESIGN.md 'Parity' lists each"
    for e in E.EXEMPT:
        assert any(E.exempted(r) is e for r in E.ROWS) and e["why"] and e["measured"]
        path, line = e["cite"].split(":")
        with open(os.path.join(C.ROOT, "optimum_quanto_amd", path)) as fh:
            assert fh.read().splitlines()[int(line) - 1].strip(), e["cite"]
    assert sum(1 for r in E.ROWS if E.exempted(r)) == 0 and len(E.ROWS) == 107


def test_float8_products_stay_inside_the_matrix_pipe_window():
    """Every float8 x float8 row - and no other - carries the "matrix-pipe window" condition in pass B; its line is the instruction the comment cites."""
    with open(os.path.join(C.ROOT, "optimum_quanto_amd", "csrc", "qconv_a8.hip")) as fh:
        assert "mfma_scale_f32_16x16x128_f8f6f4" in fh.read().splitlines()[290 - 1]
    assert E.pipe_span("e4m3fn", "e5m2") == E.PIPE_SPAN and E.pipe_span("int8", "int8") == E.pipe_span("bf16", "e4m3fn") == np.inf
    assert 3 * E.PIPE_SPAN < E.PIPE_WINDOW
    for kind in E.FP8_KINDS:
        v = E.decode(E.bounded_bytes(kind, 3 * 45, "bf16", E.PIPE_SPAN), kind)
        assert len(v) >= 60 and (v > 0).any() and (v < 0).any() and np.abs(v).max() <= E.PIPE_SPAN * E.lowbit(v).min(), (kind, len(v))
    both = 0
    for row in E.ROWS:
        f = row.f
        fp8 = f.get("a") in E.FP8_KINDS and f.get("b") in E.FP8_KINDS
        both += fp8
        with E.knobs(row):
            piped = [b for b in E.design(row, "B").bounds if b.what == "matrix-pipe window"]
        assert bool(piped) == fp8, row.id
        assert all(b.worst < 1.0 for b in piped), row.id
    assert both >= 6


def _plan_matches(row, v):
    base, plan = C.family(row).plan(row), C.family(row).plan(v)
    assert plan.status == C.OK and plan.kernel == base.kernel, (v.id, plan)
    if plan.kernel is not None:
        assert expected_name(v, plan) == row.name, (v.id, expected_name(v, plan))
    assert (plan.ws_bytes > 0) == row.wants_workspace, (v.id, plan.ws_bytes)


def _check_variant_set(row, vs):
    f = row.f
    kinds = {(v.f["dt"], v.f.get("b")) for v in vs}
    assert len(kinds) == len(vs) and vs[0] is row
    if row.entry != "qbytes_bmm" and f.get("a", f["dt"]) in ("bf16", "fp16"):
        assert {v.f["dt"] for v in vs} == {"bf16", "fp16"}, f"{row.id}: the other 16-bit type is not planned onto the same kernel"
        if row.entry in E.WEIGHT_TYPES:
            types = {v.f["b"] for v in vs}  # e4m3fnuz where the kernel decodes it (the 128-tile MFMA kernel's plan refuses it)
            assert {"int8", "e4m3fn", "e5m2"} <= types <= set(E.WEIGHT_TYPES[row.entry]), f"{row.id}: weight types {sorted(types)}"


@pytest.mark.parametrize("row", E.ROWS, ids=[r.id for r in E.ROWS])
def test_designs_cover_stay_exact_and_match_the_default_ops(monkeypatch, row):
    C.knobs_env(row, monkeypatch)
    vs = E.variants(row)
    _check_variant_set(row, vs)
    for v in vs:
        _plan_matches(row, v)
        for pas in E.passes(row):
            d = E.design(v, pas)
            what = f"{v.id} pass {pas}"
            assert 1 <= d.launches <= E.MAX_LAUNCHES, what
            assert E.coverage(d, pas) == [], what
            for b in d.bounds:
                assert b.worst < 1.0, f"{what}: {b.what}: sum |x| |w| reaches {b.worst:.3f} of 2^24 u"
            if pas != "A":
                x = d.facts["x"]
                assert abs(x.mean()) >= 0.5 or x.min() == -128, f"{what}: activations without a mean"
                assert (x < 0).any() or x.shape[0] < 4, f"{what}: no signed activation"
                assert d.bounds or v.f.get("a", row.f.get("b")) == "int8" or row.entry == "qbytes_bmm", f"{what}: a float accumulation without a bound"
                assert any(d.bias_on(l) for l in range(d.launches)) == (row.entry != "qbytes_bmm"), what
            # the registered ops on the host: pass A's first and last launch, every launch of pass B
            for l in sorted({0, d.launches - 1} if pas == "A" else range(d.launches)):
                want, got = d.want(l, l + 1), d.default_op(l)
                for name, (dtype, shape) in d.outputs.items():
                    assert got[name].dtype == dtype and tuple(got[name].shape) == tuple(shape), what
                    np.testing.assert_array_equal(to_numpy(got[name]), want[name][0], err_msg=f"{what} launch {l} '{name}'")


def test_variants_reach_every_weight_type_somewhere():
    seen = set()
    for row in E.ROWS:
        with E.knobs(row):
            seen |= {(row.entry, v.f.get("b"), v.f["dt"]) for v in E.variants(row)}
    for entry, types in E.WEIGHT_TYPES.items():
        for b in types:
            for dt in ("bf16", "fp16"):
                assert (entry, b, dt) in seen, (entry, b, dt)
    assert ("qbytes_mm_ws", "int8", "fp32") in seen and ("qbits_mm", None, "fp32") in seen


def test_a_wrong_index_or_code_changes_the_expectation():
    """The designs separate what the issue's mutations confuse: neighbouring rows and groups differ in scale, -128 is not -127, and truncation is not
    round-to-nearest-even on the dense data."""
    w = E.qbits_weight(40, 512, 4, 128, "bf16")
    s = w.regions["scale"].to(torch.float32).reshape(40, 4)
    assert bool((s[:, 1:] != s[:, :-1]).all()) and bool((s[1:] != s[:-1]).all())
    for step in (8, 16, 32, 64, 128, 256):  # tile-sized index errors
        assert (E._pot(np.arange(300)) != E._pot(np.arange(300) + step)).all()
    b = E.qbytes_weight(19, 45, "int8", "bf16")
    assert (b.codes.view(np.int8) == -128).any() and b.w64.min() <= -128 * 2.0 ** -4
    row = C.BY_ID["qbytes_mm_ws-mfma-129x131x256-bf16xint8"]
    d = E.design(row, "B")
    y = d.want(0, 1)["y"][0]
    exact = d.facts["x"] @ d.facts["weights"][0][0].w64.T
    trunc = (exact.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    assert (trunc != y).mean() > 0.2, "the dense design has too few values that need rounding"

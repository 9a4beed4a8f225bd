"""Host part of the containment tests: the arena's own checks, the case table against the library's plan entries ("needs no device") and the list of
C entries the table must cover.  The device part is tests/test_containment_gpu.py."""
import ctypes
import os

import pytest
import torch

import containment_cases as C
from containment import GUARD, SENTINEL, WS_COUNTER_BYTES, WS_GUARD, Arena, ContainmentError
from optimum_quanto_amd.library import hip


# ---- the arena on the host: a torch stand-in for a kernel breaks one rule at a time -----------------------------------------------------------------
def _arena(fill):
    a = Arena(fill, device="cpu")
    a.add_input("x", torch.arange(1001, dtype=torch.int16))         # 2002 bytes: ragged end
    a.add_input("w", torch.arange(77, dtype=torch.uint8))
    a.add_output("y", 3 * 67 * 2)
    a.add_workspace("ws", WS_COUNTER_BYTES + 12345, counters=True)
    a.add_workspace("scratch", 999, counters=False)
    return a.build()


def _good_kernel(a):
    """Stores every output byte, uses counters and partials and leaves the counters zero."""
    a.bytes("y").copy_(torch.arange(a.size("y"), dtype=torch.int32).to(torch.uint8))
    a.bytes("ws")[8:12] = 3
    a.bytes("ws")[WS_COUNTER_BYTES:] = 0x11
    a.bytes("ws")[8:12] = 0
    a.bytes("scratch").fill_(0x22)


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_arena_layout_and_fills(fill):
    a = _arena(fill)
    regions = list(a.regions.values())
    for r in regions:
        assert r.start % 256 == 0 and r.guard == (WS_GUARD if r.kind == "ws" else GUARD)
    for prev, nxt in zip(regions, regions[1:]):
        assert nxt.start - prev.end >= prev.guard + nxt.guard  # each keeps its own guard on each side
    assert regions[0].start >= GUARD and a.buf.numel() >= regions[-1].end + regions[-1].guard
    x, y, ws, scratch = (a.regions[n] for n in ("x", "y", "ws", "scratch"))
    assert bool((a.buf[x.end:x.end + GUARD] == fill).all()) and bool((a.buf[x.start - GUARD:x.start] == fill).all())      # inputs: the fill
    assert bool((a.buf[y.start - GUARD:y.start] == SENTINEL).all()) and bool((a.buf[y.end:y.end + GUARD] == SENTINEL).all())
    assert bool((a.bytes("y") == SENTINEL).all())
    assert bool((a.buf[ws.start - WS_GUARD:ws.start] == SENTINEL).all()) and bool((a.buf[ws.end:ws.end + WS_GUARD] == SENTINEL).all())
    assert not bool(a.bytes("ws")[:WS_COUNTER_BYTES].any()) and bool((a.bytes("ws")[WS_COUNTER_BYTES:] == fill).all())
    assert bool((a.bytes("scratch") == fill).all())  # no counter contract: the whole body takes the fill
    assert torch.equal(a.view("x", torch.int16, (1001,)), torch.arange(1001, dtype=torch.int16))


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_a_clean_call_passes(fill):
    a = _arena(fill)
    _good_kernel(a)
    a.check("clean")
    a.assert_written("y", 2, "clean")
    assert a.counters_are_zero("ws")


BREAKS = [  # (what the stand-in does wrong, region named, words of the message)
    ("byte behind an input", "x", lambda a, r: a.buf.__setitem__(r.end, 0x5A), ["guard behind 'x'", "1 bytes changed", "first at +0, last at +0"]),
    ("byte before an input", "w", lambda a, r: a.buf.__setitem__(r.start - 1, 0x5A), ["guard in front of 'w'", f"first at {-77 - 1:+d}"]),
    ("byte behind an output", "y", lambda a, r: a.buf.__setitem__(r.end, 0), ["guard behind 'y'", "first at +0"]),
    ("byte before an output", "y", lambda a, r: a.buf.__setitem__(r.start - 1, 0), ["guard in front of 'y'", f"first at {-402 - 1:+d}"]),
    ("byte behind a workspace", "ws", lambda a, r: a.buf.__setitem__(r.end, 0), ["guard behind 'ws'", "first at +0"]),
    ("byte before a workspace", "ws", lambda a, r: a.buf.__setitem__(r.start - 1, 0), ["guard in front of 'ws'"]),
    ("a whole stray 128 x 128 fp32 tile behind a workspace", "ws", lambda a, r: a.buf[r.end + 64:r.end + 64 + 65536].zero_(),
     ["guard behind 'ws'", "65536 bytes changed", "first at +64, last at +65599"]),
    ("flipped input byte", "x", lambda a, r: a.buf.__setitem__(r.start + 1000, int(a.buf[r.start + 1000]) ^ 0x80), ["input 'x'", "1 bytes changed", f"first at {1000 - 2002:+d}"]),
    ("counter word left non-zero", "ws", lambda a, r: a.buf.__setitem__(r.start + 40, 1), ["counters of 'ws'", "1 bytes not restored to zero"]),
]


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("what,region,wrong,words", BREAKS, ids=[b[0] for b in BREAKS])
def test_each_broken_rule_is_reported_with_its_region(fill, what, region, wrong, words):
    a = _arena(fill)
    _good_kernel(a)
    wrong(a, a.regions[region])
    with pytest.raises(ContainmentError) as e:
        a.check(what)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    for other in a.regions:
        if other != region:
            assert f"'{other}'" not in str(e.value), str(e.value)


def test_unwritten_output_elements_are_reported():
    a = _arena(0x00)
    _good_kernel(a)
    a.bytes("y")[100:104] = SENTINEL  # two bf16 elements a ragged tile never stored
    with pytest.raises(AssertionError, match="never stored"):
        a.assert_written("y", 2, "tail")
    b = _arena(0x00)
    b.assert_untouched("y", "refused call")
    _good_kernel(b)
    with pytest.raises(AssertionError, match="refused"):
        b.assert_untouched("y", "refused call")


# ---- the table against the plan entries -----------------------------------------------------------------------------------------------------------------
def expected_name(row, plan):
    """The last-kernel name the planned kernel reports (csrc/c_api.hip), None where the plan entry makes no kernel choice."""
    if row.entry in ("qbits_mm", "qbytes_mm_ws"):
        f32 = row.f["dt"] == "fp32" and plan.kernel in (C.GEMV, C.MFMA)
        return C.KERNEL_NAMES[plan.kernel] + ("_f32" if f32 else "")
    if row.entry in ("qbits_mm_multi_ws", "qbytes_mm_multi_ws"):
        if plan.kernel == C.AUTO:  # separate calls: the last member's kernel
            return C.KERNEL_NAMES[C.family(row).member_kernels(row)[-1]]
        return {C.GEMV: "gemv_multi", C.SKINNY: "skinny_multi"}[plan.kernel]
    return None


@pytest.mark.parametrize("row", C.ROWS, ids=[r.id for r in C.ROWS])
def test_row_is_served_as_the_table_says(monkeypatch, row):
    C.knobs_env(row, monkeypatch)
    plan = C.family(row).plan(row)
    assert plan.status == C.OK, f"a row its route does not serve is a wrong row: status {plan.status}"
    if plan.kernel is not None:
        if row.kernel != C.AUTO or "multi" in row.entry:
            assert plan.kernel == row.kernel
        assert expected_name(row, plan) == row.name
    assert (plan.ws_bytes > 0) == row.wants_workspace, f"workspace bytes {plan.ws_bytes}, the row says split={row.split} scratch={row.scratch}"
    if plan.ws_bytes_other is not None:
        assert plan.ws_bytes_other == plan.ws_bytes, "the *_plan and *_workspace_size entries disagree"
    if row.counters:
        assert row.split is not None or row.scratch
    if row.split and row.counters:
        assert plan.ws_bytes > WS_COUNTER_BYTES


def test_every_kernel_of_the_enum_is_in_the_table(monkeypatch):
    seen = set()
    for row in C.ROWS:
        if row.entry in ("qbits_mm", "qbytes_mm_ws"):
            with monkeypatch.context() as m:
                C.knobs_env(row, m)
                seen.add(C.family(row).plan(row).kernel)
    assert seen == set(C.KERNEL_NAMES), f"missing: {sorted(C.KERNEL_NAMES[k] for k in set(C.KERNEL_NAMES) - seen)}"
    assert any(r.kernel == C.AUTO and r.entry in ("qbits_mm", "qbytes_mm_ws") for r in C.ROWS)


def test_every_split_capable_family_is_in_the_table_split_and_unsplit():
    assert {e for e, _ in C.SPLIT_FAMILIES} >= {"qbits_mm", "qbytes_mm_ws", "qbits_mm_multi_ws", "qbytes_mm_multi_ws", "qbits_mm_a8", "qbytes_conv2d",
                                                "qbits_conv2d", "qbytes_conv2d_a8"}
    names = {n for _, n in C.SPLIT_FAMILIES}
    assert names >= {"skinny", "mfma_large", "mfma_fused4", "mfma_native8", "skinny_multi", "conv2d_mfma", "conv2d_mfma_rows", "conv2d_a8_int8", "conv2d_a8_fp8"}
    for entry, name in C.SPLIT_FAMILIES:
        states = {r.split for r in C.ROWS if (r.entry, r.name) == (entry, name)}
        if name in ("conv2d_a8_fp8_w8", "conv2d_mfma_int2", "conv2d_rows_dequant_int2"):  # one more format of a kernel that is there in both states
            continue
        assert states == {True, False}, f"{entry} / {name}: only split states {states}"


def test_every_last_kernel_name_of_the_header_is_in_the_table():
    listed = C.header_kernel_names()
    assert {"naive", "gemv", "mmv", "skinny", "skinny_multi", "mfma", "mfma_large", "mfma_native8", "mfma_fused4", "mfma_large4", "dequant_mfma",
            "conv2d_mfma", "conv2d_mfma_int4", "conv2d_a8_int8", "conv2d_a8_fp8", "conv2d_a8_fp8_w8", "bmm_i8"} <= listed
    in_table = {r.name for r in C.ROWS}
    assert listed <= in_table, f"names of the header without a row: {sorted(listed - in_table)}"


# ---- nothing escapes ------------------------------------------------------------------------------------------------------------------------------------
def _stores_into_caller_memory(argtypes):
    """An entry that takes device pointers besides its stream: operands plus an output or a workspace (the plan and size entries take none, the
    capture query takes its stream alone)."""
    if not argtypes:
        return False
    pointers = sum(1 for t in argtypes if t in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)))
    return pointers >= 3


def test_every_entry_that_stores_is_in_the_table_or_covered_elsewhere():
    storing = {name for name, (_, argtypes) in hip._PROTOTYPES.items() if _stores_into_caller_memory(argtypes)}
    assert "quanto_hip_qbits_mm" in storing and "quanto_hip_unpack" in storing and "quanto_hip_qbits_mm_plan" not in storing
    in_table = {"quanto_hip_" + r.entry for r in C.ROWS}
    assert in_table <= storing
    assert not (in_table & set(C.COVERED_ELSEWHERE)), "an entry is either in the table or covered elsewhere"
    missing = storing - in_table - set(C.COVERED_ELSEWHERE)
    assert not missing, f"entries of include/quanto_hip.h that store into caller memory and no containment test runs: {sorted(missing)}"
    assert set(C.COVERED_ELSEWHERE) <= storing, "COVERED_ELSEWHERE names an entry the binding does not have"
    for where in C.COVERED_ELSEWHERE.values():
        path, test = where.split("::")
        with open(os.path.join(C.ROOT, path)) as fh:
            assert f"def {test.split(' ')[0]}(" in fh.read(), where

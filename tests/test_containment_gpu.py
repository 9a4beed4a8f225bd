"""Every kernel writes only its output and its own workspace.

Each row of tests/containment_cases.py runs straight through the C ABI with every buffer of the call - operands, outputs, workspace - laid out in one
``containment.Arena``: regions on 256-byte boundaries that end at their natural byte, guard bytes from the very next byte on.  Three properties are asserted:

* writes stay inside the outputs and the workspace bytes the plan entry reported (``Arena.check``: no guard byte changed, no operand byte changed), with
  the workspace region EXACTLY as large as reported, 16 bytes short of it, and absent;
* a workspace under the counter contract of include/quanto_hip.h has its counter region all zero after every call, read back directly;
* the result is a function of the operand bytes only: the same call in an arena whose fill byte is 0x00 and in one whose fill is 0xFF (NaN behind every
  float operand, all-ones nibbles behind packed weights, 0xFF in the partial sums nobody wrote yet) gives bit-identical outputs, which also pass the oracle
  gate the route has elsewhere in the suite.  No tolerance is defined in this file.
"""
import pytest
import torch

import containment_cases as C
from containment import SENTINEL, WS_COUNTER_BYTES, Arena
from optimum_quanto_amd.library.hip import quanto_hip

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _layout(row, fill, ws_bytes):
    """The row's problem uploaded into a fresh arena: operands, outputs, then ``ws_bytes`` of workspace (none for 0)."""
    prob = C.problem(row)
    a = Arena(fill, DEV)
    for name, t in prob.inputs.items():
        a.add_input(name, t)
    for name, (dtype, shape) in prob.outputs.items():
        a.add_output(name, C.nbytes(dtype, shape))
    if ws_bytes > 0:
        a.add_workspace("ws", ws_bytes, counters=row.counters)
    return prob, a.build()


def _outputs(prob, a):
    return {name: a.view(name, dtype, shape) for name, (dtype, shape) in prob.outputs.items()}


def _call(row, a, ws_ptr, ws_bytes):
    st = C.family(row).call(row, a, ws_ptr, ws_bytes)
    torch.cuda.synchronize()
    return st


def _elem_size(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _for_each_row(monkeypatch, rows, body):
    """``body(row)`` for every row under the row's knobs; a row that fails does not hide the others: every failure is reported, by row."""
    failures = []
    for row in rows:
        with monkeypatch.context() as m:
            C.knobs_env(row, m)
            try:
                body(row)
            except AssertionError as e:
                failures.append(f"[{row.id}] {e}")
    assert not failures, f"{len(failures)} of {len(rows)} rows failed:\n" + "\n".join(failures)


def _exact_size_workspace_both_fills(row):
    plan = C.family(row).plan(row)
    assert plan.status == C.OK and (plan.ws_bytes > 0) == row.wants_workspace
    results = {}
    for fill in (0x00, 0xFF):
        prob, a = _layout(row, fill, plan.ws_bytes)
        st = _call(row, a, a.ptr("ws"), plan.ws_bytes)
        assert st == C.OK, f"fill {fill:#04x}: status {st}"
        if row.name is not None:
            assert quanto_hip.lib.last_kernel() == row.name
        a.check(f"fill {fill:#04x}")
        if prob.elem_check:
            for name, (dtype, _) in prob.outputs.items():
                a.assert_written(name, _elem_size(dtype), f"fill {fill:#04x}")
        results[fill] = _outputs(prob, a)
    for name in results[0x00]:
        x, y = results[0x00][name].view(torch.uint8), results[0xFF][name].view(torch.uint8)
        n = int((x != y).sum())
        assert n == 0, (f"{n} bytes of '{name}' differ between the arena filled with 0x00 and the one filled with 0xFF: the result depends on bytes "
                        f"outside the operands or on scratch nobody wrote")
    prob.gate(results[0x00], plan.ws_bytes)


# One test per group of rows (an entry of the C ABI; the elementwise entries together), every row of the group inside it: the table has 126 rows, and
# the suite's result log is not the place for one line per row and pass.
@pytest.mark.parametrize("group", list(C.GROUPS))
def test_exact_size_workspace_both_fills(monkeypatch, group):
    _for_each_row(monkeypatch, C.GROUPS[group], _exact_size_workspace_both_fills)


def _short_or_null_workspace(row, mode):
    """16 bytes less than reported, or NULL: the call runs unsplit, steps down or refuses (include/quanto_hip.h) - and stores nothing behind what it was given."""
    plan = C.family(row).plan(row)
    assert plan.ws_bytes > 16
    ws_bytes = plan.ws_bytes - 16 if mode == "short" else 0
    prob, a = _layout(row, 0xFF, ws_bytes)
    st = _call(row, a, a.ptr("ws"), ws_bytes)
    assert st in (C.OK, C.EINVAL), f"workspace {mode}: status {st}"
    a.check(f"workspace {mode}")
    if st == C.OK:
        if prob.elem_check:
            for name, (dtype, _) in prob.outputs.items():
                a.assert_written(name, _elem_size(dtype), f"workspace {mode}")
        prob.gate(_outputs(prob, a), ws_bytes)
    else:
        for name in prob.outputs:
            a.assert_untouched(name, f"workspace {mode}")


WS_GROUPS = {g: [r for r in rows if r.wants_workspace] for g, rows in C.GROUPS.items() if any(r.wants_workspace for r in rows)}


@pytest.mark.parametrize("group", list(WS_GROUPS))
def test_short_and_null_workspace(monkeypatch, group):
    for mode in ("short", "null"):
        _for_each_row(monkeypatch, WS_GROUPS[group], lambda row: _short_or_null_workspace(row, mode))


COUNTER_ROWS = [r for r in C.ROWS if r.counters]


def test_back_to_back_on_one_workspace_leaves_the_counters_zero(monkeypatch):
    """Every row under the counter contract, in table order and once more in reverse, on ONE workspace whose counter region was zeroed once: the counter
    region is read back after every call."""
    sizes = []
    for row in COUNTER_ROWS:
        with monkeypatch.context() as m:
            C.knobs_env(row, m)
            sizes.append(C.family(row).plan(row).ws_bytes)
    shared = Arena(0xFF, DEV)
    shared.add_workspace("ws", max(sizes), counters=True)
    shared.build()
    for row in COUNTER_ROWS + COUNTER_ROWS[::-1]:
        with monkeypatch.context() as m:
            C.knobs_env(row, m)
            prob, a = _layout(row, 0x00, 0)
            st = _call(row, a, shared.ptr("ws"), shared.size("ws"))
            assert st == C.OK, f"{row.id}: status {st}"
            assert quanto_hip.lib.last_kernel() == row.name
            assert shared.counters_are_zero("ws"), f"{row.id} left {int(shared.bytes('ws')[:WS_COUNTER_BYTES].count_nonzero())} counter bytes non-zero"
            shared.check(row.id)
            a.check(row.id)
            prob.gate(_outputs(prob, a), shared.size("ws"))


# ---- the Python binding: what it hands the kernels -----------------------------------------------------------------------------------------------------
def _row(prefix, **knobs):
    want = C._knobs(**knobs)
    hits = [r for r in C.ROWS if r.id.startswith(prefix) and r.knobs == want]
    assert len(hits) == 1, (prefix, [r.id for r in hits])
    return hits[0]


def _dev(prob):
    return {k: v.to(DEV) for k, v in prob.inputs.items()}


def _zero_ws_buffers(lib):
    stream = torch.cuda.current_stream().cuda_stream
    return [buf for (_, s, capture), buf in lib.__dict__.get("_zero_ws", {}).items() if s == stream and capture == 0]


def test_the_binding_keeps_its_counter_workspace_zero_and_away_from_scratch_writers(monkeypatch):
    lib = quanto_hip.lib
    splitting = [_row("qbits_mm-skinny-16x1024x8192"), _row("qbits_mm-mfma_fused4-130x264x1024", FUSED4_BM=64, FUSED4_SPLIT=2),
                 _row("qbytes_mm_ws-mfma_large-129x131x1024", LARGE_SPLIT=2), _row("qbits_mm_multi_ws-skinny_multi", SKINNY_SPLIT=2),
                 _row("qbytes_mm_multi_ws-skinny_multi", SKINNY_SPLIT=2), _row("qbits_mm_a8-a8_fused_int8-65x136x512", A8_SPLIT=2)]
    scratch = [_row("qbits_mm-dequant_mfma-130x258x384"), _row("qbits_mm-mfma-129x130x384-int4g128"),
               _row("qbytes_conv2d-conv2d_mfma-b2c29", CONV_SPLIT=2)]

    def run(row):
        prob = C.problem(row)
        t, f = _dev(prob), row.f
        if row.entry == "qbits_mm":
            M, N, K = row.shape
            out = {"y": lib.qbits_mm(t["x"], t["packed"], t["scale"], t["shift"], None, f["bits"], f["gs"] or None, N, K,
                                     kernel="auto" if row.kernel == C.AUTO else row.name)}
        elif row.entry == "qbytes_mm_ws":
            out = {"y": lib.qbytes_mm(t["a"], t["b"], t["scales"].reshape(-1), None, kernel=row.name)}
        elif row.entry == "qbits_mm_multi_ws":
            M, Ns, K = row.shape
            n = range(len(Ns))
            ys = lib.qbits_mm_multi(t["x"], [t[f"packed{i}"] for i in n], [t[f"scale{i}"] for i in n], [t[f"shift{i}"] for i in n], None, 4, 128, list(Ns), K)
            out = {f"y{i}": y for i, y in enumerate(ys)}
        elif row.entry == "qbytes_mm_multi_ws":
            M, Ns, K = row.shape
            n = range(len(Ns))
            ys = lib.qbytes_mm_multi(t["a"], [t[f"b{i}"] for i in n], [t[f"scales{i}"].reshape(-1) for i in n], None)
            out = {f"y{i}": y for i, y in enumerate(ys)}
        elif row.entry == "qbits_mm_a8":
            M, N, K = row.shape
            out = {"y": lib.qbits_mm_a8(t["a"], t["a_scale"], t["packed"], t["scale"], t["shift"], None, f["bits"], 128, N, K)}
        else:
            g = row.shape
            out = {"y": lib.qbytes_conv2d(t["x"], t["w"], t["scales"], None, g.s, g.p, g.d)}
        torch.cuda.synchronize()
        assert lib.last_kernel() == row.name, (row.id, lib.last_kernel())
        prob.gate({k: v.cpu() for k, v in out.items()})

    for row in splitting:
        with monkeypatch.context() as m:
            C.knobs_env(row, m)
            run(row)
    live = _zero_ws_buffers(lib)
    assert live, "the split-K calls above took a zero-initialised workspace for this stream"
    for buf in live:
        assert not bool(buf[:WS_COUNTER_BYTES].any()), "counter region of the binding's split-K workspace is not zero after the calls"
        buf[WS_COUNTER_BYTES:].fill_(SENTINEL)
    for row in scratch:
        with monkeypatch.context() as m:
            C.knobs_env(row, m)
            run(row)
    assert [b.data_ptr() for b in _zero_ws_buffers(lib)] == [b.data_ptr() for b in live], "a scratch-taking call replaced the split-K workspace"
    for buf in live:
        assert not bool(buf[:WS_COUNTER_BYTES].any()), "a kernel that writes from offset 0 was handed the split-K workspace: its counter region is not zero"
        assert bool((buf[WS_COUNTER_BYTES:] == SENTINEL).all()), "a kernel that takes plain scratch was handed the split-K workspace"
    with monkeypatch.context() as m:  # and the split-K kernels still find their counters zero
        C.knobs_env(splitting[0], m)
        run(splitting[0])

"""An arena for "where does a kernel write" tests: every buffer of ONE call (inputs, outputs, workspace) is a named region of one uint8 tensor.

Layout: every region starts on a 256-byte boundary and ends at its natural, ragged byte; guard bytes start at the very next byte and run to the next region.
An operand or an output has at least ``GUARD`` (4 KiB) of guard on each side, a workspace ``WS_GUARD`` (256 KiB, more than one 128 x 128 fp32 partial tile:
a whole stray tile still lands in guard bytes of this allocation).

Fills.  The arena has one selectable byte, ``fill`` (0x00 or 0xFF; 0xFF reads as NaN in bf16 / fp16 / fp32 and e4m3fn, as -1 in int8 and as all-ones nibbles
in packed int4 / int2):

* guards around inputs take ``fill`` - what a load past the end of an operand meets;
* guards around outputs and workspaces take ``SENTINEL`` (0xA5), so that a stray zero store is seen too;
* an output body is prefilled with ``SENTINEL``;
* a workspace body takes ``fill``; its counter region (the first ``WS_COUNTER_BYTES``) is zeroed when the entry's contract says "zero on entry".

``check()`` (after a device synchronisation) asserts that every guard byte is unchanged, that every input region holds the bytes that were uploaded and that
the counter region of a workspace under the counter contract is all zero again.  The message names the region, the first and last offending byte offsets
relative to the region's END (a negative offset below -size lies in front of the region) and how many bytes changed.

The same class runs on the host (``device="cpu"``) - tests/test_containment_cpu.py breaks each rule with a torch stand-in for a kernel.
"""
from typing import Dict, List, NamedTuple, Optional

import torch

SENTINEL = 0xA5          # helpers.SENTINEL
GUARD = 4096             # bytes of guard on each side of an operand / output
WS_GUARD = 256 * 1024    # ... of a workspace
WS_COUNTER_BYTES = 4096  # QUANTO_HIP_WS_COUNTER_BYTES (include/quanto_hip.h)
ALIGN = 256


class Region(NamedTuple):
    name: str
    kind: str       # "in", "out" or "ws"
    start: int
    size: int
    guard: int
    counters: bool  # ws: the counter contract holds (zero on entry, zero after the call)

    @property
    def end(self) -> int:
        return self.start + self.size


class ContainmentError(AssertionError):
    pass


class Arena:
    def __init__(self, fill: int, device="cuda"):
        assert fill in (0x00, 0xFF)
        self.fill, self.device = fill, device
        self._pending: List[tuple] = []
        self.regions: Dict[str, Region] = {}
        self.buf: Optional[torch.Tensor] = None

    # -- declaring the regions (before build) --------------------------------------------------------------------------------------------------
    def add_input(self, name: str, data: torch.Tensor):
        """``data``: a host tensor of any dtype; its bytes are uploaded."""
        raw = data.detach().cpu().contiguous().reshape(-1).view(torch.uint8)
        self._pending.append((name, "in", raw.numel(), GUARD, False, raw))

    def add_output(self, name: str, nbytes: int):
        self._pending.append((name, "out", int(nbytes), GUARD, False, None))

    def add_workspace(self, name: str, nbytes: int, counters: bool):
        self._pending.append((name, "ws", int(nbytes), WS_GUARD, bool(counters), None))

    def build(self) -> "Arena":
        names = [p[0] for p in self._pending]
        assert len(set(names)) == len(names), "region names are unique"
        offset, spans, layout = 0, [], []  # spans: (lo, hi, byte) guard fills
        for name, kind, size, guard, counters, raw in self._pending:
            assert size > 0, f"{name}: an empty region has no address (pass NULL instead)"
            start = -(-(offset + guard) // ALIGN) * ALIGN
            byte = self.fill if kind == "in" else SENTINEL
            spans.append((offset, start, byte))
            spans.append((start + size, start + size + guard, byte))
            layout.append((Region(name, kind, start, size, guard, counters), raw))
            offset = start + size + guard
        host = torch.empty((offset,), dtype=torch.uint8)
        protected = torch.zeros((offset,), dtype=torch.bool)
        for lo, hi, byte in spans:
            host[lo:hi] = byte
            protected[lo:hi] = True
        for r, raw in layout:
            body = host[r.start:r.end]
            if r.kind == "in":
                body.copy_(raw)
                protected[r.start:r.end] = True
            elif r.kind == "out":
                body.fill_(SENTINEL)
            else:
                body.fill_(self.fill)
                if r.counters:
                    body[:WS_COUNTER_BYTES].zero_()
            self.regions[r.name] = r
        raw = torch.empty((offset + ALIGN,), dtype=torch.uint8, device=self.device)  # (host allocations are 64-byte aligned)
        lead = -raw.data_ptr() % ALIGN
        self.buf = raw[lead:lead + offset]
        self.buf.copy_(host)
        assert self.buf.data_ptr() % ALIGN == 0
        self._want = self.buf.clone()
        self._protected = protected.to(self.device)
        return self

    # -- addresses and views ---------------------------------------------------------------------------------------------------------------------
    def ptr(self, name: Optional[str]) -> int:
        if name is None or name not in self.regions:
            return 0
        return self.buf.data_ptr() + self.regions[name].start

    def size(self, name: str) -> int:
        return self.regions[name].size if name in self.regions else 0

    def bytes(self, name: str) -> torch.Tensor:
        r = self.regions[name]
        return self.buf[r.start:r.end]

    def view(self, name: str, dtype: torch.dtype, shape) -> torch.Tensor:
        """The region as a tensor of ``dtype`` (a copy on the host: the region need not end on an element boundary of a wider view)."""
        return self.bytes(name).cpu().clone().view(dtype).reshape(shape)

    # -- the checks ------------------------------------------------------------------------------------------------------------------------------
    def _sync(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()

    def counters_are_zero(self, name: str) -> bool:
        self._sync()
        return not bool(self.bytes(name)[:WS_COUNTER_BYTES].any())

    def check(self, what: str = ""):
        self._sync()
        problems = []
        bad = (self.buf != self._want) & self._protected
        if bool(bad.any()):
            regions = list(self.regions.values())
            for i, r in enumerate(regions):
                lo = regions[i - 1].end + regions[i - 1].guard if i else 0
                for label, a, b in (("guard in front of", lo, r.start), ("input", r.start, r.end if r.kind == "in" else r.start),
                                    ("guard behind", r.end, r.end + r.guard)):
                    idx = bad[a:b].nonzero()
                    if idx.numel():
                        first, last = int(idx[0]) + a - r.end, int(idx[-1]) + a - r.end
                        problems.append(f"{label} '{r.name}' ({r.kind}, {r.size} bytes): {idx.numel()} bytes changed, first at {first:+d}, last at {last:+d} "
                                        f"relative to the region's end")
        for r in self.regions.values():
            if r.kind == "ws" and r.counters:
                idx = self.buf[r.start:r.start + min(r.size, WS_COUNTER_BYTES)].nonzero()
                if idx.numel():
                    problems.append(f"counters of '{r.name}' (ws, {r.size} bytes): {idx.numel()} bytes not restored to zero, first at "
                                    f"{int(idx[0]) - r.size:+d}, last at {int(idx[-1]) - r.size:+d} relative to the region's end")
        if problems:
            raise ContainmentError((what + ": " if what else "") + "; ".join(problems))

    def assert_written(self, name: str, elem_size: int, what: str = ""):
        """No run of SENTINEL bytes longer than one element survives in an output: every element was stored."""
        self._sync()
        s = (self.bytes(name) == SENTINEL).cpu()
        if s.numel() > elem_size:
            runs = s.unfold(0, elem_size + 1, 1).all(dim=1)
            idx = runs.nonzero()
            assert idx.numel() == 0, (f"{what}: '{name}' keeps {idx.numel()} windows of {elem_size + 1} prefilled bytes, first at byte {int(idx[0])}, last at "
                                      f"byte {int(idx[-1]) + elem_size} of {s.numel()}: elements that were never stored")

    def assert_untouched(self, name: str, what: str = ""):
        self._sync()
        n = int((self.bytes(name) != SENTINEL).sum())
        assert n == 0, f"{what}: {n} bytes of '{name}' were written by a call that was refused"

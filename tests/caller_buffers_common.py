"""Shared by the caller-buffer tests (``tests/test_caller_buffers_conditions.py``, ``tests/test_gpu_caller_buffers.py``); importable
without a GPU, and the arena itself works on CPU tensors as on device ones.

The contract (``include/k2b.h``, Conventions): buffers are caller-owned - an entry never writes an input, writes
every element of its outputs and nothing else, and the four fitted parameters of ``k2b_fit_world``, ``k2b_fit_image``,
``k2b_fit_multiview`` and ``k2b_fit_world_lbfgs`` may be the very buffers of their inputs.

``keypoints2body_amd.native`` hands every result out of ``torch.empty``: the caching allocator rounds a block up to 512 bytes, so a
write one element past an output lands in slack or in a neighbour's block and no comparison notices.  ``Arena`` is the caller's
buffer instead: ONE flat float32 tensor out of which every requested output is carved as a contiguous view, with guard floats in
front of and directly behind each view, everything pre-filled with one sentinel bit pattern (a quiet NaN with a payload no
arithmetic produces).  ``native.outputs_from(arena.provider)`` makes the wrappers write into the views; ``arena.check`` then holds
that every guard float still has the sentinel's bits and that no output element has.  Comparisons are on int32 views: as floats a
NaN is unequal to itself.

Layout, in floats: a view starts on a 256-byte boundary (64 floats; the arena's base is 256-byte aligned: asserted); the guard in
front of it is at least ``max(4 KiB, bytes of one row of the leading index)`` long and ends where the view begins; the guard behind
it begins at the first float after the view's last element and is as long.  A row: everything under one value of the leading index
(a frame, a sequence), so that a kernel that writes one frame too many, or one frame too early, lands inside a guard whatever the
row's length.  Neighbouring views share nothing: the space between two views holds the back guard of the first, then the front
guard of the second."""
from dataclasses import dataclass

import numpy as np
import torch

SENTINEL_BITS = 0x7FC5A5A5             # a quiet NaN; payload 0x45A5A5
ALIGN_BYTES = 256
MIN_GUARD_BYTES = 4096
_ALIGN = ALIGN_BYTES // 4
_SENTINEL_I32 = int(np.array(SENTINEL_BITS, dtype=np.uint32).view(np.int32))


def _numel(shape) -> int:
    return int(np.prod(tuple(shape), dtype=np.int64))


def guard_floats(shape) -> int:
    """Floats of each guard of an output of `shape`: at least 4 KiB, at least one row of the leading index."""
    shape = tuple(shape)
    row = _numel(shape[1:]) if len(shape) >= 1 else 1
    return max(MIN_GUARD_BYTES // 4, row)


@dataclass(frozen=True)
class Span:
    name: str
    shape: tuple
    front: int            # first float of the front guard
    start: int            # first float of the view
    stop: int             # first float behind the view = first float of the back guard
    back_stop: int        # first float behind the back guard


def layout(requests):
    """(spans, total floats) for `requests`: (name, shape) pairs or a name -> shape dict, in order."""
    items = list(requests.items()) if isinstance(requests, dict) else list(requests)
    spans, at = [], 0
    for name, shape in items:
        shape = tuple(int(n) for n in shape)
        g = guard_floats(shape)
        start = -(-(at + g) // _ALIGN) * _ALIGN
        stop = start + _numel(shape)
        spans.append(Span(name, shape, at, start, stop, stop + g))
        at = stop + g
    return spans, at


class Arena:
    """One flat float32 tensor on `device` holding every output of `requests` between guards (module docstring)."""

    def __init__(self, requests, device="cpu"):
        self.spans, total = layout(requests)
        assert len({s.name for s in self.spans}) == len(self.spans), "an output is requested twice"
        # the allocation's base is aligned far beyond 256 bytes on the device; a CPU allocation is not, so take the slack here
        raw = torch.empty(total + _ALIGN, dtype=torch.float32, device=device)
        skip = (-raw.data_ptr() // 4) % _ALIGN
        self.flat = raw[skip:skip + total]
        assert self.flat.data_ptr() % ALIGN_BYTES == 0 and raw.data_ptr() % 4 == 0
        self.bits = self.flat.view(torch.int32)
        self.bits.fill_(_SENTINEL_I32)
        self.views = {s.name: self.flat[s.start:s.stop].view(s.shape) for s in self.spans}
        self.asked = []

    def provider(self, name, shape):
        """For ``native.outputs_from``: the view of `name` (its shape is the wrapper's to check), None for an unknown name."""
        self.asked.append(name)
        return self.views.get(name)

    def outputs(self) -> dict:
        return dict(self.views)

    def guards(self):
        """(span, side, first float, end float) of every guard."""
        for s in self.spans:
            yield s, "front", s.front, s.start
            yield s, "back", s.stop, s.back_stop

    def check(self, what: str, unwritten_ok=()):
        """Every guard float still holds the sentinel, and no element of an output does (`unwritten_ok`: names whose elements
        are documented as unspecified)."""
        bits = self.bits.detach().cpu()
        for s, side, a, b in self.guards():
            bad = torch.nonzero(bits[a:b] != _SENTINEL_I32).flatten()
            if bad.numel():
                first, last = int(bad[0]), int(bad[-1])
                rel = (lambda i: i - (b - a)) if side == "front" else (lambda i: i + 1)      # floats before the view / behind its last element
                row = _numel(s.shape[1:]) if s.shape else 1
                raise AssertionError(
                    f"{what}: {int(bad.numel())} floats of the {side} guard of {s.name} {s.shape} were written: offsets {rel(first):+d} .. {rel(last):+d} "
                    f"floats from the output's {'first' if side == 'front' else 'last'} element (a row is {row} floats; first value "
                    f"{float(self.flat[a + first]):.6g})")
        for s in self.spans:
            if s.name in unwritten_ok:
                continue
            left = torch.nonzero(bits[s.start:s.stop] == _SENTINEL_I32).flatten()
            if left.numel():
                row = max(_numel(s.shape[1:]) if s.shape else 1, 1)
                raise AssertionError(f"{what}: {int(left.numel())} elements of {s.name} {s.shape} were never written: flat offsets {int(left[0])} .. "
                                     f"{int(left[-1])} (rows {int(left[0]) // row} .. {int(left[-1]) // row})")


def requests_like(outputs: dict) -> list:
    """(name, shape) of every tensor of a result dict: the arena of the same call."""
    return [(k, tuple(v.shape)) for k, v in outputs.items() if v is not None]


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _bits(a):
    if isinstance(a, torch.Tensor):
        t = a.detach()
        if t.dtype in (torch.float32, torch.int32):
            return t.contiguous().view(torch.int32)
        return t.contiguous().view(torch.uint8)
    return np.ascontiguousarray(a)


def snapshot(inputs: dict) -> dict:
    """A copy of every input of a call: device tensors (cloned, on their device), host index arrays (numpy, lists)."""
    out = {}
    for k, a in inputs.items():
        if a is None:
            continue
        out[k] = a.detach().clone() if isinstance(a, torch.Tensor) else np.array(a, copy=True)
    return out


def assert_inputs_unwritten(inputs: dict, snap: dict, what: str):
    """Every input still has the bits of its snapshot (``torch.equal`` on int32 views: a NaN input compares equal to itself)."""
    assert {k for k, a in inputs.items() if a is not None} == set(snap), (what, sorted(inputs), sorted(snap))
    for k, was in snap.items():
        now = inputs[k]
        if isinstance(was, torch.Tensor):
            a, b = _bits(now), _bits(was)
            if a.shape != b.shape or not torch.equal(a, b):
                bad = torch.nonzero((a != b).flatten()).flatten()
                raise AssertionError(f"{what}: the input {k} {tuple(now.shape)} was written: {int(bad.numel())} elements, flat offsets {int(bad[0])} .. {int(bad[-1])}")
        else:
            assert np.array_equal(np.asarray(now), was), f"{what}: the host array {k} was written"


# ---- batch sizes of the fused fit kernel ---------------------------------------------------------------------------------------------
FUSED_BATCHES = (1, 5, 17)             # every one odd: the last slot pair of the shapes that carry two frames per wave is half filled
HOST_CU_COUNTS = (1, 8, 256, 304)
SPILL_BATCH = 17                       # one frame more than the paired and the wide shape hold: a second workgroup with one frame

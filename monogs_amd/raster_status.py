"""``StatusLedger`` -- who remembers the rasteriser's device status words until somebody reads them.

Every forward leaves one int32 word on the device (``MGS_STATUS_*``, include/monogs_raster.h): capacity overflowed and
instances were dropped, or the depth sort / the tile sort gave up a look-back wait.  This module is the host bookkeeping
around those words and around the capacity hints they feed -- plain Python over one-element tensors, no native library: the
only things it does to a word are ``.item()`` and, for a device tensor, a synchronise of its device first.  It is therefore
driven with CPU ``int32`` tensors in tests/test_raster_status_host.py.  ``monogs_amd.rasterizer`` keeps the one instance.

Four kinds of memory, each bounded:

  hints      (P, W, H) -> instance count a capacity-mode forward sizes its scratch from; at most HINTS_MAX, oldest first out.
  pending    words of EAGER capacity-mode forwards, forgotten by the check that reads them; at most PENDING_MAX.
  exact      the last exact forward's word (the next exact forward of the same stream reads it at its own count read-back),
             the words parked because their successor ran on another stream, and the timeout bits collected from words that
             had to be read early.
  captured   words of forwards recorded inside a hipGraph capture.  A replay rewrites them, so every check reads them
             again, for as long as their OWNER lives: each belongs to one ``GraphFlags`` handle, and ``release()`` of that
             handle is the only thing that forgets them.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from ._lib import H

HINTS_MAX, PENDING_MAX = 64, 1024
STATUS_CAPACITY_OVERFLOW, STATUS_DEPTH_SORT_TIMEOUT = H.MGS_STATUS_CAPACITY_OVERFLOW, H.MGS_STATUS_DEPTH_SORT_TIMEOUT
STATUS_TILE_SORT_TIMEOUT = H.MGS_STATUS_TILE_SORT_TIMEOUT
_TIMEOUTS = STATUS_DEPTH_SORT_TIMEOUT | STATUS_TILE_SORT_TIMEOUT


def raise_sort_failure(bits):
    which = [n for b, n in ((STATUS_DEPTH_SORT_TIMEOUT, "depth sort"), (STATUS_TILE_SORT_TIMEOUT, "tile sort")) if bits & b]
    raise RuntimeError(f"rasteriser: a look-back spin of the {' and the '.join(which)} timed out; "
                       "the renders since the last check are invalid")


def _drain(words) -> None:
    """A status word is written by its forward's kernels on the stream (and device) that forward ran on; ``.item()`` only
    waits for the CURRENT stream, so drain the devices involved first."""
    for d in {w.device for w in words if w.is_cuda}:
        torch.cuda.synchronize(d)


class GraphFlags:
    """The status words of the forwards ONE owner captured (a driver's graphs, a test's graph).  ``with handle:`` around the
    capture routes the captured forwards here; ``release()`` when the graphs are destroyed."""

    def __init__(self, ledger: "StatusLedger"):
        self._ledger = ledger
        self.words: List[Tuple[tuple, torch.Tensor]] = []       # (key, word) per captured forward, in capture order
        self.released = False

    def __len__(self):
        return len(self.words)

    def __enter__(self):
        if self.released:
            raise RuntimeError("this GraphFlags handle was released: take a new one from graph_flags()")
        self._ledger._active.append(self)
        return self

    def __exit__(self, *exc):
        self._ledger._active.remove(self)
        return False

    def accumulate(self, sticky: torch.Tensor) -> None:
        """Inside a capture, right after a forward: ``sticky |= status`` (int32[1]) as a captured op, and the check reads
        ``sticky`` in place of that forward's own word.  A forward REWRITES its status word, so a graph that is replayed many
        times between two checks shows the last replay's only; with this the check sees an overflow (or a sort timeout) of any
        replay since the caller last zeroed ``sticky`` -- what a graph that serves cameras of different instance counts needs."""
        if not self.words:
            raise RuntimeError("GraphFlags.accumulate: this handle has recorded no forward to accumulate")
        key, word = self.words[-1]
        sticky.bitwise_or_(word)
        self.words[-1] = (key, sticky)

    def release(self) -> None:
        """Forget this handle's words (its graphs are gone).  Idempotent; nobody else's words are touched."""
        self.words = []
        if not self.released:
            self.released = True
            self._ledger._handles.remove(self)


class StatusLedger:
    def __init__(self):
        self.hints: dict = {}
        self.pending: list = []           # (key, word) of eager capacity-mode forwards not yet checked
        self.exact_pending = None         # (key, word, device index, raw stream) of the last exact forward, or None
        self.exact_other: list = []       # the same of exact forwards whose successor ran on ANOTHER stream: only check() reads them
        self.exact_failed = 0             # timeout bits collected from earlier exact forwards, raised by the next forward / check
        self._handles: List[GraphFlags] = []      # the live handles, in order of creation
        self._active: List[GraphFlags] = []       # the handles whose ``with`` block is open, innermost last
        self._anonymous: Optional[GraphFlags] = None

    # ---- capacity hints --------------------------------------------------------------------------------------------------
    def hint(self, key) -> Optional[int]:
        return self.hints.get(key)

    def remember_hint(self, key, R) -> None:
        h = self.hints
        if key not in h and len(h) >= HINTS_MAX:
            h.pop(next(iter(h)))
        h[key] = R

    def forget_hint(self, key) -> None:
        self.hints.pop(key, None)

    # ---- capacity-mode forwards ------------------------------------------------------------------------------------------
    def graph_flags(self) -> GraphFlags:
        h = GraphFlags(self)
        self._handles.append(h)
        return h

    def record_capacity(self, key, word, capturing: bool) -> None:
        if capturing:       # the innermost open handle, or the anonymous one (a bare torch.cuda.graph around a forward)
            if self._active:
                h = self._active[-1]
            else:
                if self._anonymous is None or self._anonymous.released:
                    self._anonymous = self.graph_flags()
                h = self._anonymous
            h.words.append((key, word))
            return
        self.pending.append((key, word))
        if len(self.pending) > PENDING_MAX:      # nobody is checking: the oldest half is dropped UNREAD (last item)
            del self.pending[:PENDING_MAX // 2]

    def captured_words(self) -> list:
        return [kw for h in self._handles for kw in h.words]

    def release_all(self) -> None:
        for h in list(self._handles):
            h.release()

    # ---- exact forwards --------------------------------------------------------------------------------------------------
    def exact_rider(self, device: int, stream: int) -> Optional[torch.Tensor]:
        """The previous exact forward's word, if the forward about to run on ``(device, stream)`` may read it at its count
        read-back.  A word written on another stream / device is not ordered before that read-back (the header's contract is
        "an EARLIER forward on this stream"): it is parked for check()."""
        prev = self.exact_pending
        if prev is None:
            return None
        if (prev[2], prev[3]) == (device, stream):
            return prev[1]
        self.exact_pending = None
        self.exact_other.append(prev)
        if len(self.exact_other) > PENDING_MAX:
            self._read_parked(PENDING_MAX // 2)      # (read, never dropped: a sort timeout must not pass unseen)
        return None

    def exact_rider_read(self, bits: int) -> None:
        """The count read-back happened; ``bits`` is what it found in the rider (0 without one).  Never silent."""
        self.exact_pending = None
        if bits & _TIMEOUTS:
            raise_sort_failure(bits)

    def record_exact(self, key, word, device: int, stream: int) -> None:
        self.exact_pending = (key, word, device, stream)

    def _read_parked(self, n: int) -> None:
        """Nobody calls check(): read the oldest ``n`` parked words and keep their timeout bits in ``exact_failed``, which the
        next forward raises -- the list stays bounded without losing the one signal it exists to deliver."""
        old, self.exact_other = self.exact_other[:n], self.exact_other[n:]
        _drain([e[1] for e in old])
        for e in old:
            self.exact_failed |= int(e[1].item()) & _TIMEOUTS

    def raise_failures(self) -> None:
        """Called by every forward outside a capture: what `_read_parked` collected is raised once."""
        if self.exact_failed:
            bits, self.exact_failed = self.exact_failed, 0
            raise_sort_failure(bits)

    # ---- the check -------------------------------------------------------------------------------------------------------
    def check(self) -> bool:
        """Reads every word (synchronises).  True if a capacity-mode forward dropped instances: the hints of the offending
        shapes are doubled.  Raises if a sort timed out anywhere.  Eager and exact words are forgotten, captured ones stay."""
        hit, sort_fail, self.exact_failed = False, self.exact_failed, 0
        exact = self.exact_other + ([self.exact_pending] if self.exact_pending is not None else [])
        self.exact_pending, self.exact_other = None, []
        todo = self.pending + self.captured_words() + [(e[0], e[1]) for e in exact]
        self.pending = []
        _drain([w for _, w in todo])
        for key, word in todo:
            v = int(word.item())
            if v & STATUS_CAPACITY_OVERFLOW:
                hit = True
                self.remember_hint(key, max(2 * self.hints.get(key, 1), 1024))
            sort_fail |= v & _TIMEOUTS
        if sort_fail:
            raise_sort_failure(sort_fail)
        return hit

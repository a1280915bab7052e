"""Keyframe selection and window management of the tracker, decided on the device.

Mirror of ``get_median_depth`` (/root/reference/utils/slam_utils.py:149-157), of the keyframe test in ``Tracker.run``
(/root/reference/utils/slam_tracker.py:412-452), ``should_add_as_keyframe`` (:195-221) and ``add_to_window`` (:223-284).  The
reference gathers the three quantities it decides from -- the median depth of the tracked render, the overlap of the current
frame's ``n_touched > 0`` set with every window keyframe's, the pairwise camera distances of the window -- with boolean
indexing, ``torch.median``, ``count_nonzero`` and ``.item()`` in Python loops: about ``2 K + 4`` host synchronisations per
tracked frame.  Here they are three stream-ordered calls (``mgs_masked_median``, ``mgs_covisibility``,
``mgs_keyframe_decide``; csrc/kfwindow.hip) and ONE 32-byte read-back.  The visibility sets stay in the packed words
``mgs_window_stats`` writes (``WindowMapper.packed_visibility``).

The fork hard-codes ``check_viewpoints_overlap = False`` and ``kf_interval = 1`` (slam_tracker.py:71-72: every frame is a
keyframe, ``add_to_window`` and the median still run per frame) and never sets ``is_window_full`` (:314-316 are commented
out); upstream MonoGS runs with the overlap check on and latches ``is_window_full`` once the window has filled.  Both are
supported, the defaults follow the fork.  The reference cannot be imported here (its tracker pulls in the viewer), so this
file is checked against a plain PyTorch restatement (tests/keyframe_mirror.py): parity unpinned.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import _lib
from . import window as W
from ._launch import _device_guard, _stream

MAX_KEYFRAMES = 32


class Decision(NamedTuple):
    create_kf: bool
    removed_ids: List[int]          # keyframe ids that left the window (cut-off eviction first, then the size eviction)
    iou: float
    distance: float
    median_depth: float


class DecisionRecord(NamedTuple):
    """The eight words of ``mgs_keyframe_decide``; the removed slots are positions in ``[cur] + window`` (-1: none)."""
    create_kf: bool
    removed_by_cutoff: int
    removed_by_size: int
    iou: float = float("nan")
    distance: float = float("nan")
    median_depth: float = float("nan")


def _require_device(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: no CPU path (the keyframe kernels are HIP only)")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _median_launch(values: torch.Tensor, mask: Optional[torch.Tensor], lo: float, scratch: torch.Tensor,
                   out_median: torch.Tensor, out_count: torch.Tensor):
    lib = _lib.load()
    n = values.numel()
    if mask is not None and mask.numel() != n:
        raise ValueError("median_depth: depth and mask must have the same number of elements")
    with _device_guard(values.device):
        _lib.check(lib.mgs_masked_median(values.data_ptr(), None if mask is None else mask.data_ptr(), n, float(lo),
                                         scratch.data_ptr(), out_median.data_ptr(), out_count.data_ptr(), _stream()),
                   "mgs_masked_median")


def median_scratch(n: int, device) -> torch.Tensor:
    return torch.empty(_lib.load().mgs_median_scratch_bytes(int(n)), dtype=torch.uint8, device=device)


def masked_median(values: torch.Tensor, mask: Optional[torch.Tensor] = None, lo: float = 0.0,
                  scratch: Optional[torch.Tensor] = None):
    """(median, count) as 0-d device tensors (float32, int32): the lower median of the elements with ``values > lo`` and
    ``mask != 0``; NaN and 0 when nothing counts.  No host synchronisation."""
    _require_device(values, "masked_median")
    v = _f32c(values).reshape(-1)
    m = None if mask is None else _f32c(mask).reshape(-1)
    if scratch is None:
        scratch = median_scratch(v.numel(), v.device)
    med = torch.empty((), dtype=torch.float32, device=v.device)
    cnt = torch.empty((), dtype=torch.int32, device=v.device)
    _median_launch(v, m, lo, scratch, med, cnt)
    return med, cnt


def median_depth(depth: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``get_median_depth(depth, mask)``: the median of ``depth[(depth > 0) & mask]`` as a 0-d device tensor, without a host
    synchronisation.  An empty selection gives NaN (the reference's ``torch.median`` raises there)."""
    return masked_median(depth, mask, 0.0)[0]


def pack_visibility(mask: torch.Tensor) -> torch.Tensor:
    """bool[P] (or an integer ``n_touched``: packed as ``> 0``) -> int64[ceil(P/64)], the layout of ``mgs_window_stats``'
    ``visibility_bits``."""
    b = mask if mask.dtype == torch.bool else mask > 0
    by = W.pack_bits(b.reshape(-1))
    pad = (-by.numel()) % 8
    if pad:
        by = torch.nn.functional.pad(by, (0, pad))
    return by.contiguous().view(torch.int64)


def unpack_visibility(words: torch.Tensor, P: int) -> torch.Tensor:
    """int64 words -> bool[P]; a row shorter than ``ceil(P/64)`` words is zero-extended."""
    need = (P + 63) // 64
    if words.numel() < need:
        words = torch.cat([words, torch.zeros(need - words.numel(), dtype=words.dtype, device=words.device)])
    return W.unpack_bits(words.contiguous().view(torch.uint8), P)


class KeyframeWindow:
    """The tracker's window state: ``cur_kf_list`` (most recent first), a packed visibility row per keyframe id,
    ``is_window_full`` and the thresholds.  ``kf_cutoff`` defaults to 0.4 as ``add_to_window`` does for a config without the
    key.  ``latch_window_full``: upstream's ``is_window_full = len(cur_kf_list) == window_size`` after every keyframe (the
    fork leaves the flag False for the whole run)."""

    def __init__(self, window_size: int, check_viewpoints_overlap: bool = False, kf_interval: int = 1,
                 kf_translation: float = 0.08, kf_min_translation: float = 0.05, kf_overlap: float = 0.9,
                 kf_cutoff: float = 0.4, n_dont_touch: int = 2, latch_window_full: bool = False):
        if not 1 <= int(window_size) <= MAX_KEYFRAMES:
            raise ValueError(f"window_size must lie in 1..{MAX_KEYFRAMES}")
        if int(n_dont_touch) < 1:
            raise ValueError("n_dont_touch must be at least 1")
        self.window_size = int(window_size)
        self.check_viewpoints_overlap = bool(check_viewpoints_overlap)
        self.kf_interval = int(kf_interval)
        self.kf_translation, self.kf_min_translation = float(kf_translation), float(kf_min_translation)
        self.kf_overlap, self.kf_cutoff = float(kf_overlap), float(kf_cutoff)
        self.n_dont_touch = int(n_dont_touch)
        self.latch_window_full = bool(latch_window_full)
        self.is_window_full = False
        self.cur_kf_list: List[int] = []
        self.viewpoints: Dict[int, object] = {}
        self.visibility: Dict[int, torch.Tensor] = {}       # kf id -> int64 words
        self.last_record: Optional[DecisionRecord] = None
        self.last_counts: Optional[torch.Tensor] = None     # int32[K][4] of the last launch (device)
        self._scratch = None

    # ---- state ---------------------------------------------------------------------------------------------------
    def params(self, frame_idx: int) -> _lib.MgsKeyframeParams:
        K = len(self.cur_kf_list)
        return _lib.MgsKeyframeParams(
            K=K, window_size=self.window_size, window_full=int(self.is_window_full),
            check_overlap=int(self.check_viewpoints_overlap), kf_interval=self.kf_interval,
            frames_since_last_kf=int(frame_idx) - int(self.cur_kf_list[0]) if K else 0,
            kf_translation=self.kf_translation, kf_min_translation=self.kf_min_translation, kf_overlap=self.kf_overlap,
            kf_cutoff=self.kf_cutoff, n_dont_touch=self.n_dont_touch)

    def set_visibility(self, kf_id: int, words_or_bool: torch.Tensor):
        """What the mapper produced for a keyframe: packed words (``WindowMapper.packed_visibility``; copied) or bool[P]."""
        t = words_or_bool
        if t.dtype == torch.bool:
            self.visibility[int(kf_id)] = pack_visibility(t)
        elif t.dtype == torch.int64 and t.dim() == 1:
            self.visibility[int(kf_id)] = t.detach().clone()
        else:
            raise ValueError("set_visibility: int64 packed words [ceil(P/64)] or bool[P]")

    def prune(self, keep_mask: torch.Tensor):
        """Map surgery dropped the Gaussians where ``keep_mask`` is False: every row loses the same bits
        (monogs_amd/mapping.py, ``_prune_covisibility``)."""
        P = int(keep_mask.numel())
        for k, words in list(self.visibility.items()):
            self.visibility[k] = pack_visibility(unpack_visibility(words, P)[keep_mask])

    def apply_decision(self, frame_idx: int, record: DecisionRecord, viewpoint=None,
                       row: Optional[torch.Tensor] = None) -> List[int]:
        """``add_to_window`` on the list: insert at the front, then remove both evicted ids.  Returns them."""
        self.last_record = record
        if not record.create_kf:
            return []
        new_list = [int(frame_idx)] + self.cur_kf_list
        removed = []
        for pos in (int(record.removed_by_cutoff), int(record.removed_by_size)):
            if pos < 0:
                continue
            if pos < self.n_dont_touch or pos >= len(new_list):
                raise ValueError(f"decision removes protected or missing slot {pos} of {len(new_list)}")
            if new_list[pos] not in removed:
                removed.append(new_list[pos])
        self.cur_kf_list = [k for k in new_list if k not in removed]
        self.viewpoints[int(frame_idx)] = viewpoint
        if row is not None:
            self.visibility[int(frame_idx)] = row
        for k in removed:
            self.viewpoints.pop(k, None)
            self.visibility.pop(k, None)
        if self.latch_window_full and not self.is_window_full:
            self.is_window_full = len(self.cur_kf_list) == self.window_size
        return removed

    def bootstrap(self, frame_idx: int, viewpoint=None, visibility: Optional[torch.Tensor] = None):
        """The first keyframe (``Tracker.initialize``): it enters an empty window unconditionally."""
        self.cur_kf_list = [int(frame_idx)]
        self.viewpoints = {int(frame_idx): viewpoint}
        self.visibility = {}
        if visibility is not None:
            self.set_visibility(frame_idx, visibility)

    # ---- the device path -------------------------------------------------------------------------------------------
    def launch(self, frame_idx: int, viewpoint, depth: torch.Tensor, opacity: Optional[torch.Tensor],
               n_touched: torch.Tensor):
        """The three calls, no read-back: returns (out int32[8], packed row of the current frame int64[words]), both on the
        device.  The window must hold at least one keyframe."""
        lib = _lib.load()
        K = len(self.cur_kf_list)
        if not 1 <= K <= MAX_KEYFRAMES:
            raise ValueError("observe needs 1..32 keyframes in the window (bootstrap the first one)")
        _require_device(depth, "KeyframeWindow.observe")
        dev = depth.device
        d = _f32c(depth).reshape(-1)
        m = None if opacity is None else _f32c(opacity).reshape(-1)
        nt = n_touched.detach()
        if nt.dtype != torch.int32 or not nt.is_contiguous():
            nt = nt.to(torch.int32).contiguous()
        P = int(nt.numel())
        words = (P + 63) // 64
        need = lib.mgs_median_scratch_bytes(d.numel())
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        median = torch.empty(1, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        counts = torch.empty(K, 4, dtype=torch.int32, device=dev)
        row = torch.empty(words, dtype=torch.int64, device=dev)
        out = torch.empty(8, dtype=torch.int32, device=dev)
        rows = [self.visibility.get(k) for k in self.cur_kf_list]
        kf_bits = (C.c_void_p * K)(*[None if r is None or r.numel() == 0 else r.data_ptr() for r in rows])
        kf_words = (C.c_uint64 * K)(*[0 if r is None else int(r.numel()) for r in rows])
        vps = [viewpoint] + [self.viewpoints[k] for k in self.cur_kf_list]
        keep = [(_f32c(v.R), _f32c(v.T)) for v in vps]
        poses = (C.c_void_p * (2 * (K + 1)))(*[t.data_ptr() for rt in keep for t in rt])
        prm = self.params(frame_idx)
        _median_launch(d, m, 0.0, self._scratch, median, count)
        with _device_guard(dev):
            s = _stream()
            _lib.check(lib.mgs_covisibility(P, nt.data_ptr(), None, K, kf_bits, kf_words, row.data_ptr(), counts.data_ptr(), s),
                       "mgs_covisibility")
            _lib.check(lib.mgs_keyframe_decide(C.byref(prm), counts.data_ptr(), median.data_ptr(), poses, out.data_ptr(), s),
                       "mgs_keyframe_decide")
        self.last_counts = counts
        return out, row

    @staticmethod
    def decode(out_words: Sequence[int]) -> DecisionRecord:
        w = [int(x) for x in out_words]
        f = lambda x: struct.unpack("<f", struct.pack("<i", x))[0]  # noqa: E731
        return DecisionRecord(bool(w[0]), w[1], w[2], f(w[3]), f(w[4]), f(w[5]))

    @torch.no_grad()
    def observe(self, frame_idx: int, viewpoint, render_pkg) -> Decision:
        """One tracked frame: three launches, one read-back; the window is updated exactly as ``add_to_window`` does when
        the frame becomes a keyframe.  ``render_pkg``: the tracked render's ``depth``, ``opacity``, ``n_touched``."""
        out, row = self.launch(frame_idx, viewpoint, render_pkg["depth"], render_pkg.get("opacity"), render_pkg["n_touched"])
        rec = self.decode(out.tolist())                         # the one host synchronisation
        removed = self.apply_decision(frame_idx, rec, viewpoint, row)
        return Decision(rec.create_kf, removed, rec.iou, rec.distance, rec.median_depth)

"""What every torch-side caller of the library needs around a native call: the raw handle of the current stream, a cheap device
guard, and the float32 / pointer helpers.  Nothing here knows about rasterisation."""
from typing import Optional

import torch


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor (got device {t.device}); "
                           "the rasteriser has no CPU path")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


class _device_guard:
    """``with _device_guard(dev)`` for the common case.  The stock context manager spends ~45 us per use in this
    torch build (``_get_device_index`` consults the environment on entry and exit); five uses per render + loss +
    backward were ~0.2 ms of host time per iteration (tools/host_overhead.py).  Here nothing happens unless ``dev``
    is not the current device."""
    __slots__ = ("idx", "prev")

    def __init__(self, dev):
        idx = getattr(dev, "index", dev)
        self.idx = torch._C._cuda_getDevice() if idx is None else int(idx)

    def __enter__(self):
        self.prev = torch._C._cuda_getDevice()
        if self.prev != self.idx:
            torch._C._cuda_setDevice(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev != self.idx:
            torch._C._cuda_setDevice(self.prev)
        return False


def _stream():
    """Raw handle of the caller's current stream.  torch.cuda.current_stream() costs ~40 us per call in this torch
    build (environment lookups inside _get_device_index) -- four calls per render + backward; the C-level accessor
    is ~100x cheaper (tools/host_overhead.py)."""
    if _raw_stream is not None:
        return _raw_stream(torch._C._cuda_getDevice())
    return torch.cuda.current_stream().cuda_stream

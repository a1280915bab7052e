"""ctypes binding of libmonogs_raster.so, derived from include/monogs_raster.h.

The header is the one statement of the C ABI: `_header.py` reads it on import, and the prototypes (`SIGNATURES`), the struct
classes (`MgsCamera`, `MgsTiming`, ...), the constants (`H.MGS_*`) and `ABI_VERSION` here are what it declares.  Nothing is
restated by hand: adding an entry point means declaring it in the header.  There is no fallback: if the library is missing,
stale or fails to load, importing the product path raises.  The library is built in-tree (monogs_amd/lib/) by
``__graft_entry__.build()`` or ``make -C monogs_amd/csrc``.
"""
import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGS_LIB_PATH") or os.path.join(_HERE, "lib", "libmonogs_raster.so")   # (override: kernel experiments)

_abi = _header.read()
H = _abi.constants                          # every #define MGS_* and the MGS_PLAN_* enumerators, by their C names
SIGNATURES = _abi.functions                 # symbol -> (restype, argtypes)
globals().update(_abi.structs)              # MgsCamera, MgsTiming, MgsKeyframeParams, ...: one class per typedef struct
MgsTiming.as_dict = lambda self: {n: float(getattr(self, n)) for n, _ in self._fields_}  # noqa: F821
ABI_VERSION = H.MGS_ABI_VERSION
FLAG_EXCLUSIVE_DEVICE, FLAG_INTRINSICS_GRAD = H.MGS_FLAG_EXCLUSIVE_DEVICE, H.MGS_FLAG_INTRINSICS_GRAD   # bits of mgs_camera.flags

c_float_p = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())

_lib = None


class MonoGSNativeError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises if the HIP library is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MonoGSNativeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C monogs_amd/csrc`.  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    if lib.mgs_abi_version() != ABI_VERSION:
        raise MonoGSNativeError(f"ABI mismatch: library {lib.mgs_abi_version()} vs {_header.HEADER_PATH} {ABI_VERSION}; rebuild")
    # measurement knobs for A/B runs of whole programs (tools/, bench.py): MGS_DEBUG_OPTIONS="name=value,name=value"
    # -> mgs_debug_set_option at load time (read here, once; nothing on the launch path consults the environment)
    for kv in filter(None, os.environ.get("MGS_DEBUG_OPTIONS", "").split(",")):
        k, _, v = kv.partition("=")
        if lib.mgs_debug_set_option(k.strip().encode(), int(v)) != 0:
            raise MonoGSNativeError(f"MGS_DEBUG_OPTIONS: {lib.mgs_last_error().decode()}")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().mgs_last_error().decode("utf-8", "replace")
        # argument errors mirror the upstream extension's Python exceptions
        raise Exception(msg) if rc == 1 else MonoGSNativeError(f"{what}: {msg}")

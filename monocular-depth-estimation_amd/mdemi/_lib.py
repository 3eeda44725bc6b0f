"""ctypes binding of libmdemi.so, derived from the C ABI headers (include/mdemi.h and
include/mdemi_ext.h): ``_cabi.parse`` reads their constants, structs and prototypes, so a
change to a header is a change to the binding and nothing here has to be kept in step.

The library is built in-tree (``csrc/Makefile`` -> ``mdemi/libmdemi.so``) and
loaded *after* torch so that it binds the HIP runtime torch already mapped
(one runtime per process).  There is no fallback: if the library is missing
every op raises, which is what the GPU tests and ``smoke()`` rely on.

Error behaviour mirrors the reference: failures of the device library surface
as ``RuntimeError`` (as ``utils/dist_utils.py:29,37,57`` does for invalid
collectives); shape/config errors raised in Python stay ``ValueError``.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must be imported before the HIP library is mapped)

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDEMI_LIB") or os.path.join(_HERE, "libmdemi.so")  # override: A/B benchmarking
HEADER_PATH = os.path.abspath(os.path.join(_HERE, "..", "..", "include", "mdemi.h"))
HEADER_PATHS = [HEADER_PATH, os.path.abspath(os.path.join(_HERE, "..", "..", "include", "mdemi_ext.h"))]


class MdemiLibraryError(RuntimeError):
    pass


def _read_headers():
    texts = []
    for path in HEADER_PATHS:
        if not os.path.exists(path):
            raise MdemiLibraryError(f"C ABI header not found at {path}")
        with open(path) as f:
            texts.append(f.read())
    return _cabi.parse("".join(texts))


# ---- the ABI, read from the headers once at import: nothing below restates them ----
_ABI = _read_headers()
_SIGS = _ABI.prototypes  # name -> (restype, argtypes)

# constants under their header names minus the MDEMI_ prefix: ACT_GELU, L_CONV, EW_ACT_BWD, EINVAL, ...
_CONSTANTS = {name[len("MDEMI_"):]: value for name, value in _ABI.constants.items()}
assert not set(_CONSTANTS) & set(globals()), set(_CONSTANTS) & set(globals())
globals().update(_CONSTANTS)
ACT_GRAD_OF = {_CONSTANTS[a]: _CONSTANTS[a + "_GRAD"] for a in ("ACT_GELU", "ACT_RELU", "ACT_SILU")}

ConvGeom = _ABI.structs["mdemi_conv_geom"]
GemmDesc = _ABI.structs["mdemi_gemm_desc"]
WinAttnDesc = _ABI.structs["mdemi_winattn_desc"]
TensorRef = _ABI.structs["mdemi_tensor_ref"]
AdamWGroup = _ABI.structs["mdemi_adamw_group"]
StepRecord = _ABI.structs["mdemi_step_record"]
TelemetryState = _ABI.structs["mdemi_telemetry_state"]
GuardState = _ABI.structs["mdemi_guard_state"]
EmaState = _ABI.structs["mdemi_ema_state"]
AugSample = _ABI.structs["mdemi_aug_sample"]
BoundaryThresholds = _ABI.structs["mdemi_boundary_thresholds"]

_lib = None
_lock = threading.Lock()


def load():
    """Map libmdemi.so and declare every entry point. Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise MdemiLibraryError(
                f"libmdemi.so not found at {LIB_PATH}; build it with "
                "`make -C monocular-depth-estimation_amd/csrc` (or __graft_entry__.build())")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name, None)
            if fn is None:
                if os.environ.get("MDEMI_LIB"):  # an A/B build of an older ABI
                    continue
                raise MdemiLibraryError(f"{LIB_PATH} does not export {name}")
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def exported_symbols():
    return list(_SIGS.keys())


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mdemi_last_error().decode(errors="replace")
        raise RuntimeError(f"mdemi {what} failed (rc={rc}): {msg}")


def call(name: str, *args):
    rc = getattr(load(), name)(*args)
    check(rc, name)


def ptr(t) -> int | None:
    if t is None:
        return None
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- per-device scratch (the library never allocates) ----
_ws: dict = {}
# Once a hipGraph has been captured, a workspace buffer superseded by a larger one
# (a later eager call at a bigger shape) must never return to the allocator: the
# graph keeps the raw addresses it was recorded with.  Before any capture, a
# superseded buffer is freed only after the device has drained: workspaces are
# also used on side streams (GraphedPredictor's warm-up stream), and the caching
# allocator would otherwise hand the block to a new allocation on its origin
# stream while another stream's kernels still use it.  Growth happens in
# warm-up only, so the synchronisation is rare.
_ws_retired: list = []
_graph_captured = False


def note_graph_capture() -> None:
    """Called when a workspace is handed out during a capture (and by Trainer)."""
    global _graph_captured
    _graph_captured = True


def workspace(nbytes: int, device=None, slot: int = 0) -> torch.Tensor:
    """Return a cached uint8 device buffer of at least nbytes (stream-ordered reuse)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device.index if device.index is not None else torch.cuda.current_device(), slot)
    buf = _ws.get(key)
    nbytes = max(int(nbytes), 256)
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing:
        note_graph_capture()
    if buf is None or buf.numel() < nbytes:
        if capturing:
            raise RuntimeError(f"mdemi: workspace slot {slot} must grow to {nbytes} bytes during hipGraph capture; "
                               "run the captured step eagerly first (warm-up) so every workspace is sized")
        if buf is not None:
            if _graph_captured:
                _ws_retired.append(buf)
            else:
                torch.cuda.synchronize(device)
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf

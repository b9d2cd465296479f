"""ctypes binding of libw2e.so (include/*.h; the prototypes, structs and constants are read from the headers by _abi.py).  This is the ONLY door to compute for the hot path:
if the library is missing or a tensor is not on an MI355X the ops raise -- there is no CPU or
eager-PyTorch fallback (the CPU restatement lives in oracle/ and is test-only)."""
import ctypes
import os

import torch

from . import _abi, build as _build

_PROTOS, STRUCTS, CONSTS = _abi.PROTOS, _abi.STRUCTS, _abi.CONSTS  # all of include/*.h: {entry point: (restype, [argtypes])}, ...
DemodLayer = STRUCTS["w2e_demod_layer"]

_lib = None


def header_version():
    """W2E_VERSION as include/w2e.h states it: the one place the ABI version is written down (the loader, the driver's
    build hook and the tests all compare the built library against THIS, so none of them can go stale on its own)."""
    return CONSTS["W2E_VERSION"]


def lib_path():
    return _build.LIB_PATH


def load():
    """Load libw2e.so (built in-tree by where2edit_amd.build).  Raises if it does not exist."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: run `python -m where2edit_amd.build` (hipcc, gfx950). "
                               "where2edit_amd has no fallback path without its HIP library.")
        lib = ctypes.CDLL(path)  # torch is already imported: libamdhip64.so.7 resolves to the runtime torch uses
        for name, (res, args) in _PROTOS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.w2e_version() != header_version():
            raise RuntimeError(f"libw2e.so is ABI {lib.w2e_version()}, include/w2e.h says {header_version()}: rebuild with `python -m where2edit_amd.build --force`")
        _lib = lib
    return _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


_cur_dev = torch.cuda.current_device  # (lazy CUDA init happens long before the first kernel call)


def stream_ptr():
    """The current HIP stream of the current device as a void*.  (torch.cuda.current_stream() builds a Python Stream
    object per call, ~10 us -- 2 ms of host time per mapper step; the raw accessor is ~0.3 us.)"""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(_cur_dev()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a contiguous fp32 CUDA(HIP) tensor, or NULL for None.  The tensor must live on the CURRENT
    device: the kernels are launched on the current device's stream, and a pointer of another GPU there is a memory
    fault, not a Python error (wrap multi-device use in `with torch.cuda.device(t.device):`)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("where2edit_amd ops run on the GPU only (got a CPU tensor); the CPU restatement "
                           "is oracle/, for tests")
    if t.device.index != _cur_dev():
        raise RuntimeError(f"where2edit_amd: tensor on cuda:{t.device.index} but the current device is cuda:{_cur_dev()} "
                           "(kernels launch on the current device's stream): call torch.cuda.set_device(...) or use "
                           "`with torch.cuda.device(t.device):`")
    if t.dtype != torch.float32:
        raise RuntimeError(f"where2edit_amd kernels are fp32 (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError("internal: non-contiguous tensor passed to a kernel")
    # an empty tensor has no storage: hand the ABI a non-NULL dummy address (it is never dereferenced -- every entry
    # point returns before launching when a dimension is 0) so that "NULL" keeps meaning "argument absent"
    return ctypes.c_void_p(t.data_ptr() if t.numel() else 16)


def call(name, *args):
    """Invoke an entry point; a non-zero status becomes RuntimeError(w2e_last_error())."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.w2e_last_error().decode()}")


def set_option(name, value):
    """w2e_set_option: process-wide library options ("conv_precision", "deterministic", "tune_cfg", ...; include/w2e.h)."""
    lib = load()
    v = None if value is None else str(value).encode()
    if lib.w2e_set_option(name.encode(), v) != 0:
        raise RuntimeError(lib.w2e_last_error().decode())


def get_option(name):
    lib = load()
    out = ctypes.c_int(0)
    if lib.w2e_get_option(name.encode(), ctypes.byref(out)) != 0:
        raise RuntimeError(lib.w2e_last_error().decode())
    return out.value

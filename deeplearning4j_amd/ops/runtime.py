"""Loader of ``libdl4j_amd_runtime.so`` — host (CPU) C++ runtime pieces (csrc/runtime/*.cpp):
threshold/bitmap codec for CPU tensors, tree/t-SNE helpers, data-loader helpers.

The ctypes signature of every ``rt_*`` function comes from the generated C ABI header ``csrc/include/dl4j_amd.h``
(ops/abi.py), bound once when the library is loaded. To add one: write the ``RT_API`` function, run
``python tools/gen_abi_header.py``, call it."""
import ctypes
import os
import threading

from . import abi
from .build import RUNTIME_LIB

_rt = None
_load_lock = threading.Lock()


def load():
    """Load (building on first use if needed) the host runtime library; None if no C++ toolchain."""
    global _rt
    if _rt is not None:
        return _rt
    with _load_lock:
        if _rt is None:
            if not os.path.exists(RUNTIME_LIB):
                try:
                    from .build import build_runtime
                    build_runtime(verbose=False)
                except Exception:
                    return None
            _rt = abi.bind(ctypes.CDLL(RUNTIME_LIB), "rt_")
    return _rt


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())

"""ctypes signatures of both native libraries, derived from the generated C ABI header ``csrc/include/dl4j_amd.h``.

``bind(lib, prefix)`` runs once per library at load (ops/native.py ``dl4j_``, ops/runtime.py ``rt_``); no wrapper
types a signature by hand. Every pointer is a ``c_void_p`` parameter, which takes ``byref(...)``, ctypes arrays and
pointers, bytes, ints and None alike.
"""
import ctypes
import functools
import itertools
import os
import re

from .build import CSRC

HEADER = os.path.join(CSRC, "include", "dl4j_amd.h")
_PROTO = re.compile(r"^(\w[\w\s\*]*?)\b((?:dl4j|rt)_\w+)\((.*)\);$", re.M)
_SCALAR = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double,
}
_TYPE_WORDS = {w for t in _SCALAR for w in t.split()}
_HANDLES = ("hipStream_t", "dl4j_comm_t")


def _ctype(decl, name):
    """ctypes type of one C parameter / return declaration (``const float* x``, ``long long``, ``hipStream_t s``)."""
    t = " ".join(decl.replace("*", " * ").split())
    if re.fullmatch(r"const char \*( \w+)?", t):
        return ctypes.c_char_p
    words = [w for w in t.split() if w != "const"]
    if "*" in words or words[0] in _HANDLES:
        return ctypes.c_void_p
    k = sum(1 for _ in itertools.takewhile(_TYPE_WORDS.__contains__, words))
    if len(words) - k <= 1 and " ".join(words[:k]) in _SCALAR:      # at most a parameter name after the type
        return _SCALAR[" ".join(words[:k])]
    raise TypeError(f"{name}: no ctypes mapping for C type {decl.strip()!r}")


def parse(text):
    """``{name: (argtypes, restype)}`` of the one-per-line prototypes in ``text``."""
    sigs = {}
    for ret, name, params in _PROTO.findall(text):
        args = [] if params.strip() == "void" else [_ctype(p, name) for p in params.split(",")]
        sig = (args, None if ret.strip() == "void" else _ctype(ret, name))
        if sigs.setdefault(name, sig) != sig:
            raise TypeError(f"{name}: declared twice with different signatures")
    return sigs


@functools.lru_cache(maxsize=None)
def signatures():
    with open(HEADER) as fh:
        return parse(fh.read())


def bind(lib, prefix):
    """Set ``argtypes`` / ``restype`` of every header function whose name starts with ``prefix`` on ``lib``."""
    for name, (args, res) in signatures().items():
        if not name.startswith(prefix):
            continue
        try:
            f = getattr(lib, name)
        except AttributeError:
            raise RuntimeError(f"{lib._name} lacks {name}, which {HEADER} declares: the library is stale, "
                               "rebuild it (python -m deeplearning4j_amd.ops.build)") from None
        f.argtypes, f.restype = args, res
    return lib

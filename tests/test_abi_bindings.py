"""The Python bindings of both native libraries are derived from csrc/include/dl4j_amd.h (ops/abi.py): the parser covers
the whole header, maps every C type it meets, refuses what it does not know, and nothing else in the tree types a
signature by hand."""
import ctypes
import glob
import os
import re

import pytest

from deeplearning4j_amd.ops import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, U, LL, ULL, F, D = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_ulonglong,
                          ctypes.c_float, ctypes.c_double)
I64, U64 = ctypes.c_int64, ctypes.c_uint64

# hand-written from the C definitions; together they meet every C type the header uses
EXPECTED = {
    "dl4j_bn_tiles_workspace_floats": ([LL, I], LL),
    "rt_threshold_decode": ([P, P, F], None),                     # the void return
    "dl4j_lstm_step_guard": ([], P),
    "dl4j_attn_fwd_drop_dt": ([I, P, P, P, P, I, I, I, I, F, I, F, ULL, P, P], I),
    "dl4j_lstm_fwd_coop": ([P] * 14 + [I, I, I, U, I, P], I),
    "rt_cooc_new": ([ctypes.c_char_p, I64], P),
    "rt_w2v_sg_apply": ([P, P, P, I64, P, P, P, I, P, P, P, I, P, I64, I, I, U64, I64, I], D),
    "rt_ws_create": ([LL, LL, LL, D, I, I, I], LL),
    "dl4j_conv_wrw_det": ([P] * 5 + [I] * 16 + [P], I),
    "dl4j_comm_all_reduce": ([P, P, P, LL, I, I, P], I),          # dl4j_comm_t, hipStream_t
}


def _sources():
    out = []
    for pat in ("deeplearning4j_amd/**/*.py", "tools/*.py", "tests/*.py"):
        out += glob.glob(os.path.join(ROOT, pat), recursive=True)
    return sorted(set(out))


def _header_lines():
    with open(abi.HEADER) as fh:
        return [ln for ln in fh.read().splitlines() if re.match(r"^\w.*\b(dl4j|rt)_\w+\(.*\);$", ln)]


def test_parser_covers_every_prototype():
    lines = _header_lines()
    assert len(lines) > 200
    with open(abi.HEADER) as fh:
        assert len(abi._PROTO.findall(fh.read())) == len(lines)
    sigs = abi.signatures()
    names = [re.search(r"\b((?:dl4j|rt)_\w+)\(", ln).group(1) for ln in lines]
    assert set(names) == set(sigs)
    # a function declared twice (engine.hip / nd4j_ops.hip re-declare two) parses to the same signature each time
    for name in {n for n in names if names.count(n) > 1}:
        each = [abi.parse(ln)[name] for ln in lines if f" {name}(" in ln or f"*{name}(" in ln]
        assert len(each) > 1 and all(e == sigs[name] for e in each), name


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_expected_signatures(name):
    args, res = abi.signatures()[name]
    assert (args, res) == EXPECTED[name]
    if name == "dl4j_conv_wrw_det":
        assert len(args) == 22


def test_every_mapped_type_is_exercised():
    seen = {t for args, res in EXPECTED.values() for t in args + [res]}
    assert seen >= set(abi._SCALAR.values()) | {P, ctypes.c_char_p, None}


def test_conflicting_duplicate_raises():
    with pytest.raises(TypeError, match="dl4j_x"):
        abi.parse("int dl4j_x(int a);\nint dl4j_x(long long a);\n")


@pytest.mark.parametrize("proto", ["int dl4j_x(size_t n);", "short dl4j_x(int n);", "int rt_x(struct foo f);",
                                   "int dl4j_x(unsigned char c);"])
def test_unknown_type_raises(proto):
    with pytest.raises(TypeError, match="no ctypes mapping"):
        abi.parse(proto + "\n")


def test_every_symbol_used_is_in_the_header():
    """A typo or an unexported function would otherwise get ctypes' default ``int f(...)``. The dotted module path of
    a ``from ... import`` line is not an attribute access and is left out."""
    sigs = abi.signatures()
    missing = []
    for path in _sources():
        with open(path) as fh:
            text = re.sub(r"^\s*from\s+[\w.]+\s+import\b", "", fh.read(), flags=re.M)
            for name in re.findall(r"\.(dl4j_\w+|rt_\w+)\b", text):
                if name not in sigs:
                    missing.append((os.path.relpath(path, ROOT), name))
    assert not missing, missing


def test_no_hand_written_signatures_left():
    bad = []
    this = os.path.abspath(__file__)
    pat = re.compile(r"register_sig\(|RT\.register\(|\.(dl4j|rt)_\w+\.(argtypes|restype)\s*=")
    for path in _sources():
        if os.path.abspath(path) == this:
            continue
        with open(path) as fh:
            for i, ln in enumerate(fh, 1):
                if pat.search(ln):
                    bad.append(f"{os.path.relpath(path, ROOT)}:{i}: {ln.strip()}")
    assert not bad, bad


def test_runtime_library_bound_from_header():
    from deeplearning4j_amd.ops import runtime
    lib = runtime.load()
    assert lib is not None
    names = [n for n in abi.signatures() if n.startswith("rt_")]
    assert len(names) > 30
    for name in names:
        args, res = abi.signatures()[name]
        f = getattr(lib, name)
        assert list(f.argtypes) == args and f.restype is res, name


def test_stale_library_is_an_error():
    class Stale:
        _name = "libstale.so"

    with pytest.raises(RuntimeError, match=r"libstale\.so lacks rt_\w+.*rebuild"):
        abi.bind(Stale(), "rt_")

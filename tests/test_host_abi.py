"""The C ABI seam without a GPU: every row of streammos_amd._lib.SIGNATURES against the declaration in include/smos.h --
argument count, every parameter's type, the return type -- the version number, and the two chunk formulas ops.py restates.

The table is written by hand because it carries what the header cannot: which pointers are host arrays (typed ctypes
pointers) and which are device addresses (c_void_p).  What the header can say, this file holds the table to."""
import ctypes
import re

import pytest

from streammos_amd import _lib, ops
from tests import util

SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double, "smos_stream_t": ctypes.c_void_p}
ELEMENTS = {"float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
            "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


def allowed(kind):
    """The ctypes types that may bind a parameter the header declares as `kind`; a KeyError for a kind without a rule."""
    base, stars = kind.rstrip("*"), kind.count("*")
    if stars == 0:
        return (SCALARS[base],)
    typed = () if base == "void" else (ELEMENTS[base],)
    if stars == 1:                                      # T*: a device address, or a host array of exactly T
        return (ctypes.c_void_p,) + tuple(ctypes.POINTER(t) for t in typed)
    if stars == 2:                                      # T* const*: a host array of device addresses or of host arrays of T
        return (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)) + tuple(ctypes.POINTER(ctypes.POINTER(t)) for t in typed)
    raise KeyError(kind)


def mismatches(signatures, int64_results, declared):
    """[(entry, parameter index or "count" / "return" / "name", what is wrong)] of a table against the header."""
    bad = []
    for name, argtypes in signatures.items():
        if name not in declared:
            bad.append((name, "name", "bound but not declared"))
            continue
        ret, params = declared[name]
        if len(argtypes) != len(params):
            bad.append((name, "count", "%d bound, %d declared" % (len(argtypes), len(params))))
            continue
        for i, (have, kind) in enumerate(zip(argtypes, params)):
            if have not in allowed(kind):
                bad.append((name, i, "%s bound as %s" % (kind, have.__name__)))
        if ret not in ("int", "int32_t", "int64_t"):
            bad.append((name, "return", "no rule for a %s result" % ret))
        elif (ret == "int64_t") != (name in int64_results):
            bad.append((name, "return", "%s result, %s INT64_RESULTS" % (ret, "in" if name in int64_results else "not in")))
    for name in int64_results:
        if name not in signatures:
            bad.append((name, "name", "in INT64_RESULTS but not bound"))
    return bad


DECLARED = util.header_declarations()


def test_the_header_uses_only_parameter_kinds_with_a_rule():
    kinds = {k for _, params in DECLARED.values() for k in params}
    assert kinds == {"double", "double*", "double**", "float", "float*", "float**", "int32_t", "int32_t*", "int64_t", "int64_t*",
                     "smos_stream_t", "uint16_t*", "uint32_t", "uint32_t*", "uint64_t", "uint64_t*", "uint8_t*", "uint8_t**",
                     "void*", "void**"}
    for kind in kinds:
        assert allowed(kind)
    for kind in ("char", "int16_t*", "float***", "size_t"):
        with pytest.raises(KeyError):
            allowed(kind)


def test_every_binding_has_the_declared_types():
    assert len(_lib.SIGNATURES) > 80
    assert set(DECLARED) == set(_lib.SIGNATURES) | {"smos_last_error"}
    assert DECLARED["smos_last_error"] == ("char*", [])
    assert mismatches(_lib.SIGNATURES, _lib.INT64_RESULTS, DECLARED) == []
    assert len(set(_lib.INT64_RESULTS)) == len(_lib.INT64_RESULTS) and "smos_abi_version" not in _lib.INT64_RESULTS


def _mutant(name, index, new):
    table = {k: list(v) for k, v in _lib.SIGNATURES.items()}
    assert table[name][index] is not new
    table[name][index] = new
    return table


@pytest.mark.parametrize("name,index,old,new", [
    ("smos_dbscan", 1, ctypes.c_int64, ctypes.c_int32),                                           # an i64 written as i32
    ("smos_conv_cl", 1, ctypes.c_int64, ctypes.c_int32),
    ("smos_dbscan", 3, ctypes.c_double, ctypes.c_float),                                          # a double as a float
    ("smos_seg_loss_fwd", 7, ctypes.c_float, ctypes.c_double),
    ("smos_vote_accumulate", 4, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)),  # a host array of the wrong element
    ("smos_voxel_maxpool_fwd", 1, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)),
    ("smos_box_vote_dev", 5, ctypes.POINTER(ctypes.POINTER(ctypes.c_double)), ctypes.POINTER(ctypes.POINTER(ctypes.c_float))),
    ("smos_conv_wino_cl", 16, ctypes.c_void_p, ctypes.c_int64),                                    # a stream as an integer
])
def test_a_wrong_parameter_type_is_named(name, index, old, new):
    assert _lib.SIGNATURES[name][index] is old
    assert [(n, i) for n, i, _ in mismatches(_mutant(name, index, new), _lib.INT64_RESULTS, DECLARED)] == [(name, index)]


def test_a_wrong_count_or_return_type_is_named():
    short = {k: list(v) for k, v in _lib.SIGNATURES.items()}
    short["smos_point_head"].pop()
    assert [(n, i) for n, i, _ in mismatches(short, _lib.INT64_RESULTS, DECLARED)] == [("smos_point_head", "count")]
    for gone in ("smos_seg_loss_work_bytes", "smos_conv_cl_sum_chunks"):              # a forgotten 64-bit result
        fewer = tuple(n for n in _lib.INT64_RESULTS if n != gone)
        assert [(n, i) for n, i, _ in mismatches(_lib.SIGNATURES, fewer, DECLARED)] == [(gone, "return")]
    more = _lib.INT64_RESULTS + ("smos_segsum_chunk",)                                # and an int result read as 64 bits
    assert [(n, i) for n, i, _ in mismatches(_lib.SIGNATURES, more, DECLARED)] == [("smos_segsum_chunk", "return")]


def test_the_version_is_written_in_two_places_that_agree():
    assert util.header_abi_version() == _lib.ABI_VERSION
    lib = ctypes.CDLL(_lib.LIB_PATH)          # loads without a GPU; no compute call is made
    lib.smos_abi_version.argtypes, lib.smos_abi_version.restype = [], ctypes.c_int
    assert lib.smos_abi_version() == _lib.ABI_VERSION


def test_the_chunk_formulas_of_ops_are_the_library_s():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    pairs = ((ops.conv_sum_chunks, lib.smos_conv_cl_sum_chunks), (ops.conv_wino_sum_chunks, lib.smos_conv_wino_sum_chunks))
    for _, fn in pairs:
        fn.argtypes, fn.restype = _lib.SIGNATURES[fn.__name__], ctypes.c_int64
    for h in range(1, 71):
        for w in (1, 31, 32, 33, 63, 64, 65, 200):
            for restated, fn in pairs:
                assert restated(h, w) == fn(h, w), (fn.__name__, h, w)


def test_every_entry_the_wrappers_name_is_bound():
    """ops.py and device_preprocess.py name their entries in strings (_lib.call / _lib.query): each is a row of the table, and
    no status is checked by hand."""
    import inspect

    from streammos_amd import device_preprocess
    for mod in (ops, device_preprocess):
        src = inspect.getsource(mod)
        assert "_lib.load(" not in src and src.count("_lib.check(") == (1 if mod is ops else 0)      # ops._conv_launch's fast path
        named = re.findall(r'_lib\.(?:call|query)\("(smos_[a-z0-9_]+)"', src)
        assert named and set(named) <= set(_lib.SIGNATURES), set(named) - set(_lib.SIGNATURES)

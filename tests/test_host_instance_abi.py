"""The C ABI of the device-resident instance vote (include/smos.h, libsmos_hip.so, streammos_amd._lib): declared, exported,
bound with the declared argument counts, and the workspace query -- host code only, no GPU."""
import ctypes

from streammos_amd import _lib
from tests import util

NEW = ("smos_instance_work_bytes", "smos_instance_cluster", "smos_box_vote_dev", "smos_instance_apply")


def test_header_declares_and_library_exports_the_entry_points():
    declared = util.header_declarations()
    lib = ctypes.CDLL(_lib.LIB_PATH)          # loads without a GPU; no compute call is made
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_bindings_have_the_declared_argument_counts():
    declared = util.header_declarations()
    for name in NEW:
        args = declared[name][1]
        assert len(_lib.SIGNATURES[name]) == len(args), (name, len(_lib.SIGNATURES[name]), len(args))
    # every other binding too: the header is the one place the argument lists are written down
    for name, argtypes in _lib.SIGNATURES.items():
        assert len(argtypes) == len(declared[name][1]), name


def test_work_bytes_is_positive_and_monotonic():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.smos_instance_work_bytes.argtypes = [ctypes.c_int64]
    lib.smos_instance_work_bytes.restype = ctypes.c_int64
    sizes = [lib.smos_instance_work_bytes(n) for n in (1, 256, 257, 120000)]
    assert sizes[0] > 0 and sizes == sorted(sizes), sizes
    assert all(s % 256 == 0 for s in sizes)
    for n in (0, -1, -(1 << 40)):
        assert lib.smos_instance_work_bytes(n) <= 0

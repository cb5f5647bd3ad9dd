"""The fixed-order backward sums (csrc/segsum.hip) without a GPU: the numpy restatement of tests/segsum_cases.py against the
float64 references' bounds, the C ABI of the five new symbols, the workspace queries, and how ops.is_deterministic()
is resolved."""
import ctypes
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import bilinear_bwd_cases as bcases
from tests import segsum_cases as cases
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smos_segsum_chunk", "smos_bilinear_gather_bwd_det_work_bytes", "smos_bilinear_gather_bwd_det",
       "smos_msda_bwd_det_work_bytes", "smos_msda_bwd_det")


def _host_lib():
    lib = ctypes.CDLL(_lib.LIB_PATH)                  # loads without a GPU; no compute call is made
    lib.smos_segsum_chunk.restype = ctypes.c_int32
    for name in ("smos_bilinear_gather_bwd_det_work_bytes", "smos_msda_bwd_det_work_bytes"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _lib.SIGNATURES[name], ctypes.c_int64
    return lib


CHUNK = int(_host_lib().smos_segsum_chunk())
CHUNKS = (CHUNK, cases.OTHER_L)


def test_chunk_is_a_small_positive_constant():
    assert 1 < CHUNK <= 4096 and CHUNK != cases.OTHER_L


@pytest.mark.parametrize("key", cases.bilinear_keys(CHUNKS), ids=cases.key_id)
def test_bilinear_restatement_is_inside_the_float64_bound(key):
    """(m + 8) * 2^-24 * A of tests/bilinear_bwd_cases.py, exactly 0 where m = 0, and the reference's count of terms."""
    case = cases.bilinear_case(key)
    for chunk in CHUNKS:
        got, m = cases.bilinear_restated(key, chunk)
        assert got.dtype == np.float32 and got.shape == case.S.shape and np.array_equal(m, case.m)
        ok, ratio = bcases.worst_ratio(got, case)
        print("segsum-host-ratio %-36s L=%-4d %.4f" % (cases.key_id(key), chunk, ratio))
        assert ok, "%s L=%d: worst error / bound = %g" % (key, chunk, ratio)
        assert not got[np.broadcast_to(case.m == 0, got.shape)].any()


def test_chunk_edge_cases_cross_the_chunk_and_the_two_lengths_differ():
    for n in cases.onecell_sizes(CHUNK):
        assert cases.onecell_case(n).m.max() == n
    big = ("onecell", 2 * cases.OTHER_L + 3)
    a, _ = cases.bilinear_restated(big, CHUNK)
    b, _ = cases.bilinear_restated(big, cases.OTHER_L)
    assert not np.array_equal(a, b)                    # the chunk length is part of the number's definition
    small = ("onecell", min(CHUNK, cases.OTHER_L) - 1)
    assert np.array_equal(cases.bilinear_restated(small, CHUNK)[0], cases.bilinear_restated(small, cases.OTHER_L)[0])


def test_chunked_sum_on_a_hand_made_list():
    """Five terms into row 1 with L = 2: ((t0 + t1) + (t2 + t3)) + t4, rows 0 and 2 empty, an absent pair ignored."""
    t = np.array([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 7.0], dtype=np.float32)
    keys = np.array([1, 1, 1, 1, 1, 3])
    got, m = cases.chunked_sum(keys, np.ones(6, dtype=np.float32), np.arange(6), t[:, None], 3, 2)
    f = np.float32
    want = f(f(f(t[0] + t[1]) + f(t[2] + t[3])) + t[4])
    assert got[1, 0] == want and want != f(f(f(f(t[0] + t[1]) + t[2]) + t[3]) + t[4])
    assert m.tolist() == [0, 5, 0] and got[0, 0] == 0 and got[2, 0] == 0


@pytest.mark.parametrize("name", list(util.MSDA_BWD_CASES))
def test_msda_restatement_is_inside_the_float64_bound(name):
    c = util.msda_bwd_case(name)
    b_value, _, _ = util.msda_backward_bounds(c, "float32")
    for chunk in CHUNKS:
        got, m = cases.msda_restated(name, chunk)
        ok, ratio = util.msda_worst_ratio(got, c.want_value, b_value)
        print("segsum-host-ratio %-36s L=%-4d %.4f" % (name, chunk, ratio))
        assert ok, "%s L=%d: worst error / bound = %g" % (name, chunk, ratio)
        assert not got[m == 0].any() and not c.want_value[m == 0].any()
    if name == "bwd_d33_second_sweep":                                     # 16 500 heads on 16 cells: thousands of terms per row
        assert cases.msda_restated(name, CHUNK)[1].max() > 2 * max(CHUNKS)


def test_header_library_and_signatures_agree():
    declared = util.header_declarations()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name]) == len(declared[name][1]), name
    # the deterministic entries take the atomic entries' arguments (msda: without dtype), then work, work_bytes, stream
    sig = _lib.SIGNATURES
    assert sig["smos_bilinear_gather_bwd_det"] == sig["smos_bilinear_gather_bwd"][:-1] + [_lib.vp, _lib.i64, _lib.vp]
    assert sig["smos_msda_bwd_det"] == sig["smos_msda_bwd"][:-2] + [_lib.vp, _lib.i64, _lib.vp]
    assert util.header_abi_version() == _lib.ABI_VERSION
    assert "smos_bilinear_gather_bwd_det" in open(os.path.join(ROOT, "include", "smos.h")).read().split("smos_debug_set_conv_grid_cap(int32_t")[0]


def test_work_bytes_queries():
    lib = _host_lib()
    bil, msda = lib.smos_bilinear_gather_bwd_det_work_bytes, lib.smos_msda_bwd_det_work_bytes
    sizes = [bil(2, 32, 16, 16, n) for n in (1, 7, 100, 1000, 130000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert bil(2, 32, 16, 16, 0) == 0 and bil(0, 32, 16, 16, 5) == 0 and bil(2, 0, 16, 16, 5) == 0
    assert bil(4, 32, 16, 16, 1 << 27) == -1                       # B * N = 2^29
    assert bil(2, 32, 1 << 15, 1 << 15, 5) == -1                   # B * H * W = 2^31
    assert bil(2, 32, 0, 16, 5) == -1
    sizes = [msda(2, 100, 3, 32, 2, lq, 4) for lq in (1, 7, 100, 10000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert msda(2, 100, 3, 32, 2, 0, 4) == 0 and msda(0, 100, 3, 32, 2, 7, 4) == 0
    assert msda(2, 100, 3, 32, 2, 1 << 28, 4) == -1 and msda(2, 1 << 30, 3, 32, 2, 7, 4) == -1
    assert msda(2, 100, 0, 32, 2, 7, 4) == -1


def test_is_deterministic_resolution_order(monkeypatch, request):
    """The explicit setting, then SMOS_DETERMINISTIC, then torch's flag; every call looks again."""
    request.addfinalizer(lambda prev=ops.set_deterministic(None): ops.set_deterministic(prev))
    monkeypatch.delenv("SMOS_DETERMINISTIC", raising=False)
    flag = {"v": False}
    monkeypatch.setattr(torch, "are_deterministic_algorithms_enabled", lambda: flag["v"])
    assert ops.is_deterministic() is False
    flag["v"] = True
    assert ops.is_deterministic() is True                           # torch's flag where nothing else speaks
    monkeypatch.setenv("SMOS_DETERMINISTIC", "0")
    assert ops.is_deterministic() is False                          # the environment goes before torch ...
    flag["v"] = False
    monkeypatch.setenv("SMOS_DETERMINISTIC", "1")
    assert ops.is_deterministic() is True
    assert ops.set_deterministic(False) is None
    assert ops.is_deterministic() is False                          # ... and the explicit setting before the environment
    monkeypatch.setenv("SMOS_DETERMINISTIC", "0")
    assert ops.set_deterministic(True) is False
    assert ops.is_deterministic() is True
    assert ops.set_deterministic(None) is True
    assert ops.is_deterministic() is False
    monkeypatch.delenv("SMOS_DETERMINISTIC")
    assert ops.is_deterministic() is False


def test_msda_bwd_refuses_float64_when_asked_explicitly():
    """Before any device check or call: CPU tensors are enough to see it."""
    c = util.msda_bwd_case("bwd_d1")
    t = lambda a: torch.tensor(np.asarray(a))
    args = (t(c.value), t(c.shapes), t(c.lsi), t(c.loc), t(c.attn), t(c.grad_out))
    assert args[0].dtype == torch.float64
    with pytest.raises(RuntimeError, match="float32 only"):
        ops.msda_bwd(*args, deterministic=True)
    with pytest.raises(RuntimeError, match="GPU memory"):           # an ambient setting leaves float64 to the atomic path's checks
        prev = ops.set_deterministic(True)
        try:
            ops.msda_bwd(*args)
        finally:
            ops.set_deterministic(prev)

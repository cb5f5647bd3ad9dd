"""The float64 reference of ops.point_mlp_train (tests/point_mlp_cases.py::restate) against torch.autograd through the
float64 modules on the CPU, the six value-only mutants of it against the GPU test's bar, and the host side of the new
entry points (switch, bindings, work-space query).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import point_mlp_cases as cases
from tests import util

NEW = ("smos_point_mlp_chunk", "smos_point_mlp_fold_floats", "smos_point_mlp_stat_doubles", "smos_point_mlp_work_bytes",
       "smos_point_mlp_fwd", "smos_point_mlp_bwd")

_cache = {}


def _reference(name, shape, mode):
    key = (name, shape, mode)
    if key not in _cache:
        c = cases.make_case(name, *shape)
        _cache[key] = (c, cases.restate(c, mode == "train"))
    return _cache[key]


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.CASES)
def test_restatement_equals_autograd_of_the_float64_modules(name, shape, mode):
    """1e-12 relative on y, the eight gradients and the six buffers.  One result cannot be held to it by any two float64
    evaluations: the BN1 running mean of `bigmean` in training.  It is W1 times the mean of xhat0, and xhat0 is (x - mean)
    times 1 / 0.01 on a channel near 1000, so a last-place difference in the two means (numpy's pairwise sum against
    torch's) is magnified by 1e5.  The float32 module path shows the same thing at 2.2e-3 (the exception named where the
    GPU bar is defined); the float64 figure is that times the ratio of the unit roundoffs, 2.2e-3 * 2^-29 = 4.1e-12,
    and that is the bound used for this one result."""
    c, ref = _reference(name, shape, mode)
    got, _ = cases.run_modules(c, mode == "train", torch.float64)
    errs = {k: cases.metric(got, ref, k) for k in cases.RESULTS}
    worst = max((v, k) for k, v in errs.items())
    print("point-mlp restatement %-8s %dx%-5d %-5s worst %.2e (%s)" % (name, shape[0], shape[1], mode, worst[0], worst[1]))
    for k, v in errs.items():
        assert v <= (2.2e-3 * 2.0 ** -29 if (name, mode, k) == ("bigmean", "train", "rm1") else 1e-12), (k, v)


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("name", cases.CASES)
def test_closed_forms_of_the_kernels_equal_the_restatement(name, mode):
    """The kernels take BN1's statistics from the second moments of x and every gradient below layer 2 from one 64 x 8 sum;
    in float64 that route gives the restatement's results (to the conditioning of `bigmean`: a channel scaled by 1e2)."""
    for shape in cases.SHAPES[:4]:
        c, ref = _reference(name, shape, mode)
        got = cases.closed_forms(c, mode == "train")
        worst = max((cases.metric(got, ref, k), k) for k in cases.RESULTS)
        assert worst[0] <= 1e-9, (shape, worst)


@pytest.mark.parametrize("mutant", cases.MUTANTS)
def test_each_mutant_exceeds_the_bar_on_a_listed_case(mutant):
    """The bar of tests/test_gpu_point_mlp.py is max(8 x the float32 module path's error, 1e-6) per tensor; here the float32
    module path runs on the CPU.  A mutant counts where one of its results is off by more than that bar."""
    best = (0.0, None)
    for name in cases.CASES:
        for shape in cases.SHAPES[:4]:
            for mode in cases.MODES:
                c, ref = _reference(name, shape, mode)
                mut = cases.restate(c, mode == "train", mutant)
                f32, _ = cases.run_modules(c, mode == "train", torch.float32)
                for k in cases.RESULTS:
                    bar = max(8.0 * cases.metric(f32, ref, k), cases.FLOOR)
                    ratio = cases.metric(mut, ref, k) / bar
                    if ratio > best[0]:
                        best = (ratio, "%s %dx%d %s %s" % (name, shape[0], shape[1], mode, k))
    print("point-mlp mutant %-16s largest error / bar %.3g (%s)" % (mutant, best[0], best[1]))
    assert best[0] > 1.0, best


def test_switch_setting_wins_over_the_environment(monkeypatch):
    monkeypatch.delenv("SMOS_POINT_MLP", raising=False)
    prev = ops.set_point_mlp_fused(None)
    try:
        assert ops.point_mlp_fused() is False                     # default 0
        monkeypatch.setenv("SMOS_POINT_MLP", "1")
        assert ops.point_mlp_fused() is True                      # read per call
        assert ops.set_point_mlp_fused(False) is None and ops.point_mlp_fused() is False
        assert ops.set_point_mlp_fused(True) is False and ops.point_mlp_fused() is True
        monkeypatch.setenv("SMOS_POINT_MLP", "0")
        assert ops.point_mlp_fused() is True
        assert ops.set_point_mlp_fused(None) is True and ops.point_mlp_fused() is False
    finally:
        ops.set_point_mlp_fused(prev)


def test_switch_on_keeps_cpu_and_float64_inputs_on_the_module_path():
    c = cases.make_case("normal", 3, 45)
    want, _ = cases.run_modules(c, True, torch.float64)
    prev = ops.set_point_mlp_fused(True)
    try:
        got, _ = cases.run_modules(c, True, torch.float64)
    finally:
        ops.set_point_mlp_fused(prev)
    for k in cases.RESULTS:
        assert np.array_equal(got[k], want[k]), k


def test_header_library_and_signatures_agree():
    declared = util.header_declarations()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name]) == len(declared[name][1]), name


def test_work_space_query_and_the_python_refusals():
    lib = _lib.load()
    chunk = int(lib.smos_point_mlp_chunk())
    assert chunk == 512 and ops.point_mlp_chunk() == chunk
    sizes = [lib.smos_point_mlp_work_bytes(p) for p in (1, chunk, chunk + 1, 12 * 130000)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes[0] == sizes[1] < sizes[2] < sizes[3]
    assert sizes[3] < 80 << 20                                   # the training shape: tens of MB, not an activation
    assert lib.smos_point_mlp_work_bytes(0) == -1 and lib.smos_point_mlp_work_bytes(1 << 31) == -1
    # pinned: 4096 + chunks * row * 4 + groups * row * 8 with rows of 4608 floats, groups of 64 chunks
    pins = {1: 59392, 512: 59392, 513: 77824, 32769: 1275904, 1560000: 57935872, 0: -1, (1 << 31) - chunk: -1}
    assert {p: lib.smos_point_mlp_work_bytes(p) for p in pins} == pins
    assert lib.smos_point_mlp_work_bytes((1 << 31) - chunk - 1) > 0
    assert (lib.smos_point_mlp_fold_floats(), lib.smos_point_mlp_stat_doubles()) == (9296, 280)
    m = cases.build_modules(cases.make_case("normal", 1, 5), torch.float32)
    a, b = m.layer[0].layer, m.layer[1].layer
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.point_mlp_train(torch.zeros(1, 7, 5, 1), a[0], a[1], a[2], b[0], b[1])

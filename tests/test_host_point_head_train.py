"""The float64 reference of ops.point_head_train (tests/point_head_train_cases.py::restate) against torch.autograd through
the float64 CatFusion / PredBranch modules on the CPU, its six mutants against the GPU test's bar, the keep-bit generator
restated in numpy, and the host side of the new entry points (switch, routing, bindings, queries, refusals).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops, preprocess
from streammos_amd.refapi.networks import backbone
from tests import point_head_train_cases as cases
from tests import util

NEW = ("smos_point_head_train_chunk", "smos_point_head_train_fold_floats", "smos_point_head_train_stat_doubles",
       "smos_point_head_train_work_bytes", "smos_point_head_train_mask_words", "smos_point_head_train_masks",
       "smos_point_head_train_fwd", "smos_point_head_train_bwd")
SHAPES = cases.shapes()
KEEP_BELOW = 3435973837          # include/smos.h: a value is kept iff its 32-bit draw is below ceil(0.8 * 2^32)

_cache = {}


def _reference(name, shape, mode):
    key = (name, shape, mode)
    if key not in _cache:
        c = cases.make_case(name, *shape)
        _cache[key] = (c, cases.restate(c, mode == "train"))
    return _cache[key]


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.CASES)
def test_restatement_equals_autograd_of_the_float64_modules(name, shape, mode):
    """1e-12 relative on the logits, the three input gradients, the eight parameter gradients and the four buffers, with one
    derived exception: two points in training (shape 1x2).

    A batch norm over two values has zhat = +-s with s^2 = var / (var + eps), and its backward
    dz = gamma r (da - mean(da) - zhat mean(da zhat)) collapses to gamma r (da0 - da1) / 2 * eps / (var + eps): a difference of
    O(1) terms that cancels down to eps / (var + eps) of their size.  zhat itself is (z - mean) r, exact to 2^-53 |z| / sd
    when z is large next to the spread sd of its two values.  Two float64 evaluations therefore differ by up to
    2^-53 max(1, |z| / sd) (var + eps) / eps relative in dz, and every gradient in front of that batch norm inherits it.
    The bound for this shape is that figure for the worst channel of the case (`restate` reports it as _amp1, _amp2), times
    16 for the handful of roundings that enter: some 1e-10 for the cases with z of order 1, and 1e-7 for `bigmean`, whose
    z1 is near 90 with a spread below 1.  (The float32 module path and the op meet the same cancellation at 2^-24; the GPU
    test measures one against the other.)"""
    c, ref = _reference(name, shape, mode)
    got, _ = cases.run_modules(c, mode == "train", torch.float64)
    errs = {k: cases.metric(got, ref, k) for k in cases.RESULTS}
    worst = max((v, k) for k, v in errs.items())
    bound = 1e-12
    if mode == "train" and shape == (1, 2):
        bound = max(bound, 16 * 2.0 ** -53 * max(ref["_amp1"], ref["_amp2"]))
    print("point-head-train restatement %-8s %dx%-5d %-5s worst %.2e (%s) bound %.1e" % (name, shape[0], shape[1], mode, worst[0],
                                                                                         worst[1], bound))
    for k, v in errs.items():
        assert v <= bound, (k, v)


LISTED = {"no_scale_bwd": ("plain", (3, 70), "train"), "biased_running": ("plain", (2, 33), "train"),
          "no_mean_term": ("plain", (3, 70), "train"), "relu_wrong_layer": ("plain", (3, 70), "eval"),
          "keep2_before_bn": ("plain", (3, 70), "train"), "dw1_unmasked_x": ("dropped", (3, 70), "train")}


@pytest.mark.parametrize("mutant", cases.MUTANTS)
def test_each_mutant_exceeds_the_bar_on_its_listed_case(mutant):
    """The bar of tests/test_gpu_point_head_train.py is max(8 x the float32 module path's error, 1e-6) per result; here the
    float32 module path runs on the CPU.  A mutant counts where one of its results is off by more than that bar.
    (`keep2_before_bn`: a keep mask in front of the ReLU alone changes nothing, ReLU commutes with a non-negative factor;
    the mutant puts it in front of BN2, where it changes the statistics.)"""
    name, shape, mode = LISTED[mutant]
    c, ref = _reference(name, shape, mode)
    mut = cases.restate(c, mode == "train", mutant)
    f32, _ = cases.run_modules(c, mode == "train", torch.float32)
    best = (0.0, "")
    for k in cases.RESULTS:
        bar = max(8.0 * cases.metric(f32, ref, k), cases.FLOOR)
        best = max(best, (cases.metric(mut, ref, k) / bar, k))
    print("point-head-train mutant %-18s largest error / bar %.3g (%s)" % (mutant, best[0], best[1]))
    assert best[0] > 1.0, best


def test_steered_cases_are_what_they_say():
    b, n = 3, 70
    c = cases.make_case("dead", b, n)
    ref = cases.restate(c, True)
    assert ref["dg1"][cases.DEAD1] == 0.0 and ref["dbe1"][cases.DEAD1] == 0.0 and not ref["dw1"][cases.DEAD1].any()
    assert ref["dg2"][cases.DEAD2] == 0.0 and ref["dbe2"][cases.DEAD2] == 0.0 and not ref["dw2"][cases.DEAD2].any()
    c = cases.make_case("const", b, n)
    assert not cases.restate(c, True)["dw2"][cases.CONST2].any()
    c = cases.make_case("dropped", b, n)
    ref = cases.restate(c, True)
    pb, pn = cases.dropped_point(b, n)
    assert np.array_equal(ref["logits"][pb, :, pn, 0], c["b3"])
    assert not ref["dxa"][:, cases.DROPPED_CHANNEL].any() and not ref["dw1"][:, cases.DROPPED_CHANNEL].any()
    c = cases.make_case("bigmean", b, n)
    big = np.concatenate([c[k] for k in cases.INPUTS], 1)[:, cases.BIG_CHANNEL]
    assert abs(big.mean() - 1000.0) < 0.01 and 0.005 < big.std() < 0.02
    for name in cases.CASES:
        assert all((cases.make_case(name, b, n)[k] >= 0).all() for k in cases.INPUTS)
    assert SHAPES[:4] == ((1, 2), (2, 33), (3, 70), (6, 97))
    chunk = ops.point_head_train_chunk()
    assert SHAPES[4][0] == 2 and 3 * chunk < 2 * SHAPES[4][1] <= 3 * chunk + 2


def keep_words(seed, points):
    """The generator of csrc/point_head_train.hip in numpy -> [8, P] uint32 word planes: Philox4x32-10, key = the halves of
    seed[0], counter (point, 8 word + i, halves of seed[1]); output v of call i decides bit 4 i + v."""
    s0, s1 = (int(v) & 0xFFFFFFFFFFFFFFFF for v in seed)
    p = np.arange(points, dtype=np.uint64)
    words = np.zeros((8, points), dtype=np.uint32)
    for w in range(8):
        for i in range(8):
            ctr = np.stack([p, np.full(points, 8 * w + i, np.uint64), np.full(points, s1 & 0xFFFFFFFF, np.uint64),
                            np.full(points, s1 >> 32, np.uint64)], 1)
            key = np.tile(np.array([s0 & 0xFFFFFFFF, s0 >> 32], dtype=np.uint64), (points, 1))
            draw = np.asarray(preprocess.philox4x32(ctr, key), dtype=np.uint64).reshape(points, 4)
            for v in range(4):
                words[w] |= ((draw[:, v] < KEEP_BELOW).astype(np.uint32) << np.uint32(4 * i + v))
    return words


def keep_statistics_ok(words):
    """the checks of the GPU test on generated bits: the overall keep fraction within 5 sigma of 0.8, each of the 256 channels
    within 6 sigma"""
    points = words.shape[1]
    bits = ((words[:, None, :] >> np.arange(32, dtype=np.uint32)[None, :, None]) & 1).reshape(256, points)
    sigma = np.sqrt(0.8 * 0.2 / points)
    return abs(bits.mean() - 0.8) <= 5 * sigma / 16.0 and bool((np.abs(bits.mean(1) - 0.8) <= 6 * sigma).all())


def test_generator_restated_in_numpy_keeps_four_fifths():
    assert KEEP_BELOW == -(-4 * 2 ** 32 // 5) and abs(KEEP_BELOW / 2.0 ** 32 - 0.8) < 2.0 ** -16
    a = keep_words((0x0123456789ABCDEF, -5), 2 * 4096)
    assert keep_statistics_ok(a)
    assert np.array_equal(a, keep_words((0x0123456789ABCDEF, -5), 2 * 4096))
    assert (a != keep_words((0x0123456789ABCDEF, -4), 2 * 4096)).mean() > 0.9
    assert np.array_equal(a[:, :100], keep_words((0x0123456789ABCDEF, -5), 100))       # a point's bits do not depend on P


def test_switch_setting_wins_over_the_environment(monkeypatch):
    monkeypatch.delenv("SMOS_POINT_HEAD_TRAIN", raising=False)
    prev = ops.set_point_head_fused(None)
    try:
        assert ops.point_head_fused() is False                     # default 0
        monkeypatch.setenv("SMOS_POINT_HEAD_TRAIN", "1")
        assert ops.point_head_fused() is True                      # read per call
        assert ops.set_point_head_fused(False) is None and ops.point_head_fused() is False
        assert ops.set_point_head_fused(True) is False and ops.point_head_fused() is True
        monkeypatch.setenv("SMOS_POINT_HEAD_TRAIN", "0")
        assert ops.point_head_fused() is True
        assert ops.set_point_head_fused(None) is True and ops.point_head_fused() is False
    finally:
        ops.set_point_head_fused(prev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_switch_on_keeps_cpu_inputs_on_the_module_path(dtype, monkeypatch):
    c = cases.make_case("plain", 2, 33)
    calls = []
    monkeypatch.setattr(ops, "point_head_train", lambda *a, **k: calls.append(1))
    outs = []
    for flag in (False, True):
        fusion, pred = cases.build_modules(c, dtype)
        fusion.train()
        pred.train()
        xs, _, _ = cases.case_tensors(c, dtype, "cpu")
        prev = ops.set_point_head_fused(flag)
        try:
            torch.manual_seed(5)
            outs.append(backbone.point_head(fusion, pred, *xs))
        finally:
            ops.set_point_head_fused(prev)
    assert not calls and torch.equal(outs[0], outs[1])
    fusion, pred = cases.build_modules(c, dtype)
    torch.manual_seed(5)
    assert torch.equal(outs[0], pred.train()(fusion.train()(*cases.case_tensors(c, dtype, "cpu")[0])))


def test_header_library_and_signatures_agree():
    declared = util.header_declarations()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name]) == len(declared[name][1]), name
        assert (declared[name][0] == "int64_t") == (name in _lib.INT64_RESULTS)


def test_queries_and_the_python_refusals():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW[:5]:
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int64 if name in _lib.INT64_RESULTS else ctypes.c_int
    chunk = lib.smos_point_head_train_chunk()
    assert chunk == ops.point_head_train_chunk() and chunk % 256 == 0
    assert lib.smos_point_head_train_fold_floats() > 192 * 96 + 64 * 96 and lib.smos_point_head_train_stat_doubles() == 2 * (96 + 64)
    sizes = [lib.smos_point_head_train_work_bytes(p) for p in (1, chunk, chunk + 1, 4 * 130000)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes[0] == sizes[1] < sizes[2] < sizes[3]
    assert sizes[3] < 48 << 20                                   # the training shape: tens of MB, not an activation
    assert [lib.smos_point_head_train_mask_words(p) for p in (1, 7, 4 * 130000)] == [8, 56, 8 * 4 * 130000]      # 32 bytes a point
    for q in (lib.smos_point_head_train_work_bytes, lib.smos_point_head_train_mask_words):
        assert q(0) == -1 and q(1 << 31) == -1
        assert q((1 << 31) - chunk) == -1 and q((1 << 31) - chunk - 1) > 0
    # pinned: 4096 + chunks * row * 4 + groups * row * 8 with rows of 18432 floats, groups of 64 chunks
    pins = {1: 225280, 1024: 225280, 1025: 299008, 65537: 5091328, 520000: 38637568}
    assert {p: lib.smos_point_head_train_work_bytes(p) for p in pins} == pins
    assert (lib.smos_point_head_train_fold_floats(), lib.smos_point_head_train_stat_doubles()) == (25828, 320)
    assert all(lib.smos_point_head_train_mask_words(p) == 8 * p for p in pins)
    c = cases.make_case("plain", 1, 2)
    fusion, pred = cases.build_modules(c, torch.float32)
    m, head = fusion.merge_layer, pred.pred_layer[0]
    xs, _, _ = cases.case_tensors(c, torch.float32, "cpu", grad=False)
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.point_head_train(*xs, m[0], m[1], m[3], m[4], head)

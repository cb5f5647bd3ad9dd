"""The references, bounds, restatements, mutants and cases of tests/point_head_cases.py without a GPU, and the prepared weight
block of ops.point_head_prepare walked on the host as the kernel walks it (pytest -s prints every figure)."""
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import gather_cases
from tests import point_head_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_NAMES = tuple(cases.BOUND_SPECS) + tuple(cases.WALK_SPECS)


def test_both_launches_pass_their_grid_through_the_cap():
    assert cases.launch_honours_cap() == (True, True)
    for name in ("smos_common.h",):
        with open(os.path.join(ROOT, "streammos_amd", "csrc", name)) as f:
            text = f.read()
        assert "point_head (csrc/point_head.hip)" in text and "tta_argmax (csrc/vote.hip)" in text


@pytest.mark.parametrize("name", RANDOM_NAMES)
def test_restatement_stays_inside_the_bound(name):
    c = cases.case(name)
    for form in cases.FORMS:
        rest = cases.restatement(name, form)
        for g, rows in c.rows.items():
            ok, r = cases.worst_ratio(rest[:, :, rows], c.ref[form][:, :, rows], c.lim[form][:, :, rows])
            print("restatement %-14s %-6s %-9s worst error / bound %.4f" % (name, form, g, r))
            assert ok and r < 1.0, (name, form, g, r)
        assert np.isfinite(c.lim[form]).all() and (c.lim[form] > 0).all()


@pytest.mark.parametrize("mutant", sorted(cases.MUTANTS))
def test_mutants_leave_the_bound(mutant):
    name, form = cases.MUTANTS[mutant]
    c = cases.case(name)
    out = cases.mutant_out(mutant)
    ok, r = cases.worst_ratio(out, c.ref[form], c.lim[form])
    outside = float((np.abs(out - c.ref[form]) > c.lim[form]).mean())
    print("mutant %-16s on %-10s %-6s worst error / bound %.3g, %.1f %% of the logits outside" % (mutant, name, form, r, 100 * outside))
    assert not ok and r >= cases.MUTANT_MARGIN, (mutant, r)


def test_mutant_cases_are_what_the_mutants_need():
    assert cases.case(cases.MUTANTS["rows16_half0"][0]).m3 > 20          # a row >= 16 in lane half 1
    assert cases.case(cases.MUTANTS["b3_xor4"][0]).m3 >= 8
    c = cases.case(cases.MUTANTS["stale_coord"][0])
    assert c.n > 32 and not np.array_equal(cases.stale_coords(c)[..., :2], c.gcoord[..., :2], equal_nan=True)
    assert set(cases.MUTANTS) == {"swap_l2", "relu_missing", "drop_last_kstep", "rows16_half0", "b3_xor4", "stale_coord"}


@pytest.mark.parametrize("name", cases.EXACT_NAMES)
def test_exact_twins_are_exact(name):
    c = cases.case(name)
    for form in cases.FORMS:
        assert cases.exact_condition(c, form)
        want = c.ref[form].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), c.ref[form])        # the reference is a float32 number
        assert np.array_equal(cases.restatement(name, form).view(np.int32), want.view(np.int32)), (name, form)
        assert (c.lim[form] > 0).all()
    taps = gather_cases.taps(c.gcoord, c.scale, c.hg, c.wg)[3]
    assert c.n < 9 or (taps.any(0).any() and not taps.any(0).all() and (taps.sum(0) == 2).any())   # inside, outside, on a border


def test_cases_cover_what_they_are_named_for():
    sp = cases.BOUND_SPECS
    assert {v["m3"] for v in sp.values()} == {1, 3, 8, 9, 20, 32}
    assert {v["n"] for v in sp.values()} == {1, 31, 32, 33, 70, 300}
    assert {v["b"] for v in sp.values()} == {1, 2, 3} and {v["pitch"] for v in sp.values()} == {192, 200}
    assert (cases.WALK_SPECS["walk_b2_n300"]["b"], cases.WALK_SPECS["walk_b2_n300"]["n"]) == (2, 300)
    assert (cases.WALK_SPECS["walk_b3_n70"]["b"], cases.WALK_SPECS["walk_b3_n70"]["n"]) == (3, 70)
    for name, v in sp.items():
        c = cases.case(name)
        if v["steered"]:
            assert tuple(c.rows) == cases.GROUPS
            seen = np.flatnonzero(c.x[0, c.rows["one_hot"]])
            assert sorted(np.nonzero(c.x[0, c.rows["one_hot"]])[1].tolist()) == list(range(192)) and len(seen) == 192
            assert np.abs(c.x[:, c.rows["big"]]).mean() > 500
        if v["n"] >= 31:                                   # the specials of gather_cases: NaN, inf and padding coordinates
            xy = c.gcoord[..., :2]
            assert np.isnan(xy).any() and np.isinf(xy).any() and (xy == -1000.0).any()


def test_walk_cases_reach_the_loop():
    """From the grid formula, on any CU count >= 2: which (case, cap) pairs take a wave through >= 3 tiles and across a sample
    boundary.  8 waves per block: B = 3, N = 70 (9 tiles) cannot give a wave a third tile under any cap."""
    full = set()
    for name, caps in cases.WALKS.items():
        sp = cases.WALK_SPECS[name]
        for cap in caps:
            for cus in (2, 256, 304):
                blocks = cases.head_blocks(sp["b"], sp["n"], cus, cap)
                assert blocks == min(cap, cus, -(-(sp["b"] * -(-sp["n"] // 32)) // 8))
                most, cross = cases.walk_facts(cases.walk_tiles(sp["b"], sp["n"], None, blocks))
                print("walk %-14s cap %d (%3d CUs): %d blocks, most tiles of a wave %d, crosses a sample boundary %s" % (
                    name, cap, cus, blocks, most, cross))
                if most >= 3 and cross:
                    full.add((name, cap))
                if name != "walk_b3_n70" or cap == 1:
                    assert most >= 2 and cross, (name, cap)
    assert full == set(cases.WALK_FULL)
    # without the cap no wave of these shapes takes a second tile on a device of 8 CUs or more
    for name in cases.WALKS:
        sp = cases.WALK_SPECS[name]
        assert cases.walk_facts(cases.walk_tiles(sp["b"], sp["n"], None, cases.head_blocks(sp["b"], sp["n"], 8, 0)))[0] == 1


# ---- ops.point_head_prepare ---------------------------------------------------------------------------------------------

def _prepared(c):
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))            # noqa: E731
    flat, m3 = ops.point_head_prepare((t(c.w1).view(96, 192, 1, 1), t(c.b1)), (t(c.w2).view(64, 96, 1, 1), t(c.b2)),
                                      (t(c.w3).view(c.m3, 64, 1, 1), t(c.b3)))
    assert m3 == c.m3
    return flat.double().numpy()


@pytest.mark.parametrize("name", ["n1_m1/x", "n32_m8/x", "n33_m9/x", "n70_m20/x", "n70_m32/x", "n31_m3"])
def test_prepared_block_walked_in_accumulator_order(name):
    """The layer 2 / 3 twin of test_layer1_operand_order_reproduces_w1_times_row: walking the A2 and A3 blocks with the hidden
    channels in accumulator order reproduces W2 @ h and W3 @ h (exactly, on the exact twins' weights); the biases sit at their
    offsets; rows >= M3 of A3 and of b3 are zero; the block has smos_point_head_weight_floats() floats."""
    c = cases.case(name)
    flat = _prepared(c)
    assert flat.size == _lib.query("smos_point_head_weight_floats") == cases.BLOCK_FLOATS
    assert np.array_equal(cases.k_order(), ops.point_head_k_order().numpy())
    rng = np.random.default_rng(5)
    h1, h2 = rng.integers(-8, 9, 96).astype(np.float64), rng.integers(-8, 9, 64).astype(np.float64)
    got2, got3 = cases.walk_block(flat, c.m3, h1, h2)
    want3 = np.zeros(32)
    want3[:c.m3] = c.w3 @ h2
    if c.exact:
        assert np.array_equal(got2, c.w2 @ h1) and np.array_equal(got3, want3)
    else:
        assert np.abs(got2 - c.w2 @ h1).max() <= 1e-12 and np.abs(got3 - want3).max() <= 1e-12
    # one channel at a time: every (row, channel) slot of both blocks
    for k in range(96):
        e = np.zeros(96)
        e[k] = 1.0
        assert np.array_equal(cases.walk_block(flat, c.m3, e, np.zeros(64))[0], c.w2[:, k]), k
    for k in range(64):
        e = np.zeros(64)
        e[k] = 1.0
        col = cases.walk_block(flat, c.m3, np.zeros(96), e)[1]
        assert np.array_equal(col[:c.m3], c.w3[:, k]) and not col[c.m3:].any(), k
    a3 = flat[cases.A1_FLOATS + cases.A2_FLOATS:cases.A1_FLOATS + cases.A2_FLOATS + cases.A3_FLOATS].reshape(32, 2, 32)
    assert not a3[:, :, c.m3:].any()
    tail = flat[cases.A1_FLOATS + cases.A2_FLOATS + cases.A3_FLOATS:]
    b3p = np.zeros(32)
    b3p[:c.m3] = c.b3
    assert np.array_equal(tail, np.concatenate((c.b1, c.b2, b3p)))


# ---- tta_argmax -----------------------------------------------------------------------------------------------------------

def test_tta_restatement_inside_its_bound_and_the_constant_is_the_measured_one():
    worst, at = 0.0, None
    for name in cases.TTA_SPECS:
        c = cases.tta_case(name)
        prob, labels = cases.tta_f32(c.pred)
        err = float(np.abs(prob.astype(np.float64) - c.prob).max())
        print("tta restatement %-20s worst error %.3f u, bound %4.1f u, left out %.4f" % (name, err / cases.U, c.lim / cases.U,
                                                                                          cases.left_out(c)))
        assert err <= c.lim, (name, err / cases.U)
        assert np.array_equal(labels[c.decided], c.labels[c.decided]), name
        if err > worst:
            worst, at = err, name
    measured = 2.0 ** np.ceil(np.log2(2.0 * worst / cases.U))
    print("tta: worst restatement error %.3f u on %s -> TTA_EXP_ULP %g" % (worst / cases.U, at, measured))
    assert measured == cases.TTA_EXP_ULP, (worst / cases.U, at)


def test_tta_cases_decide_their_labels_and_hold_what_they_are_named_for():
    sp = cases.TTA_SPECS
    assert {v["k"] for v in sp.values()} == {1, 2, 3, 8} and {v["b"] for v in sp.values()} == {1, 2, 4, 5}
    assert {v["n"] for v in sp.values()} == {1, 255, 256, 257, 1000}
    for name, v in sp.items():
        c = cases.tta_case(name)
        assert cases.left_out(c) <= cases.MAX_LEFT_OUT, (name, cases.left_out(c))
        assert np.abs(c.prob.sum(1) - 1.0).max() < 1e-12
        if v["k"] == 1:
            assert (c.prob == 1.0).all() and not c.labels.any()
            prob, labels = cases.tta_f32(c.pred)
            assert (prob == 1.0).all() and not labels.any()
        if v["kind"] == "big":
            with np.errstate(over="ignore"):
                naive = np.exp(c.pred.astype(np.float32))
            shifted = np.exp((c.pred - c.pred.max(1, keepdims=True)).astype(np.float32))
            assert np.isinf(naive).any() and (naive < 2.0 ** -126).any()   # without the max subtraction: overflow, subnormal terms
            assert (shifted == 0).any()                                    # with it: the classes 160 below the maximum flush
        if v["kind"] == "ties":
            assert len(c.ties) == len(cases.TIE_POINTS) and {len(t) for t in c.ties.values()} == ({2} if v["k"] == 2 else {2, 3})
            assert any(t[0] > 0 for t in c.ties.values()) or v["k"] == 2
            prob, labels = cases.tta_f32(c.pred)
            for p, cls in c.ties.items():
                assert len({c.pred[:, k, p].tobytes() for k in cls}) == 1
                assert len({prob[p, k].tobytes() for k in cls}) == 1 and labels[p] == cls[0], (name, p)
                assert not c.decided[p] and c.labels[p] in cls

"""The float64 reference, the bounds, the float32 restatements and the case tables of tests/conv_cases.py without a GPU: the
reference against torch's float64 CPU conv2d, the sum tables against a plain loop, each algorithm's float32 restatement inside
its derived bound (and exact on the exact cases), and the capped cases checked to be what they are named for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as cases

ALL = sorted(cases.SPECS)
RANDOM = sorted(set(cases.BOUND_SPECS) | set(cases.PAD_SPECS) | {k for k in cases.WALK_SPECS})
EXACT = sorted(k for k in cases.SPECS if cases.SPECS[k]["exact"])


@pytest.mark.parametrize("name", ALL)
def test_reference_equals_float64_conv2d(name):
    """Odd padding, stride 2 and even kernels included (the padding cases)."""
    c = cases.case(name)
    x, w = torch.tensor(c.x).permute(0, 3, 1, 2), torch.tensor(c.wt)
    v = F.conv2d(x, w, None if c.bias is None else torch.tensor(c.bias), c.stride, c.pad)
    if c.res is not None:
        v = v + torch.tensor(c.res).permute(0, 3, 1, 2)
    slope = torch.tensor(cases.ACT_SLOPE[c.act], dtype=torch.float64)
    want = (v.clamp_min(0) + slope * v.clamp_max(0)).permute(0, 2, 3, 1).numpy()
    assert want.shape == c.ref.shape == (c.b, c.ho, c.wo, c.cout)
    assert np.abs(c.ref - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    mag = F.conv2d(x.abs(), w.abs(), None, c.stride, c.pad).permute(0, 2, 3, 1).numpy()
    assert np.abs(c.mag - mag).max() <= 1e-12 * mag.max()
    assert (c.mag >= np.abs(cases.conv_direct(c.x, c.wt, c.stride, c.pad)) - 1e-12).all()
    # outputs whose whole window is padding: nothing but the bias arrives
    if c.all_pad.any():
        want_pad = cases.act_apply(np.zeros(c.cout) if c.bias is None else c.bias, c.act)
        if c.res is None:
            assert np.array_equal(c.ref[:, c.all_pad], np.broadcast_to(want_pad, c.ref[:, c.all_pad].shape))
        assert not c.mag[:, c.all_pad].any()


def test_padding_cases_have_wholly_padded_rows_and_columns():
    rows = cases.case("p_3x3_rows_out").all_pad
    cols = cases.case("p_3x3_over").all_pad
    assert rows[0].all() and rows[-1].all() and not rows[1:-1].any()
    assert cols[:, 0].all() and cols[:, -1].all() and not cols[:, 1:-1].any()
    assert cases.case("p_3x3_s2_over").all_pad[:, 0].all()
    for name in ("p_3x3_none", "p_3x3_h", "p_3x3_w", "p_2x2_s2", "p_4x2", "p_3x3_s2_none"):
        assert not cases.case(name).all_pad.any()


@pytest.mark.parametrize("rows", (1, 2))
def test_sum_tables_equal_a_plain_loop(rows):
    rng = np.random.default_rng(5)
    for b, ho, wo, c in ((2, 9, 33, 3), (1, 8, 32, 2), (3, 1, 1, 1), (2, 17, 65, 2), (1, 3, 31, 4)):
        out = np.round(rng.standard_normal((b, ho, wo, c)) * 64)
        tab = cases.sum_table(out, rows)
        assert tab.shape == (b, -(-ho // (4 * rows)) * -(-wo // 32) * 4, c)
        assert np.array_equal(tab, cases.sum_table_loop(out, rows))
        assert np.array_equal(tab.sum(1), out.sum((1, 2)))


def test_sum_table_sizes_are_the_wrappers():
    from streammos_amd import ops
    for ho, wo in ((1, 1), (4, 32), (5, 33), (9, 31), (17, 65)):
        out = np.zeros((1, ho, wo, 1))
        assert cases.sum_table(out, 1).shape[1] == ops.conv_sum_chunks(ho, wo)
        assert cases.sum_table(out, 2).shape[1] == ops.conv_wino_sum_chunks(ho, wo)


def _families(c):
    return [f for f in cases.FAMILIES if cases.family_takes(f, c)]


@pytest.mark.parametrize("name", RANDOM)
def test_float32_restatements_stay_inside_the_bound(name):
    """Direct form: a k-ordered float32 fma chain.  Winograd forms: float32 transforms with U rounded once.  conv_bf16: the
    chain on bf16-rounded operands.  Prints error / bound and the RMS error relative to the RMS of the float64 reference."""
    c = cases.case(name)
    fams = _families(c)
    assert fams
    for fam in fams:
        if fam == "rows":
            continue                                          # the direct form again
        ref, lim = cases.reference(name, fam)
        got = cases.restatement(name, fam)
        assert got.dtype == np.float32 and got.shape == ref.shape
        ok, ratio = cases.worst_ratio(got, ref, lim)
        print("%-18s %-7s restatement: max error / bound %.4f, RMS error / RMS reference %.3e" % (
            name, fam, ratio, cases.rms(got - ref) / max(cases.rms(ref), 1e-300)))
        assert ok and 0 < ratio <= 1, (name, fam, ratio)
        if c.sums and fam != "wino1d" and c.res is None:
            rows = cases.sum_rows(fam)
            tab = cases.sum_table(got.astype(np.float64), rows).astype(np.float32)        # at least one rounding per entry
            ok, sratio = cases.worst_ratio(tab, cases.sum_table(ref, rows), cases.sum_bound(ref, lim, rows))
            assert ok and sratio <= 1, (name, fam, sratio)


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_are_exact_in_every_algorithm(name):
    """The generator's sufficient condition holds per algorithm, and each float32 restatement returns float32(reference) bit for
    bit -- at Cin = 128 (x_k3x3_c128) the float32 F(2x2, 3x3) emulation equals the float64 direct form exactly."""
    c = cases.case(name)
    for fam in _families(c):
        assert cases.exact_condition(c, fam), (name, fam)
        ref, _ = cases.reference(name, fam)
        assert np.array_equal(ref, c.ref)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) or c.act == 2
        if fam != "rows":
            assert np.array_equal(cases.restatement(name, fam), ref.astype(np.float32)), (name, fam)
    if c.sums:
        for fam in _families(c):
            if fam != "wino1d":
                assert cases.exact_condition(c, fam, sums=True), (name, fam)


def test_exactness_condition_refuses_what_is_not_exact():
    assert not cases.exact_condition(cases.case("k3x3_9x33"), "igemm")
    assert not cases.exact_condition(cases.case("x_k3x3_res"), "igemm", sums=True)          # LeakyReLU outputs


def test_bf16_rounding_is_round_to_nearest_even():
    a = np.array([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0, 0.0, 4.0], dtype=np.float32)
    want = torch.tensor(a).to(torch.bfloat16).double().numpy()
    assert np.array_equal(cases.bf16_round(a), want)
    rng = np.random.default_rng(3)
    r = rng.standard_normal(4096).astype(np.float32)
    assert np.array_equal(cases.bf16_round(r), torch.tensor(r).to(torch.bfloat16).double().numpy())


def test_bound_cases_cover_what_the_kernels_branch_on():
    per = {f: [cases.case(n) for n in cases.BOUND_SPECS if cases.family_takes(f, cases.case(n))] for f in cases.FAMILIES}
    for fam, cs in per.items():
        assert {c.act for c in cs} == {0, 1, 2}, fam
        assert {c.bias is None for c in cs} == {False, True}, fam
        want_cin = {16, 32, 48, 64, 128} if fam in ("wino", "wino1d") else {32, 64, 128}
        assert {c.cin for c in cs} == want_cin, fam
        assert {t for c in cs for t in cases.tiles(fam, c)} == {"igemm": {1, 2, 4}, "bf16": {0}}.get(fam, {1, 2}), fam
        assert any((c.h, c.w) == (1, 1) for c in cs), fam
        if fam != "wino1d":
            assert {c.res is None for c in cs} == {False, True} and any(c.sums and c.res is None for c in cs), fam
        if fam in ("igemm", "bf16"):
            assert {c.stride for c in cs} == {1, 2}
            assert {(1, 1), (3, 3), (7, 3), (3, 7), (5, 3), (3, 5)} <= {c.k for c in cs}
    assert {(c.h, c.w) for c in per["wino"]} >= set(cases.SIZES) and {(c.h, c.w) for c in per["igemm"]} >= set(cases.SIZES)
    assert {c.k for c in per["wino1d"]} == set(cases.WINO1D_KERNELS)
    assert {c.k for c in per["rows"]} >= {(1, 3), (3, 3), (7, 3), (3, 7), (5, 3), (3, 5)}


def test_xcd_remap_is_a_bijection_for_every_grid():
    for grid in list(range(1, 70)) + [255, 256, 509, 512]:
        assert sorted(cases.xcd_remap(grid)) == list(range(grid)), grid
    assert (11 >> 3, 11 & 7) == (1, 3)


@pytest.mark.parametrize("name", sorted(cases.WALK_SPECS))
def test_walk_cases_give_a_block_several_items(name):
    fam, tile, sums, caps, _ = cases.WALK_SPECS[name]
    c = cases.case(name)
    assert cases.family_takes(fam, c) and tile in cases.tiles(fam, c)
    n = cases.items(fam, c, tile, sums)
    for cap in caps:
        assert n > cap, (name, n, cap)
        shares = cases.block_shares(n, cap)
        assert sum(shares) == n and max(shares) >= 2
    x = cases.case(name + "/x")
    assert x.exact and (x.b, x.h, x.w, x.cin, x.cout, x.k) == (c.b, c.h, c.w, c.cin, c.cout, c.k)
    assert cases.exact_condition(x, fam, sums=sums) or (sums and x.act == 2)


def test_walk_cases_reach_the_short_streams_and_every_wrap():
    W = cases.WALK_SPECS
    shares = lambda name, cap: cases.block_shares(cases.items(W[name][0], cases.case(name), W[name][1], W[name][2]), cap)
    # conv_igemm, one stage per item: 2, 3, 4 items in one block; 2 + 2 + 1; three per block under 11
    for n in (2, 3, 4):
        c = cases.case("igemm_1x1_%ditems" % n)
        assert c.K == 32 and shares("igemm_1x1_%ditems" % n, 1) == [n]
    assert shares("igemm_1x1_5items", 3) == [2, 2, 1]
    assert shares("igemm_1x1_24items", 11) == [3] * 8 + [0] * 3 and shares("igemm_1x1_24items", 3) == [8, 8, 8]
    # conv_rows: one group per item at (1, 3) / Cin 32, three at (3, 3)
    assert cases.case("rows_1x3").k == (1, 3) and cases.case("rows_1x3").cin == 32 and cases.case("rows_3x3").cin == 32
    # an odd number of cout tiles; sample, row and column wraps inside one block
    for name in ("igemm_3x3_nct3", "rows_3x3_nct3"):
        c = cases.case(name)
        assert c.cout // 32 == 3 and c.b > 1 and -(-c.ho // 4) > 1 and -(-c.wo // 32) > 1
        assert shares(name, 1) == [24] and shares(name, 11) == [3] * 8 + [0] * 3
    # conv_bf16: the block shapes the cases reach
    got = {}
    for name in W:
        if W[name][0] == "bf16":
            c = cases.case(name)
            cfg = cases.bf16_cfg(c.b, c.ho, c.wo, c.cout, c.k, c.stride, c.res is not None)
            got[name] = (cfg.mt, cfg.wc, cfg.rw, cfg.rb)
    assert got["bf16_3x3_c32"] == (1, 1, 1, 4) and got["bf16_3x3_res"] == (1, 2, 1, 2) and got["bf16_3x3_c128"] == (1, 4, 1, 1), got
    assert {v[0] for v in got.values()} == {1} and {v[2] for v in got.values()} == {1}       # <MT 1, RW 1> at these sizes


def test_bf16_block_shape_restatement_refuses_what_the_kernel_refuses():
    """Cout 32 at stride 2 with a 3 x 3 kernel: the only block shape (4 rows) stages 9 x 65 pixels, more than 2048 units."""
    assert cases.bf16_cfg(2, 2, 17, 32, (3, 3), 2, False) is None
    assert cases.bf16_cfg(2, 2, 17, 64, (3, 3), 2, False) is not None
    assert cases.bf16_cfg(1, 1, 1, 2048, (1, 1), 1, False) is not None


def test_inf_pixel_reach():
    c = cases.case("n_3x3")
    r = cases.reach(c, 0, 0)
    assert r[:2, :2].all() and r.sum() == 4
    t = cases.tile_reach(c, "wino", 2, c.w - 1)
    assert (t >= cases.reach(c, 2, c.w - 1)).all() and t.sum() > cases.reach(c, 2, c.w - 1).sum()
    for name in ("n_7x3", "n_3x5"):
        c = cases.case(name)
        for y, x in ((0, 0), (2, c.w - 1), (c.h - 1, 5)):
            r, t = cases.reach(c, y, x), cases.tile_reach(c, "wino1d", y, x)
            assert (t >= r).all() and t.sum() <= 2 * r.sum() + 2 * max(c.k)

"""The references, cases and bounds behind tests/test_gpu_upconv.py, checked on the host (tests/util.py).

(a) the float64 decomposition (tap products at source resolution, x pass, y pass, dropped border taps) equals the direct
    float64 form act(conv2d(cat(x0, up(x1), up(x2))) + bias) of torch to 1e-12 of the output range on every case: double
    rounding over at most 9 * 128 terms.  That pins the conventions -- which taps are dropped, what Hs == 1, Ws == 1,
    Ho == 1 and Wo == 1 mean -- before any kernel is involved;
(b) the same decomposition in float32 numpy, with the interpolation weights computed as lerp_of computes them and the tap
    products from a float32 matmul, stays inside the bound the GPU tests use: the bound leaves room for float32
    arithmetic in the kernels' own operation order;
(c) the "exact" inputs are exact: their float32 tap products equal the float64 ones bit for bit;
(d) the bookkeeping the GPU tests rely on: which geometries get the one-launch form, which strip height, where the
    window of a strip slides, which outputs never read a poisoned border element.
"""
import numpy as np
import pytest

from tests import util

_ALL = sorted(util.UPCONV_CASES)
_EXACT = [n for n in _ALL if util.UPCONV_CASES[n][5] == "exact"]


def _f32_products(c):
    return [util.tap_products_ref(x.astype(np.float32), nk.astype(np.float32), np.float32).reshape(z.shape)
            for x, nk, z in zip(c.x, c.nk, c.z)]


@pytest.mark.parametrize("name", _ALL)
def test_float64_decomposition_equals_direct_form(name):
    c = util.upconv_case(name)
    for act in ((0, 2) if c.b * c.ho * c.wo * c.c < 1 << 20 else (2,)):
        want = util.upconv_want(name, act)
        got = util.upconv_passes_ref(c.conv_a, c.bias, c.z64, act)
        assert got.shape == want.shape == (c.b, c.ho, c.wo, c.c)
        diff = np.abs(got - want).max() / np.abs(want).max()
        print("upconv-host %-20s act %d decomposition-vs-direct %.3e of range" % (name, act, diff))
        assert diff <= 1e-12


@pytest.mark.parametrize("name", _ALL)
def test_float32_emulation_stays_inside_the_bound(name):
    c = util.upconv_case(name)
    got = util.upconv_passes_ref(c.conv_a.astype(np.float32), c.bias.astype(np.float32), _f32_products(c), 2, np.float32)
    assert got.dtype == np.float32
    ok, ratio = util.msda_worst_ratio(got, util.upconv_want(name, 2), util.upconv_bound(name))
    print("upconv-host %-20s float32-emulation error/bound %.3f (whole op)" % (name, ratio))
    assert ok, ratio
    if name in util.UPCONV_PASS_CASES:                       # the passes alone, from the known float32 z
        got = util.upconv_passes_ref(c.conv_a.astype(np.float32), c.bias.astype(np.float32), c.z, 2, np.float32)
        ok, ratio = util.msda_worst_ratio(got, util.upconv_passes_want(name, 2), util.upconv_passes_bound(name))
        print("upconv-host %-20s float32-emulation error/bound %.3f (passes)" % (name, ratio))
        assert ok, ratio


@pytest.mark.parametrize("name", _EXACT)
def test_exact_inputs_have_exact_float32_tap_products(name):
    c = util.upconv_case(name)
    for x, nk, z64, z, got in zip(c.x, c.nk, c.z64, c.z, _f32_products(c)):
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8
        assert np.array_equal(nk * 64, np.round(nk * 64)) and np.abs(nk).max() <= 1
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), z64) and np.array_equal(z, z64)
        assert np.abs(util.tap_products_ref(np.abs(x), np.abs(nk))).max() <= 2.0 ** 10      # every partial sum fits 24 bits
        # and in another summation order: the reversed one
        rev = util.tap_products_ref(x[..., ::-1].astype(np.float32), nk[:, ::-1].astype(np.float32), np.float32)
        assert np.array_equal(rev.reshape(z.shape).astype(np.float64), z64)


def test_float32_weights_are_exact_for_dyadic_ratios_only():
    for n_src, n_dst, dyadic in ((5, 9, True), (3, 9, True), (6, 6, True), (1, 7, True), (3, 1, True), (2, 9, True),
                                 (5, 10, False), (15, 20, False), (10, 37, True), (10, 21, False), (9, 33, True)):
        assert util.upconv_dyadic(n_src, n_dst) == dyadic, (n_src, n_dst)
        a, b = util.upconv_lerp(n_src, n_dst, np.float32), util.upconv_lerp(n_src, n_dst)
        same = all(np.array_equal(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)) for u, v in zip(a, b))
        assert same or not dyadic, (n_src, n_dst)
    # the perturbation the bound allows for a non-dyadic axis covers what lerp_of's float32 s does: |ds| <= 2 u (n_src - 1)
    for n_src, n_dst in ((5, 10), (15, 20), (13, 47), (97, 200), (128, 255), (10, 21)):
        i0, _, _, w1 = util.upconv_lerp(n_src, n_dst, np.float32)
        j0, _, _, v1 = util.upconv_lerp(n_src, n_dst)
        ds = np.abs((i0 + w1.astype(np.float64)) - (j0 + v1))
        assert ds.max() <= 2 * util.UPCONV_U * (n_src - 1), (n_src, n_dst, ds.max())


def test_geometries_reach_the_launches_and_strips_they_are_named_for():
    fused = {n: all(util.upconv_xy_ok(hs, util.UPCONV_CASES[n][1][0]) for hs, _ in util.UPCONV_CASES[n][2]) for n in _ALL}
    assert fused["fused_5to10"] and fused["fused_3to9_dyadic"] and fused["two_ratios"] and fused["hs1"] and fused["all_one"]
    assert not fused["pair_5to9_dyadic"] and not fused["pair_15to20"] and not fused["identity"] and not fused["ho1"]
    assert util.upconv_xy_ok(5, 10) and not util.upconv_xy_ok(5, 9) and util.upconv_xy_ok(1, 1) and not util.upconv_xy_ok(2, 1)
    for name, strip in (("strip8", 8), ("strip16", 16), ("strip32", 32)):
        b, (ho, wo), sizes, ch, _, _ = util.UPCONV_CASES[name]
        assert fused[name] and util.upconv_strip(b, ho, wo, ch) == strip and ho % strip and ho > strip
        hs = sizes[0][0]
        i0 = util.upconv_lerp(hs, ho, np.float32)[0]
        y0 = ho // strip * strip                                  # the last, partial strip
        base = i0[y0 - 1]
        assert base > 0 and y0 + 1 < ho and i0[y0] == base + 1     # row y0 + 1 asks for lo = i0[y0] > base: the window slides there
        assert (np.diff(i0) <= 1).all()                           # it never has to slide by two


@pytest.mark.parametrize("name", ["fused_3to9_dyadic", "pair_5to9_dyadic"])
def test_border_outputs_never_read_the_poisoned_elements(name):
    """With Inf in the elements upconv_poison_borders names, the reference's outputs on that border stay finite and equal the
    clean ones; somewhere inside they do not (the Inf is really read there).  Dyadic ratios: the float32 weights pick the
    same source samples as the reference's, so the set of finite outputs is the kernels' too."""
    c = util.upconv_case(name)
    clean = util.upconv_passes_want(name, 0)
    for sides in [(s,) for s in util.UPCONV_SIDES] + [util.UPCONV_SIDES]:
        got = util.upconv_passes_ref(c.conv_a, c.bias, [util.upconv_poison_borders(z, sides) for z in c.z], 0)
        finite = np.isfinite(got)
        assert np.array_equal(got[finite], clean[finite]) and not finite.all()
        if len(sides) == 1:
            assert finite[util.upconv_border_line(sides[0], c.ho, c.wo)].all()
        else:
            assert finite[:, 0, 0].all() and finite[:, -1, -1].all()
        f32 = util.upconv_passes_ref(c.conv_a, c.bias, [util.upconv_poison_borders(z, sides) for z in c.z], 0, np.float32)
        assert np.array_equal(np.isfinite(f32), finite)

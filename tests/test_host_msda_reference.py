"""The references and case generators behind tests/test_gpu_msda.py, checked on the host (tests/util.py).

(a) the two float64 references agree: the numpy oracle (pinned to the reference's golden outputs, used for the forward)
    and the torch formulation (whose autograd is the backward reference) to 1e-14 of the output range;
(b) no backward case samples an integer pixel coordinate, where the reference is not differentiable;
(c) the numpy oracle run in float32 stays inside the forward bound the GPU tests use: the bound leaves room for float32
    arithmetic in the oracle's own operation order.

The qp cases take (c) only: their reference is the oracle itself, fed by a float64 softmax and ref + off / (W, H).
"""
import numpy as np
import pytest

from tests import util

_LOC_CASES = sorted(util.MSDA_FWD_CASES) + sorted(util.MSDA_BORDER_CASES) + sorted(util.MSDA_BWD_CASES)


def _case(name):
    return util.msda_bwd_case(name) if name in util.MSDA_BWD_CASES else util.msda_any_fwd_case(name)


def _forward_ref(c, name):
    return util.msda_forward_ref(c) if name in util.MSDA_BWD_CASES else (c.want, c.mag)


@pytest.mark.parametrize("name", _LOC_CASES)
def test_torch_formulation_equals_numpy_oracle_in_float64(name):
    c = _case(name)
    want, _ = _forward_ref(c, name)
    got = util.msda_torch_formulation(c)
    assert got.shape == want.shape
    diff = np.abs(got - want).max()
    print("msda-host %s torch-vs-numpy %.3e of range" % (name, diff / np.abs(want).max()))
    assert diff <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("name", sorted(util.MSDA_BWD_CASES))
def test_backward_cases_avoid_integer_pixel_coordinates(name):
    c = util.msda_bwd_case(name)
    size = c.shapes[:, ::-1].astype(np.float64)[None, None, None, :, None, :]              # (W, H) per level
    pix = c.loc * size - 0.5
    assert np.array_equal((pix + 0.5) / size, c.loc)                                       # exact: dyadic coordinates
    assert not (pix == np.floor(pix)).any()
    assert np.array_equal(pix.astype(np.float32).astype(np.float64), pix)                 # the same number in float32


@pytest.mark.parametrize("name", sorted(util.MSDA_FWD_CASES) + sorted(util.MSDA_BORDER_CASES))
def test_forward_cases_have_the_same_coordinates_in_both_precisions(name):
    c = util.msda_any_fwd_case(name)
    size = c.shapes[:, ::-1].astype(np.float64)[None, None, None, :, None, :]
    pix = c.loc * size - 0.5
    pix32 = c.loc.astype(np.float32) * size.astype(np.float32) - np.float32(0.5)
    assert pix32.dtype == np.float32 and np.array_equal(pix32.astype(np.float64), pix)


def test_border_cases_hold_every_pair_of_border_coordinates():
    for name in util.MSDA_BORDER_CASES:
        c = util.msda_border_case(name)
        h, w = c.shapes[0]
        assert np.array_equal(c.loc[0, :, 0, 0, 0, 1] * h - 0.5, c.pix_y) and np.array_equal(c.loc[0, :, 0, 0, 0, 0] * w - 0.5, c.pix_x)
        assert len(set(zip(c.pix_y, c.pix_x))) == 81
        for v in (-1.0, -1 + 2.0 ** -10, -0.5, 0.0, h - 1.0, h - 1 + 2.0 ** -10, h - 0.5, h - 2.0 ** -10, float(h)):
            assert (c.pix_y == v).sum() == 9
        # on the validity border nothing is sampled; one step inside, something is
        out = c.want.reshape(c.lq, c.m, c.d)
        dead = (c.pix_y == -1) | (c.pix_y == h) | (c.pix_x == -1) | (c.pix_x == w)
        assert (out[dead] == 0).all() and (out[~dead] != 0).all()
    q = util.msda_qp_case("qp_border")
    pix = q.loc * np.array([q.w, q.h], dtype=np.float64) - 0.5
    pairs = set(zip(pix[..., 1].reshape(-1), pix[..., 0].reshape(-1)))
    want = set((y, x) for y in util.msda_border_coords(q.h) for x in util.msda_border_coords(q.w))
    assert pairs == want


@pytest.mark.parametrize("name", _LOC_CASES)
def test_float32_oracle_stays_inside_the_forward_bound(name):
    c = _case(name)
    want, mag = _forward_ref(c, name)
    bound = (4 * c.l * c.p + 2) * util.MSDA_EPS["float32"] * mag
    if name not in util.MSDA_BWD_CASES:
        assert np.array_equal(bound, util.msda_forward_bound(c, "float32"))
    ok, ratio = util.msda_worst_ratio(util.msda_forward_float32_oracle(c), want, bound)
    print("msda-host %s float32-oracle error/bound %.3f" % (name, ratio))
    assert ok, ratio


@pytest.mark.parametrize("name", sorted(util.MSDA_QP_CASES))
def test_float32_qp_oracle_stays_inside_the_qp_bound(name):
    c = util.msda_qp_case(name)
    assert np.array_equal(c.qp.astype(np.float32).astype(np.float64), c.qp)
    if name != "qp_border":
        outside = (c.loc < 0) | (c.loc > 1)
        assert 0.1 < outside.any(-1).mean() < 0.9, "a good share of the samples leaves the map, a good share stays"
    ok, ratio = util.msda_worst_ratio(util.msda_qp_float32_oracle(c), c.want, util.msda_qp_bound(c))
    print("msda-host %s float32-oracle error/bound %.3f" % (name, ratio))
    assert ok, ratio

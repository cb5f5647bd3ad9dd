"""The fused point head (csrc/point_head.hip, through ops.point_head in both forms) and the TTA reduce (csrc/vote.hip: tta_argmax)
on the GPU against the float64 references of tests/point_head_cases.py.

Bars.  (a) Every logit inside its derived bound (gather_cases.worst_ratio: bound 0 means error 0, a NaN is outside), and the
RMS error of a case at most RMS_FACTOR (2) x that of the float32 restatement in the kernel's order -- the restatement is
measured against the reference, never against the kernel.  (b) The exact twins bit for bit float32(reference).  (c) Walks
under tests/util.py::conv_grid_cap: the trips of a wave are computed from the grid formula and asserted, the logits are bit for
bit those of the uncapped launch on [0, n_live) and exact zeros behind it.  (d) Nothing a kernel does not need is read: every
launch of this file takes its rows from a buffer whose floats [192, pitch), whose BEV third (gather form) and whose rows behind
B N are NaN, its map from channels [16, 80) of a 96-channel NaN buffer, its coordinates from a buffer with NaN rows behind N,
and writes into a slice of a NaN buffer whose neighbours have to stay NaN.  (e) Refusals through the C entries leave the
output alone.  (f) tta_argmax: probabilities inside (K + B + 2 + TTA_EXP_ULP) 2^-24, labels equal to the float64 argmax
wherever the float64 top-two gap is beyond twice that, exact ties to the lowest class with bitwise equal probabilities.

With SMOS_POINT_HEAD_RATIOS_FILE set, the per-case figures are appended to that file (profiles/point_head_error_ratios.txt is
made from it)."""
import functools
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import point_head_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PAD = 32                        # NaN floats on either side of the logits
TAIL = 33                       # NaN rows behind the last point row / coordinate row
RANDOM_NAMES = tuple(cases.BOUND_SPECS) + tuple(cases.WALK_SPECS)
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("SMOS_POINT_HEAD_RATIOS_FILE")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("\n".join(_LINES) + "\n")


def _note(line):
    print(line)
    _LINES.append(line)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _wprep(name):
    c = cases.case(name)
    flat, m3 = ops.point_head_prepare((_t(c.w1).view(96, 192, 1, 1), _t(c.b1)), (_t(c.w2).view(64, 96, 1, 1), _t(c.b2)),
                                      (_t(c.w3).view(c.m3, 64, 1, 1), _t(c.b3)))
    assert m3 == c.m3
    return flat


def _buffers(c, form, clean=False):
    """-> (rows [B, N, 192] view, gather tuple or None).  clean: dense buffers without a NaN anywhere (the comparison launch)."""
    b, n = c.b, c.n
    pitch = 192 if clean else c.pitch
    flat = torch.full((b * n + (0 if clean else TAIL), pitch), 0.0 if clean else NAN, device=DEV)
    rows = flat[:b * n].view(b, n, pitch)[:, :, :192]
    rows.copy_(_t(c.x))
    if form == "rows":
        return rows, None
    rows[:, :, 64:128] = 0.0 if clean else NAN
    if clean:
        grid = _t(c.grid).permute(0, 3, 1, 2)
        coord = _t(c.gcoord)
    else:
        wide = torch.full((b, c.hg, c.wg, 96), NAN, device=DEV)
        wide[..., 16:80] = _t(c.grid)
        grid = wide[..., 16:80].permute(0, 3, 1, 2)
        cw = torch.full((b, n + TAIL, cases.KG), NAN, device=DEV)
        cw[:, :n] = _t(c.gcoord)
        coord = cw[:, :n]
    return rows, (grid, coord, c.scale)


def launch(c, form, n_live=None, clean=False):
    """One ops.point_head launch -> logits [B, M3, N] float32 numpy.  The output is a slice of a NaN buffer; its neighbours
    have to stay NaN and every logit has to be written."""
    rows, gather = _buffers(c, form, clean)
    total = c.b * c.m3 * c.n
    wide = torch.full((total + 2 * PAD,), NAN, device=DEV)
    out = wide[PAD:PAD + total].view(c.b, c.m3, c.n)
    live = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=DEV)
    got = ops.point_head(rows, _wprep(c.name), c.m3, out=out, n_live=live, gather=gather)
    assert got.data_ptr() == out.data_ptr()
    host = wide.cpu().numpy()
    assert np.isnan(host[:PAD]).all() and np.isnan(host[PAD + total:]).all(), "written outside the logits"
    res = host[PAD:PAD + total].reshape(c.b, c.m3, c.n)
    assert np.isfinite(res).all(), "a logit left unwritten, or a NaN that nobody should have read"
    if form == "gather" and not clean:
        assert torch.isnan(rows[:, :, 64:128]).all()                       # and nobody wrote the BEV third
    return res


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- (a) bound and rms -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RANDOM_NAMES)
def test_bound_and_rms_against_float64(name):
    c = cases.case(name)
    for form in cases.FORMS:
        got = launch(c, form)
        ref, lim, rest = c.ref[form], c.lim[form], cases.restatement(name, form)
        ok, worst = cases.worst_ratio(got, ref, lim)
        _, rest_worst = cases.worst_ratio(rest, ref, lim)
        r = cases.ratio(cases.rms(got - ref), cases.rms(rest.astype(np.float64) - ref))
        groups = "  ".join("%s %.2f" % (g, cases.ratio(cases.rms(got[:, :, rows] - ref[:, :, rows]),
                                                         cases.rms(rest[:, :, rows].astype(np.float64) - ref[:, :, rows])))
                           for g, rows in c.rows.items())
        _note("bound  %-14s %-6s kernel error / bound %.5f  restatement %.5f  rms kernel / restatement %.3f  (per group: %s)" % (
            name, form, worst, rest_worst, r, groups))
        assert ok, (name, form, "worst error / bound", worst)
        assert r <= cases.RMS_FACTOR, (name, form, "RMS error against float64 over twice the float32 restatement's", r)
    if c.steered:
        # all_dead rows: one constant logit vector
        dead = launch(c, "rows")[:, :, c.rows["all_dead"]]
        assert (dead == dead[:1, :, :1]).all()


# ---- (b) exact twins -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.EXACT_NAMES)
def test_exact_twin_bit_for_bit(name):
    c = cases.case(name)
    for form in cases.FORMS:
        assert cases.exact_condition(c, form)
        got = launch(c, form)
        want = c.ref[form].astype(np.float32)
        wrong = int((_bits(got) != _bits(want)).sum())
        assert wrong == 0, (name, form, "%d of %d logits differ from float32(reference)" % (wrong, want.size))


# ---- (c) walks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.WALKS))
def test_walk_of_several_tiles_per_wave(name):
    c, cx = cases.case(name), cases.case(name + "/x")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    honoured = cases.launch_honours_cap()[0]
    base = {(form, nl): launch(c, form, nl) for form in cases.FORMS for nl in _n_lives(c)}
    for (form, nl), got in base.items():
        live = c.n if nl is None else min(nl, c.n)
        assert np.array_equal(_bits(got[:, :, :live]), _bits(base[form, None][:, :, :live])) and not got[:, :, live:].any(), (form, nl)
    for cap in cases.WALKS[name]:
        blocks = cases.head_blocks(c.b, c.n, cus, cap if honoured else 0)
        most, cross = cases.walk_facts(cases.walk_tiles(c.b, c.n, None, blocks))
        if (name, cap) in cases.WALK_FULL:
            assert most >= 3 and cross, (name, cap, "no wave takes three tiles across a sample boundary", blocks, most, cross)
        elif (name, cap) != ("walk_b3_n70", 2):         # 9 tiles: two blocks are the uncapped grid
            assert most >= 2 and cross, (name, cap, blocks, most, cross)
        with util.conv_grid_cap(cap):
            for form in cases.FORMS:
                for nl in _n_lives(c):
                    got = launch(c, form, nl)
                    live = c.n if nl is None else min(nl, c.n)
                    assert np.array_equal(_bits(got), _bits(base[form, nl])), (name, cap, form, nl, "differs from the uncapped launch")
                    assert not got[:, :, live:].any(), (name, cap, form, nl, "padding tail not zero")
                ok, worst = cases.worst_ratio(launch(c, form), c.ref[form], c.lim[form])
                assert ok, (name, cap, form, worst)
                gx = launch(cx, form)
                assert np.array_equal(_bits(gx), _bits(cx.ref[form].astype(np.float32))), (name, cap, form, "exact twin")
        trips = [cases.walk_facts(cases.walk_tiles(c.b, c.n, nl, blocks))[0] for nl in _n_lives(c)]
        _note("walk   %-14s cap %d: %d blocks, most tiles of a wave per n_live %s: %s" % (
            name, cap, blocks, list(_n_lives(c)), trips))
    again = launch(c, "gather")
    assert np.array_equal(_bits(again), _bits(base["gather", None]))       # the cap is lifted again


def _n_lives(c):
    """None, 0, 1, 45, 64, 290 (beyond N = 70: the kernel clamps it) and N."""
    return tuple(c.n if v == "N" else v for v in cases.WALK_N_LIVE)


# ---- (d) unread floats, out= ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n1_m1", "n33_m9", "n70_m20", "n300_m32"])
def test_nan_around_every_operand_reaches_no_logit(name):
    """The launch from NaN-surrounded buffers (pitch floats [192, pitch), the BEV third of the fold's rows, map channels outside
    the slice, the rows and coordinates behind the last point: a ragged last tile clamps its lanes) equals, bit for bit, the
    launch from dense buffers that hold no NaN."""
    c = cases.case(name)
    for form in cases.FORMS:
        for nl in (None, 1):
            assert np.array_equal(_bits(launch(c, form, nl)), _bits(launch(c, form, nl, clean=True))), (name, form, nl)


@pytest.mark.parametrize("form", cases.FORMS)
def test_out_is_fully_overwritten_and_nothing_else(form):
    c = cases.case("n70_m20")
    rows, gather = _buffers(c, form)
    want = launch(c, form)
    for nl in (None, 45, 0):
        live = None if nl is None else torch.tensor([nl], dtype=torch.int32, device=DEV)
        # a poisoned out
        out = torch.full((c.b, c.m3, c.n), NAN, device=DEV)
        ops.point_head(rows, _wprep(c.name), c.m3, out=out, n_live=live, gather=gather)
        k = c.n if nl is None else nl
        host = out.cpu().numpy()
        assert np.array_equal(_bits(host[:, :, :k]), _bits(want[:, :, :k])) and (host[:, :, k:] == 0).all(), nl
        # samples 1 .. B - 1 of a wider buffer: sample 0 and the tail stay
        wide = torch.full((c.b + 2, c.m3, c.n), -7.5, device=DEV)
        ops.point_head(rows, _wprep(c.name), c.m3, out=wide[1:1 + c.b], n_live=live, gather=gather)
        host = wide.cpu().numpy()
        assert (host[0] == -7.5).all() and (host[1 + c.b] == -7.5).all()
        assert np.array_equal(_bits(host[1:1 + c.b, :, :k]), _bits(want[:, :, :k])) and (host[1:1 + c.b, :, k:] == 0).all(), nl


# ---- (e) refusals ----------------------------------------------------------------------------------------------------------

def _refusal_args():
    """Real, fully sized buffers: rows of pitch 200 with a tail, a 5 x 7 x 64 map, coordinates at -1000 (no tap), an output
    sized for 33 rows."""
    c = cases.case("n33_m9")
    rows = torch.zeros((c.b * c.n + TAIL, 200), device=DEV)
    grid = torch.zeros((c.b, cases.HG, cases.WG, 64), device=DEV)
    coord = torch.full((c.b, c.n, cases.KG), -1000.0, device=DEV)
    out = torch.full((c.b * 33 * c.n,), NAN, device=DEV)
    return c, rows, grid, coord, out


REFUSALS = {          # name -> (entries, overrides)
    "k1_191": ("both", dict(K1=191)), "k1_200": ("both", dict(K1=200)),
    "m3_0": ("both", dict(M3=0)), "m3_33": ("both", dict(M3=33)),
    "pitch_190": ("both", dict(pitch=190)), "pitch_194": ("both", dict(pitch=194)),
    "rows_unaligned": ("both", dict(row_off=4)),
    "grid_pitch_60": ("gather", dict(gp=60)), "kg_1": ("gather", dict(Kg=1)),
    "grid_2gib": ("gather", dict(Hg=8192, Wg=8192)),                       # 2 x 8192 x 8192 x 64 floats
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_leave_the_output_alone(name):
    entries, over = REFUSALS[name]
    c, rows, grid, coord, out = _refusal_args()
    stream = ops._stream(rows)

    def args(**over):
        p = dict(K1=192, M3=c.m3, pitch=200, row_off=0, gp=64, Kg=cases.KG, Hg=cases.HG, Wg=cases.WG)
        p.update(over)
        head = (rows.data_ptr() + p["row_off"], p["pitch"], _wprep(c.name).data_ptr(), out.data_ptr(), c.b, c.n, p["K1"], 96, 64, p["M3"], None)
        tail = (grid.data_ptr(), p["gp"], p["Hg"], p["Wg"], coord.data_ptr(), p["Kg"], c.n * cases.KG, _lib.f32_array(c.scale), stream)
        return head, tail

    head, tail = args(**over)
    calls = [("smos_point_head_gather", head + tail)]
    if entries == "both":
        calls.append(("smos_point_head", head + (stream,)))
    for entry, a in calls:
        with pytest.raises(RuntimeError, match="point_head"):
            _lib.call(entry, *a)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), (name, entry, "a refused call wrote")
    # the same buffers are accepted as they are
    head, tail = args()
    _lib.call("smos_point_head_gather", *(head + tail))
    torch.cuda.synchronize()
    got = out[:c.b * c.m3 * c.n]
    assert torch.isfinite(got).all() and torch.isnan(out[c.b * c.m3 * c.n:]).all()


# ---- (f) tta_argmax --------------------------------------------------------------------------------------------------------

def _tta(c, want_prob=True):
    res = ops.tta_argmax(_t(c.pred), want_prob=want_prob)
    if want_prob:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy()


@pytest.mark.parametrize("name", sorted(cases.TTA_SPECS))
def test_tta_argmax_against_float64(name):
    c = cases.tta_case(name)
    labels, prob = _tta(c)
    assert labels.dtype == np.uint8 and prob.shape == (c.n, c.k)
    rest, _ = cases.tta_f32(c.pred)
    err = float(np.abs(prob.astype(np.float64) - c.prob).max()) if np.isfinite(prob).all() else float("inf")
    rest_err = float(np.abs(rest.astype(np.float64) - c.prob).max())
    left = cases.left_out(c)
    _note("tta    %-20s kernel error / bound %.4f  restatement %.4f  (bound %.0f u, %.2f %% of the points left to the gap rule)" % (
        name, err / c.lim, rest_err / c.lim, c.lim / cases.U, 100 * left))
    assert err <= c.lim, (name, err / cases.U)
    assert left <= cases.MAX_LEFT_OUT
    assert np.array_equal(labels[c.decided], c.labels[c.decided]), name
    assert np.array_equal(_tta(c, want_prob=False), labels)
    for p, cls in c.ties.items():
        assert len({prob[p, k].tobytes() for k in cls}) == 1 and labels[p] == cls[0], (name, p, cls, prob[p])
    if c.k == 1:
        assert not labels.any() and (prob == 1.0).all()


@pytest.mark.parametrize("name", sorted(k for k, v in cases.TTA_SPECS.items() if v["n"] == 1000))
def test_tta_argmax_grid_stride_trips(name):
    """N = 1000 under a cap of one block of 256 threads: four trips of the grid-stride loop, the bits of the uncapped launch."""
    c = cases.tta_case(name)
    blocks = min(-(-c.n // 256), 1 if cases.launch_honours_cap()[1] else 1 << 30)
    assert -(-c.n // (256 * blocks)) == 4, "no second trip of the grid-stride loop"
    labels, prob = _tta(c)
    with util.conv_grid_cap(1):
        l1, p1 = _tta(c)
        l0 = _tta(c, want_prob=False)
    assert np.array_equal(l1, labels) and np.array_equal(l0, labels) and np.array_equal(_bits(p1), _bits(prob))

"""The five channels-last convolution kernels (csrc/conv_igemm.hip, conv_rows.hip, conv_wino.hip, conv_wino1d.hip, conv_bf16.hip)
against the float64 reference of tests/conv_cases.py at small shapes: (a) a derived per-element bound and the RMS error against
the float32 restatement of the same algorithm, (b) exact inputs on which all five must return one answer bit for bit, (c) walks
of several items per block under the grid cap, (d) the padding= argument, (e) non-finite surroundings and one Inf pixel,
(f) the Cout limit and the refusals.  Operands are channel slices of wider channels-last buffers (x, residual and out at
different pitches) whose other channels hold NaN, and the output and the sum table start NaN-filled.

The one measured quantity is the factor 2 of the RMS comparison in (a): a margin for another summation order over the same
number of roundings.  Every other bar is derived in tests/conv_cases.py or is bitwise equality.
With SMOS_CONV_RATIOS_FILE set, the per-case figures are appended to that file (profiles/conv_error_ratios.txt is made from it)."""
import functools
import os

import numpy as np
import pytest
import torch

from streammos_amd import ops
from tests import conv_cases as cases
from tests.util import conv_grid_cap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
RMS_FACTOR = 2.0
X_SLICE, RES_SLICE, OUT_SLICE = (8, 4), (12, 8), (16, 4)          # (extra channels, channel offset) of the wide buffers
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("SMOS_CONV_RATIOS_FILE")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("\n".join(_LINES) + "\n")


def _note(line):
    print(line)
    _LINES.append(line)


def _wide(a, extra, off):
    """a [B, H, W, C] float64 numpy -> (buffer [B, H, W, C + extra] with NaN around the slice, the [B, C, H, W] view of the slice)"""
    b, h, w, c = a.shape
    buf = torch.full((b, h, w, c + extra), NAN, device=DEV)
    buf[..., off:off + c] = torch.tensor(np.asarray(a), dtype=torch.float32)
    return buf, buf[..., off:off + c].permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _weights(name, family, tile):
    c = cases.case(name)
    w = torch.tensor(c.wt, dtype=torch.float32, device=DEV)
    if family == "igemm":
        return ops.conv_prepare(w, tile)
    if family == "rows":
        return ops.conv_prepare(w, tile, order="rows")
    if family == "wino":
        return ops.conv_wino_prepare(w, tile)
    if family == "wino1d":
        return ops.conv_wino1d_prepare(w, tile)
    return ops.conv_bf16_prepare(w)


def _launch(family, c, tile, x, wp, bias, res, out, sums):
    if family == "igemm":
        return ops.conv_cl(x, wp, bias, c.act, c.cout, c.k, stride=c.stride, padding=None if cases.same_padding(c) else c.pad,
                           mt=tile, residual=res, out=out, chan_sums=sums)
    if family == "rows":
        return ops.conv_rows_cl(x, wp, bias, c.act, c.cout, c.k, mt=tile, residual=res, out=out, chan_sums=sums)
    if family == "wino":
        return ops.conv_wino_cl(x, wp, bias, c.act, c.cout, mb=tile, residual=res, out=out, chan_sums=sums)
    if family == "wino1d":
        assert res is None and sums is None
        return ops.conv_wino1d_cl(x, wp, bias, c.act, c.cout, c.k, mb=tile, out=out)
    return ops.conv_bf16_cl(x, wp, bias, c.act, c.cout, c.k, stride=c.stride, padding=None if cases.same_padding(c) else c.pad,
                            residual=res, out=out, chan_sums=sums)


def _sum_chunks(family, c):
    return ops.conv_wino_sum_chunks(c.ho, c.wo) if family == "wino" else ops.conv_sum_chunks(c.ho, c.wo)


def _run(family, c, tile, sums=False, x=None, sample=None):
    """One launch on NaN-surrounded slices -> (out [B, Ho, Wo, Cout] float32 numpy, sum table or None).  Asserts that the
    neighbour channels of the output buffer are still NaN and that the sample count is the input's."""
    xs = c.x if x is None else x
    rs = c.res
    if sample is not None:
        xs, rs = xs[sample:sample + 1], None if rs is None else rs[sample:sample + 1]
    b = xs.shape[0]
    _, xv = _wide(xs, *X_SLICE)
    rv = None if rs is None else _wide(rs, *RES_SLICE)[1]
    obuf, ov = _wide(np.full((b, c.ho, c.wo, c.cout), NAN), *OUT_SLICE)
    tab = torch.full((b, _sum_chunks(family, c), c.cout), NAN, device=DEV) if sums else None
    bias = None if c.bias is None else torch.tensor(c.bias, dtype=torch.float32, device=DEV)
    y = _launch(family, c, tile, xv, _weights(c.name, family, tile), bias, rv, ov, tab)
    assert y.data_ptr() == ov.data_ptr() and tuple(y.shape) == (b, c.cout, c.ho, c.wo)
    off = OUT_SLICE[1]
    assert bool(torch.isnan(obuf[..., :off]).all()) and bool(torch.isnan(obuf[..., off + c.cout:]).all()), "neighbour channels written"
    return obuf[..., off:off + c.cout].cpu().numpy(), None if tab is None else tab.cpu().numpy()


def _want_sums(family, name):
    ref, lim = cases.reference(name, family)
    rows = cases.sum_rows(family)
    return cases.sum_table(ref, rows), cases.sum_bound(ref, lim, rows)


def _check_bound(tag, family, name, got, tab=None):
    """every element inside its bound (a NaN left in the output is outside every bound); -> worst error / bound"""
    ref, lim = cases.reference(name, family)
    assert got.shape == ref.shape and got.dtype == np.float32
    ok, ratio = cases.worst_ratio(got, ref, lim)
    assert ok, (tag, "error over the bound", ratio)
    if tab is not None:
        want, slim = _want_sums(family, name)
        sok, sratio = cases.worst_ratio(tab, want, slim)
        assert tab.shape == want.shape and sok, (tag, "channel sums over the bound", sratio)
    return ratio


def _check_exact(tag, family, name, got, tab=None):
    c = cases.case(name)
    ref, _ = cases.reference(name, family)
    assert np.array_equal(got, ref.astype(np.float32)), (tag, "not the float64 result bit for bit", float(np.abs(got - ref).max()))
    if tab is not None and cases.exact_condition(c, family, sums=True):
        assert np.array_equal(tab, _want_sums(family, name)[0].astype(np.float32)), (tag, "channel sums")


def _pairs(specs):
    return [(f, n) for n in sorted(specs) for f in cases.FAMILIES if cases.family_takes(f, cases.case(n))]


# ---- (a) per-element bound, RMS against the float32 restatement --------------------------------------------------------

@pytest.mark.parametrize("family,name", _pairs(cases.BOUND_SPECS))
def test_bound_and_rms_against_float64(family, name):
    c = cases.case(name)
    ref, _ = cases.reference(name, family)
    rest = cases.restatement(name, "igemm" if family == "rows" else family)
    rest_rms = cases.rms(rest - ref)
    assert rest_rms > 0
    with_sums = c.sums and c.res is None and family != "wino1d"
    for tile in cases.tiles(family, c):
        tag = "%-6s tile %d %-16s" % (family, tile, name)
        got, tab = _run(family, c, tile, sums=with_sums)
        ratio = _check_bound(tag, family, name, got, tab)
        rel = cases.rms(got - ref) / rest_rms
        _note("%s max error / bound %.4f   RMS error / RMS of the float32 restatement %.3f   (%d elements%s)" % (
            tag, ratio, rel, got.size, ", sums" if with_sums else ""))
        assert rel <= RMS_FACTOR, (tag, "RMS error against float64 over twice the float32 restatement's", rel)


# ---- (b) exact inputs: five kernels, one answer -------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.EXACT_SPECS))
def test_exact_inputs_five_kernels_one_answer(name):
    c = cases.case(name)
    ran = []
    for family in cases.FAMILIES:
        if not cases.family_takes(family, c):
            continue
        assert cases.exact_condition(c, family)
        with_sums = c.sums and c.res is None and family != "wino1d"
        for i, tile in enumerate(cases.tiles(family, c)):
            tag = "%s tile %d %s" % (family, tile, name)
            got, tab = _run(family, c, tile, sums=with_sums)
            _check_exact(tag, family, name, got, tab)
            ran.append(tag)
            if i == 0:
                again, tab2 = _run(family, c, tile, sums=with_sums)
                assert np.array_equal(again, got) and (tab is None or np.array_equal(tab2, tab)), (tag, "second call differs")
                s = c.b - 1
                alone, tab1 = _run(family, c, tile, sums=with_sums, sample=s)
                assert np.array_equal(alone[0], got[s]) and (tab is None or np.array_equal(tab1[0], tab[s])), (tag, "sample alone differs")
    assert len({t.split()[0] for t in ran}) >= 2, ran
    print("%s: %d launches equal float32(float64 reference): %s" % (name, len(ran), sorted({t.split()[0] for t in ran})))


# ---- (c) walks under the grid cap ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.WALK_SPECS))
def test_walk_of_several_items_per_block(name):
    family, tile, with_sums, caps, _ = cases.WALK_SPECS[name]
    c, cx = cases.case(name), cases.case(name + "/x")
    n_items = cases.items(family, c, tile, with_sums)
    base, base_tab = _run(family, cx, tile, sums=with_sums)
    _check_exact(name + " uncapped", family, cx.name, base, base_tab)
    for cap in caps:
        assert n_items > cap, (name, n_items, cap)                    # a block really walks more than one item
        with conv_grid_cap(cap):
            got, tab = _run(family, cx, tile, sums=with_sums)
            rnd, rnd_tab = _run(family, c, tile, sums=with_sums)
        tag = "%s cap %d (%s items per block)" % (name, cap, "/".join(str(s) for s in sorted(set(cases.block_shares(n_items, cap)), reverse=True)))
        _check_exact(tag, family, cx.name, got, tab)
        assert np.array_equal(got, base) and (tab is None or np.array_equal(tab, base_tab)), (tag, "differs from the uncapped launch")
        ratio = _check_bound(tag, family, name, rnd, rnd_tab)
        _note("walk   %-62s max error / bound %.4f" % (tag, ratio))
    # the cap is lifted again: an uncapped launch gives the same bits
    again, _ = _run(family, cx, tile, sums=with_sums)
    assert np.array_equal(again, base)


# ---- (d) padding= ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.PAD_SPECS))
def test_padding_argument(name):
    c, cx = cases.case(name), cases.case(name + "/x")
    for family in ("igemm", "bf16"):
        assert cases.family_takes(family, c)
        for tile in cases.tiles(family, c):
            tag = "%-6s tile %d %-16s" % (family, tile, name)
            got, _ = _run(family, c, tile)
            ratio = _check_bound(tag, family, name, got)
            if c.all_pad.any() and c.res is None:
                # nothing but the bias arrives where the whole window is padding: act(bias), exactly
                want = cases.act_apply(np.zeros(c.cout) if c.bias is None else c.bias, c.act).astype(np.float32)
                assert np.array_equal(got[:, c.all_pad], np.broadcast_to(want, got[:, c.all_pad].shape)), (tag, "padded window")
            gx, _ = _run(family, cx, tile)
            _check_exact(tag, family, cx.name, gx)
            _note("pad    %s padding %s stride %d  max error / bound %.4f  (%d outputs with a window of padding only)" % (
                tag, c.pad, c.stride, ratio, int(c.all_pad.sum())))


def test_bf16_refuses_the_shape_without_a_block_shape():
    """Cout 32, 3 x 3, stride 2 (tests/conv_cases.py::bf16_cfg: the one block shape stages too large a region): refused, the
    output untouched -- and taken by conv_cl."""
    x = torch.randn(2, 5, 35, 32, device=DEV).permute(0, 3, 1, 2)
    w = torch.randn(32, 32, 3, 3, device=DEV) * 0.1
    assert not ops.conv_bf16_ok(x, 32, (3, 3), 2) and cases.bf16_cfg(2, 2, 17, 32, (3, 3), 2, False) is None
    obuf = torch.full((2, 2, 17, 40), 7.25, device=DEV)
    out = obuf[..., 4:36].permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError):
        ops.conv_bf16_cl(x, ops.conv_bf16_prepare(w), None, 0, 32, (3, 3), stride=2, padding=(0, 0), out=out)
    torch.cuda.synchronize()
    assert bool((obuf == 7.25).all())
    y = ops.conv_cl(x, ops.conv_prepare(w, 1), None, 0, 32, (3, 3), stride=2, padding=(0, 0), out=out)
    want = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), None, 2, 0)
    assert tuple(y.shape) == tuple(want.shape) and bool(torch.isfinite(y).all())


# ---- (e) non-finite surroundings ---------------------------------------------------------------------------------------

_POISON = [(f, n) for n in sorted(cases.POISON_SPECS) for f in cases.FAMILIES if cases.family_takes(f, cases.case(n))]


@pytest.mark.parametrize("family,name", _POISON)
def test_nan_in_every_neighbour_channel(family, name):
    """_run puts NaN into every channel outside the x and residual slices and around the output slice, and asserts that the
    output's neighbours are still NaN; here: a padded tap is dropped, not multiplied -- every output is finite and inside its bound."""
    c = cases.case(name)
    for tile in cases.tiles(family, c):
        got, _ = _run(family, c, tile)
        assert np.isfinite(got).all()
        _check_bound("%s tile %d %s" % (family, tile, name), family, name, got)


@pytest.mark.parametrize("where", ("corner", "row_end", "last_row"))
@pytest.mark.parametrize("family,name", _POISON)
def test_one_inf_pixel_shows_where_it_may(family, name, where):
    """A corner, the last pixel of a row (the next row's left halo must not see it) and the last row of sample 0 (the top halo
    of sample 1 must not see it).  Direct kernels: the non-finite outputs are exactly the reference's.  Winograd kernels: they
    contain the reference's and stay inside the tiles whose input window holds the pixel (the input transform spreads Inf - Inf
    over its tile).  No other output, and none of sample 1, is non-finite; the rest stays inside its bound."""
    c = cases.case(name)
    y, x = {"corner": (0, 0), "row_end": (2, c.w - 1), "last_row": (c.h - 1, 5)}[where]
    xin = np.array(c.x)
    xin[0, y, x, :] = np.inf
    want = ~np.isfinite(cases.conv_ref(xin, c.wt, c.bias, c.res, c.act, c.stride, c.pad))
    reach = cases.reach(c, y, x)
    assert np.array_equal(want[0], np.broadcast_to(reach[:, :, None], want[0].shape)) and not want[1:].any()
    ref, lim = cases.reference(name, family)
    for tile in cases.tiles(family, c):
        got, _ = _run(family, c, tile, x=xin)
        bad = ~np.isfinite(got)
        tag = (family, tile, name, where)
        assert not bad[1:].any(), (tag, "another sample")
        if family in ("wino", "wino1d"):
            allowed = cases.tile_reach(c, family, y, x)
            assert (bad[0] >= want[0]).all(), (tag, "a reached output is finite")
            assert not bad[0][~allowed].any(), (tag, "outside the tiles that hold the pixel")
        else:
            allowed = reach
            assert np.array_equal(bad, want), (tag, "not the reference's reach")
        clean = np.ones(got.shape, dtype=bool)
        clean[0][allowed] = False
        assert (np.abs(got.astype(np.float64) - ref)[clean] <= lim[clean]).all(), (tag, "an output the pixel does not reach changed")


# ---- (f) limits and refusals -------------------------------------------------------------------------------------------

def test_cout_2048():
    """bias_r[8] with tid + 256 k ends at exactly 2048 channels: every bias entry is its own number."""
    c = cases.case("cout2048")
    assert c.cout == 2048 and len(set(c.bias.tolist())) == 2048
    for family in ("igemm", "bf16"):
        for tile in cases.tiles(family, c):
            got, _ = _run(family, c, tile)
            ratio = _check_bound("%s tile %d cout2048" % (family, tile), family, "cout2048", got)
            gx, _ = _run(family, cases.case("cout2048_x"), tile)
            _check_exact("%s tile %d cout2048_x" % (family, tile), family, "cout2048_x", gx)
            _note("limit  %-6s tile %d Cout 2048                    max error / bound %.4f" % (family, tile, ratio))
    assert 4 in cases.tiles("igemm", c)


def _sentinel_out(b, cout, ho, wo):
    buf = torch.full((b, max(ho, 4), wo, cout + 8), 7.25, device=DEV)
    return buf, buf[:, :ho, :, 4:4 + cout].permute(0, 3, 1, 2)


def _refusals():
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    cl = lambda b, c, h, w: rnd(b, h, w, c).permute(0, 3, 1, 2)
    zeros = lambda n: torch.zeros(n, device=DEV)
    x32, x48, x8 = cl(1, 32, 6, 34), cl(1, 48, 6, 34), cl(1, 8, 6, 34)
    w128 = rnd(128, 32, 3, 3)
    r = []
    r.append(("conv_cl residual with mt 4", (1, 128, 6, 34),
              lambda o: ops.conv_cl(x32, ops.conv_prepare(w128, 4), None, 0, 128, (3, 3), mt=4, residual=cl(1, 128, 6, 34), out=o)))
    for fam, fn in (("conv_cl", lambda o, t, s: ops.conv_cl(x32, ops.conv_prepare(w128, 2), None, 0, 128, (3, 3), mt=2, residual=s, out=o, chan_sums=t)),
                    ("conv_rows_cl", lambda o, t, s: ops.conv_rows_cl(x32, ops.conv_prepare(w128, 2, order="rows"), None, 0, 128, (3, 3), mt=2, residual=s, out=o, chan_sums=t)),
                    ("conv_wino_cl", lambda o, t, s: ops.conv_wino_cl(x32, ops.conv_wino_prepare(w128, 2), None, 0, 128, residual=s, out=o, chan_sums=t)),
                    ("conv_bf16_cl", lambda o, t, s: ops.conv_bf16_cl(x32, ops.conv_bf16_prepare(w128), None, 0, 128, (3, 3), residual=s, out=o, chan_sums=t))):
        chunks = ops.conv_wino_sum_chunks(6, 34) if fam == "conv_wino_cl" else ops.conv_sum_chunks(6, 34)
        r.append((fam + " chan_sums with a residual", (1, 128, 6, 34),
                  lambda o, fn=fn, chunks=chunks: fn(o, torch.full((1, chunks, 128), 7.25, device=DEV), cl(1, 128, 6, 34))))
    r.append(("conv_cl Cin 48", (1, 32, 6, 34), lambda o: ops.conv_cl(x48, zeros(32 * 48 * 9), None, 0, 32, (3, 3), out=o)))
    r.append(("conv_rows_cl Cin 48", (1, 32, 6, 34), lambda o: ops.conv_rows_cl(x48, zeros(32 * 48 * 9), None, 0, 32, (3, 3), out=o)))
    r.append(("conv_bf16_cl Cin 48", (1, 32, 6, 34),
              lambda o: ops.conv_bf16_cl(x48, zeros(32 * 48 * 9).to(torch.bfloat16), None, 0, 32, (3, 3), out=o)))
    r.append(("conv_wino_cl Cin 8", (1, 32, 6, 34), lambda o: ops.conv_wino_cl(x8, zeros(16 * 32 * 8), None, 0, 32, out=o)))
    r.append(("conv_wino1d_cl Cin 8", (1, 32, 6, 34), lambda o: ops.conv_wino1d_cl(x8, zeros(4 * 7 * 32 * 8), None, 0, 32, (7, 3), out=o)))
    r.append(("conv_wino1d_cl 5x5", (1, 32, 6, 34), lambda o: ops.conv_wino1d_cl(x32, zeros(4 * 5 * 32 * 32), None, 0, 32, (5, 5), out=o)))
    r.append(("conv_wino1d_cl 3x3", (1, 32, 6, 34), lambda o: ops.conv_wino1d_cl(x32, zeros(4 * 3 * 32 * 32), None, 0, 32, (3, 3), out=o)))
    # empty output: a 7 x 3 window on 6 rows without padding; and at stride 2 a window one row taller than the padded image,
    # where (H + 2 pad - KH) / 2 rounds to 0 in C and to -1 in Python -- no output row exists
    for fam, call in (("conv_cl", lambda o, k, s, p, wz: ops.conv_cl(x32, wz, None, 0, 32, k, stride=s, padding=p, out=o)),
                      ("conv_bf16_cl", lambda o, k, s, p, wz: ops.conv_bf16_cl(x32, wz.to(torch.bfloat16), None, 0, 32, k, stride=s, padding=p, out=o))):
        r.append((fam + " empty output 7x3 on 6 rows", (1, 32, 0, 32), lambda o, call=call: call(o, (7, 3), 1, (0, 0), zeros(32 * 32 * 21))))
        r.append((fam + " empty output 7x1 stride 2 on 6 rows", (1, 32, 0, 17), lambda o, call=call: call(o, (7, 1), 2, (0, 0), zeros(32 * 32 * 7))))
    return r


@pytest.mark.parametrize("index", range(16))
def test_refusals_raise_and_leave_the_output_untouched(index):
    """Every refusal a caller reaches through ops: RuntimeError, and a sentinel-filled output buffer (for an empty output: the
    buffer the empty view lies in) keeps every sentinel."""
    table = _refusals()
    assert len(table) == 16
    what, shape, call = table[index]
    buf, out = _sentinel_out(*shape)
    assert tuple(out.shape) == shape
    with pytest.raises(RuntimeError):
        call(out)
    torch.cuda.synchronize()
    assert bool((buf == 7.25).all()), what
    print("refused: " + what)

"""gather_scatter_cl / gather_scatter_cl4 (csrc/cl_kernels.hip) and the forward kernels of csrc/bilinear_gather.hip on the GPU
against the float64 reference of tests/gather_cases.py, through ops.gather_scatter_cl and ops.bilinear_gather.

Bars.  A gathered value: |got - S| <= 12 * 2^-24 * A, exactly 0 where A = 0 (derivation in tests/gather_cases.py).  The scatter
target: (a) bit for bit the numpy max-scatter (from 0) of the point rows the same launch wrote, and (b) inside max_p bound_p of
max(0, max_p S_p) over the members of the cell.  Every buffer a kernel writes lies inside a wider one filled with NaN, which has
to stay.  Every check prints its worst error / bound (pytest -s); the figures of the MI355X run are kept in
profiles/gather_error_ratios.txt.

Kernel forms: "vec" = the 16-byte-lane kernels gather_scatter_cl4 (rows and target 16-byte aligned: what the engine's maps
get), "lane" = the one-lane-per-channel kernels gather_scatter_cl, selected by a row pitch of C + 1 floats.
"""
import os

import numpy as np
import pytest
import torch

from streammos_amd import ops
from tests import gather_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = ("vec", "lane")
MODES = ("rows", "target", "both")            # gather only, scatter only, both
LAYOUTS = ("dense", "slices", "strided", "slices+strided")
HO, WO, HG, WG = cases.HO, cases.WO, cases.HG, cases.WG

RATIOS = {}
RATIO_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gather_error_ratios.txt")
RATIO_HEADER = """Grid -> point gather and max scatter (csrc/cl_kernels.hip: gather_scatter_cl / _cl4; csrc/bilinear_gather.hip: bil_points /
bil_rows) against the float64 reference: worst error / bound per check.  Written by tests/test_gpu_gather_scatter.py when the
whole file has run.

Each line is the largest |kernel - reference| / bound over EVERY element of every launch of one check (all point counts N of
tests/gather_cases.py::NS), bound = 12 * 2^-24 * A for a gathered value and the largest bound among a cell's members for a
scatter target (tests/gather_cases.py: derived, not tuned; the value has to be exactly 0 where the bound is 0).  "vec": the
16-byte-lane kernels, "lane": one lane per channel; rows / target / both: gather only, scatter only, both in one launch.
The kernels are deterministic (the scatter is an integer maximum): the figures do not move from run to run.
"""


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _note(label, ratio):
    RATIOS[label] = max(RATIOS.get(label, 0.0), ratio)


def _check(label, got, want, lim):
    ok, ratio = cases.worst_ratio(got, want, lim)
    _note(label, ratio)
    assert ok, "%s: worst error / bound = %g" % (label, ratio)
    return ratio


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    """profiles/gather_error_ratios.txt from this run, once every test of the file has run (not for a -k selection)."""
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 100 or len(ran) < 60:
        return
    for label, ratio in sorted(RATIOS.items()):
        print("gather-ratio %-60s %.4f" % (label, ratio))
    worst = max(RATIOS.items(), key=lambda r: r[1])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  %d checks, the largest ratio %.4f (%s).\n\n" % (
                torch.cuda.get_device_name(0), len(RATIOS), worst[1], worst[0]))
            f.writelines("%-64s %.4f\n" % r for r in sorted(RATIOS.items()))
    except OSError:
        pass                                   # a read-only checkout: the figures were printed


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def launch(case, form, mode, layout="dense", n_live=None):
    """One ops.gather_scatter_cl launch -> (rows [B, N, C] or None, target [B, HO * WO, C] or None) as float32 numpy.  The rows
    lie in a [B, N + 2, C + pad] buffer and the target in channels [off, off + C) of a [B + 1, HO, WO, off + C + pad] buffer,
    both NaN outside; that NaN has to survive.  pad = 4 keeps every row 16-byte aligned (the 16-byte-lane kernels), pad = 1
    does not (one lane per channel)."""
    b, n, c = case.b, case.n, case.c
    pad = 4 if form == "vec" else 1
    off = 8 if "slices" in layout else 0
    grid = _t(case.grid)
    if "slices" in layout:
        wide = torch.full((b, HG, WG, c + 32), float("nan"), device=DEV)
        wide[..., 16:16 + c] = grid
        grid = wide[..., 16:16 + c]
    grid = grid.permute(0, 3, 1, 2)
    gcoord, scoord = _t(case.gcoord), _t(case.scoord)
    if "strided" in layout:                                   # slices of the reference's [B, T, N, 3, 1] / [B, T, N, 2, 1] tensors
        g5 = torch.full((b, 3, n, cases.KG, 1), 7.0, device=DEV)
        s5 = torch.full((b, 3, n, cases.KS, 1), 7.0, device=DEV)
        g5[:, 0, :, :, 0], s5[:, 0, :, :, 0] = gcoord, scoord
        gcoord, scoord = g5[:, 0, :, :, 0], s5[:, 0, :, :, 0]
        assert gcoord.stride() == (3 * n * cases.KG, cases.KG, 1) and scoord.stride() == (3 * n * cases.KS, cases.KS, 1)
    rows_w = tgt_w = rows = tgt = None
    if mode != "target":
        rows_w = torch.full((b, n + 2, c + pad), float("nan"), device=DEV)
        rows = rows_w[:, :n, :c]
    if mode != "rows":
        tgt_w = torch.full((b + 1, HO, WO, off + c + pad), float("nan"), device=DEV)
        tgt_w[:b, :, :, off:off + c] = 0.0
        tgt = tgt_w[:b, :, :, off:off + c].permute(0, 3, 1, 2)
    live = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=DEV)
    ops.gather_scatter_cl(grid, gcoord, case.scale, scoord if tgt is not None else None, case.scale if tgt is not None else None,
                          out=tgt, pts_out=rows, n_live=live)
    out_rows = out_tgt = None
    if rows_w is not None:
        host = rows_w.cpu().numpy()
        assert np.isnan(host[:, n:]).all() and np.isnan(host[:, :, c:]).all(), "written beyond row N or beyond C channels"
        out_rows = host[:, :n, :c]
    if tgt_w is not None:
        host = tgt_w.cpu().numpy()
        assert np.isnan(host[b:]).all() and np.isnan(host[..., :off]).all() and np.isnan(host[..., off + c:]).all(), "written outside the target slice"
        out_tgt = host[:b, :, :, off:off + c].reshape(b, HO * WO, c)
        assert not np.isnan(out_tgt).any()
    return out_rows, out_tgt


def check_rows(label, rows, case, upto=None):
    assert not np.isnan(rows[:, :upto]).any(), label
    return _check(label, rows[:, :upto], case.S[:, :upto], case.lim[:, :upto])


def check_target(label, tgt, rows, case):
    """(a) the numpy max-scatter from 0 of the rows of the same launch, bit for bit (rows = None: a scatter-only launch, no rows);
    (b) the float64 reference."""
    if rows is not None:
        assert np.array_equal(_bits(tgt), _bits(cases.scatter_max0(rows, case.cell))), label + ": target != max(0, own rows)"
    assert (tgt >= 0).all()
    return _check(label, tgt, case.T, case.T_lim)


def all_modes(case, tag, forms=FORMS, layout="dense"):
    """Every form and mode of one case; -> {form: (rows, target)} of the combined launch."""
    res = {}
    for form in forms:
        rows_only, _ = launch(case, form, "rows", layout)
        _, tgt_only = launch(case, form, "target", layout)
        rows, tgt = launch(case, form, "both", layout)
        check_rows("%s %s rows" % (tag, form), rows_only, case)
        check_rows("%s %s both:rows" % (tag, form), rows, case)
        check_target("%s %s both:target" % (tag, form), tgt, rows, case)
        check_target("%s %s target" % (tag, form), tgt_only, None, case)
        assert np.array_equal(_bits(rows_only), _bits(rows)), "%s %s: gather-only rows != combined rows" % (tag, form)
        assert np.array_equal(_bits(tgt_only), _bits(tgt)), "%s %s: scatter-only target != combined target" % (tag, form)
        res[form] = (rows, tgt)
    if len(res) == 2:
        assert np.array_equal(_bits(res["vec"][0]), _bits(res["lane"][0])), tag + ": rows differ between the kernel forms"
        assert np.array_equal(_bits(res["vec"][1]), _bits(res["lane"][1])), tag + ": targets differ between the kernel forms"
    return res


@pytest.mark.parametrize("scale", list(cases.SCALES))
@pytest.mark.parametrize("c", cases.GS_CHANNELS)
@pytest.mark.parametrize("struct", cases.STRUCTURES)
def test_gather_scatter_against_float64_reference(struct, c, scale):
    for n in cases.NS:
        case = cases.gs_case(struct, c, n, scale)
        res = all_modes(case, "%s/c%d/%s" % (struct, c, scale))
        if struct == "negative_grid":                           # the contract: max(0, .) into a zero-filled target
            rows, tgt = res["vec"]
            assert (rows < 0).all() and not tgt.any() and not _bits(tgt).any()


@pytest.mark.parametrize("c", cases.GS_CHANNELS)
@pytest.mark.parametrize("layout", LAYOUTS[1:])
def test_channel_slices_and_strided_coordinates_give_the_same_bits(layout, c):
    """Grid and target as channel slices of wider channels-last buffers (NaN around them), the coordinates as strided views of
    [B, T, N, 3, 1] / [B, T, N, 2, 1] tensors: what the dense copies give."""
    for struct, n in (("lone0", 130), ("runs", 65), ("notap_runs", 130), ("holes", 33)):
        case = cases.gs_case(struct, c, n, "nondyadic")
        for form in FORMS:
            want_rows, want_tgt = launch(case, form, "both")
            rows, tgt = launch(case, form, "both", layout)
            assert np.array_equal(_bits(rows), _bits(want_rows)) and np.array_equal(_bits(tgt), _bits(want_tgt))
            check_rows("layout %s/c%d %s rows" % (layout, c, form), rows, case)
            check_target("layout %s/c%d %s target" % (layout, c, form), tgt, rows, case)
            rows_only, _ = launch(case, form, "rows", layout)
            _, tgt_only = launch(case, form, "target", layout)
            assert np.array_equal(_bits(rows_only), _bits(want_rows)) and np.array_equal(_bits(tgt_only), _bits(want_tgt))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", cases.GS_CHANNELS)
def test_n_live(c, form):
    """Rows below the count equal the plain launch bit for bit; a row above it is either untouched (the NaN it arrived with) or
    inside the bound -- the one-lane kernel ignores the count; the target does not depend on it."""
    for struct in ("notap_runs", "cell_notap", "lone0"):
        case = cases.gs_case(struct, c, 130, "dyadic")
        n = case.n
        want_rows, want_tgt = launch(case, form, "both")
        for n_live in (0, 1, 63, 64, 65, n, n + 7):
            for mode in ("rows", "both"):
                label = "n_live %s/c%d %s %s" % (struct, c, form, mode)
                b, pad = case.b, (4 if form == "vec" else 1)
                rows_w = torch.full((b, n + 2, c + pad), float("nan"), device=DEV)
                tgt_w = torch.full((b + 1, HO, WO, c + pad), float("nan"), device=DEV)
                tgt_w[:b, :, :, :c] = 0.0
                tgt = tgt_w[:b, :, :, :c].permute(0, 3, 1, 2) if mode == "both" else None
                ops.gather_scatter_cl(_t(case.grid).permute(0, 3, 1, 2), _t(case.gcoord), case.scale,
                                      _t(case.scoord) if tgt is not None else None, case.scale if tgt is not None else None, out=tgt,
                                      pts_out=rows_w[:, :n, :c], n_live=torch.tensor([n_live], dtype=torch.int32, device=DEV))
                host = rows_w.cpu().numpy()
                assert np.isnan(host[:, n:]).all() and np.isnan(host[:, :, c:]).all()
                rows = host[:, :n, :c]
                lo = min(n_live, n)
                assert np.array_equal(_bits(rows[:, :lo]), _bits(want_rows[:, :lo])), (label, n_live)
                untouched = np.isnan(rows).all(2)                                   # whole rows that kept their NaN
                assert not untouched[:, :lo].any() and not np.isnan(rows[~untouched]).any(), (label, n_live)
                filled = np.where(untouched[..., None], case.S, rows)
                _check(label, filled, case.S, case.lim)
                if form == "lane":
                    assert not untouched.any()
                if tgt is not None:
                    host = tgt_w.cpu().numpy()
                    assert np.isnan(host[b:]).all() and np.isnan(host[..., c:]).all()
                    assert np.array_equal(_bits(host[:b, :, :, :c].reshape(b, HO * WO, c)), _bits(want_tgt)), (label, n_live)


@pytest.mark.parametrize("c", cases.GS_CHANNELS)
def test_run_loop_under_the_grid_cap(c):
    """One block (and two) walks all 21 runs of 64 points / 39 runs of 32 points of tests/gather_cases.py::loop_case: the second
    and later trips of the run loop, the LDS tile of gather_scatter_cl4 refilled behind its read-out, the early `continue`s
    followed by more work, and the run -> (sample, first point) arithmetic across both sample boundaries.  The rows are the same
    expression and the scatter is an integer maximum: the capped launches equal the uncapped one bit for bit."""
    case = cases.loop_case(c)
    free = all_modes(case, "loop/c%d cap0" % c)
    for cap in (1, 2):
        with util.conv_grid_cap(cap):
            capped = all_modes(case, "loop/c%d cap%d" % (c, cap))
        for form in FORMS:
            assert np.array_equal(_bits(capped[form][0]), _bits(free[form][0])), (cap, form)
            assert np.array_equal(_bits(capped[form][1]), _bits(free[form][1])), (cap, form)
    rows, tgt = free["vec"]
    assert tgt.any() and (rows[~cases.has_tap(case)] == 0).all()


def _bil_grid(case, channels_last):
    g = _t(case.grid)                                            # [B, H, W, C]
    return g.permute(0, 3, 1, 2) if channels_last else g.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("scale", list(cases.SCALES))
@pytest.mark.parametrize("c", cases.BIL_CHANNELS)
def test_bilinear_gather_forward_against_float64_reference(c, scale):
    """bil_points (an NCHW grid or a channel-major result; C >= 16 in channel chunks over blockIdx.y, the last one ragged) and
    bil_rows<8|16|32|64> (channels-last grid, point-major result, C >= 8)."""
    for n in cases.NS:
        case = cases.bil_case(c, n, scale)
        coord = _t(case.gcoord)
        want, lim = case.S.transpose(0, 2, 1), case.lim.transpose(0, 2, 1)
        for channels_last in (False, True):
            grid = _bil_grid(case, channels_last)
            for point_major in (False, True):
                got = ops.bilinear_gather(grid, coord, case.scale, point_major=point_major)
                assert got.shape == (case.b, c, n) and (n == 1 or (got.stride(1) == 1) == point_major)
                _check("bilinear c%d/%s grid=%s out=%s" % (c, scale, "nhwc" if channels_last else "nchw",
                                                         "point_major" if point_major else "channel_major"),
                       got.cpu().numpy(), want, lim)
        if c <= 128:
            # out= into channels [64, 64 + C) of a wider [B, N, 192] row buffer: the neighbouring columns keep their NaN
            for channels_last in (False, True):
                buf = torch.full((case.b, n, 192), float("nan"), device=DEV)
                res = ops.bilinear_gather(_bil_grid(case, channels_last), coord, case.scale, out=buf[:, :, 64:64 + c].permute(0, 2, 1))
                assert res.data_ptr() == buf[:, :, 64:].data_ptr()
                host = buf.cpu().numpy()
                assert np.isnan(host[:, :, :64]).all() and np.isnan(host[:, :, 64 + c:]).all()
                _check("bilinear c%d/%s grid=%s out=row-buffer slice" % (c, scale, "nhwc" if channels_last else "nchw"),
                       host[:, :, 64:64 + c], case.S, case.lim)

"""The fused training transfer (csrc/gather_scatter_train.hip) on the GPU, through the three C entries, the wrappers of
ops.py and the autograd op ops.gather_scatter_train.

Forward and point gradient: bit for bit what ops.bilinear_gather followed by deep_point.VoxelMaxPool gives.  Backward, fused
launch: per grid element |got - S| <= (m + 8) * 2^-24 * A, (m + 9) with grad_pts (derivation in tests/cross_view_cases.py),
with the winner mask taken from the device's own forward; exactly 0 where nothing arrives.  Backward, deterministic: the
module path's bits.  Every bounded check prints its worst error / bound (pytest -s); the figures of the MI355X run are kept
in profiles/cross_view_error_ratios.txt.
"""
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from streammos_amd.refapi import deep_point
from streammos_amd.refapi.networks import backbone
from tests import cross_view_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAP_LAYOUTS = ("nchw", "channels_last", "slice")
NAN = float("nan")

RATIOS = []
RATIO_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cross_view_error_ratios.txt")
RATIO_HEADER = """Backward of the fused training transfer (csrc/gather_scatter_train.hip, smos_gather_scatter_train_bwd) against the float64
reference: worst error / bound per check.  Written by tests/test_gpu_cross_view_train.py when the whole file has run.

Each line is the largest |kernel - S| / bound over EVERY element of one gradient map, bound = (m + 8) * 2^-24 * A, or
(m + 9) with grad_pts ("+pts") (tests/cross_view_cases.py: derived, not tuned; 0 where nothing arrives).  "rows": a
channels-last destination (gst_bwd_rows for C >= 8, gst_bwd_points for C = 3); "nchw": an NCHW destination (gst_bwd_points);
"<-layout": how grad_out lies in memory ("cat_slice": a channel slice of a wider tensor).  The sums are float atomics: the
last bits, and so the ratios, move a little from run to run.
"""


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _map(a, layout):
    """a [B, C, H, W] on the device: NCHW-contiguous, channels-last strides, or inside a wider buffer of NaN (a gap behind
    every row and channels to both sides), which a read or a write outside the tensor would show."""
    t = _t(a)
    b, c, h, w = t.shape
    if layout == "nchw":
        return t, None
    if layout == "channels_last":
        return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), None
    wide = torch.full((b, c + 3, h, w + 2), NAN, device=DEV)
    view = wide[:, 2:2 + c, :, 1:1 + w]
    view.copy_(t)
    return view, wide


def _gaps_are_nan(wide, c, w):
    mask = torch.ones_like(wide, dtype=torch.bool)
    mask[:, 2:2 + c, :, 1:1 + w] = False
    return bool(torch.isnan(wide[mask]).all())


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _head(case, grid, out):
    gc, sc = _t(case.gcoord), _t(case.scoord)
    keep = (gc, sc)
    return keep, (grid.data_ptr(), _lib.i64_array(grid.stride()), gc.data_ptr(), cases.KG, _lib.f32_array(cases.GSCALE), sc.data_ptr(),
                  cases.KS, _lib.f32_array(cases.SSCALE), out.data_ptr(), _lib.i64_array(out.stride()))


def _sizes(case):
    return case.b, case.c, case.hg, case.wg, case.n, case.ho, case.wo


def _forward_entry(case, grid, out, pts):
    """smos_gather_scatter_train_fwd as it is declared: any strides on grid, out and pts."""
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    keep, head = _head(case, grid, out)
    _lib.call("smos_gather_scatter_train_fwd", *head, None if pts is None else pts.data_ptr(),
              None if pts is None else _lib.i64_array(pts.stride()), *_sizes(case), flag.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return int(flag.item())


def _module_forward(case):
    """pts, out of the two launches the op stands for."""
    pts = ops.bilinear_gather(_t(case.grid), _t(case.gcoord), cases.GSCALE)
    out = deep_point.VoxelMaxPool(pts.unsqueeze(-1), _t(case.scoord).unsqueeze(-1), (case.ho, case.wo), cases.SSCALE)
    return pts, out


@pytest.fixture(scope="module")
def forward_of():
    """(pts, out, winner mask) of the module path per case, computed once."""
    memo = {}

    def get(case):
        if case.name not in memo:
            pts, out = _module_forward(case)
            memo[case.name] = (pts, out, cases.winners(pts.cpu().numpy(), case.cell, out.cpu().numpy()))
        return memo[case.name]
    return get


def _all_cases():
    return [pytest.param(cases.case_of, (s, k), id="%s-%s" % (s, k)) for s, k in cases.ALL] + [pytest.param(cases.signed_case, (), id="signed")]


def _check(label, got, ref):
    ok, ratio = cases.worst_ratio(got.detach().cpu().numpy(), ref)
    print("cross-view-ratio %-58s %.4f" % (label, ratio))
    RATIOS.append((label, ratio))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    """profiles/cross_view_error_ratios.txt from this run, once every test of the file has run (not for a -k selection)."""
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 300 or len(ran) < 100:
        return
    worst = max(RATIOS, key=lambda r: r[1])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  %d checks, the largest ratio %.4f (%s).\n\n" % (
                torch.cuda.get_device_name(0), len(RATIOS), worst[1], worst[0]))
            f.writelines("%-62s %.4f\n" % r for r in RATIOS)
    except OSError:
        pass                                   # a read-only checkout: the figures were printed


@pytest.mark.parametrize("make,args", _all_cases())
def test_forward_has_the_bits_of_gather_then_maxpool(make, args, forward_of):
    case = make(*args)
    pts_want, out_want, _ = forward_of(case)
    if case.signed:
        assert (out_want < 0).any()
    for layout in MAP_LAYOUTS:
        grid, _ = _map(case.grid, layout)
        out, wide = _map(np.zeros((case.b, case.c, case.ho, case.wo)), layout)
        pts_wide = torch.full((case.b, case.c + 2, case.n + 3), NAN, device=DEV)
        pts = pts_wide[:, 1:1 + case.c, 2:2 + case.n] if layout == "slice" else torch.full((case.b, case.c, case.n), NAN, device=DEV)
        flag = _forward_entry(case, grid, out, pts)
        assert flag == int(case.signed and case.n > 0)
        assert torch.equal(_bits(out), _bits(out_want)), (case.name, layout)
        assert torch.equal(_bits(pts), _bits(pts_want)), (case.name, layout)
        if wide is not None:
            assert _gaps_are_nan(wide, case.c, case.wo)
            gap = torch.ones_like(pts_wide, dtype=torch.bool)
            gap[:, 1:1 + case.c, 2:2 + case.n] = False
            assert torch.isnan(pts_wide[gap]).all()
        # without the point values: the same target
        out2, _ = _map(np.zeros((case.b, case.c, case.ho, case.wo)), layout)
        _forward_entry(case, grid, out2, None)
        assert torch.equal(_bits(out2), _bits(out_want))


def _grad_out(case, layout):
    """grad_out [B, C, Ho, Wo] as the backward meets it; cat_slice: the channels C.. of a [B, 2C + 1, Ho, Wo] gradient, what
    torch.cat hands the second of its inputs."""
    if layout != "cat_slice":
        return _map(case.grad_out, layout)[0]
    wide = torch.full((case.b, 2 * case.c + 1, case.ho, case.wo), NAN, device=DEV)
    view = wide[:, case.c:2 * case.c]
    view.copy_(_t(case.grad_out))
    return view


@pytest.mark.parametrize("make,args", _all_cases())
def test_point_gradient_has_the_expected_bits(make, args, forward_of):
    """x for the device's own winners: ties, zero-valued winners, dropped points, NaN rows and grad_pts."""
    case = make(*args)
    _, out, win = forward_of(case)
    grid, gc, sc = _t(case.grid), _t(case.gcoord), _t(case.scoord)
    for with_pts in (False, True):
        want = _t(cases.point_grad(case, win, with_pts, dtype=np.float32))
        for layout in ("nchw", "cat_slice"):
            gp = None
            if with_pts:
                gp = torch.full((case.b, case.n + 1, case.c + 2), NAN, device=DEV)[:, :case.n, 1:1 + case.c].permute(0, 2, 1)
                gp.copy_(_t(case.grad_pts))
            x = torch.full((case.b, case.c, case.n), NAN, device=DEV)
            got = ops.gather_scatter_train_point_grad(grid, gc, cases.GSCALE, sc, cases.SSCALE, out, _grad_out(case, layout), gp, x=x)
            assert got is x and torch.equal(_bits(x), _bits(want)), (case.name, with_pts, layout)


@pytest.mark.parametrize("make,args", _all_cases())
def test_fused_backward_against_float64_reference(make, args, forward_of):
    case = make(*args)
    _, out, win = forward_of(case)
    gc, sc = _t(case.gcoord), _t(case.scoord)
    shape = (case.b, case.c, case.hg, case.wg)
    for with_pts in (False, True):
        ref = cases.reference(case, win, with_pts)
        gp = _t(case.grad_pts) if with_pts else None
        for layout in MAP_LAYOUTS + ("cat_slice",):
            grid = _map(case.grid, layout if layout != "cat_slice" else "nchw")[0]
            go = _grad_out(case, layout)
            for channels_last in (True, False):
                got = ops.gather_scatter_train_backward(grid, gc, cases.GSCALE, sc, cases.SSCALE, out, go, gp,
                                                        channels_last=channels_last, deterministic=False)
                assert got.shape == shape and (got.permute(0, 2, 3, 1) if channels_last else got).is_contiguous()
                _check("%s %s%s<-%s" % (case.name, "rows" if channels_last else "nchw", "+pts" if with_pts else "", layout), got, ref)


def test_backward_entry_with_a_destination_inside_a_wider_buffer(forward_of):
    """Destination strides as given, zeroed by the strided fill; the gaps keep their NaN."""
    case = cases.case_of("c32", "mix")
    _, out, win = forward_of(case)
    ref = cases.reference(case, win, True)
    grid, go, gp = _t(case.grid), _t(case.grad_out), _t(case.grad_pts)
    b, c, h, w = case.b, case.c, case.hg, case.wg
    for name, wide, view in (
            ("nhwc", torch.full((b, h, w, c + 3), NAN, device=DEV), lambda t: t[..., 1:1 + c].permute(0, 3, 1, 2)),
            ("nchw", torch.full((b, c, h, w + 2), NAN, device=DEV), lambda t: t[..., 2:])):
        dst = view(wide)
        keep, head = _head(case, grid, out)
        _lib.call("smos_gather_scatter_train_bwd", *head, go.data_ptr(), _lib.i64_array(go.stride()), gp.data_ptr(),
                  _lib.i64_array(gp.stride()), dst.data_ptr(), _lib.i64_array(dst.stride()), *_sizes(case),
                  torch.cuda.current_stream().cuda_stream)
        _check("c32/mix C entry %s slice +pts" % name, dst, ref)
        mask = torch.ones_like(wide, dtype=torch.bool)
        view(mask).fill_(False)
        assert torch.isnan(wide[mask]).all()


def _module_path(case, leaf, want_points):
    sampler = backbone.BilinearSample(case.c, cases.GSCALE)
    pts = sampler(leaf, _t(case.gcoord[..., :2]).unsqueeze(-1))
    out = deep_point.VoxelMaxPool(pts, _t(case.scoord).unsqueeze(-1), (case.ho, case.wo), cases.SSCALE)
    return out, (pts[..., 0] if want_points else None)


def _op_path(case, leaf, want_points):
    res = ops.gather_scatter_train(leaf, _t(case.gcoord[..., :2]).unsqueeze(-1), cases.GSCALE, _t(case.scoord).unsqueeze(-1),
                                   (case.ho, case.wo), cases.SSCALE, want_points=want_points)
    return res if want_points else (res, None)


def _grad(case, path, want_points):
    leaf = _t(case.grid).requires_grad_()
    out, pts = path(case, leaf, want_points)
    loss = (out * _t(case.grad_out)).sum()
    if want_points:
        loss = loss + (pts * _t(case.grad_pts)).sum()
    loss.backward()
    return out.detach(), leaf.grad


@pytest.mark.parametrize("want_points", [False, True])
@pytest.mark.parametrize("make,args", [p for p in _all_cases() if p.id.endswith(("-mix", "-runs", "signed"))])
def test_deterministic_backward_has_the_module_path_s_bits(make, args, want_points, request):
    case = make(*args)
    request.addfinalizer(lambda prev=ops.set_deterministic(True): ops.set_deterministic(prev))
    out_m, grad_m = _grad(case, _module_path, want_points)
    out_o, grad_o = _grad(case, _op_path, want_points)
    out_2, grad_2 = _grad(case, _op_path, want_points)
    assert torch.equal(_bits(out_o), _bits(out_m))
    assert grad_o.stride() == grad_m.stride() and torch.equal(_bits(grad_o), _bits(grad_m)), case.name
    assert torch.equal(_bits(grad_2), _bits(grad_o))


@pytest.mark.parametrize("want_points", [False, True])
def test_autograd_through_the_op(want_points, forward_of):
    """The fused launch behind the autograd node, against the reference; what the node keeps; no graph where none is asked for."""
    case = cases.case_of("c64", "mix")
    _, _, win = forward_of(case)
    prev = ops.set_deterministic(False)
    try:
        leaf = _t(case.grid).requires_grad_()
        out, pts = _op_path(case, leaf, want_points)
        saved = out.grad_fn.saved_tensors
        assert len(saved) == 4 and not any(tuple(t.shape) == (case.b, case.c, case.n) for t in saved)      # never a [B,C,N] tensor
        loss = (out * _t(case.grad_out)).sum()
        if want_points:
            loss = loss + (pts * _t(case.grad_pts)).sum()
        grad, = torch.autograd.grad(loss, leaf)
    finally:
        ops.set_deterministic(prev)
    assert grad.permute(0, 2, 3, 1).is_contiguous()       # the node hands on the rows as written, like bilinear_gather's
    _check("autograd c64/mix want_points=%s" % want_points, grad, cases.reference(case, win, want_points))
    with torch.no_grad():
        assert ops.gather_scatter_train(leaf, _t(case.gcoord), cases.GSCALE, _t(case.scoord), (case.ho, case.wo), cases.SSCALE).grad_fn is None


def test_only_the_point_values_used(forward_of):
    """pts alone carries the gradient: out's arrives as None, not as a map of zeros somebody had to fill."""
    case = cases.case_of("c8", "uniform")
    leaf = _t(case.grid).requires_grad_()
    prev = ops.set_deterministic(False)
    try:
        _, pts = _op_path(case, leaf, True)
        (pts * _t(case.grad_pts)).sum().backward()
    finally:
        ops.set_deterministic(prev)
    ref = cases.reference(case, np.zeros((case.b, case.c, case.n), dtype=bool), True)
    _check("autograd c8/uniform pts only", leaf.grad, ref)


@pytest.mark.parametrize("cap", [1, 2])
@pytest.mark.parametrize("shape", ["c3", "c8", "c64", "c71_ragged"])
def test_results_do_not_depend_on_the_grid(shape, cap, forward_of):
    """One or two blocks walk every point and tile: the second trip of every grid-stride loop."""
    case = cases.case_of(shape, "mix")
    pts_want, out_want, win = forward_of(case)
    grid, gc, sc, go, gp = _t(case.grid), _t(case.gcoord), _t(case.scoord), _t(case.grad_out), _t(case.grad_pts)
    try:
        with util.conv_grid_cap(cap):
            out = torch.zeros_like(out_want)
            pts = torch.empty_like(pts_want)
            _forward_entry(case, grid, out, pts)
            x = ops.gather_scatter_train_point_grad(grid, gc, cases.GSCALE, sc, cases.SSCALE, out, go, gp)
            det = ops.gather_scatter_train_backward(grid, gc, cases.GSCALE, sc, cases.SSCALE, out, go, gp, deterministic=True)
            rows = ops.gather_scatter_train_backward(grid, gc, cases.GSCALE, sc, cases.SSCALE, out, go, gp, deterministic=False)
            nchw = ops.gather_scatter_train_backward(grid, gc, cases.GSCALE, sc, cases.SSCALE, out, go, gp, channels_last=False,
                                                     deterministic=False)
            torch.cuda.synchronize()
    finally:
        _lib.load().smos_debug_set_conv_grid_cap(0)
    assert torch.equal(_bits(out), _bits(out_want)) and torch.equal(_bits(pts), _bits(pts_want))
    assert torch.equal(_bits(x), _bits(_t(cases.point_grad(case, win, True, dtype=np.float32))))
    free = ops.gather_scatter_train_backward(grid, gc, cases.GSCALE, sc, cases.SSCALE, out, go, gp, deterministic=True)
    assert torch.equal(_bits(det), _bits(free))
    ref = cases.reference(case, win, True)
    _check("%s/mix cap %d rows+pts" % (shape, cap), rows, ref)
    _check("%s/mix cap %d nchw+pts" % (shape, cap), nchw, ref)


def test_refusals_and_frozen_inputs(monkeypatch):
    case = cases.case_of("c8", "mix")
    grid, gc, sc = _t(case.grid), _t(case.gcoord), _t(case.scoord)
    size, gs, ss = (case.ho, case.wo), cases.GSCALE, cases.SSCALE
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.gather_scatter_train(grid.cpu(), gc, gs, sc, size, ss)
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.gather_scatter_train(grid, gc, gs, sc.cpu(), size, ss)
    with pytest.raises(RuntimeError, match="float32 only"):
        ops.gather_scatter_train(grid.half(), gc, gs, sc, size, ss)
    with pytest.raises(RuntimeError, match="float32 only"):
        ops.gather_scatter_train(grid, gc.double(), gs, sc, size, ss)
    with pytest.raises(RuntimeError, match="coordinates"):
        ops.gather_scatter_train(grid, gc.clone().requires_grad_(), gs, sc, size, ss)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gather_scatter_train(grid, gc, gs, sc[:, :-1], size, ss)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gather_scatter_train(grid, gc[:1], gs, sc[:1], size, ss)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gather_scatter_train(grid, gc, gs, sc, (case.ho,), ss)
    # a grid that needs no gradient (stage 2's frozen trunk): forward only, nothing kept, no backward kernel entered
    entered = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (entered.append(name), real(name, *a))[1])
    w = torch.ones((), device=DEV, requires_grad=True)
    out, pts = ops.gather_scatter_train(grid, gc, gs, sc, size, ss, want_points=True)
    assert out.grad_fn is None and pts.grad_fn is None
    ((out * w).sum() + (pts * w).sum()).backward()
    assert w.grad is not None and entered == ["smos_gather_scatter_train_fwd"]
    # and one that does: the fused launch, once
    del entered[:]
    leaf = grid.clone().requires_grad_()
    prev = ops.set_deterministic(False)
    try:
        ops.gather_scatter_train(leaf, gc, gs, sc, size, ss).sum().backward()
    finally:
        ops.set_deterministic(prev)
    assert entered == ["smos_gather_scatter_train_fwd", "smos_gather_scatter_train_bwd"]

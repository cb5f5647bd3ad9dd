"""smos_bilinear_gather_bwd (csrc/bilinear_gather.hip) on the GPU against the float64 reference of
tests/bilinear_bwd_cases.py, through ops.bilinear_gather_backward, the C entry point, the autograd node of
ops.bilinear_gather and BilinearSample.

Bar, per grid element: |got - S| <= (m + 8) * 2^-24 * A (derivation in tests/bilinear_bwd_cases.py; independent of the
order of the additions, so it holds for the atomics), exactly 0 where nothing arrives.  Every check prints its worst
error / bound (pytest -s); the figures of the MI355X run are kept in profiles/bilinear_bwd_error_ratios.txt.
"""
import os
import types

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from streammos_amd.refapi.networks import backbone
from tests import bilinear_bwd_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GRAD_LAYOUTS = ("channel_major", "point_major", "channel_major_slice", "point_major_slice")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _grad_out(case, layout):
    """case.grad_out [B, C, N] on the device in one of the layouts the kernel reads; the slices sit inside a wider buffer
    of NaN, which a read outside the tensor would bring in."""
    g = _t(case.grad_out)
    b, c, n = g.shape
    if layout == "channel_major":
        return g
    if layout == "point_major":
        return g.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    if layout == "channel_major_slice":
        wide = torch.full((b, c + 5, n + 3), float("nan"), device=DEV)
        view = wide[:, 2:2 + c, 1:1 + n]
    else:
        wide = torch.full((b, n + 2, c + 3), float("nan"), device=DEV)
        view = wide[:, 1:1 + n, 2:2 + c].permute(0, 2, 1)
    view.copy_(g)
    assert not view.is_contiguous() or n == 0
    return view


RATIOS = []
RATIO_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bilinear_bwd_error_ratios.txt")
RATIO_HEADER = """Backward of the bilinear gather (csrc/bilinear_gather.hip, smos_bilinear_gather_bwd) against the float64 reference:
worst error / bound per check.  Written by tests/test_gpu_bilinear_backward.py when the whole file has run.

Each line is the largest |kernel - S| / bound over EVERY element of one gradient map, bound = (m + 8) * 2^-24 * A
(tests/bilinear_bwd_cases.py: derived, not tuned; 0 where nothing arrives).  "rows<-layout": a channels-last destination
(bil_bwd_rows for C >= 8, bil_bwd_points for C = 3) reading grad_out in that layout; "nchw<-layout": an NCHW destination
(bil_bwd_points); "C entry": destination strides of a slice of a wider NaN buffer.  The sums are float atomics: the last
bits, and so the ratios, move a little from run to run.
"""


def _check(label, got, case, factor=1.0):
    ok, ratio = cases.worst_ratio(got.detach().cpu().numpy(), case, factor)
    print("bilinear-bwd-ratio %-58s %.4f" % (label, ratio))
    RATIOS.append((label, ratio))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    """profiles/bilinear_bwd_error_ratios.txt from this run, once every test of the file has run (not for a -k selection)."""
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 100 or len(ran) < 30:
        return
    worst = max(RATIOS, key=lambda r: r[1])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  %d checks, the largest ratio %.4f (%s).\n\n" % (
                torch.cuda.get_device_name(0), len(RATIOS), worst[1], worst[0]))
            f.writelines("%-62s %.4f\n" % r for r in RATIOS)
    except OSError:
        pass                                   # a read-only checkout: the figures were printed


@pytest.mark.parametrize("kind", cases.COORD_SETS)
@pytest.mark.parametrize("shape", list(cases.SHAPES))
def test_backward_against_float64_reference(shape, kind):
    case = cases.case_of(shape, kind)
    coord = _t(case.coord)
    grid_shape = (case.b, case.c, case.h, case.w)
    for layout in GRAD_LAYOUTS:
        go = _grad_out(case, layout)
        got = ops.bilinear_gather_backward(go, coord, case.scale, grid_shape)
        assert got.shape == grid_shape and got.permute(0, 2, 3, 1).is_contiguous()       # a view of a [B, H, W, C] buffer
        _check("%s/%s rows<-%s" % (shape, kind, layout), got, case)
    # NCHW destination: the points form, whatever C
    for layout in ("channel_major", "point_major_slice"):
        got = ops.bilinear_gather_backward(_grad_out(case, layout), coord, case.scale, grid_shape, channels_last=False)
        assert got.is_contiguous()
        _check("%s/%s nchw<-%s" % (shape, kind, layout), got, case)


@pytest.mark.parametrize("shape", ["c3_points", "c32", "c71_ragged"])
def test_c_entry_point_with_a_destination_inside_a_wider_buffer(shape):
    """Destination strides as given: a channels-last map whose pixels are 3 floats apart from the next (rows form for
    C >= 8, zeroed by the strided fill) and an NCHW map with a gap behind every row (points form).  The gaps keep their
    NaN: nothing is written outside the tensor."""
    case = cases.case_of(shape, "mix")
    b, c, h, w = case.b, case.c, case.h, case.w
    lib = _lib.load()
    go, coord = _t(case.grad_out), _t(case.coord)
    for name, wide, view in (
            ("nhwc", torch.full((b, h, w, c + 3), float("nan"), device=DEV), lambda t: t[..., 1:1 + c].permute(0, 3, 1, 2)),
            ("nchw", torch.full((b, c, h, w + 2), float("nan"), device=DEV), lambda t: t[..., 2:])):
        dst = view(wide)
        rc = lib.smos_bilinear_gather_bwd(go.data_ptr(), _lib.i64_array(go.stride()), coord.data_ptr(), cases.K, dst.data_ptr(),
                                          _lib.i64_array(dst.stride()), b, c, h, w, case.n, _lib.f32_array(case.scale),
                                          torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "smos_bilinear_gather_bwd")
        _check("%s/mix C entry %s slice" % (shape, name), dst, case)
        mask = torch.ones_like(wide, dtype=torch.bool)
        view(mask).fill_(False)
        assert torch.isnan(wide[mask]).all()


def test_waves_walk_several_tiles_and_skip_padding_tiles():
    """More tiles than the largest grid has waves, across a sample boundary, with whole tiles of padding rows: the
    grid-stride step, a second fill of the LDS tile behind a read-out, and a skipped tile followed by more work."""
    case = cases.grid_stride_case()
    coord = _t(case.coord)
    for layout in ("channel_major", "point_major"):
        got = ops.bilinear_gather_backward(_grad_out(case, layout), coord, case.scale, (case.b, case.c, case.h, case.w))
        _check("grid stride rows<-%s" % layout, got, case)


def test_destination_arrives_poisoned():
    """The result is allocated uninitialised: a freed NaN buffer of its size is what the caching allocator hands out next."""
    case = cases.sparse_case()
    go, coord = _t(case.grad_out), _t(case.coord)
    untouched = torch.from_numpy(np.broadcast_to(case.m == 0, case.S.shape).copy()).to(DEV)
    assert untouched.any()
    for channels_last in (True, False):
        poison = torch.full((case.b * case.c * case.h * case.w,), float("nan"), device=DEV)
        ptr = poison.data_ptr()
        del poison
        got = ops.bilinear_gather_backward(go, coord, case.scale, (case.h, case.w), channels_last=channels_last)
        assert got.data_ptr() == ptr, "the allocator did not reuse the poisoned block: the case checks nothing"
        assert not torch.isnan(got).any() and (got[untouched] == 0).all()
        _check("sparse poisoned channels_last=%s" % channels_last, got, case)


@pytest.mark.parametrize("point_major", [False, True])
def test_autograd_through_the_op(point_major):
    case = cases.case_of("c64", "mix")
    coord = _t(case.coord)
    grid = torch.randn((case.b, case.c, case.h, case.w), device=DEV)
    plain = ops.bilinear_gather(grid, coord, case.scale, point_major=point_major)
    assert plain.grad_fn is None
    leaf = grid.clone().requires_grad_()
    out = ops.bilinear_gather(leaf, coord, case.scale, point_major=point_major)
    assert out.grad_fn is not None and out.stride() == plain.stride()
    assert torch.equal(out.detach().view(torch.int32), plain.view(torch.int32))           # same launch, same bits
    (out * _t(case.grad_out)).sum().backward()
    _check("autograd c64/mix point_major=%s" % point_major, leaf.grad, case)
    # out=: the returned tensor shares out's memory and carries the graph
    leaf.grad = None
    buf = torch.empty_like(plain)
    out2 = ops.bilinear_gather(leaf, coord, case.scale, out=buf, point_major=point_major)
    assert out2.data_ptr() == buf.data_ptr() and torch.equal(buf.view(torch.int32), plain.view(torch.int32))
    (out2 * _t(case.grad_out)).sum().backward()
    _check("autograd c64/mix out= point_major=%s" % point_major, leaf.grad, case)
    # the node hands on the rows as written: a permuted view of a [B, H, W, C] buffer, no transposition pass
    grad = torch.autograd.grad(ops.bilinear_gather(leaf, coord, case.scale), leaf, _t(case.grad_out))[0]
    assert grad.permute(0, 2, 3, 1).is_contiguous()
    # no graph where none is asked for
    with torch.no_grad():
        assert ops.bilinear_gather(leaf, coord, case.scale).grad_fn is None
    with pytest.raises(RuntimeError, match="coord"):
        ops.bilinear_gather(leaf, coord.clone().requires_grad_(), case.scale)


def test_autograd_of_a_sum_has_an_expanded_gradient():
    """g.sum().backward() hands the node a gradient of ones with every stride 0."""
    ones = cases.case_of("c32", "runs")
    grid = torch.randn((ones.b, ones.c, ones.h, ones.w), device=DEV, requires_grad=True)
    ops.bilinear_gather(grid, _t(ones.coord), ones.scale).sum().backward()
    s, a, m = cases.backward_ref(np.ones_like(ones.grad_out), ones.coord, ones.scale, ones.h, ones.w)
    _check("autograd c32/runs sum()", grid.grad, types.SimpleNamespace(S=s, A=a, m=m))


def test_module_in_training_mode_takes_the_own_path(monkeypatch, request):
    """BilinearSample with the switch at 1 on a grid that needs a gradient: forward and backward on the own kernels (counted on ops), the
    gradient against the F.grid_sample formulation the switch at 0 keeps, inside the sum of both bounds.  The case is
    dyadic (tests/bilinear_bwd_cases.py::dyadic_case), so both sample the same positions."""
    case = cases.dyadic_case()
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.bilinear_gather, ops.bilinear_gather_backward

    def count(key, fn):
        def wrapped(*args, **kwargs):
            calls[key] += 1
            return fn(*args, **kwargs)
        return wrapped
    monkeypatch.setattr(ops, "bilinear_gather", count("fwd", fwd))
    monkeypatch.setattr(ops, "bilinear_gather_backward", count("bwd", bwd))
    request.addfinalizer(lambda prev=ops.set_bilinear_bwd_own(True): ops.set_bilinear_bwd_own(prev))     # SMOS_BILINEAR_BWD=1
    mod = backbone.BilinearSample(case.c, case.scale).train()
    feat = torch.randn((case.b, case.c, case.h, case.w), device=DEV)
    coord = _t(case.coord[..., :2]).unsqueeze(-1)                                        # (BS, N, 2, 1)
    go = _t(case.grad_out).unsqueeze(-1)

    own = feat.clone().requires_grad_()
    out = mod(own, coord)
    assert out.shape == (case.b, case.c, case.n, 1) and calls == {"fwd": 1, "bwd": 0}
    out.backward(go)
    assert calls == {"fwd": 1, "bwd": 1}
    _check("module dyadic own", own.grad, case)

    ref = feat.clone().requires_grad_()
    want = cases.grid_sample_formulation(torch, ref, coord, case.scale)
    want.backward(go)
    assert calls == {"fwd": 1, "bwd": 1}
    _check("module dyadic grid_sample", ref.grad, case)
    assert (out - want).abs().max().item() <= 2e-6 * feat.abs().max().item() * 4
    diff = (own.grad - ref.grad).abs().double().cpu().numpy()
    assert (diff <= 2.0 * cases.bound(case)).all()

    # the switch at 0, and a coordinate gradient whatever the switch: F.grid_sample as before
    ops.set_bilinear_bwd_own(False)
    off = feat.clone().requires_grad_()
    mod(off, coord).backward(go)
    assert calls == {"fwd": 1, "bwd": 1}
    _check("module dyadic switch 0", off.grad, case)
    ops.set_bilinear_bwd_own(True)
    cg = coord.clone().requires_grad_()
    mod(feat.clone().requires_grad_(), cg).backward(go)
    assert calls == {"fwd": 1, "bwd": 1} and cg.grad is not None
    # inference keeps the direct launch
    with torch.no_grad():
        assert torch.equal(mod(own, coord), out.detach()) and calls == {"fwd": 2, "bwd": 1}

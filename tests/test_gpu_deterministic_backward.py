"""smos_bilinear_gather_bwd_det and smos_msda_bwd_det (csrc/segsum.hip) on the GPU: bit for bit the float32 restatement of
tests/segsum_cases.py -- through ops, the C entry points and the autograd nodes -- and inside the float64 references' bounds.

Every comparison is array_equal unless a bound is named.  The bilinear bound is (m + 8) * 2^-24 * A
(tests/bilinear_bwd_cases.py), the grad_value bound util.msda_backward_bounds; the worst error / bound of every check is
printed (pytest -s) and kept in profiles/segsum_error_ratios.txt.
"""
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from streammos_amd.refapi.deformattn._msda import MSDeformAttnFunction
from streammos_amd.refapi.networks import backbone
from tests import bilinear_bwd_cases as bcases
from tests import segsum_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

RATIOS = []
RATIO_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "segsum_error_ratios.txt")
RATIO_HEADER = """Fixed-order backward sums (csrc/segsum.hip: smos_bilinear_gather_bwd_det, smos_msda_bwd_det) against the float64
references: worst error / bound per check.  Written by tests/test_gpu_deterministic_backward.py when the whole file has run.

Every result named here is first of all bit-equal to the numpy float32 restatement of tests/segsum_cases.py (the test
asserts array_equal), so the ratios do not move from run to run.  Bilinear: bound = (m + 8) * 2^-24 * A per element
(tests/bilinear_bwd_cases.py), 0 where nothing arrives.  MSDA: grad_value against util.msda_backward_bounds.
"""


@pytest.fixture(scope="module")
def chunk():
    return ops.segsum_chunk()


@pytest.fixture(autouse=True)
def _restore_setting():
    prev = ops.set_deterministic(None)
    ops.set_deterministic(prev)
    yield
    ops.set_deterministic(prev)


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 100 or len(ran) < 40:
        return                                     # a -k selection
    worst = max(RATIOS, key=lambda r: r[1])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  Chunk %d.  %d checks, the largest ratio %.4f (%s).\n\n" % (
                torch.cuda.get_device_name(0), ops.segsum_chunk(), len(RATIOS), worst[1], worst[0]))
            f.writelines("%-66s %.4f\n" % r for r in RATIOS)
    except OSError:
        pass                                       # a read-only checkout: the figures were printed


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)             # a copy: the cases are read-only


def _bits(t):
    return t.detach().cpu().contiguous().numpy()


def _grad_out(case, point_major):
    g = _t(case.grad_out)
    return g.permute(0, 2, 1).contiguous().permute(0, 2, 1) if point_major else g


def _check_bilinear(label, got, key, chunk):
    """array_equal to the restatement; inside the float64 bound."""
    case = cases.bilinear_case(key)
    want, _ = cases.bilinear_restated(key, chunk)
    got = _bits(got)
    ok, ratio = bcases.worst_ratio(got, case)
    print("segsum-ratio %-62s %.4f" % (label, ratio))
    RATIOS.append((label, ratio))
    assert np.array_equal(got, want), "%s: %d elements differ from the restatement, largest difference %g" % (
        label, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want).max()))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


def _all_layouts(key, chunk):
    case = cases.bilinear_case(key)
    coord = _t(case.coord)
    shape = (case.b, case.c, case.h, case.w)
    for point_major in (False, True):
        for channels_last in (True, False):
            got = ops.bilinear_gather_backward(_grad_out(case, point_major), coord, case.scale, shape,
                                               channels_last=channels_last, deterministic=True)
            assert got.shape == shape
            assert got.permute(0, 2, 3, 1).is_contiguous() if channels_last else got.is_contiguous()
            _check_bilinear("%s %s<-%s" % (cases.key_id(key), "nhwc" if channels_last else "nchw",
                                           "point_major" if point_major else "channel_major"), got, key, chunk)


@pytest.mark.parametrize("kind", bcases.COORD_SETS)
@pytest.mark.parametrize("shape", list(bcases.SHAPES))
def test_bilinear_equals_the_restatement(shape, kind, chunk):
    _all_layouts(("shape", shape, kind), chunk)


@pytest.mark.parametrize("name", ["sparse", "dyadic", "grid_stride"])
def test_bilinear_special_cases(name, chunk):
    _all_layouts((name,), chunk)


def test_chunk_edges(chunk):
    """One cell with L - 1, L, L + 1 and 2 L + 3 points: a list that ends just before, on and just after a chunk end, and one of
    three chunks."""
    for n in cases.onecell_sizes(chunk):
        assert cases.onecell_case(n).m.max() == n
        _all_layouts(("onecell", n), chunk)


@pytest.mark.parametrize("shape", ["c3_points", "c32", "c71_ragged"])
def test_c_entry_point_with_a_destination_inside_a_wider_buffer(shape, chunk):
    """Destination strides as given, guard bands untouched; a destination and a workspace poisoned with NaN and with 0xFF
    bytes before the call give the same bits."""
    key = ("shape", shape, "mix")
    case = cases.bilinear_case(key)
    b, c, h, w = case.b, case.c, case.h, case.w
    lib = _lib.load()
    go, coord = _t(case.grad_out), _t(case.coord)
    need = int(lib.smos_bilinear_gather_bwd_det_work_bytes(b, c, h, w, case.n))
    assert need > 0 and need % 256 == 0
    for name, wide_shape, view in (("nhwc", (b, h, w, c + 3), lambda t: t[..., 1:1 + c].permute(0, 3, 1, 2)),
                                   ("nchw", (b, c, h, w + 2), lambda t: t[..., 2:])):
        results = []
        for fill in ("nan", "ff"):
            wide = torch.full(wide_shape, float("nan"), device=DEV)
            work = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
            if fill == "ff":
                wide.view(torch.int32).fill_(-1)                                   # 0xFF bytes: a NaN with every bit set
                work.fill_(255)
            else:
                work.view(torch.float32).fill_(float("nan"))
            guard, tail = wide.clone(), work[need:].clone()
            dst = view(wide)
            rc = lib.smos_bilinear_gather_bwd_det(go.data_ptr(), _lib.i64_array(go.stride()), coord.data_ptr(), bcases.K,
                                                  dst.data_ptr(), _lib.i64_array(dst.stride()), b, c, h, w, case.n,
                                                  _lib.f32_array(case.scale), work.data_ptr(), need,
                                                  torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "smos_bilinear_gather_bwd_det")
            _check_bilinear("%s/mix C entry %s slice, %s fill" % (shape, name, fill), dst, key, chunk)
            mask = torch.ones(wide_shape, dtype=torch.bool, device=DEV)
            view(mask).fill_(False)
            assert torch.equal(wide.view(torch.int32)[mask], guard.view(torch.int32)[mask])      # the gaps keep their bytes
            assert torch.equal(work[need:], tail)                                               # nothing past work_bytes
            results.append(_bits(dst))
        assert np.array_equal(results[0], results[1])


def test_workspace_too_small_is_refused():
    case = bcases.sparse_case()
    lib = _lib.load()
    go, coord = _t(case.grad_out), _t(case.coord)
    need = int(lib.smos_bilinear_gather_bwd_det_work_bytes(case.b, case.c, case.h, case.w, case.n))
    dst = torch.empty((case.b, case.c, case.h, case.w), device=DEV)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.smos_bilinear_gather_bwd_det(go.data_ptr(), _lib.i64_array(go.stride()), coord.data_ptr(), bcases.K, dst.data_ptr(),
                                          _lib.i64_array(dst.stride()), case.b, case.c, case.h, case.w, case.n,
                                          _lib.f32_array(case.scale), work.data_ptr(), need - 256,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"workspace" in lib.smos_last_error()


def _msda_args(c):
    return (_t(c.value), _t(c.shapes, np.int64), _t(c.lsi, np.int64), _t(c.loc), _t(c.attn), _t(c.grad_out))


def _check_msda(label, got, name, chunk):
    c = util.msda_bwd_case(name)
    want, _ = cases.msda_restated(name, chunk)
    got = _bits(got)
    ok, ratio = util.msda_worst_ratio(got, c.want_value, util.msda_backward_bounds(c, "float32")[0])
    print("segsum-ratio %-62s %.4f" % (label, ratio))
    RATIOS.append((label, ratio))
    assert np.array_equal(got, want), "%s: %d elements differ from the restatement, largest difference %g" % (
        label, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want).max()))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


@pytest.mark.parametrize("name", list(util.MSDA_BWD_CASES))
def test_msda_equals_the_restatement(name, chunk):
    c = util.msda_bwd_case(name)
    args = _msda_args(c)
    gv, gl, ga = ops.msda_bwd(*args, deterministic=True)
    _check_msda("msda %s grad_value" % name, gv, name, chunk)
    _, gl_at, ga_at = ops.msda_bwd(*args, deterministic=False)
    assert np.array_equal(_bits(gl), _bits(gl_at)) and np.array_equal(_bits(ga), _bits(ga_at))
    # a second call: the same bits, not twice them (nothing is accumulated into what a call finds)
    gv2, gl2, ga2 = ops.msda_bwd(*args, deterministic=True)
    assert np.array_equal(_bits(gv2), _bits(gv)) and np.array_equal(_bits(gl2), _bits(gl)) and np.array_equal(_bits(ga2), _bits(ga))


def test_msda_c_entry_point_with_poisoned_destination_and_workspace(chunk):
    name = "bwd_d33"
    c = util.msda_bwd_case(name)
    value, shapes, lsi, loc, attn, go = _msda_args(c)
    lib = _lib.load()
    need = int(lib.smos_msda_bwd_det_work_bytes(c.n, c.s, c.m, c.d, c.l, c.lq, c.p))
    assert need > 0 and need % 256 == 0
    results = []
    for fill in ("nan", "ff"):
        gv = torch.full_like(value, float("nan"))
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        if fill == "ff":
            gv.view(torch.int32).fill_(-1)
            work.fill_(255)
        else:
            work.view(torch.float32).fill_(float("nan"))
        gl, ga = torch.empty_like(loc), torch.empty_like(attn)
        rc = lib.smos_msda_bwd_det(go.data_ptr(), value.data_ptr(), shapes.data_ptr(), lsi.data_ptr(), loc.data_ptr(),
                                   attn.data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), c.n, c.s, c.m, c.d, c.l, c.lq, c.p,
                                   work.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "smos_msda_bwd_det")
        _check_msda("msda %s C entry, %s fill" % (name, fill), gv, name, chunk)
        results.append(_bits(gv))
    assert np.array_equal(results[0], results[1])


def test_results_do_not_depend_on_the_grid(chunk):
    """The grid cap at 1 and at 3 makes one block walk every work item of every kernel of the three steps."""
    key = ("shape", "c64", "runs")
    case = cases.bilinear_case(key)
    coord, shape = _t(case.coord), (case.b, case.c, case.h, case.w)
    margs = _msda_args(util.msda_bwd_case("bwd_d33_second_sweep"))
    got = {}
    try:
        for cap in (1, 3, 0):
            with util.conv_grid_cap(cap):
                bil = [ops.bilinear_gather_backward(_grad_out(case, pm), coord, case.scale, shape, deterministic=True)
                       for pm in (False, True)]
                got[cap] = [_bits(t) for t in bil] + [_bits(t) for t in ops.msda_bwd(*margs, deterministic=True)]
    finally:
        _lib.load().smos_debug_set_conv_grid_cap(0)
    for cap in (1, 3):
        for a, b in zip(got[cap], got[0]):
            assert np.array_equal(a, b)
    _check_bilinear("c64/runs grid cap 1", torch.from_numpy(got[1][0]), key, chunk)
    _check_msda("msda bwd_d33_second_sweep grid cap 1", torch.from_numpy(got[1][2]), "bwd_d33_second_sweep", chunk)


class _CountingLib:
    """The library handle with the calls of the four backward entries counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("smos_bilinear_gather_bwd", "smos_bilinear_gather_bwd_det", "smos_msda_bwd", "smos_msda_bwd_det"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_bilinear_module_through_autograd(monkeypatch, request, chunk):
    """BilinearSample in training mode with the setting on: the fixed-order entry, the same bits on two runs and the bits of
    the direct op; with the setting off the atomic entry."""
    key = ("dyadic",)
    case = cases.bilinear_case(key)
    lib = _CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", lib)
    request.addfinalizer(lambda prev=ops.set_bilinear_bwd_own(True): ops.set_bilinear_bwd_own(prev))
    monkeypatch.delenv("SMOS_DETERMINISTIC", raising=False)
    mod = backbone.BilinearSample(case.c, case.scale).train()
    feat = torch.randn((case.b, case.c, case.h, case.w), device=DEV)
    coord = _t(case.coord[..., :2]).unsqueeze(-1)
    go = _t(case.grad_out).unsqueeze(-1)

    def run():
        leaf = feat.clone().requires_grad_()
        mod(leaf, coord).backward(go)
        return leaf.grad

    ops.set_deterministic(True)
    first, second = run(), run()
    assert lib.calls == {"smos_bilinear_gather_bwd_det": 2}
    assert np.array_equal(_bits(first), _bits(second))
    direct = ops.bilinear_gather_backward(go, _t(case.coord), case.scale, feat.shape, deterministic=True)
    assert np.array_equal(_bits(first), _bits(direct))
    _check_bilinear("module dyadic through autograd", first, key, chunk)

    ops.set_deterministic(False)
    lib.calls.clear()
    atomic = run()
    assert lib.calls == {"smos_bilinear_gather_bwd": 1}
    assert bcases.worst_ratio(_bits(atomic), case)[0]
    ops.set_deterministic(None)                                   # nothing set anywhere: off
    lib.calls.clear()
    run()
    assert lib.calls == {"smos_bilinear_gather_bwd": 1}


def test_msda_function_through_autograd(monkeypatch, chunk):
    name = "bwd_d32"
    c = util.msda_bwd_case(name)
    lib = _CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", lib)
    monkeypatch.delenv("SMOS_DETERMINISTIC", raising=False)
    value, shapes, lsi, loc, attn, go = _msda_args(c)

    def run():
        leaves = [t.clone().requires_grad_() for t in (value, loc, attn)]
        out = MSDeformAttnFunction.apply(leaves[0], shapes, lsi, leaves[1], leaves[2], 64)
        out.backward(go)
        return [t.grad for t in leaves]

    ops.set_deterministic(True)
    first, second = run(), run()
    assert lib.calls == {"smos_msda_bwd_det": 2}
    direct = ops.msda_bwd(value, shapes, lsi, loc, attn, go, deterministic=True)
    for a, b, d in zip(first, second, direct):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(d))
    _check_msda("msda %s through autograd" % name, first[0], name, chunk)

    ops.set_deterministic(False)
    lib.calls.clear()
    atomic = run()
    assert lib.calls == {"smos_msda_bwd": 1}
    assert np.array_equal(_bits(atomic[1]), _bits(first[1])) and np.array_equal(_bits(atomic[2]), _bits(first[2]))
    # float64 under an ambient setting stays on the atomic kernel; asked for explicitly it is refused
    ops.set_deterministic(True)
    lib.calls.clear()
    args64 = (value.double(), shapes, lsi, loc.double(), attn.double(), go.double())
    ops.msda_bwd(*args64)
    assert lib.calls == {"smos_msda_bwd": 1}
    with pytest.raises(RuntimeError, match="float32 only"):
        ops.msda_bwd(*args64, deterministic=True)

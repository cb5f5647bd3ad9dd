"""The backward of the decoder's conv_1 path on the GPU: the adjoint kernels of csrc/upconv_bwd.hip alone (ops.upconv_adjoint)
and the whole autograd op (ops.upconv3x3_train) against the float64 references of tests/upconv_bwd_cases.py, element by
element, inside the bounds derived there (checked on the host by tests/test_host_upconv_bwd.py).

  upconv_bwd_ypass +   every geometry of util.UPCONV_PASS_CASES: Hs = 1, Ws = 1, Ho = 1, Wo = 1 and all of them, the identity,
  upconv_bwd_xpass     dyadic and non-dyadic ratios, one and two sources, C/4 = 1, 9, 32, multi-block inputs.  g is read
                       from a pitched buffer, G written into a column range of a wider and taller sentinel-filled matrix,
                       the y adjoint's scratch has a sentinel tail.  Exact twins (dyadic geometry, integer g) bit for bit;
                       a second call, a sample alone, and a capped grid (a block walks the elements in several trips) give
                       the same bits; one Inf in g makes the elements non-finite that the float32 restatement names.
  ops.upconv3x3_train  the four 128-channel cases: the forward is ops.upconv3x3 bit for bit, grad conv_a is g, dX and dW of
                       each source inside their bounds, frozen inputs yield None and run no matrix product; the refusals.

Every check prints its worst error / bound (pytest -s); the figures of the MI355X run are kept in
profiles/upconv_bwd_error_ratios.txt.
"""
import os

import numpy as np
import pytest
import torch

from streammos_amd import ops
from tests import upconv_bwd_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = []
RATIO_FILE = os.path.join(ROOT, "profiles", "upconv_bwd_error_ratios.txt")
RATIO_HEADER = """Backward of the decoder's conv_1 path (csrc/upconv_bwd.hip, ops.upconv_adjoint, ops.upconv3x3_train) against the float64
references of tests/upconv_bwd_cases.py.  Written by tests/test_gpu_upconv_bwd.py when the whole file has run.

Per check: the largest error / bound over the elements.  Bounds, u = 2^-24 (derivation in tests/upconv_bwd_cases.py):
G: u ((n_y + n_x + 8) A + Q); dX: E_G |nk| + u 9C (A + E_G) |nk|; dW: E_G^T |X| + u P (A + E_G)^T |X|.
"""


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _check(label, got, want, bound):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.size == want.size, (label, got.shape, want.shape)
    ok, ratio = util.msda_worst_ratio(got, want, bound)
    print("upconv-bwd-ratio %-60s %.4f" % (label, ratio))
    RATIOS.append((label, ratio))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    """profiles/upconv_bwd_error_ratios.txt from this run, once every test of the file has run (not for a -k selection)."""
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 30 or len(ran) < 60:
        return
    worst = max(RATIOS, key=lambda r: r[1])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  %d checks; the largest error / bound %.4f (%s).\n\n" % (
                torch.cuda.get_device_name(0), len(RATIOS), worst[1], worst[0]))
            f.writelines("%-64s %.4f\n" % r for r in RATIOS)
    except OSError:
        pass                                   # a read-only checkout: the figures were printed


def _g_view(g, pitch_extra=12, at=4):
    """g [B, Ho, Wo, C] as channels [at, at + C) of a sentinel-filled buffer of pitch C + pitch_extra -> [B, C, Ho, Wo] view."""
    b, h, w, c = g.shape
    buf = torch.full((b, h, w, c + pitch_extra), SENTINEL, dtype=torch.float32, device=DEV)
    buf[..., at:at + c] = _t(g)
    return buf[..., at:at + c].permute(0, 3, 1, 2)


_PAD_L, _PAD_R, _PAD_ROWS, _TAIL = 8, 12, 3, 64


def _adjoint(g, c, i, max_blocks=0, samples=slice(None), pitched=True):
    """ops.upconv_adjoint of source i of case c on g [B, Ho, Wo, C] (host) -> G [B, Hs, Ws, 3, 3, C] on the host.  pitched: g
    read from a pitched view, G written into a view of a wider and taller sentinel matrix, the scratch with a sentinel tail;
    everything around the results must survive."""
    hs, ws = c.sizes[i]
    g = np.asarray(g)[samples]
    b = g.shape[0]
    rows, width = b * hs * ws, 9 * c.c
    if not pitched:
        out = ops.upconv_adjoint(_t(g).permute(0, 3, 1, 2), hs, ws, max_blocks)
        return out.cpu().numpy().reshape(b, hs, ws, 3, 3, c.c)
    buf = torch.full((rows + _PAD_ROWS, _PAD_L + width + _PAD_R), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[:rows, _PAD_L:_PAD_L + width]
    n_s = b * 3 * hs * c.wo * c.c
    sbuf = torch.full((n_s + _TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
    got = ops.upconv_adjoint(_g_view(g), hs, ws, max_blocks, out=view, scratch=sbuf[:n_s].view(b, 3, hs, c.wo, c.c))
    assert got is view
    assert bool((buf[:, :_PAD_L] == SENTINEL).all()) and bool((buf[:, _PAD_L + width:] == SENTINEL).all()), "columns next to G were written"
    assert bool((buf[rows:] == SENTINEL).all()), "rows past G were written"
    assert bool((sbuf[n_s:] == SENTINEL).all()), "floats past the y adjoint's scratch were written"
    return view.cpu().numpy().reshape(b, hs, ws, 3, 3, c.c)


@pytest.mark.parametrize("name", cases.PASS_CASES)
def test_adjoint_kernels_against_float64(name):
    """Every source of the case: inside the bound of G; bit for bit on the exact twins; nothing written outside the results; a
    second call and the dense layout give the same bits."""
    c = cases.case(name)
    for i in range(len(c.sizes)):
        got = _adjoint(c.g, c, i)
        _check("%s source %d G" % (name, i), got, c.gz[i], c.gz_bound[i])
        if name in cases.EXACT_CASES:
            assert np.array_equal(got.astype(np.float64), c.gz[i]), "exact twin: not bit for bit"
        assert np.array_equal(got, _adjoint(c.g, c, i)), "a second call gave other bits"
        assert np.array_equal(got, _adjoint(c.g, c, i, pitched=False)), "the dense layout gave other bits"


@pytest.mark.parametrize("name", cases.PASS_CASES)
def test_adjoint_of_a_sample_alone_equals_the_sample_in_its_batch(name):
    c = cases.case(name)
    for i in range(len(c.sizes)):
        whole = _adjoint(c.g, c, i, pitched=False)
        for b in sorted({0, c.b - 1}):
            assert np.array_equal(_adjoint(c.g, c, i, samples=slice(b, b + 1), pitched=False), whole[b:b + 1]), (name, i, b)


@pytest.mark.parametrize("name", cases.PASS_CASES)
def test_adjoint_under_a_block_cap_gives_the_same_bits(name):
    """One block and three blocks of 256 threads: with more than 256 (768) float4 elements a block's grid-stride loop runs its
    second trip -- the same bits as the uncapped launch (which cases have that many in both launches:
    tests/test_host_upconv_bwd.py)."""
    c = cases.case(name)
    for i in range(len(c.sizes)):
        free = _adjoint(c.g, c, i, pitched=False)
        for cap in (1, 3):
            assert np.array_equal(_adjoint(c.g, c, i, max_blocks=cap, pitched=False), free), (name, i, cap)


@pytest.mark.parametrize("name", cases.DYADIC_CASES)
def test_one_inf_in_g_makes_the_restatement_s_elements_non_finite(name):
    """Every dyadic pass geometry, the degenerate ones included (ws1: n_src = 1, the window is the whole axis; all_one and the
    last source index: step = 0, both selects take the same value): the non-finite elements are those of the float32
    restatement and of the forward stencil; on the exact twins every other element keeps its bits."""
    c = cases.case(name)
    for pixel in cases.inf_pixels(name):
        g = np.array(c.g)
        g[pixel] = np.inf
        want = cases.upconv_adjoint_ref(g, c.sizes, np.float32)
        masks = cases.stencil_mask(c.sizes, g.shape, pixel)
        for i in range(len(c.sizes)):
            got = _adjoint(g, c, i)
            assert np.array_equal(~np.isfinite(got), ~np.isfinite(want[i])), (name, pixel, i)
            assert np.array_equal(~np.isfinite(got), masks[i]), (name, pixel, i)
            if name in cases.EXACT_CASES:
                assert np.array_equal(got[masks[i] == 0].astype(np.float64), c.gz[i][masks[i] == 0]), (name, pixel, i)


def test_adjoint_refusals_leave_the_output_alone():
    c = cases.case("fused_3to9_dyadic")
    hs, ws = c.sizes[0]
    g = _t(c.g).permute(0, 3, 1, 2)
    out = torch.full((c.b * hs * ws, 9 * c.c), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="expected a tensor in GPU memory"):
        ops.upconv_adjoint(g.cpu(), hs, ws, out=out)
    with pytest.raises(RuntimeError, match="channels-last"):
        ops.upconv_adjoint(g.contiguous(), hs, ws, out=out)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.upconv_adjoint(g, hs, ws, out=out[:, :-4])
    with pytest.raises(RuntimeError, match="scratch must be"):
        ops.upconv_adjoint(g, hs, ws, out=out, scratch=torch.empty(5, device=DEV))
    with pytest.raises(RuntimeError, match="upconv_bwd_ypass: bad sizes"):
        ops.upconv_adjoint(g, hs, ws, max_blocks=-1, out=out)
    g6 = torch.zeros((1, 9, 9, 6), device=DEV).permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError, match="upconv_bwd_ypass: bad sizes"):
        ops.upconv_adjoint(g6, hs, ws)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------
# the whole op
# ------------------------------------------------------------------------------------------
def _op_inputs(c, layout="nchw"):
    f = c.fwd
    conv_a = _t(f.conv_a).permute(0, 3, 1, 2)
    xs = [_t(x).permute(0, 3, 1, 2) for x in f.x]
    if layout == "nchw":
        conv_a, xs = conv_a.contiguous(), [x.contiguous() for x in xs]
    ws = [_t(w) for w in f.w]
    return conv_a, xs, ws


class _Spy:
    def __init__(self, monkeypatch):
        self.seen = {"adjoint": 0, "dx": 0, "dw": 0, "mm": 0}
        for key, owner, attr in (("adjoint", ops, "upconv_adjoint"), ("dx", ops, "_upconv_dx"), ("dw", ops, "_upconv_dw"), ("mm", torch, "mm")):
            monkeypatch.setattr(owner, attr, self._counted(key, getattr(owner, attr)))

    def _counted(self, key, fn):
        def call(*a, **kw):
            self.seen[key] += 1
            return fn(*a, **kw)
        return call


@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("name", cases.TF_CASES)
def test_upconv3x3_train_forward_and_backward(name, layout, monkeypatch):
    c = cases.case(name)
    f = c.fwd
    conv_a, xs, ws = _op_inputs(c, layout)
    leaves = [t.requires_grad_() for t in [conv_a] + xs + ws]
    spy = _Spy(monkeypatch)
    out = ops.upconv3x3_train(conv_a, list(zip(xs, ws)))
    assert tuple(out.shape) == (f.b, f.c, f.ho, f.wo) and spy.seen == {"adjoint": 0, "dx": 0, "dw": 0, "mm": 0}
    # the forward is ops.upconv3x3 on the same operands, bit for bit
    a_cl, x_cl, _ = _op_inputs(c, "cl")
    twin = ops.upconv3x3(a_cl.clone(memory_format=torch.preserve_format), torch.zeros(f.c, device=DEV),
                         [(x, ops.upconv_tap_weights(w.detach(), 0, f.cin)) for x, w in zip(x_cl, ws)], 0)
    assert torch.equal(out.detach(), twin), "the forward differs from ops.upconv3x3"
    _check("%s %s forward" % (name, layout), out.permute(0, 2, 3, 1), util.upconv_want(name, 0) - f.bias, util.upconv_bound(name))
    g = _t(c.g).permute(0, 3, 1, 2)
    if layout == "nchw":
        g = g.contiguous()
    out.backward(g)
    assert spy.seen == {"adjoint": len(xs), "dx": len(xs), "dw": len(xs), "mm": 2 * len(xs)}, spy.seen
    assert torch.equal(leaves[0].grad, g), "grad conv_a is not g"
    for i in range(len(xs)):
        _check("%s %s source %d dX" % (name, layout, i), xs[i].grad.permute(0, 2, 3, 1), c.dx[i], c.dx_bound[i])
        _check("%s %s source %d dW" % (name, layout, i), ws[i].grad, cases.fold_weight(c.dnk[i], f.c, f.cin),
               cases.fold_weight(c.dnk_bound[i], f.c, f.cin))


@pytest.mark.parametrize("frozen", ["weights", "inputs", "source0", "all"])
def test_upconv3x3_train_skips_what_nobody_needs(frozen, monkeypatch):
    c = cases.case("tf_random")
    f = c.fwd
    conv_a, xs, ws = _op_inputs(c)
    n = len(xs)
    need_x = [frozen not in ("inputs", "all") and not (frozen == "source0" and i == 0) for i in range(n)]
    need_w = [frozen not in ("weights", "all") and not (frozen == "source0" and i == 0) for i in range(n)]
    conv_a.requires_grad_()
    for i in range(n):
        xs[i].requires_grad_(need_x[i])
        ws[i].requires_grad_(need_w[i])
    spy = _Spy(monkeypatch)
    out = ops.upconv3x3_train(conv_a, list(zip(xs, ws)))
    out.backward(_t(c.g).permute(0, 3, 1, 2))
    want = {"adjoint": sum(a or b for a, b in zip(need_x, need_w)), "dx": sum(need_x), "dw": sum(need_w), "mm": sum(need_x) + sum(need_w)}
    assert spy.seen == want, (spy.seen, want)
    for i in range(n):
        assert (xs[i].grad is not None) == need_x[i] and (ws[i].grad is not None) == need_w[i]
        if need_x[i]:
            _check("frozen %s source %d dX" % (frozen, i), xs[i].grad.permute(0, 2, 3, 1), c.dx[i], c.dx_bound[i])
        if need_w[i]:
            _check("frozen %s source %d dW" % (frozen, i), ws[i].grad, cases.fold_weight(c.dnk[i], f.c, f.cin),
                   cases.fold_weight(c.dnk_bound[i], f.c, f.cin))
    assert conv_a.grad is not None


def test_upconv3x3_train_without_gradients_runs_the_forward_only(monkeypatch):
    c = cases.case("tf_fused_dyadic")
    conv_a, xs, ws = _op_inputs(c)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        out = ops.upconv3x3_train(conv_a, list(zip(xs, ws)))
    assert not out.requires_grad and spy.seen == {"adjoint": 0, "dx": 0, "dw": 0, "mm": 0}
    assert np.array_equal(out.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64), util.upconv_want("tf_fused_dyadic", 0) - c.fwd.bias)


def test_upconv3x3_train_refusals_leave_the_inputs_alone():
    c = cases.case("tf_fused_dyadic")
    conv_a, xs, ws = _op_inputs(c)
    before = conv_a.clone()
    with pytest.raises(RuntimeError, match="expected a tensor in GPU memory"):
        ops.upconv3x3_train(conv_a.cpu(), list(zip(xs, ws)))
    with pytest.raises(RuntimeError, match="expected a tensor in GPU memory"):
        ops.upconv3x3_train(conv_a, [(xs[0].cpu(), ws[0])])
    with pytest.raises(RuntimeError, match="want float32 \\[2,128,Hs,Ws\\]"):
        ops.upconv3x3_train(conv_a, [(xs[0][:, :64], ws[0])])
    with pytest.raises(RuntimeError, match="want float32 \\[2,128,Hs,Ws\\]"):
        ops.upconv3x3_train(conv_a, [(xs[0][:1], ws[0])])
    with pytest.raises(RuntimeError, match="want float32 \\[128,128,3,3\\]"):
        ops.upconv3x3_train(conv_a, [(xs[0], ws[0][:64])])
    with pytest.raises(RuntimeError, match="want float32 \\[128,128,3,3\\]"):
        ops.upconv3x3_train(conv_a, [(xs[0], ws[0][:, :, :1, :1])])
    with pytest.raises(RuntimeError, match="want float32 \\[128,128,3,3\\]"):
        ops.upconv3x3_train(conv_a, [(xs[0], ws[0].double())])
    with pytest.raises(RuntimeError, match="one or two upsampled sources"):
        ops.upconv3x3_train(conv_a, [])
    with pytest.raises(RuntimeError, match="output channels"):
        ops.upconv3x3_train(conv_a[:, :6], [(xs[0], ws[0][:6])])
    torch.cuda.synchronize()
    assert torch.equal(conv_a, before)


def test_the_switch_follows_the_setter_then_the_environment(monkeypatch):
    monkeypatch.delenv("SMOS_CONV1_TRAIN", raising=False)
    prev = ops.set_conv1_fused(None)
    try:
        assert ops.conv1_fused() is False
        monkeypatch.setenv("SMOS_CONV1_TRAIN", "1")
        assert ops.conv1_fused() is True
        assert ops.set_conv1_fused(False) is None and ops.conv1_fused() is False
        monkeypatch.setenv("SMOS_CONV1_TRAIN", "0")
        assert ops.set_conv1_fused(True) is False and ops.conv1_fused() is True
        assert ops.set_conv1_fused(None) is True and ops.conv1_fused() is False
    finally:
        ops.set_conv1_fused(prev)

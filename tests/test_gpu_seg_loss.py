"""ops.seg_loss (csrc/seg_loss.hip) on the GPU against the float64 reference of tests/loss_cases.py: the value and every
gradient element inside the derived bounds (derivation there), through ops.seg_loss, the C entry points and
AttNet._seg_loss.  Every check prints its worst error / bound (pytest -s); the figures of the MI355X run are kept in
profiles/seg_loss_error_ratios.txt.
"""
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, engine, ops
from streammos_amd.refapi.config import StreamMOS as cfg
from streammos_amd.refapi.models import StreamMOS, losses
from tests import loss_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("contiguous", "point_major", "slice", "point_major_slice")

RATIOS = []
RATIO_FILE = os.path.join(ROOT, "profiles", "seg_loss_error_ratios.txt")
RATIO_HEADER = """Fused training loss (csrc/seg_loss.hip, ops.seg_loss) against the float64 reference: worst error / bound per check.
Written by tests/test_gpu_seg_loss.py when the whole file has run.

Each line: |value - reference| / value bound, then the largest |gradient element - reference| / its bound over EVERY
element (tests/loss_cases.py: derived, not tuned; where a bound is 0 the result has to be exact).  A gradient ratio
near 1 is an element whose sort key is closer to a neighbour's than float32 resolves: the two come out in the other
order than in float64 and the element takes the neighbour's coefficient, which the bound allows for exactly.

Value-only mutants of the kernels (diagnostic builds, one per run of this file on the MI355X; 61 tests):
  the coefficient of the first sorted element dropped (the i = 0 convention): 55 fail.  Pass: the tile / workspace test,
      shapes 1x3x1, 1x3x2, 2x3x1 (no class present, or the first element's share below the bound), all_ignored, the
      two-runs test (it compares runs, not values).
  the foreground carry into every tile after the first off by one: 17 fail, every case with more than one tile and foreground
      behind the first: shapes 1xCx6149, 2xCx6149, 2xCx2047, 2x3x2048, 2x3x2049, top-k 2047 / 2048 / 2049, last_tile_fg,
      ignored_border, equal, the C entry, the NaN run, the no-sync run.
  ignored positions given a real key, so that they count into the union: 50 fail.  Pass: the tile / workspace test, six
      shapes with P <= 2, all_ignored, last_tile_fg (no ignored position), equal (all foreground sorts first: the union of
      the foreground prefix does not see them), the two-runs test.
"""


def _pred(case, layout):
    """case.pred [B, C, P, 1] on the device in one of the layouts the kernel reads through strides; the slices sit inside a
    wider buffer of NaN, which a read outside the tensor would bring in."""
    g = torch.from_numpy(case.pred.copy()).to(DEV)
    b, c, p = case.b, case.c, case.p
    if layout == "contiguous":
        return g
    if layout == "point_major":                                  # the point head's [B, P, C]-backed view
        return g[..., 0].permute(0, 2, 1).contiguous().permute(0, 2, 1).unsqueeze(-1)
    if layout == "slice":
        wide = torch.full((b, c + 2, p + 3), float("nan"), device=DEV)
        view = wide[:, 1:1 + c, 2:2 + p]
    else:
        wide = torch.full((b, p + 2, c + 3), float("nan"), device=DEV)
        view = wide[:, 1:1 + p, 2:2 + c].permute(0, 2, 1)
    view.copy_(g[..., 0])
    return view.unsqueeze(-1)


def _target(case):
    return torch.from_numpy(case.target.copy()).to(DEV)


def _run(case, layout="contiguous", grad_out=None):
    pred = _pred(case, layout).detach().requires_grad_()
    loss = ops.seg_loss(pred, _target(case), ignore_index=case.ignore_index)
    assert loss.shape == () and loss.is_cuda and loss.dtype == torch.float32
    if grad_out is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_out, device=DEV))
    assert pred.grad.shape == pred.shape
    return loss.detach(), pred.grad


def _check(label, value, grad, ref, scale=1.0):
    ok, rv, rg = cases.worst_ratio(value.item() / scale, cases.grad_rows(grad.cpu().numpy()) / scale, ref)
    print("seg-loss-ratio %-44s value %.4f gradient %.4f" % (label, rv, rg))
    RATIOS.append((label, rv, rg))
    assert ok, "%s: worst error / bound: value %g, gradient %g" % (label, rv, rg)


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    """profiles/seg_loss_error_ratios.txt from this run, once every test of the file has run (not for a -k selection)."""
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 80 or len(ran) < 60:
        return
    worst_v, worst_g = max(RATIOS, key=lambda r: r[1]), max(RATIOS, key=lambda r: r[2])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  %d checks; the largest value ratio %.4f (%s), the largest gradient ratio %.4f (%s).\n\n" % (
                torch.cuda.get_device_name(0), len(RATIOS), worst_v[1], worst_v[0], worst_g[2], worst_g[0]))
            f.writelines("%-48s %.4f %.4f\n" % r for r in RATIOS)
    except OSError:
        pass                                   # a read-only checkout: the figures were printed


def test_tile_and_workspace_size():
    assert ops.seg_loss_tile() == cases.TILE
    lib = _lib.load()
    n = 4 * 130000
    assert lib.smos_seg_loss_work_bytes(n, 3) >= 2 * 4 * n * 12                       # keys and payloads, in and out
    assert lib.smos_seg_loss_work_bytes(n, 2) < lib.smos_seg_loss_work_bytes(n, 3)


@pytest.mark.parametrize("p", cases.SHAPE_P)
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("c", [2, 3])
def test_shapes_against_float64_reference(c, b, p):
    case = cases.shape_case(b, c, p)
    for layout in LAYOUTS:
        value, grad = _run(case, layout)
        _check("%s %s" % (case.name, layout), value, grad, case.ref)
        if layout == "point_major":
            assert grad[..., 0].permute(0, 2, 1).is_contiguous()                       # laid out like pred


@pytest.mark.parametrize("k", list(cases.TOPK_N))
def test_topk_sizes_around_the_tile(k):
    case = cases.topk_case(k)
    value, grad = _run(case)
    _check(case.name, value, grad, case.ref)


@pytest.mark.parametrize("name", list(cases.STEERED))
def test_steered_labels_and_logits(name):
    case = cases.steered_case(name)
    for layout in ("contiguous", "point_major"):
        value, grad = _run(case, layout)
        _check("%s %s" % (case.name, layout), value, grad, case.ref)
        if name == "all_ignored":
            assert value.item() == 0.0 and (grad == 0).all() and not torch.isnan(grad).any()
        if name in ("equal", "equal_c2", "pm200", "pm200_c2"):
            # every sorted value is exact here, so the order is the position order and nothing but the roundings of
            # the backward separates the kernel from float64
            assert not case.ref.top_open.any()


def test_upstream_gradient_scales_the_result():
    case = cases.steered_case("three_present")
    value, grad = _run(case, "point_major", grad_out=0.25)                              # a power of two: the same roundings
    _check("three_present grad_out=0.25", value, grad * 4.0, case.ref)


def test_c_entry_points_write_through_the_strides_of_a_slice():
    """grad with the strides of pred, both slices of wider NaN buffers: the surround keeps its NaN."""
    lib = _lib.load()
    for name, layout in (("three_present", "slice"), ("ignored_border", "point_major_slice")):
        case = cases.steered_case(name)
        b, c, p, n = case.b, case.c, case.p, case.n
        pred = _pred(case, layout)[..., 0]
        if layout == "slice":
            wide = torch.full((b, c + 2, p + 3), float("nan"), device=DEV)
            view = lambda t: t[:, 1:1 + c, 2:2 + p]
        else:
            wide = torch.full((b, p + 2, c + 3), float("nan"), device=DEV)
            view = lambda t: t[:, 1:1 + p, 2:2 + c].permute(0, 2, 1)
        grad = view(wide)
        assert grad.stride() == pred.stride()
        tgt = _target(case).reshape(b, p)
        need = lib.smos_seg_loss_work_bytes(n, c)
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        coef = torch.full((c + 1, n), float("nan"), device=DEV)
        loss, stats, go = torch.empty(1, device=DEV), torch.empty(2, device=DEV), torch.ones(1, device=DEV)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.smos_seg_loss_fwd(pred.data_ptr(), _lib.i64_array(pred.stride()), tgt.data_ptr(), b, c, p, case.k, 4.0, 3.0,
                                         case.ignore_index, coef.data_ptr(), loss.data_ptr(), stats.data_ptr(), work.data_ptr(), need, st),
                   "smos_seg_loss_fwd")
        _lib.check(lib.smos_seg_loss_bwd(pred.data_ptr(), _lib.i64_array(pred.stride()), tgt.data_ptr(), coef.data_ptr(),
                                         stats.data_ptr(), go.data_ptr(), b, c, p, case.k, 4.0, 3.0, case.ignore_index, grad.data_ptr(),
                                         _lib.i64_array(grad.stride()), st), "smos_seg_loss_bwd")
        _check("%s C entry %s" % (name, layout), loss[0], grad.unsqueeze(-1), case.ref)
        assert not torch.isnan(coef).any() and stats[1].item() == len(case.ref.present)
        top = coef[c].bool().cpu().numpy()
        assert top.sum() == case.k and (top == case.ref.top)[~case.ref.top_open].all()
        mask = torch.ones_like(wide, dtype=torch.bool)
        view(mask).fill_(False)
        assert torch.isnan(wide[mask]).all()
        with pytest.raises(RuntimeError, match="workspace"):
            _lib.check(lib.smos_seg_loss_fwd(pred.data_ptr(), _lib.i64_array(pred.stride()), tgt.data_ptr(), b, c, p, case.k, 4.0, 3.0,
                                             case.ignore_index, coef.data_ptr(), loss.data_ptr(), stats.data_ptr(), work.data_ptr(),
                                             need - 1, st), "smos_seg_loss_fwd")


def test_one_nan_logit_gives_a_nan_loss_and_the_call_returns():
    case = cases.shape_case(2, 3, cases.TILE + 1)
    pred = torch.from_numpy(case.pred.copy())
    q = int(np.flatnonzero(case.ref.valid)[7])
    pred[q // case.p, 2, q % case.p, 0] = float("nan")
    pred = pred.to(DEV).requires_grad_()
    loss = ops.seg_loss(pred, _target(case))
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isnan(loss).item()
    rows = cases.grad_rows(pred.grad.cpu().numpy())
    assert np.isnan(rows[q]).all() and not rows[~case.ref.valid].any()
    # at an ignored position it changes nothing, as with the torch formulation
    pred2 = torch.from_numpy(case.pred.copy())
    q = int(np.flatnonzero(~case.ref.valid)[3])
    pred2[q // case.p, 0, q % case.p, 0] = float("nan")
    pred2 = pred2.to(DEV).requires_grad_()
    loss2 = ops.seg_loss(pred2, _target(case))
    loss2.backward()
    _check("NaN at an ignored position", loss2.detach(), pred2.grad, case.ref)


def test_two_runs_are_bit_identical():
    for case in (cases.shape_case(2, 3, 3 * cases.TILE + 5), cases.steered_case("equal_c2"), cases.steered_case("ce_ties")):
        v1, g1 = _run(case, "point_major")
        v2, g2 = _run(case, "point_major")
        assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))


def test_golden_losses_through_the_gpu_path():
    """Value: the bars of test_training_losses_match_reference_golden on ohem + 3 * lovasz.  Gradient: the golden one is the
    reference implementation's float32 and lies outside rtol = 1e-5, atol = 1e-8 of float64 itself
    (tests/test_host_seg_loss.py prints by how much), so each element may differ from it by |ref64 - golden| + the bound."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "losses.npz"))
    ref = cases.reference(g["pred"], g["gt"])
    pred = torch.from_numpy(g["pred"]).to(DEV).requires_grad_()
    loss = ops.seg_loss(pred, torch.from_numpy(g["gt"]).to(DEV))
    loss.backward()
    want = float(g["ohem"]) + 3.0 * float(g["lovasz"])
    print("seg-loss-golden value |got - golden| = %.3g (bar %.3g)" % (abs(loss.item() - want), 1e-6 * abs(float(g["ohem"])) + 3e-6))
    assert abs(loss.item() - want) <= 1e-6 * abs(float(g["ohem"])) + 3e-6
    _check("golden", loss.detach(), pred.grad, ref)
    gold = cases.grad_rows(g["grad"]).astype(np.float64)
    got = cases.grad_rows(pred.grad.cpu().numpy()).astype(np.float64)
    assert (np.abs(got - gold) <= np.abs(ref.grad - gold) + ref.grad_bound).all()


def _model(own):
    model = StreamMOS.AttNet.__new__(StreamMOS.AttNet)           # _seg_loss needs the config and the switch, not the network
    engine.read_switches(model, engine.TRAIN_SWITCHES)
    model.pModel = cfg.get_config()[2]
    model.seg_loss_own = own
    return model


def test_seg_loss_method_with_the_switch_at_1_and_at_0(monkeypatch):
    case = cases.shape_case(2, 3, 65)
    calls = []
    own_fn = ops.seg_loss
    monkeypatch.setattr(ops, "seg_loss", lambda *a, **k: calls.append(1) or own_fn(*a, **k))
    tgt = _target(case)
    p1 = _pred(case, "point_major").detach().requires_grad_()
    v1 = _model(True)._seg_loss(p1, tgt)
    v1.backward()
    assert len(calls) == 1
    _check("_seg_loss switch 1", v1.detach(), p1.grad, case.ref)          # the gradient against float64, not against torch
    p0 = _pred(case, "point_major").detach().requires_grad_()
    v0 = _model(False)._seg_loss(p0, tgt)
    v0.backward()
    assert len(calls) == 1 and v0.grad_fn is not None
    # the torch path: float32 cumulative sums and a dot over n terms, n * u relative; the own path: its derived bound
    assert abs(v1.item() - v0.item()) <= case.ref.value_bound + case.n * cases.U * abs(case.ref.value)
    assert (p0.grad - p1.grad).abs().max().item() <= 1e-3 * p1.grad.abs().max().item()
    # what stays on the torch path whatever the switch: loss_mode "ce", CPU tensors
    model = _model(True)
    model.pModel = type("P", (), {"loss_mode": "ce"})
    model._seg_loss(p0.detach(), tgt)
    _model(True)._seg_loss(p0.detach().cpu(), tgt.cpu())
    assert len(calls) == 1
    # without a graph: the same value, no node
    with torch.no_grad():
        v = _model(True)._seg_loss(p1, tgt)
    assert v.grad_fn is None and torch.equal(v, v1.detach()) and len(calls) == 2


def test_loss_and_backward_do_not_wait_for_the_stream():
    """_seg_loss + backward return while the stream is still busy with work queued before them: nothing in either direction
    reads a device value on the host.  (The torch formulation blocks on its first ``.sum() == 0``.)"""
    case = cases.shape_case(2, 3, 3 * cases.TILE + 5)
    model, tgt = _model(True), _target(case)
    pred = _pred(case, "point_major").detach().requires_grad_()
    model._seg_loss(pred, tgt).backward()                                       # allocates the scratch, loads the code objects
    pred.grad = None
    a = torch.randn((8192, 8192), device=DEV)
    c = torch.empty_like(a)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(a, a, out=c)
    start.record()
    for _ in range(4):
        torch.mm(a, a, out=c)
    stop.record()
    stop.synchronize()
    reps = int(np.ceil(150.0 / (start.elapsed_time(stop) / 4)))                 # at least 100 ms of plain work, with a margin
    for _ in range(reps):
        torch.mm(a, a, out=c)
    busy = torch.cuda.Event()
    busy.record()
    loss = model._seg_loss(pred, tgt)
    loss.backward()
    waited = busy.query()
    torch.cuda.synchronize()
    assert not waited
    _check("no-sync run", loss.detach(), pred.grad, case.ref)


def test_refusals():
    case = cases.shape_case(1, 3, 64)
    pred, tgt = _pred(case, "contiguous"), _target(case)
    with pytest.raises(RuntimeError, match="classes"):
        ops.seg_loss(torch.zeros((1, 4, 64, 1), device=DEV), tgt)
    with pytest.raises(RuntimeError, match="float32"):
        ops.seg_loss(pred.half(), tgt)
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.seg_loss(pred.cpu(), tgt)
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.seg_loss(pred, tgt.cpu())
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.seg_loss(pred, tgt[:, :63])
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.seg_loss(pred[0], tgt)
    with pytest.raises(RuntimeError, match="integer"):
        ops.seg_loss(pred, tgt.float())
    # the reference functions keep their behaviour next to the fused one
    want = losses.ohem_cross_entropy(pred, tgt) + 3 * losses.lovasz_softmax(pred, tgt, ignore=0)
    assert abs(want.item() - ops.seg_loss(pred, tgt).item()) <= 1e-5 * abs(want.item())

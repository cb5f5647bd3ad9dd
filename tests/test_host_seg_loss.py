"""The fused training loss without a GPU: the float64 reference of tests/loss_cases.py against the golden loss values and
against torch's CPU autograd of refapi/models/losses.py, the closed-form Lovasz coefficients against ``_lovasz_grad``, the
float32 restatement of the kernels against the derived bounds, the sort-key mapping, the C ABI and the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, engine, ops
from streammos_amd.refapi.models import losses
from tests import loss_cases as cases
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "losses.npz"))


def test_reference_meets_the_golden_bars_for_both_values():
    """The bars of test_training_losses_match_reference_golden (tests/test_host_cpu.py)."""
    g = _golden()
    ref = cases.reference(g["pred"], g["gt"])
    print("seg-loss-golden ohem |ref64 - golden| / golden = %.3g, lovasz |ref64 - golden| = %.3g"
          % (abs(ref.ohem - float(g["ohem"])) / abs(float(g["ohem"])), abs(ref.lovasz - float(g["lovasz"]))))
    assert abs(ref.ohem - float(g["ohem"])) <= 1e-6 * abs(float(g["ohem"]))
    assert abs(ref.lovasz - float(g["lovasz"])) <= 1e-6


def test_distance_of_the_reference_to_the_golden_gradient_is_recorded():
    """The golden gradient is the reference implementation's own float32: it sits outside rtol = 1e-5, atol = 1e-8 of float64
    (the figure is printed: the worst element at 1.61 times that bar, 1.7e-6 of the largest element; the two values differ by
    3.8e-8 relative and 4.3e-8), so the GPU test allows |ref64 - golden| + the derived bound per element instead of that bar.
    What is asserted here is that the distance is a float32 artefact: small against the largest element."""
    g = _golden()
    ref = cases.reference(g["pred"], g["gt"])
    gold = cases.grad_rows(g["grad"]).astype(np.float64)
    dist = np.abs(ref.grad - gold)
    bar = 1e-8 + 1e-5 * np.abs(gold)
    print("seg-loss-golden gradient: worst |ref64 - golden| / (atol + rtol |golden|) = %.3f, worst / largest element = %.3g"
          % ((dist / bar).max(), dist.max() / np.abs(gold).max()))
    assert dist.max() <= 1e-5 * np.abs(gold).max()
    assert ((gold == 0) == (ref.grad == 0)).all()               # the ignored positions, and only they


def _lovasz_softmax_any_dtype(logits, labels, ignore):
    """losses.lovasz_softmax with the foreground flags in the logits' dtype (the module says ``.float()``, which ties it to
    float32): the same steps, the same ``_lovasz_grad``."""
    prob = torch.softmax(logits, dim=1)
    c = prob.shape[1]
    prob = prob.permute(0, 2, 3, 1).reshape(-1, c)
    lab = labels.reshape(-1)
    keep = lab != ignore
    prob, lab = prob[keep], lab[keep]
    out = []
    for cls in range(c):
        fg = (lab == cls).to(prob.dtype)
        if fg.sum() == 0:
            continue
        err_sorted, perm = torch.sort((fg - prob[:, cls]).abs(), dim=0, descending=True, stable=True)
        out.append(torch.dot(err_sorted, losses._lovasz_grad(fg[perm])))
    return sum(out) / len(out)


@pytest.mark.parametrize("name", ["three_present", "absent", "one_valid", "ce_ties", "ignored_border"])
def test_reference_matches_torch_cpu_autograd_in_float64(name):
    case = cases.steered_case(name)
    pred = torch.tensor(case.pred.astype(np.float64), requires_grad=True)
    gt = torch.tensor(case.target)
    a = losses.ohem_cross_entropy(pred, gt, top_ratio=0.2, top_weight=4.0, ignore_index=case.ignore_index)
    b = _lovasz_softmax_any_dtype(pred, gt, case.ignore_index)
    if name == "three_present":                  # float32, through the module itself: the same quantity
        b32 = losses.lovasz_softmax(pred.detach().float(), gt, ignore=case.ignore_index)
        assert abs(float(b32) - case.ref.lovasz) <= 1e-5
    assert abs(a.detach().item() - case.ref.ohem) <= 1e-12 * max(abs(a.detach().item()), 1.0)
    assert abs(b.detach().item() - case.ref.lovasz) <= 1e-12
    grad = cases.grad_rows(torch.autograd.grad(a + 3 * b, pred)[0].numpy())
    # torch's top-k may pick another member of a tie at the k boundary, and its jac[1:] - jac[:-1] still cancels in
    # float64 (about 1e-16 / d relative): compare where the top-k flag is settled
    settled = ~case.ref.top_open
    if name == "ce_ties":
        settled &= case.ref.ce != np.sort(case.ref.ce)[::-1][case.k - 1]
        assert (~settled).sum() > 1
    assert np.abs(grad - case.ref.grad)[settled].max() <= 1e-9 * np.abs(case.ref.grad).max()


def test_closed_form_equals_lovasz_grad_in_float64():
    rng = np.random.default_rng(5)
    for n, frac in ((1, 1.0), (1, 0.0), (2, 0.5), (7, 0.3), (500, 0.02), (500, 0.98), (4099, 0.5)):
        fg = (rng.random(n) < frac).astype(np.float64)
        if frac in (0.0, 1.0):
            fg[:] = frac
        want = losses._lovasz_grad(torch.from_numpy(fg)).numpy()
        got = cases.closed_form(fg)
        if fg.sum() == 0:
            assert not got.any()                                 # an absent class: the kernel writes zeros, the formula is 0 / 0
            continue
        assert np.abs(got - want).max() <= 4e-16 * n, (n, frac)
        assert got[0] == (1.0 / fg.sum() if fg[0] else 1.0 / (fg.sum() + 1.0))        # i = 0: I_{-1} = U_{-1} = G


def test_sort_key_is_order_preserving_and_stays_inside_its_segment():
    rng = np.random.default_rng(6)
    v = np.concatenate((rng.random(2000), [0.0, 1.0, 2.0 ** -149, 2.0 ** -126, 1.0 - 2.0 ** -24])).astype(np.float32)
    key = cases.sort_key(v, cases.ONE_BITS)
    order = np.argsort(v, kind="stable")
    assert (np.diff(key[order].astype(np.int64)) <= 0).all()                          # larger value, smaller key
    assert ((np.diff(key[order].astype(np.int64)) == 0) == (np.diff(v[order]) == 0)).all()        # equal keys only for equal values
    assert np.array_equal(cases.key_value(key, cases.ONE_BITS), v)
    big = np.array([0.0, 1e-30, 1.0, 399.5, 3e38, np.inf], dtype=np.float32)
    kb = cases.sort_key(big, cases.INF_BITS)
    assert (np.diff(kb.astype(np.int64)) < 0).all() and np.array_equal(cases.key_value(kb, cases.INF_BITS), big)
    # NaN, Inf, negative zero and values above the segment's top: clamped to the segment's first key, never outside [0, top]
    odd = np.array([np.nan, -np.nan, np.inf, -np.inf, 7.0, -0.0], dtype=np.float32)
    assert cases.sort_key(odd, cases.ONE_BITS).tolist() == [0, 0, 0, 0, 0, cases.ONE_BITS]
    assert cases.sort_key(odd[:4], cases.INF_BITS).tolist() == [0, 0, 0, 0]
    assert cases.ONE_BITS + 1 < 2 ** 31 and cases.INF_BITS < 2 ** 31                  # an ignored key and every CE key fit the field
    # a NaN logit: every segment of the restated key array still holds exactly its n keys (asserted inside restate_f32)
    case = cases.shape_case(2, 3, 65)
    pred = case.pred.copy()
    valid = np.flatnonzero(case.ref.valid)[3]
    pred[valid // 65, 1, valid % 65, 0] = np.nan
    value, grad, keys = cases.restate_f32(pred, case.target)
    assert np.isnan(value) and ((keys >> np.uint64(31)) == np.arange(4, dtype=np.uint64)[:, None]).all()


def test_float32_restatement_stays_inside_the_derived_bounds_on_every_case():
    worst = (0.0, 0.0)
    for case in cases.all_cases():
        value, grad, _ = cases.restate_f32(case.pred, case.target, ignore_index=case.ignore_index)
        ok, rv, rg = cases.worst_ratio(value, grad, case.ref)
        print("seg-loss-restated %-28s value %.4f gradient %.4f" % (case.name, rv, rg))
        assert ok, (case.name, rv, rg)
        worst = (max(worst[0], rv), max(worst[1], rg))
        if case.labels == "all_ignored":
            assert value == 0 and not grad.any()
    assert worst[0] > 0.001 and worst[1] > 0.001                 # the bounds are not so wide that they bind nothing


def test_bounds_bind_a_wrong_coefficient():
    """The three value mutations of the scan, applied to the restatement: each leaves the bounds on some case."""
    case = cases.steered_case("three_present")
    _, grad, _ = cases.restate_f32(case.pred, case.target, ignore_index=255)
    lim = case.ref.grad_bound
    assert (np.abs(grad - case.ref.grad) <= lim).all()
    ref0 = cases.reference(case.pred, case.target, ignore_index=255)
    # a coefficient table shifted by one rank moves single elements far outside their bound
    shifted = np.roll(ref0.grad, 1, axis=0)
    assert (np.abs(shifted - case.ref.grad) > lim).any()
    # ignored positions counted into the union: the reference with nothing ignored differs by more than the value bound
    with_ignored = cases.reference(case.pred, np.where(case.target == 255, 0, case.target), ignore_index=255)
    assert abs(with_ignored.value - case.ref.value) > case.ref.value_bound


def test_cases_cover_what_they_are_named_for():
    t = cases.TILE
    assert cases.steered_case("all_ignored").ref.value == 0 and not cases.steered_case("all_ignored").ref.valid.any()
    assert cases.steered_case("one_valid").ref.valid.sum() == 1 and cases.steered_case("one_valid_c2").ref.valid.sum() == 1
    assert cases.steered_case("three_present").ref.present == [0, 1, 2] and cases.steered_case("absent").ref.present == [0, 2]
    assert cases.shape_case(2, 3, 65).ref.present == [1, 2]                           # ignore_index 0: class 0 is never present
    last = cases.steered_case("last_tile_fg")
    fgc = 2
    err = np.abs((last.target.reshape(-1) == fgc) - last.ref.p[:, fgc])
    rank = np.argsort(np.argsort(-err, kind="stable"), kind="stable")
    assert rank[last.target.reshape(-1) == fgc].min() >= (last.n // t) * t and last.n % t
    border = cases.steered_case("ignored_border")
    assert border.ref.valid.sum() == t + 1 and not border.ref.valid[t - 20:t + 21].any()
    eq = cases.steered_case("equal")
    assert len(np.unique(eq.ref.p)) == 1 and not eq.ref.top_open.any()
    # C = 2, p = 0.5: foreground and background tie, so the coefficients follow the position order
    assert len(np.unique(cases.steered_case("equal_c2").ref.coef[1])) > 100
    pm = cases.steered_case("pm200")
    assert set(np.unique(pm.ref.p.astype(np.float32))) == {0.0, 1.0} and set(np.unique(pm.ref.ce)) == {0.0, 400.0}
    ties = cases.steered_case("ce_ties")
    srt = np.sort(ties.ref.ce)[::-1]
    assert srt[ties.k - 1] == srt[ties.k] and not ties.ref.top_open.any()             # an exact tie across the boundary
    assert [cases.topk_case(k).k for k in cases.TOPK_N] == [1, t - 1, t, t + 1]


def test_header_declares_and_library_exports_the_loss():
    declared = util.header_declarations()
    lib = ctypes.CDLL(_lib.LIB_PATH)          # loads without a GPU; no compute call is made
    for name in ("smos_seg_loss_tile", "smos_seg_loss_work_bytes", "smos_seg_loss_fwd", "smos_seg_loss_bwd"):
        assert name in declared and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name]) == len(declared[name][1]), name
    assert lib.smos_seg_loss_tile() == cases.TILE
    lib.smos_seg_loss_work_bytes.restype = ctypes.c_int64
    lib.smos_seg_loss_work_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32]
    # (the size at the training shape is asked on the GPU: the sort library sizes its scratch for the device it finds)
    assert lib.smos_seg_loss_work_bytes(1, 2) >= 2 * 3 * 12 and lib.smos_seg_loss_work_bytes(5, 3) >= 2 * 4 * 5 * 12
    assert lib.smos_seg_loss_work_bytes(100, 4) == 0 and lib.smos_seg_loss_work_bytes(0, 3) == 0
    assert lib.smos_seg_loss_work_bytes(2 ** 28, 3) == 0                              # (C + 1) n past the sort's index range


def test_refusals_name_their_reason():
    pred, gt = torch.zeros((2, 3, 10, 1)), torch.ones((2, 10, 1), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.seg_loss(pred, gt)


def test_switch_is_in_the_training_table_and_cpu_keeps_the_torch_path(monkeypatch):
    assert [(a, v, d, k) for a, v, d, k in engine.TRAIN_SWITCHES] == [("seg_loss_own", "SMOS_SEG_LOSS", True, "bool")]
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS

    def built(value):
        if value is None:
            monkeypatch.delenv("SMOS_SEG_LOSS", raising=False)
        else:
            monkeypatch.setenv("SMOS_SEG_LOSS", value)
        model = StreamMOS.AttNet.__new__(StreamMOS.AttNet)
        engine.read_switches(model, engine.TRAIN_SWITCHES)
        return model
    assert built(None).seg_loss_own is True and built("1").seg_loss_own is True and built("0").seg_loss_own is False
    model = built(None)
    model.pModel = cfg.get_config()[2]
    assert model.pModel.loss_mode == "ohem"
    g = _golden()
    pred = torch.from_numpy(g["pred"])
    monkeypatch.setattr(ops, "seg_loss", lambda *a, **k: pytest.fail("a CPU tensor reached the device path"))
    got = StreamMOS.AttNet._seg_loss(model, pred, torch.from_numpy(g["gt"]))
    assert abs(got.item() - (float(g["ohem"]) + 3 * float(g["lovasz"]))) <= 1e-5

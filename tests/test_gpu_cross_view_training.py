"""The golden training steps of tests/golden/training.npz with the cross-view transfers on ops.gather_scatter_train
(ops.set_cross_view_fused): AttNet.forward on cases.training_batch() (three chained samples) against the reference's loss,
gradients and running buffers at the bars of tests/test_gpu_training.py.  Every sample runs _cross_view twice and every run
has two transfers: 12 calls of the op per step.  In stage 1 the op's backward feeds the whole trunk below it; in stage 2 the
trunk is frozen and the op is forward-only."""
import numpy as np
import pytest
import torch

from streammos_amd import ops, synth
from tests import cases
from tests.test_gpu_point_mlp_training import _check_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _count_calls(monkeypatch):
    calls, backwards = [], []
    real, real_bwd = ops.gather_scatter_train, ops.gather_scatter_train_backward
    monkeypatch.setattr(ops, "gather_scatter_train", lambda *a, **kw: (calls.append(kw.get("want_points", False)), real(*a, **kw))[1])
    monkeypatch.setattr(ops, "gather_scatter_train_backward", lambda *a, **kw: (backwards.append(a[7] is not None), real_bwd(*a, **kw))[1])
    return calls, backwards


def _stage1(golden, mode, monkeypatch, fused=True, others=False):
    import torch.nn.functional as F
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    from tests.util import check_inputs
    g = golden("training")
    nb = cases.training_batch()
    check_inputs(g, "train_in_sha", *[nb[k] for k in sorted(nb)])
    batch = {k: torch.from_numpy(v).to(DEV) for k, v in nb.items()}
    model = StreamMOS.AttNet(cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(DEV).train(mode == "train")
    calls, backwards = _count_calls(monkeypatch)
    if mode == "train":                          # dropout masks depend on the device's generator: removed on both sides
        monkeypatch.setattr(F, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
        if others:
            real_head = ops.point_head_train
            monkeypatch.setattr(ops, "point_head_train", lambda *a, **kw: real_head(*a, **dict(kw, p=0.0)))
    prev = ops.set_cross_view_fused(fused)
    prev_others = (ops.set_point_head_fused(True), ops.set_point_mlp_fused(True), ops.set_conv1_fused(True)) if others else None
    try:
        loss = model(batch)
        loss.backward()
    finally:
        ops.set_cross_view_fused(prev)
        if others:
            ops.set_point_head_fused(prev_others[0])
            ops.set_point_mlp_fused(prev_others[1])
            ops.set_conv1_fused(prev_others[2])
    return g, model, loss, calls, backwards


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_stage1_training_step_with_the_transfers_on_the_op_matches_reference_golden(golden, mode, monkeypatch):
    g, model, loss, calls, backwards = _stage1(golden, mode, monkeypatch)
    # per sample: x0's two transfers without point values, x1's way there without and its way back with them
    assert calls == [False, False, False, True] * 3
    assert len(backwards) == 12 and sum(backwards) == 3      # grad_pts only where the point values were handed on
    want = float(g["stage1_%s_loss" % mode])
    rel = abs(loss.item() - want) / abs(want)
    worst = _check_grads(g, "stage1_%s" % mode, model, cases.TRAINING_GRAD_KEYS, 2e-3 if mode == "eval" else 2e-2)
    print("stage 1 (%s, transfers on the op): loss %.6g vs %.6g (rel %.1e), worst gradient deviation %.1e" % (mode, loss.item(), want, rel, worst))
    assert rel <= 1e-4
    if mode == "train":
        sd = model.state_dict()
        for k in ("point_pre.layer.0.layer.2.running_mean", "bev_net.res2.1.layer.1.running_var", "bev_net.conv_1.bn.running_mean"):
            ref = g["stage1_train_bn_%s" % k]
            assert np.abs(sd[k].cpu().numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-6), k


def test_stage2_training_step_with_the_transfers_on_the_op_matches_reference_golden(golden, monkeypatch):
    """Everything but `refine.*` frozen, eval mode, gradients enabled: the transfers run on the op and its backward is never
    entered (no map needs a gradient)."""
    from streammos_amd.refapi.config import StreamMOS_seg as seg_cfg
    from streammos_amd.refapi.models import StreamMOS_seg
    g = golden("training")
    batch = {k: torch.from_numpy(v).to(DEV) for k, v in cases.training_batch().items()}
    model = StreamMOS_seg.AttNet(seg_cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    trainable = StreamMOS_seg.freeze_for_stage2(model)
    assert len(trainable) == 8
    model = model.to(DEV).eval()
    calls, backwards = _count_calls(monkeypatch)
    prev = ops.set_cross_view_fused(True)
    try:
        loss = model(batch)
        loss.backward()
    finally:
        ops.set_cross_view_fused(prev)
    assert len(calls) == 12 and not backwards
    with_grad = [k for k, p in model.named_parameters() if p.grad is not None]
    assert with_grad == [str(k) for k in g["stage2_params_with_grad"]]
    want = float(g["stage2_eval_loss"])
    rel = abs(loss.item() - want) / abs(want)
    worst = _check_grads(g, "stage2_eval", model, with_grad, 2e-3)
    print("stage 2 (transfers on the op): loss %.6g vs %.6g (rel %.1e), worst gradient deviation %.1e" % (loss.item(), want, rel, worst))
    assert rel <= 1e-4


def test_stage1_train_step_with_all_four_fused_switches_gives_the_same_loss(golden, monkeypatch):
    g, _, loss, calls, _ = _stage1(golden, "train", monkeypatch, others=True)
    assert len(calls) == 12
    want = float(g["stage1_train_loss"])
    assert abs(loss.item() - want) / abs(want) <= 1e-4


def test_with_the_switch_off_the_op_is_never_called(golden, monkeypatch):
    g, _, loss, calls, backwards = _stage1(golden, "eval", monkeypatch, fused=False)
    assert not calls and not backwards
    want = float(g["stage1_eval_loss"])
    assert abs(loss.item() - want) / abs(want) <= 1e-4

"""The golden training steps of tests/golden/training.npz with the fused point head switched on
(ops.set_point_head_fused): AttNet.forward on cases.training_batch() (three chained samples, 2 x 2048 points) against the
reference's loss, gradients and running buffers at the bars of tests/test_gpu_training.py.  In stage 1 the head's logits
feed the loss and its input gradients head the whole backward; in stage 2 the refine head is all that has a gradient."""
import numpy as np
import pytest
import torch

from streammos_amd import ops, synth
from tests import cases
from tests.test_gpu_point_mlp_training import _check_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _count_calls(monkeypatch, p=None):
    """counts the op's calls; with ``p`` the op is also made to run with that dropout probability"""
    calls = []
    real = ops.point_head_train

    def spy(*args, **kw):
        calls.append(1)
        if p is not None:
            kw["p"] = p
        return real(*args, **kw)
    monkeypatch.setattr(ops, "point_head_train", spy)
    return calls


def _stage1(golden, mode, monkeypatch, point_mlp=False):
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
    calls = _count_calls(monkeypatch, p=0.0 if mode == "train" else None)
    if mode == "train":                          # dropout masks depend on the device's generator: removed on both sides
        monkeypatch.setattr(F, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
    prev = ops.set_point_head_fused(True)
    prev_mlp = ops.set_point_mlp_fused(True) if point_mlp else None
    try:
        loss = model(batch)
        loss.backward()
    finally:
        ops.set_point_head_fused(prev)
        if point_mlp:
            ops.set_point_mlp_fused(prev_mlp)
    assert len(calls) == 3                       # one point head per chained sample, all on the op
    return g, model, loss


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_stage1_training_step_with_the_fused_point_head_matches_reference_golden(golden, mode, monkeypatch):
    g, model, loss = _stage1(golden, mode, monkeypatch)
    want = float(g["stage1_%s_loss" % mode])
    rel = abs(loss.item() - want) / abs(want)
    worst = _check_grads(g, "stage1_%s" % mode, model, cases.TRAINING_GRAD_KEYS, 2e-3 if mode == "eval" else 2e-2)
    print("stage 1 (%s, fused point head): loss %.6g vs %.6g (rel %.1e), worst gradient deviation %.1e" % (mode, loss.item(), want, rel, worst))
    assert rel <= 1e-4
    if mode == "train":
        sd = model.state_dict()
        for k in ("point_pre.layer.0.layer.2.running_mean", "bev_net.res2.1.layer.1.running_var", "bev_net.conv_1.bn.running_mean"):
            ref = g["stage1_train_bn_%s" % k]
            assert np.abs(sd[k].cpu().numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-6), k
        assert int(sd["point_post.merge_layer.1.num_batches_tracked"]) == 3
        assert int(sd["point_post.merge_layer.4.num_batches_tracked"]) == 3


def test_stage2_training_step_with_the_fused_point_head_matches_reference_golden(golden, monkeypatch):
    """Everything but `refine.*` frozen, eval mode: the refine head runs on the op (parameters need a gradient, inputs do
    not, so no input gradient is computed); the frozen first head needs none and stays on the modules."""
    from streammos_amd.refapi.config import StreamMOS_seg as seg_cfg
    from streammos_amd.refapi.models import StreamMOS_seg
    g = golden("training")
    batch = {k: torch.from_numpy(v).to(DEV) for k, v in cases.training_batch().items()}
    model = StreamMOS_seg.AttNet(seg_cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    trainable = StreamMOS_seg.freeze_for_stage2(model)
    assert len(trainable) == 8
    model = model.to(DEV).eval()
    calls = _count_calls(monkeypatch)
    prev = ops.set_point_head_fused(True)
    try:
        loss = model(batch)
        loss.backward()
    finally:
        ops.set_point_head_fused(prev)
    assert len(calls) == 3
    with_grad = [k for k, p in model.named_parameters() if p.grad is not None]
    assert with_grad == [str(k) for k in g["stage2_params_with_grad"]]
    want = float(g["stage2_eval_loss"])
    rel = abs(loss.item() - want) / abs(want)
    worst = _check_grads(g, "stage2_eval", model, with_grad, 2e-3)
    print("stage 2 (fused point head): loss %.6g vs %.6g (rel %.1e), worst gradient deviation %.1e" % (loss.item(), want, rel, worst))
    assert rel <= 1e-4


def test_stage1_train_step_with_both_fused_switches_gives_the_same_loss(golden, monkeypatch):
    g, _, loss = _stage1(golden, "train", monkeypatch, point_mlp=True)
    want = float(g["stage1_train_loss"])
    assert abs(loss.item() - want) / abs(want) <= 1e-4

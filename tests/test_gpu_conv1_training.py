"""The golden training steps of tests/golden/training.npz with the decoder's conv_1 on ops.upconv3x3_train
(ops.set_conv1_fused): AttNet.forward on cases.training_batch() (three chained samples) against the reference's loss,
gradients and running buffers at the bars of tests/test_gpu_training.py.  In stage 1 the op's backward feeds the whole
trunk below it (bev_net.conv_1.conv.weight and the auxiliary heads are among the checked gradients); in stage 2 the trunk
is frozen and the op is forward-only."""
import numpy as np
import pytest
import torch

from streammos_amd import ops, synth
from tests import cases
from tests.test_gpu_point_mlp_training import _check_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _count_calls(monkeypatch):
    calls = []
    real = ops.upconv3x3_train

    def spy(*args, **kw):
        calls.append(1)
        return real(*args, **kw)
    monkeypatch.setattr(ops, "upconv3x3_train", spy)
    return calls


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
    calls = _count_calls(monkeypatch)
    if mode == "train":                          # dropout masks depend on the device's generator: removed on both sides
        monkeypatch.setattr(F, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
        if others:
            real_head = ops.point_head_train
            monkeypatch.setattr(ops, "point_head_train", lambda *a, **kw: real_head(*a, **dict(kw, p=0.0)))
    prev = ops.set_conv1_fused(fused)
    prev_others = (ops.set_point_head_fused(True), ops.set_point_mlp_fused(True)) if others else None
    try:
        loss = model(batch)
        loss.backward()
    finally:
        ops.set_conv1_fused(prev)
        if others:
            ops.set_point_head_fused(prev_others[0])
            ops.set_point_mlp_fused(prev_others[1])
    return g, model, loss, calls


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_stage1_training_step_with_conv1_on_the_op_matches_reference_golden(golden, mode, monkeypatch):
    g, model, loss, calls = _stage1(golden, mode, monkeypatch)
    assert len(calls) == 3                       # one conv_1 per chained sample, all on the op
    assert "bev_net.conv_1.conv.weight" in cases.TRAINING_GRAD_KEYS and "bev_net.aux_head2.weight" in cases.TRAINING_GRAD_KEYS
    want = float(g["stage1_%s_loss" % mode])
    rel = abs(loss.item() - want) / abs(want)
    worst = _check_grads(g, "stage1_%s" % mode, model, cases.TRAINING_GRAD_KEYS, 2e-3 if mode == "eval" else 2e-2)
    print("stage 1 (%s, conv_1 on the op): loss %.6g vs %.6g (rel %.1e), worst gradient deviation %.1e" % (mode, loss.item(), want, rel, worst))
    assert rel <= 1e-4
    if mode == "train":
        sd = model.state_dict()
        for k in ("point_pre.layer.0.layer.2.running_mean", "bev_net.res2.1.layer.1.running_var", "bev_net.conv_1.bn.running_mean"):
            ref = g["stage1_train_bn_%s" % k]
            assert np.abs(sd[k].cpu().numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-6), k
        assert int(sd["bev_net.conv_1.bn.num_batches_tracked"]) == 3


def test_stage2_training_step_with_conv1_on_the_op_matches_reference_golden(golden, monkeypatch):
    """Everything but `refine.*` frozen, eval mode, gradients enabled: conv_1 runs on the op and its backward is never
    entered (no input of it needs a gradient)."""
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
    adjoints = []
    real_adjoint = ops.upconv_adjoint
    monkeypatch.setattr(ops, "upconv_adjoint", lambda *a, **kw: (adjoints.append(1), real_adjoint(*a, **kw))[1])
    prev = ops.set_conv1_fused(True)
    try:
        loss = model(batch)
        loss.backward()
    finally:
        ops.set_conv1_fused(prev)
    assert len(calls) == 3 and not adjoints
    with_grad = [k for k, p in model.named_parameters() if p.grad is not None]
    assert with_grad == [str(k) for k in g["stage2_params_with_grad"]]
    want = float(g["stage2_eval_loss"])
    rel = abs(loss.item() - want) / abs(want)
    worst = _check_grads(g, "stage2_eval", model, with_grad, 2e-3)
    print("stage 2 (conv_1 on the op): loss %.6g vs %.6g (rel %.1e), worst gradient deviation %.1e" % (loss.item(), want, rel, worst))
    assert rel <= 1e-4


def test_stage1_train_step_with_all_three_fused_switches_gives_the_same_loss(golden, monkeypatch):
    g, _, loss, calls = _stage1(golden, "train", monkeypatch, others=True)
    assert len(calls) == 3
    want = float(g["stage1_train_loss"])
    assert abs(loss.item() - want) / abs(want) <= 1e-4


def test_with_the_switch_off_the_op_is_never_called(golden, monkeypatch):
    g, _, loss, calls = _stage1(golden, "eval", monkeypatch, fused=False)
    assert not calls
    want = float(g["stage1_eval_loss"])
    assert abs(loss.item() - want) / abs(want) <= 1e-4

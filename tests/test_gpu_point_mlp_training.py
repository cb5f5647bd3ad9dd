"""The stage-1 training step of tests/golden/training.npz with the fused point MLP switched on (ops.set_point_mlp_fused):
AttNet.forward on cases.training_batch() (three chained samples, 2 x 2048 points), in eval and in train mode, against the
reference's loss, gradients and running buffers at the bars of tests/test_gpu_training.py.  The keys include
point_pre.layer.0.layer.1.weight and point_pre.layer.0.layer.2.running_mean, which ops.point_mlp_train now produces."""
import numpy as np
import pytest
import torch

from streammos_amd import ops, synth
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check_grads(g, prefix, model, keys, tol):
    named = dict(model.named_parameters())
    worst, errs = 0.0, []
    for k in keys:
        grad = named[k].grad
        assert grad is not None, k
        flat = grad.detach().reshape(-1)
        want_norm = float(g["%s_grad_norm_%s" % (prefix, k)])
        want_head = g["%s_grad_head_%s" % (prefix, k)]
        got_head = flat[:: max(1, flat.numel() // 512)][:512].cpu().numpy()
        scale = max(np.abs(want_head).max(), want_norm / max(flat.numel(), 1) ** 0.5, 1e-12)
        err = max(abs(flat.double().norm().item() - want_norm) / max(want_norm, 1e-12),
                  np.abs(got_head - want_head).max() / scale)
        worst = max(worst, err)
        errs.append((k, float(err)))
    assert worst <= tol, sorted(errs, key=lambda kv: -kv[1])[:5]
    return worst


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_stage1_training_step_with_the_fused_point_mlp_matches_reference_golden(golden, mode, monkeypatch):
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
    calls = []
    real = ops.point_mlp_train
    monkeypatch.setattr(ops, "point_mlp_train", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    if mode == "train":                          # dropout masks depend on the device's generator: removed on both sides
        monkeypatch.setattr(F, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
    prev = ops.set_point_mlp_fused(True)
    try:
        loss = model(batch)
        loss.backward()
    finally:
        ops.set_point_mlp_fused(prev)
    assert len(calls) == 3                       # one point_pre forward per chained sample, all on the op
    want = float(g["stage1_%s_loss" % mode])
    rel = abs(loss.item() - want) / abs(want)
    worst = _check_grads(g, "stage1_%s" % mode, model, cases.TRAINING_GRAD_KEYS, 2e-3 if mode == "eval" else 2e-2)
    print("stage 1 (%s, fused point MLP): loss %.6g vs %.6g (rel %.1e), worst gradient deviation %.1e" % (mode, loss.item(), want, rel, worst))
    assert rel <= 1e-4
    if mode == "train":
        sd = model.state_dict()
        for k in ("point_pre.layer.0.layer.2.running_mean", "bev_net.res2.1.layer.1.running_var", "bev_net.conv_1.bn.running_mean"):
            ref = g["stage1_train_bn_%s" % k]
            assert np.abs(sd[k].cpu().numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-6), k
        assert int(sd["point_pre.layer.0.layer.2.num_batches_tracked"]) == 3

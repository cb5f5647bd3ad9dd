"""ops.point_head_train (csrc/point_head_train.hip) on the GPU against the float64 restatement of
tests/point_head_train_cases.py.

Per result (logits, three input gradients, eight parameter gradients, four running buffers): max|got - ref64| / max|ref64| (a
bias gradient on the scale of its weight's), held to max(8 x the same figure of the float32 MODULE path on the same inputs
and masks, measured here on the GPU; 1e-6).  The yardstick is the module path, never the op.  Every check prints its worst
error / bar (pytest -s); the figures of the MI355X run are kept in profiles/point_head_train_error_ratios.txt.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from streammos_amd import _lib, ops
from streammos_amd.refapi.networks import backbone
from tests import point_head_train_cases as cases
from tests.test_host_point_head_train import keep_statistics_ok, keep_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = cases.shapes()
RATIOS = []
RATIO_FILE = os.path.join(ROOT, "profiles", "point_head_train_error_ratios.txt")
RATIO_HEADER = """Training point head (csrc/point_head_train.hip, ops.point_head_train) against the float64 restatement of tests/point_head_train_cases.py.
Written by tests/test_gpu_point_head_train.py when the whole file has run.

Per check: the largest error / bar over the logits, the three input gradients, the eight parameter gradients and the four
running buffers, and the result that has it.  error = max|got - ref64| / max|ref64| (a bias gradient on the scale of its
weight's); bar = max(8 x the same figure of the float32 module path on the same inputs and masks on the same GPU, 1e-6).  The
third figure is the op's largest error itself, the fourth the module path's largest error.  "capped" runs walk every chunk
with one block and must give the bits of the uncapped run.
"""


class _fused:
    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        self.prev = ops.set_point_head_fused(self.flag)

    def __exit__(self, *exc):
        ops.set_point_head_fused(self.prev)
        return False


def _op(fusion, pred, xs, training, **kw):
    m = fusion.merge_layer
    return ops.point_head_train(*xs, m[0], m[1], m[3], m[4], pred.pred_layer[0], training=training, **kw)


def _run_op(c, mode, cap=0, modules=None, grad=True, keep="case"):
    """forward + backward through the op with the case's masks -> (results, (fusion, pred), logits)"""
    fusion, pred = cases.build_modules(c, torch.float32, DEV) if modules is None else modules
    fusion.train(mode == "train")
    pred.train(mode == "train")
    xs, g, own = cases.case_tensors(c, torch.float32, DEV, grad=grad)
    lib = _lib.load()
    lib.smos_debug_set_conv_grid_cap(cap)
    try:
        logits = _op(fusion, pred, xs, mode == "train", keep=own if keep == "case" else keep)
        logits.backward(g)
        torch.cuda.synchronize()
    finally:
        lib.smos_debug_set_conv_grid_cap(0)
    return cases.collect(logits, xs, fusion, pred, c), (fusion, pred), logits


def _check(label, c, mode, got, ref=None, base=None, keys=cases.RESULTS):
    ref = cases.restate(c, mode == "train") if ref is None else ref
    if base is None:
        base, _ = cases.run_modules(c, mode == "train", torch.float32, DEV)
    worst = (0.0, None)
    emax = bmax = 0.0
    for k in keys:
        e, b = cases.metric(got, ref, k), cases.metric(base, ref, k)
        bar = max(8.0 * b, cases.FLOOR)
        emax, bmax = max(emax, e), max(bmax, b)
        if e / bar >= worst[0]:
            worst = (e / bar, k)
    print("point-head-train-ratio %-30s error / bar %.4f (%s)   op %.2e   module path %.2e" % (label, worst[0], worst[1], emax, bmax))
    RATIOS.append((label, worst[0], worst[1], emax, bmax))
    assert worst[0] <= 1.0, "%s: error / bar %g on %s" % (label, worst[0], worst[1])


def _same_bits(a, b, keys=cases.RESULTS):
    for k in keys:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    """profiles/point_head_train_error_ratios.txt from this run, once every test of the file has run (not for a -k selection)."""
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 60 or len(ran) < 70:
        return
    worst = max(RATIOS, key=lambda r: r[1])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  %d checks; the largest error / bar %.4f (%s, %s).\n\n" % (
                torch.cuda.get_device_name(0), len(RATIOS), worst[1], worst[0], worst[2]))
            f.writelines("%-32s %.4f %-6s %.2e %.2e\n" % r for r in RATIOS)
    except OSError:
        pass                                   # a read-only checkout: the figures were printed


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.CASES)
def test_against_float64_reference(name, shape, mode):
    c = cases.make_case(name, *shape)
    got, (fusion, _), logits = _run_op(c, mode)
    assert logits.shape == (shape[0], 3, shape[1], 1)
    tracked = [bn.num_batches_tracked.item() for bn in (fusion.merge_layer[1], fusion.merge_layer[4])]
    assert tracked == [1 if mode == "train" else 0] * 2
    label = "%s %dx%d %s" % (name, shape[0], shape[1], mode)
    _check(label, c, mode, got)
    if mode == "train":
        k1, k2 = ops.point_head_keep_bits(logits)               # the packed words the kernels read hold the case's masks
        assert np.array_equal(k1.cpu().numpy(), c["keep1"]) and np.array_equal(k2.cpu().numpy(), c["keep2"])
        if name == "dropped":
            pb, pn = cases.dropped_point(*shape)
            assert np.array_equal(got["logits"][pb, :, pn, 0], c["b3"])                  # all of keep2 off: the bias, bit for bit
            assert not got["dxa"][:, cases.DROPPED_CHANNEL].any() and not got["dw1"][:, cases.DROPPED_CHANNEL].any()
        if name == "dead":
            for k, i in (("dg1", cases.DEAD1), ("dbe1", cases.DEAD1), ("dw1", cases.DEAD1), ("dg2", cases.DEAD2),
                         ("dbe2", cases.DEAD2), ("dw2", cases.DEAD2)):
                assert not np.any(got[k][i]), k
    else:
        assert ops.point_head_keep_bits(logits) is None
    if shape == SHAPES[4]:                      # just over three chunks: one block walks them all
        capped, _, _ = _run_op(c, mode, cap=1)
        _same_bits(capped, got)
        RATIOS.append((label + " capped", RATIOS[-1][1], RATIOS[-1][2], RATIOS[-1][3], RATIOS[-1][4]))


@pytest.mark.parametrize("mode", cases.MODES)
def test_more_than_one_group_of_chunks(mode):
    """More than 64 chunks, so the second level of the fixed-order sums has two groups; under a cap of three blocks every
    block walks over twenty chunks and the bits stay."""
    n = 32 * ops.point_head_train_chunk() + 40
    c = cases.make_case("plain", 2, n)
    assert 2 * n > 64 * ops.point_head_train_chunk()
    got, _, _ = _run_op(c, mode)
    capped, _, _ = _run_op(c, mode, cap=3)
    _same_bits(capped, got)
    assert all(np.isfinite(got[k]).all() for k in cases.RESULTS)


@pytest.mark.parametrize("mode", cases.MODES)
def test_two_runs_give_the_same_bits(mode):
    c = cases.make_case("plain", 6, 97)
    a, _, _ = _run_op(c, mode)
    b, _, _ = _run_op(c, mode)
    _same_bits(a, b)


def _generated(seed, c, modules=None):
    fusion, pred = cases.build_modules(c, torch.float32, DEV) if modules is None else modules
    fusion.train()
    pred.train()
    xs, _, _ = cases.case_tensors(c, torch.float32, DEV, grad=False)
    if seed is not None:
        torch.manual_seed(seed)
    return _op(fusion, pred, xs, True), (fusion, pred)


def test_generated_masks_follow_torch_manual_seed():
    """2 x 4096 points under torch.manual_seed(1234).  The seed words come from the device's generator, so the CPU cannot
    know them beforehand; the words this run drew are read back and the bits held to the numpy restatement of the generator
    (tests/test_host_point_head_train.py), which settles the statistics for exactly these bits."""
    c = cases.make_case("plain", 2, 4096)
    first, modules = _generated(1234, c)
    again, _ = _generated(1234, c)
    nxt, _ = _generated(None, c, modules)
    words, seed, _, _ = first._smos_point_head
    assert torch.equal(words, again._smos_point_head[0]) and torch.equal(first, again)
    assert (words != nxt._smos_point_head[0]).float().mean().item() > 0.9
    got = words.cpu().numpy().view(np.uint32).reshape(8, -1)
    assert np.array_equal(got, keep_words(seed.cpu().tolist(), 2 * 4096))
    assert keep_statistics_ok(got)
    k1, k2 = ops.point_head_keep_bits(first)
    bits = torch.cat((k1, k2), 1).permute(1, 0, 2).reshape(256, -1).float()
    sigma = (0.8 * 0.2 / (2 * 4096)) ** 0.5
    assert abs(bits.mean().item() - 0.8) <= 5 * sigma / 16
    assert (bits.mean(1) - 0.8).abs().max().item() <= 6 * sigma
    # the same bits handed in as explicit masks give the same forward
    fusion, pred = cases.build_modules(c, torch.float32, DEV)
    fusion.train()
    pred.train()
    xs, _, _ = cases.case_tensors(c, torch.float32, DEV, grad=False)
    assert torch.equal(_op(fusion, pred, xs, True, keep=(k1, k2)), first)


def test_running_buffers_after_one_and_two_training_forwards():
    c = cases.make_case("plain", 3, 70)
    modules = cases.build_modules(c, torch.float32, DEV)
    base_modules = cases.build_modules(c, torch.float32, DEV)
    ref_c = dict(c)
    for step in (1, 2):
        got, _, _ = _run_op(c, "train", modules=modules)
        base, _ = cases.run_modules(c, True, torch.float32, DEV, modules=base_modules)
        ref = cases.restate(ref_c, True)
        _check("plain 3x70 forward %d buffers" % step, c, "train", got, ref=ref, base=base, keys=cases.BUFFERS)
        bns = (modules[0].merge_layer[1], modules[0].merge_layer[4])
        assert [bn.num_batches_tracked.item() for bn in bns] == [step, step]
        ref_c.update({k: ref[k] for k in cases.BUFFERS})


@pytest.mark.parametrize("frozen", [("w1",), ("xa", "xb", "xc"), ("xa", "xb", "xc", "w1", "g1", "be1"), ("w2", "g2", "be2"),
                                    ("xb", "b3", "w3"), ("w1", "g1", "be1", "w2")])
def test_what_needs_no_gradient_gets_none_and_the_rest_is_unchanged(frozen, monkeypatch):
    c = cases.make_case("plain", 3, 70)
    full, _, _ = _run_op(c, "train")
    fusion, pred = cases.build_modules(c, torch.float32, DEV)
    params, _ = cases.module_tensors(fusion, pred)
    for k in frozen:
        if k in params:
            params[k].requires_grad_(False)
    fusion.train()
    pred.train()
    xs, g, keep = cases.case_tensors(c, torch.float32, DEV)
    for k, x in zip(cases.INPUTS, xs):
        x.requires_grad_(k not in frozen)
    passed = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (passed.append(list(a[11])) if name == "smos_point_head_train_bwd" else None,
                                                        real(name, *a))[1])
    logits = _op(fusion, pred, xs, True, keep=keep)
    logits.backward(g)
    torch.cuda.synchronize()
    got = cases.collect(logits, xs, fusion, pred, c)
    for k in cases.INPUTS + cases.PARAMS:
        if k in frozen:
            assert got["d" + k] is None, k
        else:
            assert np.array_equal(got["d" + k], full["d" + k]), k
    assert np.array_equal(got["logits"], full["logits"])
    # a NULL pointer is what removes the work: without input gradients the kernels are handed no buffer to write to
    assert len(passed) == 1
    if all(k in frozen for k in cases.INPUTS):
        assert passed[0][:3] == [None, None, None]
    for i, k in enumerate(cases.PARAMS):
        assert (passed[0][3 + i] is None) == (k in frozen), k


def test_nothing_needs_a_gradient_no_backward_launch(monkeypatch):
    c = cases.make_case("plain", 2, 33)
    fusion, pred = cases.build_modules(c, torch.float32, DEV)
    for p in list(fusion.parameters()) + list(pred.parameters()):
        p.requires_grad_(False)
    xs, _, keep = cases.case_tensors(c, torch.float32, DEV, grad=False)
    out = _op(fusion.train(), pred.train(), xs, True, keep=keep)
    assert not out.requires_grad


def test_one_point_raises_in_training_as_torch_does():
    c = cases.make_case("plain", 1, 2)
    fusion, pred = cases.build_modules(c, torch.float32, DEV)
    xs = [torch.from_numpy(c[k][:, :, :1]).float().to(DEV) for k in cases.INPUTS]
    with _fused(True):
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            backbone.point_head(fusion.train(), pred.train(), *xs)
        xs[0].requires_grad_()
        y = backbone.point_head(fusion.eval(), pred.eval(), *xs)          # eval has no such limit
    assert y.shape == (1, 3, 1, 1) and torch.isfinite(y).all()


def test_switch_off_is_the_module_path_bit_for_bit():
    c = cases.make_case("plain", 3, 70)
    for mode in cases.MODES:
        a = cases.build_modules(c, torch.float32, DEV)
        b = cases.build_modules(c, torch.float32, DEV)
        for m in a + b:
            m.train(mode == "train")
        xs, _, _ = cases.case_tensors(c, torch.float32, DEV)
        with _fused(False):
            torch.manual_seed(77)
            got = backbone.point_head(a[0], a[1], *xs)
        torch.manual_seed(77)
        want = b[1](b[0](*xs))
        assert torch.equal(got, want)
        for p, q in zip(list(a[0].buffers()), list(b[0].buffers())):
            assert torch.equal(p, q)


@pytest.mark.parametrize("what", ["autocast", "float64", "other_widths", "sync_bn_world_2", "different_modes", "no_grad_eval"])
def test_switch_on_keeps_unsupported_configurations_on_the_module_path(what, monkeypatch):
    c = cases.make_case("plain", 3, 70)
    dtype = torch.float64 if what == "float64" else torch.float32

    def build():
        if what == "other_widths":
            torch.manual_seed(3)
            return backbone.CatFusion((64, 64, 64), 32).to(DEV), backbone.PredBranch(32, 3).to(DEV)
        fusion, pred = cases.build_modules(c, dtype, DEV)
        if what == "sync_bn_world_2":
            fusion = nn.SyncBatchNorm.convert_sync_batchnorm(fusion)
        return fusion, pred
    a, b = build(), build()
    train = what != "no_grad_eval"
    for m in a + b:
        m.train(train)
    if what == "different_modes":
        a[1].eval()
        b[1].eval()
    if what == "sync_bn_world_2":
        monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
        monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    xs, _, _ = cases.case_tensors(c, dtype, DEV, grad=what != "no_grad_eval")
    calls = []
    real = ops.point_head_train
    monkeypatch.setattr(ops, "point_head_train", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    with _fused(True):
        if what == "sync_bn_world_2":
            assert backbone._point_head_modules(a[0], a[1], xs) is None       # (a forward would need the process group)
            monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 1)
            assert backbone._point_head_modules(a[0], a[1], xs) is not None
            return
        torch.manual_seed(9)
        if what == "autocast":
            with torch.autocast("cuda", dtype=torch.float16):
                got = backbone.point_head(a[0], a[1], *xs)
        elif what == "no_grad_eval":
            with torch.no_grad():
                got = backbone.point_head(a[0], a[1], *xs)
        else:
            got = backbone.point_head(a[0], a[1], *xs)
        torch.manual_seed(9)
        if what == "autocast":
            with torch.autocast("cuda", dtype=torch.float16):
                want = b[1](b[0](*xs))
        elif what == "no_grad_eval":
            with torch.no_grad():
                want = b[1](b[0](*xs))
        else:
            want = b[1](b[0](*xs))
        assert not calls and torch.equal(got, want)
        # and a supported call right after does reach the op
        fusion, pred = cases.build_modules(c, torch.float32, DEV)
        backbone.point_head(fusion.train(), pred.train(), *cases.case_tensors(c, torch.float32, DEV)[0])
        assert calls


def test_nan_in_the_tail_of_an_over_allocated_input_is_never_read():
    """N = 33 inside a point axis of 64 whose other 31 entries are NaN: the inputs are read in place (pitch 64) and give the
    bits of the dense inputs."""
    c = cases.make_case("plain", 2, 33)
    for mode in cases.MODES:
        want, _, _ = _run_op(c, mode)
        fusion, pred = cases.build_modules(c, torch.float32, DEV)
        fusion.train(mode == "train")
        pred.train(mode == "train")
        dense, g, keep = cases.case_tensors(c, torch.float32, DEV, grad=False)
        xs = []
        for x in dense:
            big = torch.full((2, 64, 64, 1), float("nan"), device=DEV)
            big[:, :, :33] = x
            xs.append(big[:, :, :33].requires_grad_())
            assert not xs[-1].is_contiguous()
        logits = _op(fusion, pred, xs, mode == "train", keep=keep)
        logits.backward(g)
        got = cases.collect(logits, xs, fusion, pred, c)
        _same_bits(got, want)

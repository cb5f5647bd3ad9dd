"""ops.point_mlp_train (csrc/point_mlp_train.hip) on the GPU against the float64 restatement of tests/point_mlp_cases.py.

Per result (y, eight gradients, six running buffers): max|got - ref64| / max|ref64| (dbeta0 on the scale of dgamma0), held to
max(8 x the same figure of the float32 MODULE path on the same inputs, measured here on the GPU; 1e-6).  The yardstick is
the module path, never the op.  Every check prints its worst error / bar (pytest -s); the figures of the MI355X run are kept
in profiles/point_mlp_error_ratios.txt.  The op is reached through PointNetStacker.forward with the switch on, so the
routing is under test as well.
"""
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import point_mlp_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = []
RATIO_FILE = os.path.join(ROOT, "profiles", "point_mlp_error_ratios.txt")
RATIO_HEADER = """Training point MLP (csrc/point_mlp_train.hip, ops.point_mlp_train) against the float64 restatement of tests/point_mlp_cases.py.
Written by tests/test_gpu_point_mlp.py when the whole file has run.

Per check: the largest error / bar over y, the eight gradients and the six running buffers, and the result that has it.
error = max|got - ref64| / max|ref64| (dbeta0 on the scale of dgamma0); bar = max(8 x the same figure of the float32 module
path on the same inputs on the same GPU, 1e-6).  The third figure is the op's largest error itself, the fourth the module
path's largest error.  "capped" runs walk every chunk with one block and must give the bits of the uncapped run.
"""


def _fused(flag):
    class _Ctx:
        def __enter__(self):
            self.prev = ops.set_point_mlp_fused(flag)

        def __exit__(self, *exc):
            ops.set_point_mlp_fused(self.prev)
            return False
    return _Ctx()


def _run(c, mode, fused, cap=0, module=None):
    lib = _lib.load()
    lib.smos_debug_set_conv_grid_cap(cap)
    try:
        with _fused(fused):
            out, m = cases.run_modules(c, mode == "train", torch.float32, DEV, module=module)
        torch.cuda.synchronize()
    finally:
        lib.smos_debug_set_conv_grid_cap(0)
    return out, m


def _check(label, c, mode, got, ref=None):
    ref = cases.restate(c, mode == "train") if ref is None else ref
    base, _ = _run(c, mode, False)
    worst = (0.0, None)
    emax = bmax = 0.0
    for k in cases.RESULTS:
        e, b = cases.metric(got, ref, k), cases.metric(base, ref, k)
        bar = max(8.0 * b, cases.FLOOR)
        emax, bmax = max(emax, e), max(bmax, b)
        if e / bar >= worst[0]:
            worst = (e / bar, k)
    print("point-mlp-ratio %-34s error / bar %.4f (%s)   op %.2e   module path %.2e" % (label, worst[0], worst[1], emax, bmax))
    RATIOS.append((label, worst[0], worst[1], emax, bmax))
    assert worst[0] <= 1.0, "%s: error / bar %g on %s" % (label, worst[0], worst[1])


def _same_bits(a, b):
    for k in cases.RESULTS:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module", autouse=True)
def _ratio_file(request):
    """profiles/point_mlp_error_ratios.txt from this run, once every test of the file has run (not for a -k selection)."""
    yield
    ran = {item.nodeid for item in request.session.items if item.fspath == request.fspath}
    if len(RATIOS) < 50 or len(ran) < 58:
        return
    worst = max(RATIOS, key=lambda r: r[1])
    try:
        with open(RATIO_FILE, "w") as f:
            f.write(RATIO_HEADER + "\nDevice: %s.  %d checks; the largest error / bar %.4f (%s, %s).\n\n" % (
                torch.cuda.get_device_name(0), len(RATIOS), worst[1], worst[0], worst[2]))
            f.writelines("%-36s %.4f %-4s %.2e %.2e\n" % r for r in RATIOS)
    except OSError:
        pass                                   # a read-only checkout: the figures were printed


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.CASES)
def test_against_float64_reference(name, shape, mode):
    c = cases.make_case(name, *shape)
    got, m = _run(c, mode, True)
    assert got["y"].shape == (shape[0], 64, shape[1], 1)
    tracked = [bn.num_batches_tracked.item() for bn in (m.layer[0].layer[0], m.layer[0].layer[2], m.layer[1].layer[1])]
    assert tracked == [1 if mode == "train" else 0] * 3
    label = "%s %dx%d %s" % (name, shape[0], shape[1], mode)
    _check(label, c, mode, got)
    if shape == (2, 1000):                      # four chunks: one block walks them all, about 16 trips per wave
        capped, _ = _run(c, mode, True, cap=1)
        _same_bits(capped, got)
        RATIOS.append((label + " capped", RATIOS[-1][1], RATIOS[-1][2], RATIOS[-1][3], RATIOS[-1][4]))


@pytest.mark.parametrize("mode", cases.MODES)
def test_more_than_one_group_of_chunks(mode):
    """3 x 11000 points: 65 chunks, so the second level of the fixed-order sums has two groups; under a cap of three blocks
    every block walks some twenty chunks and the bits stay."""
    c = cases.make_case("kitti", 3, 11000)
    assert 3 * 11000 > 64 * ops.point_mlp_chunk()
    got, _ = _run(c, mode, True)
    _check("kitti 3x11000 %s" % mode, c, mode, got)
    capped, _ = _run(c, mode, True, cap=3)
    _same_bits(capped, got)


@pytest.mark.parametrize("mode", cases.MODES)
def test_two_runs_give_the_same_bits(mode):
    c = cases.make_case("kitti", 6, 97)
    a, _ = _run(c, mode, True)
    b, _ = _run(c, mode, True)
    _same_bits(a, b)


def test_one_point_raises_in_training_as_torch_does():
    c = cases.make_case("normal", 1, 5)
    m = cases.build_modules(c, torch.float32, DEV).train()
    x = torch.from_numpy(c["x"][:, :, :1]).float().to(DEV)
    with _fused(True):
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            m(x)
        y = m.eval()(x)                          # eval has no such limit
    assert y.shape == (1, 64, 1, 1) and torch.isfinite(y).all()


@pytest.mark.parametrize("frozen", [("w2",), ("g0", "b0", "w1", "g1", "b1"), ("g2", "b2", "w2"), ("b1",)])
def test_a_frozen_parameter_gets_no_gradient_and_the_others_are_unchanged(frozen):
    c = cases.make_case("kitti", 3, 45)
    full, _ = _run(c, "train", True)
    m = cases.build_modules(c, torch.float32, DEV)
    params, _ = cases.module_tensors(m)
    for k in frozen:
        params[k].requires_grad_(False)
    got, _ = _run(c, "train", True, module=m)
    for k in cases.PARAMS:
        if k in frozen:
            assert got["d" + k] is None
        else:
            assert np.array_equal(got["d" + k], full["d" + k]), k
    assert np.array_equal(got["y"], full["y"])


def test_switch_off_is_the_module_path_bit_for_bit():
    c = cases.make_case("kitti", 3, 45)
    x = torch.from_numpy(c["x"]).float().to(DEV)
    for mode in cases.MODES:
        a = cases.build_modules(c, torch.float32, DEV).train(mode == "train")
        b = cases.build_modules(c, torch.float32, DEV).train(mode == "train")
        with _fused(False):
            got = a(x)
        want = b.layer(x)
        assert torch.equal(got, want)
        for p, q in zip(a.buffers(), b.buffers()):
            assert torch.equal(p, q)


@pytest.mark.parametrize("what", ["x_requires_grad", "float64", "autocast", "no_grad_eval"])
def test_switch_on_keeps_unsupported_configurations_on_the_module_path(what, monkeypatch):
    c = cases.make_case("normal", 3, 45)
    dtype = torch.float64 if what == "float64" else torch.float32
    a = cases.build_modules(c, dtype, DEV).train(what != "no_grad_eval")
    b = cases.build_modules(c, dtype, DEV).train(what != "no_grad_eval")
    x = torch.from_numpy(c["x"]).to(device=DEV, dtype=dtype)
    calls = []
    real = ops.point_mlp_train
    monkeypatch.setattr(ops, "point_mlp_train", lambda *args, **kw: calls.append(1) or real(*args, **kw))
    with _fused(True):
        if what == "x_requires_grad":
            x1, x2 = x.clone().requires_grad_(), x.clone().requires_grad_()
            got, want = a(x1), b.layer(x2)
            got.sum().backward()
            want.sum().backward()
            assert torch.equal(x1.grad, x2.grad)
        elif what == "autocast":
            with torch.autocast("cuda", dtype=torch.float16):
                got, want = a(x), b.layer(x)
        elif what == "no_grad_eval":
            with torch.no_grad():
                got, want = a(x), b.layer(x)
        else:
            got, want = a(x), b.layer(x)
        assert not calls and torch.equal(got, want)
        if what in ("float64", "autocast"):        # and the supported call right after does reach the op
            cases.build_modules(c, torch.float32, DEV).train()(x.to(torch.float32))
            assert calls

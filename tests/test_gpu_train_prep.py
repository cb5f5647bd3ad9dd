"""Training samples built on the device (csrc/train_prep.hip, device_preprocess.DeviceTrainPreprocessor) against the host
restatement (preprocess.build_train_sample), which equals the reference's arithmetic (tests/test_host_train_prep.py)."""
import ctypes

import numpy as np
import pytest
import torch

from streammos_amd import _lib, device_preprocess, preprocess

from . import train_prep_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPEC = preprocess.VoxelSpec()
# the bars of tests/test_gpu_preprocess.py for the two range-view angles (device asinf / atan2f against numpy's routines), taken
# like there over everything one build writes (here: the three windows of a sample).  A 1-ulp difference moves a value that
# sits on a half-cell boundary into the next cell: one such value of the 6000 of a single window at N = 1000 is 1.7e-4.
ANGLE_MAX, ANGLE_SAME_CELL = 2e-3, 0.9999


def _host(built, slot=0):
    return {k: v[slot].cpu().numpy() for k, v in built.items()}


def _check(got, want, names=("pcds_target",)):
    exact, angles = tc.compare_sample(got, want, names)
    print("mismatching values:", {k: v for k, v in exact.items() if v} or 0, "angles (max diff, same half cell):", angles)
    assert all(v == 0 for v in exact.values()), exact
    assert angles[0] <= ANGLE_MAX and angles[1] >= ANGLE_SAME_CELL, angles
    assert np.array_equal(got["in_range_counts"], want["in_range_counts"])


@pytest.fixture(scope="module")
def small():
    """One shared sample (N = 2048) with explicit draws and its host build."""
    scans, words, poses, n, draws = tc.device_case("n2048")
    want = preprocess.build_train_sample(scans, words, poses, n, SPEC, None, draws, label_maps=tc.label_maps(two=True))
    return scans, words, poses, n, draws, want


@pytest.mark.parametrize("name", [c[0] for c in tc.DEVICE_CASES])
def test_device_build_matches_host(name):
    scans, words, poses, n, draws = tc.device_case(name)
    want = preprocess.build_train_sample(scans, words, poses, n, SPEC, None, draws)
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n)
    built = pre.build(scans, words, poses, draws=draws)
    got = _host(built)
    _check(got, want)
    counts = want["in_range_counts"]
    opt = dict([c for c in tc.DEVICE_CASES if c[0] == name][0][4])
    if opt.get("lone"):
        assert counts[2, 2] == 1
        pre.check_counts(built)
    if opt.get("empty"):
        assert counts[2, 2] == 0 and counts.reshape(-1)[:8].min() > 0
        with pytest.raises(ValueError, match="window 2, frame 2"):
            pre.check_counts(built)
        pad = got["pcds_xyzi_2"][2, :4, :, 0]
        assert np.array_equal(pad, np.repeat(np.array([[-1000.0], [-1000.0], [-4000.0], [-1000.0]], dtype=np.float32), n, axis=1))
    if "shift" in opt:          # pushed out of the grid on both sides; the BEV grid skips those points like the CPU twin
        q = got["pcds_coord_0"][0, :, :2, 0]
        assert (q < 0).any() and (q >= 512).any()
    if name == "n2048":         # the steering reached the device: kept and dropped face points, every label class
        assert counts[0, 0] < scans[0].shape[0] and set(np.unique(got["pcds_target_0"])) == {0, 1, 2}


def test_device_build_matches_host_with_scans_already_on_the_device(small):
    scans, words, poses, n, draws, want = small
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n, label_maps=tc.label_maps(two=True))
    dev_draws = preprocess.TrainDraws(torch.from_numpy(draws.words.view(np.int32)).to(DEV), torch.from_numpy(draws.noise).to(DEV),
                                      draws.shift, draws.scale, draws.h_flip, draws.v_flip, draws.theta_z)
    dev_scans = [torch.from_numpy(s).to(DEV) for s in scans]
    built = pre.build(dev_scans, [torch.from_numpy(w.view(np.int32)).to(DEV) for w in words], poses, draws=dev_draws)
    _check(_host(built), want, ("pcds_target", "pcds_bf_target"))
    # some scans on the device, the others on the host
    mixed = pre.build(dev_scans[:2] + scans[2:], words, poses, draws=draws)
    for k in built:
        assert torch.equal(mixed[k], built[k]), k


def test_scans_aligned_on_the_host_skip_the_first_alignment(small):
    """aligned=True takes scans as the reference's copy-paste leaves them: after Trans(scan, inv(P_0) P_k).  Same sample."""
    scans, words, poses, n, draws, want = small
    inv0 = np.linalg.inv(poses[0])
    moved = [preprocess.pose_align(s, inv0.dot(p)) for s, p in zip(scans, poses)]
    host = preprocess.build_train_sample(moved, words, poses, n, SPEC, None, draws, label_maps=tc.label_maps(two=True), aligned=True)
    for k in want:
        assert np.array_equal(host[k], want[k]), k
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n, label_maps=tc.label_maps(two=True))
    _check(_host(pre.build(moved, words, poses, draws=draws, aligned=True)), want, ("pcds_target", "pcds_bf_target"))


def test_reference_fixture_through_the_device_path(golden):
    g = golden("train_prep")
    scans, words, poses, _ = tc.fixture_inputs()
    draws, want = tc.fixture_draws(g), tc.fixture_sample(g)
    want["in_range_counts"] = np.stack([g["counts_%d" % w] for w in range(3)])
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, tc.FIXTURE_N)
    _check(_host(pre.build(scans, words, poses, draws=draws)), want)


def test_stage2_targets_from_two_label_maps(small):
    scans, words, poses, n, draws, want = small
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n, label_maps=tc.label_maps(two=True))
    got = _host(pre.build(scans, words, poses, draws=draws))
    _check(got, want, ("pcds_target", "pcds_bf_target"))
    assert any((got["pcds_bf_target_%d" % w] != got["pcds_target_%d" % w]).any() for w in range(3))
    # a word whose semantic id is the table's last entry, and ids past the table
    sem = [(w & np.uint32(0xFFFF)) for w in words]
    assert any((s == 359).any() for s in sem) and any((s >= 360).any() for s in sem) and any((w >> np.uint32(16)).any() for w in words)


def test_seeded_build_equals_build_from_the_exported_draws(small):
    scans, words, poses, n, _, _ = small
    aug = preprocess.AugParam(noise_mean=0.001, noise_std=0.02)
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n, aug=aug)
    seed, sample = 2 ** 63 + 12345, 2 ** 32 + 7
    exported = pre.seeded_draws(seed, sample)
    a = pre.build(scans, words, poses, seed=seed, sample_index=sample)
    b = pre.build(scans, words, poses, draws=exported)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    host = preprocess.draws_from_seed(seed, sample, n, aug)
    assert np.array_equal(exported.words.cpu().numpy().view(np.uint32), host.words)
    assert (exported.shift, exported.scale, exported.h_flip, exported.v_flip, exported.theta_z) == \
        (host.shift, host.scale, host.h_flip, host.v_flip, host.theta_z)
    # the exported noise against float64 Box-Muller of the same words, in units of noise_std (bound: train_prep_cases.py)
    noise = exported.noise.cpu().numpy()
    z = (noise - np.float64(np.float32(aug.noise_mean))) / np.float64(np.float32(aug.noise_std))
    err = np.abs(z - tc.seeded_z64(seed, sample, n))
    print("device Box-Muller against float64: max |dz| = %.3e (bar %.1e)" % (float(err.max()), tc.BOX_MULLER_BOUND))
    assert np.isfinite(noise).all() and err.max() <= tc.BOX_MULLER_BOUND
    # a second run and two launch-grid caps give the same bits; another sample index gives other draws
    lib = _lib.load()
    try:
        for cap in (0, 3, 7):
            lib.smos_debug_set_conv_grid_cap(cap)
            c = pre.build(scans, words, poses, seed=seed, sample_index=sample)
            again = pre.seeded_draws(seed, sample)
            for k in a:
                assert torch.equal(a[k], c[k]), (cap, k)
            assert torch.equal(again.words, exported.words) and torch.equal(again.noise, exported.noise), cap
    finally:
        lib.smos_debug_set_conv_grid_cap(0)
    other = pre.seeded_draws(seed, sample + 1)
    assert (other.words != exported.words).float().mean().item() > 0.99 and other.shift != exported.shift
    d = pre.build(scans, words, poses, seed=seed, sample_index=sample + 1)
    assert not torch.equal(a["pcds_xyzi_0"], d["pcds_xyzi_0"])


def test_explicit_draws_under_a_grid_cap(small):
    """Several units per block in every kernel (count / compact walk chunks, emit walks slot blocks): same bits."""
    scans, words, poses, n, draws, want = small
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n, label_maps=tc.label_maps(two=True))
    lib = _lib.load()
    try:
        lib.smos_debug_set_conv_grid_cap(2)
        got = _host(pre.build(scans, words, poses, draws=draws))
    finally:
        lib.smos_debug_set_conv_grid_cap(0)
    _check(got, want, ("pcds_target", "pcds_bf_target"))


def test_build_batch_equals_single_builds_and_honours_pitched_out(small):
    scans, words, poses, n, draws, _ = small
    scans2, words2, poses2 = tc.sample_inputs(16, 120, empty=True)
    draws2 = tc.explicit_draws(n, 31, v_flip=1, h_flip=1, theta_z=-180.0)
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n)
    one = [pre.build(scans, words, poses, draws=draws), pre.build(scans2, words2, poses2, draws=draws2)]
    # out: slices 1 and 2 of a poisoned batch of four whose batch stride is larger than a sample (a view of a wider buffer)
    wide, out = {}, {}
    for k, (shape, dtype) in pre.output_shapes().items():
        per = int(np.prod(shape))
        wide[k] = torch.full((4, per + 5), float("nan") if dtype.is_floating_point else -1, dtype=dtype, device=DEV)
        out[k] = wide[k][:, 2:2 + per].view((4,) + tuple(shape))
        assert not out[k].is_contiguous() and out[k][1].is_contiguous()
    sub = {k: v[1:3] for k, v in out.items()}
    got = pre.build_batch([(scans, words, poses), (scans2, words2, poses2)], draws=[draws, draws2], out=sub)
    assert got is sub
    for k, v in out.items():
        for b in range(2):
            assert torch.equal(v[1 + b], one[b][k][0]), (k, b)
        poison = torch.isnan(v[1:3]).any() if v.dtype.is_floating_point else ((v[1:3] == -1).any() if k != "in_range_counts" else False)
        assert not poison, k
        untouched = wide[k].clone()
        untouched[1:3, 2:2 + v[0].numel()] = untouched[0, 0]
        assert (torch.isnan(untouched).all() if v.dtype.is_floating_point else (untouched == -1).all()), k
    # a fresh batch from build_batch: the same values, stacked
    fresh = pre.build_batch([(scans, words, poses), (scans2, words2, poses2)], draws=[draws, draws2])
    for k, v in fresh.items():
        assert v.shape[0] == 2 and torch.equal(v, torch.cat([one[0][k], one[1][k]])), k


def test_build_and_build_batch_do_not_wait_for_the_stream(small):
    """Both return while the stream is still busy with work queued before them (the method of
    tests/test_gpu_seg_loss.py::test_loss_and_backward_do_not_wait_for_the_stream): nothing reads a device value on the host."""
    scans, words, poses, n, draws, _ = small
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n)
    want = pre.build_batch([(scans, words, poses)] * 2, seed=5)                # allocates scratch and staging, loads the code
    want1 = pre.build(scans, words, poses, draws=draws)
    torch.cuda.synchronize()
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
    got1 = pre.build(scans, words, poses, draws=draws)
    got = pre.build_batch([(scans, words, poses)] * 2, seed=5)
    waited = busy.query()
    torch.cuda.synchronize()
    assert not waited
    for k in want:
        assert torch.equal(got[k], want[k]) and torch.equal(got1[k], want1[k]), k


def test_stage1_step_on_a_device_built_batch_equals_the_host_built_step(small):
    """Two eval-mode steps of one model at the shapes of tests/test_gpu_training.py (B = 2, N = 2048).  Where this is the
    first training step of the process it also pays the convolution library's one-off search for the backward kernels."""
    from streammos_amd import synth
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    scans, words, poses, n, draws, _ = small
    scans2, words2, poses2 = tc.sample_inputs(16, 120)
    draws2 = tc.explicit_draws(n, 32, v_flip=0, h_flip=1, theta_z=12.5)
    samples, all_draws = [(scans, words, poses), (scans2, words2, poses2)], [draws, draws2]
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n)
    batch = pre.build_batch(samples, draws=all_draws)
    hosts = [preprocess.build_train_sample(s, w, p, n, SPEC, None, d) for (s, w, p), d in zip(samples, all_draws)]
    host_batch = {k: torch.from_numpy(np.stack([h[k] for h in hosts])).to(DEV) for k in hosts[0]}
    model = StreamMOS.AttNet(cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(DEV).eval()
    losses = []
    for b in (batch, host_batch):
        model.zero_grad(set_to_none=True)
        loss = model(b)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
        losses.append(loss.item())
    rel = abs(losses[0] - losses[1]) / abs(losses[1])
    print("stage-1 loss on the device-built batch %.6f, on the host-built batch %.6f, relative difference %.2e" % (losses[0], losses[1], rel))
    # the angles may differ in the last bit: the relative bar test_step_raw_equals_host_preprocessed_step uses for logits
    assert np.isfinite(losses[0]) and rel <= 2e-4


def test_refusals(small):
    scans, words, poses, n, draws, _ = small
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n)
    good = dict(scans=scans, label_words=words, poses=poses, draws=draws)

    def refused(match, **change):
        args = dict(good, **change)
        with pytest.raises(RuntimeError, match=match):
            pre.build(args.pop("scans"), args.pop("label_words"), args.pop("poses"), **args)

    wide = np.zeros((scans[0].shape[0], 8), dtype=np.float32)
    refused("contiguous", scans=[wide[:, :4]] + scans[1:])
    refused("contiguous", scans=[scans[0].astype(np.float64)] + scans[1:])
    refused("contiguous", scans=[torch.from_numpy(wide).to(DEV)[:, :4]] + scans[1:])
    refused("label words", label_words=[words[0][:-1]] + words[1:])
    refused("label words", label_words=[words[0].astype(np.int64)] + words[1:])
    refused("5 scans", scans=scans + scans[:1], label_words=words + words[:1], poses=poses + poses[:1])
    refused("5 scans", scans=scans[:4], label_words=words[:4], poses=poses[:4])
    refused("5 poses", poses=poses[:4])
    bad = preprocess.TrainDraws(draws.words[:, :, :-1], draws.noise, draws.shift, draws.scale, draws.h_flip, draws.v_flip, draws.theta_z)
    refused("draws.words", draws=bad)
    bad = preprocess.TrainDraws(draws.words.astype(np.int64), draws.noise, draws.shift, draws.scale, draws.h_flip, draws.v_flip, draws.theta_z)
    refused("draws.words", draws=bad)
    bad = preprocess.TrainDraws(draws.words, draws.noise.astype(np.float32), draws.shift, draws.scale, draws.h_flip, draws.v_flip, draws.theta_z)
    refused("draws.noise", draws=bad)
    bad = preprocess.TrainDraws(draws.words, draws.noise[:, :-1], draws.shift, draws.scale, draws.h_flip, draws.v_flip, draws.theta_z)
    refused("draws.noise", draws=bad)
    refused("either draws or seed", seed=3)
    refused("either draws or seed", draws=None)
    with pytest.raises(RuntimeError, match="either draws or seed"):
        pre.build_batch([(scans, words, poses)])
    out = pre.alloc_batch(1)
    out["pcds_xyzi_1"] = out["pcds_xyzi_1"].double()
    refused("pcds_xyzi_1", out=out)
    refused(r"out\[", out=pre.alloc_batch(1), batch_slot=1)
    for n_bad in (0, -5):
        with pytest.raises(RuntimeError, match="frame_point_num"):
            device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n_bad)
    # the C entry points refuse on their own: N <= 0, a missing half of the draws
    lib = _lib.load()
    assert lib.smos_train_prep_work_bytes(0) == -1 and lib.smos_train_prep_work_bytes(1920) > 0
    assert lib.smos_train_prep_draws(1, 0, 0, 0.0, 1.0, ctypes.c_void_p(16), ctypes.c_void_p(16), None) == 1
    assert b"frame_point_num" in lib.smos_last_error()

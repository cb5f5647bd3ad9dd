"""Copy-paste augmentation on the device (csrc/copy_paste.hip, device_preprocess.DeviceCopyPaste) against the host restatement
(preprocess.copy_paste_sample) and the reference's own run (tests/golden/copy_paste.npz)."""
import numpy as np
import pytest
import torch

from streammos_amd import _lib, device_preprocess, preprocess

from . import copy_paste_cases as cc
from . import train_prep_cases as tc
from .test_gpu_train_prep import ANGLE_MAX, ANGLE_SAME_CELL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPEC = preprocess.VoxelSpec()
PASTE_LABELS = {"pcds_target": (0, 1, 2), "pcds_bf_target": (2, 2, 2)}
NAMES = ("pcds_target", "pcds_bf_target")


@pytest.fixture(scope="module")
def case(golden):
    """The sample of tests/copy_paste_cases.py, the fixture, the stage and one run of it with the explicit draws."""
    g = golden("copy_paste")
    s = cc.fixture_sample(g)
    paste = device_preprocess.DeviceCopyPaste(device_preprocess.DeviceObjectBank(DEV, s["bank"]), SPEC, cc.LABEL_BASE)
    scans, words, status = paste.apply(s["scans"], s["words"], s["poses"], draws=s["draws"])
    return s, g, paste, (scans, words, status)


def _host(run):
    scans, words, status = run
    return [t.cpu().numpy() for t in scans], [t.cpu().numpy().view(np.uint32) for t in words], status.cpu().numpy()


def test_device_matches_twin_and_reference(case):
    s, g, paste, run = case
    scans, words, status = _host(run)
    assert np.array_equal(status, s["status"]) and tuple(status) == cc.EXPECTED
    worst = {}
    for name, want in (("reference", None), ("twin", s)):
        if want is None:
            bad, ratios = cc.compare_with_reference(scans, words, status, s, g)
        else:
            # against the twin everything but the pasted z is equal, row for row (padding rows and words included)
            bad = {"status": int((status != want["status"]).sum()), "xyi": 0, "word": 0, "pad": 0}
            for k in range(5):
                a, b = scans[k], want["out_scans"][k]
                bad["xyi"] += int((a[:, [0, 1, 3]] != b[:, [0, 1, 3]]).sum())
                bad["word"] += int((words[k] != want["out_words"][k]).sum())
                bad["pad"] += int(((a[:, 2] == np.float32(preprocess.PAD_Z)) != (b[:, 2] == np.float32(preprocess.PAD_Z))).sum())
            _, ratios = cc.compare_with_reference(scans, words, status, s, g)
        print(name, bad, dict((i, "%.3f" % float(r.max())) for i, r in ratios.items()))
        assert all(v == 0 for v in bad.values()), (name, bad)
        # per element: |dz| <= lifts * ((ceil(log2 12) + 2) 2^-24 max|z_road| + 2^-22), cc.z_bound
        for i, r in ratios.items():
            assert float(r.max()) <= 1.0, (name, i, float(r.max()))
            worst[i] = max(worst.get(i, 0.0), float(r.max()))
    print("z ratios |dz| / bound per object:", worst)


def test_apply_then_build_matches_the_host_chain(case):
    s, g, paste, run = case
    maps, base = preprocess.paste_label_maps(tc.label_maps(two=True), PASTE_LABELS)
    draws = tc.explicit_draws(2048, 616)
    want = preprocess.build_train_sample(s["out_scans"], s["out_words"], s["poses"], 2048, SPEC, None, draws, label_maps=maps, aligned=True)
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, 2048, label_maps=tc.label_maps(two=True), paste_labels=PASTE_LABELS)
    assert pre.paste_label_base == base == paste.label_base
    built = pre.build(run[0], run[1], s["poses"], draws=draws, aligned=True)
    got = {k: v[0].cpu().numpy() for k, v in built.items()}
    # the pasted z differs from the host's within cc.z_bound (a few 1e-7 m): the existing bars of the train-prep tests apply to
    # everything else; the z-derived values of pasted points are held to that bound
    exact, angles = tc.compare_sample(got, want, NAMES)
    print(exact, angles)
    bound = cc.z_bound(s["road"][:, 2], 12, 3) * 1.05 + 2.0 ** -22          # scale <= 1.05, one more rounding
    for w in range(3):
        for k in ("pcds_coord", "pcds_bev_target") + NAMES:
            if k == "pcds_coord":
                assert np.array_equal(got["pcds_coord_%d" % w][:, :, :2], want["pcds_coord_%d" % w][:, :, :2])
                cell = (SPEC.range_z[1] - SPEC.range_z[0]) / SPEC.bev_shape[2]
                assert np.abs(got["pcds_coord_%d" % w][:, :, 2] - want["pcds_coord_%d" % w][:, :, 2]).max() <= bound / cell + 2.0 ** -20
            else:
                assert exact["%s_%d" % (k, w)] == 0, (k, w)
        a, b = got["pcds_xyzi_%d" % w], want["pcds_xyzi_%d" % w]
        assert np.array_equal(a[:, [0, 1, 3, 5, 6]], b[:, [0, 1, 3, 5, 6]])
        assert np.abs(a[:, [2, 4]] - b[:, [2, 4]]).max() <= bound + 2.0 ** -20
    assert angles[0] <= ANGLE_MAX and angles[1] >= ANGLE_SAME_CELL, angles
    assert np.array_equal(got["in_range_counts"], want["in_range_counts"])
    assert any((got["pcds_bf_target_%d" % w] == 2).any() for w in range(3))
    # the builder alone, on what the device pasted: the bars of tests/test_gpu_train_prep.py as they are (everything equal but
    # the two range-view angles)
    scans, words, _ = _host(run)
    same_input = preprocess.build_train_sample(scans, words, s["poses"], 2048, SPEC, None, draws, label_maps=maps, aligned=True)
    exact, angles = tc.compare_sample(got, same_input, NAMES)
    print(exact, angles)
    assert all(v == 0 for v in exact.values()), exact
    assert angles[0] <= ANGLE_MAX and angles[1] >= ANGLE_SAME_CELL, angles
    assert np.array_equal(got["in_range_counts"], same_input["in_range_counts"])
    # build_batch(paste=...) is the same two calls
    batch = pre.build_batch([(s["scans"], s["words"], s["poses"])], draws=[draws], paste=paste, paste_draws=[s["draws"]])
    for k in built:
        assert torch.equal(batch[k], built[k]), k
    assert torch.equal(batch["paste_status"][0], run[2])


def test_bits_do_not_depend_on_the_grid(case):
    s, g, paste, run = case
    lib = _lib.load()
    try:
        for cap in (3, 7):
            lib.smos_debug_set_conv_grid_cap(cap)
            again = paste.apply(s["scans"], s["words"], s["poses"], draws=s["draws"])
            for a, b in zip(run[0] + run[1] + [run[2]], again[0] + again[1] + [again[2]]):
                assert torch.equal(a, b), cap
    finally:
        lib.smos_debug_set_conv_grid_cap(0)


def test_seeded_runs_repeat_and_equal_their_exported_draws(case):
    s, g, paste, run = case
    seed = 2 ** 63 + 99
    index = next(i for i in range(64) if len(preprocess.seeded_paste_scalars(seed, i, paste.bank.categories)[0]) >= 4)
    a = paste.apply(s["scans"], s["words"], s["poses"], seed=seed, sample_index=index)
    b = paste.apply(s["scans"], s["words"], s["poses"], seed=seed, sample_index=index)
    exported = paste.seeded_draws(seed, index)
    c = paste.apply(s["scans"], s["words"], s["poses"], draws=exported)
    for x, y, z in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]], c[0] + c[1] + [c[2]]):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert a[2].shape[0] == exported.count >= 4
    other = paste.seeded_draws(seed, index + 1)
    assert other.count != exported.count or other.index != exported.index or other.velocity != exported.velocity
    # the exported noise against the host restatement of the generator (numpy's float32 log / cos: tc.BOX_MULLER_BOUND in units of
    # the standard deviation)
    for i, nz in enumerate(exported.noise):
        host = preprocess.seeded_paste_noise(seed, index, i, nz.shape[1])
        assert np.abs(nz.cpu().numpy() - host).max() <= tc.BOX_MULLER_BOUND * preprocess.PASTE_NOISE_STD


def test_without_paste_the_builder_is_todays(case):
    s, g, paste, run = case
    scans, words, poses, n, draws = tc.device_case("n2048")
    plain = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n, label_maps=tc.label_maps(two=True))
    assert plain.paste_label_base is None and tuple(plain._lut.shape) == (2, 360)
    assert np.array_equal(plain._lut.cpu().numpy()[0], tc.label_maps()["pcds_target"])
    a = plain.build_batch([(scans, words, poses)], draws=[draws])
    b = plain.build_batch([(scans, words, poses)], draws=[draws], paste=None)
    c = plain.build(scans, words, poses, draws=draws)
    assert sorted(a) == sorted(b) == sorted(c)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    # with paste_labels the LUT only grows: a sample without pasted points builds to the same bits
    ext = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, n, label_maps=tc.label_maps(two=True), paste_labels=PASTE_LABELS)
    assert np.array_equal(ext._lut.cpu().numpy()[:, :360], plain._lut.cpu().numpy())
    # ids 360..362 occur in these words (tc.SEM_IDS has 360): only their targets may differ
    d = ext.build(scans, words, poses, draws=draws)
    for k in a:
        if not k.startswith(NAMES):
            assert torch.equal(a[k][0], d[k][0]) or k.startswith("pcds_bev_target"), k


def test_argument_errors_come_before_the_first_launch(case):
    s, g, paste, run = case
    d = s["draws"]
    good = (s["scans"], s["words"], s["poses"])

    def draws(index=None, order=None, noise=None):
        return preprocess.PasteDraws(d.index if index is None else index, d.velocity, d.order if order is None else order,
                                     d.noise if noise is None else noise)

    plain = device_preprocess.DeviceTrainPreprocessor(DEV, SPEC, 64)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    order = d.order.copy()
    order[2, 5] = order[2, 6]
    with pytest.raises(RuntimeError, match="permutation"):
        paste.apply(*good, draws=draws(order=order))
    with pytest.raises(RuntimeError, match="bank index"):
        paste.apply(*good, draws=draws(index=[len(s["bank"])] + d.index[1:]))
    noise = list(d.noise)
    noise[3] = noise[3][:, :-1]
    with pytest.raises(RuntimeError, match="noise"):
        paste.apply(*good, draws=draws(noise=noise))
    with pytest.raises(RuntimeError, match="either draws or seed"):
        paste.apply(*good)
    far = [p.copy() for p in s["poses"]]
    far[1][0, 3] += 5000.0
    with pytest.raises(RuntimeError, match="padding point"):
        paste.apply(s["scans"], s["words"], far, draws=d)
    with pytest.raises(RuntimeError, match="paste_labels"):
        plain.build_batch([good], seed=1, paste=paste)
    assert torch.cuda.memory_allocated() == before            # nothing was allocated, so nothing was launched

"""run_sequence(device_preprocess=True): the overlapped loop (reader / writer threads, label kernel, one readback per
sequence) against the serial device-preprocessing loop it replaces, and the label kernel against numpy."""
import os
import threading

import numpy as np
import pytest
import torch

from streammos_amd import kitti, ops, preprocess, run_sequence, streaming, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FPN = 2048


@pytest.fixture(scope="module")
def model():
    return run_sequence.load_model(None, DEV)


@pytest.fixture(scope="module")
def seg_model():
    return run_sequence.load_model(None, DEV, seg=True)


def _gt_words(rng, n):
    ids = np.array((0, 1, 52, 99, 258) + kitti.STATIC_IDS + kitti.MOVING_IDS, dtype=np.uint32)   # 1, 52, 99: map to 0
    return ids[rng.integers(0, ids.size, n)] | (rng.integers(0, 1 << 16, n).astype(np.uint32) << 16)


def _np_counts(gt_words, pred_cls):
    m = kitti.MovingIoU()
    m.add(kitti.learning_map_lut()[gt_words & 0xFFFF], pred_cls)
    return np.concatenate((m.tp, m.pred, m.gt)).astype(np.int64)


def test_label_kernel_equals_numpy():
    rng = np.random.default_rng(7)
    gt_map = torch.from_numpy(kitti.learning_map_lut()).to(DEV)
    lut = np.array([0, 9, 251], dtype=np.int32)
    for n in (0, 1, 63, 64, 65, 1000, 131071):
        labels = rng.integers(0, 3, n).astype(np.uint8)
        gt = _gt_words(rng, n)
        lab_d, gt_d = torch.from_numpy(labels).to(DEV), torch.from_numpy(gt.view(np.int32)).to(DEV)
        counts = torch.zeros(6, dtype=torch.int64, device=DEV)
        words = ops.label_words(lab_d, gt=gt_d, gt_map=gt_map, counts=counts)
        assert np.array_equal(words.cpu().numpy(), lut[labels]), n
        assert np.array_equal(ops.label_words(lab_d, lut=False).cpu().numpy(), labels.astype(np.int32)), n
        want = _np_counts(gt, labels)
        assert np.array_equal(counts.cpu().numpy(), want), (n, counts.cpu().numpy(), want)
        ops.label_words(lab_d, words=words, gt=gt_d, gt_map=gt_map, counts=counts)         # a second launch accumulates
        assert np.array_equal(counts.cpu().numpy(), 2 * want), n
        # voted LUT words (anything but 9 / 251 counts as class 0)
        voted = np.array([0, 9, 251, 5, 1, 2], dtype=np.int32)[rng.integers(0, 6, n)]
        v_counts = torch.zeros(6, dtype=torch.int64, device=DEV)
        copy = torch.full((n + 4,), -7, dtype=torch.int32, device=DEV)
        ops.voted_label_counts(torch.from_numpy(voted).to(DEV), gt_d, gt_map, v_counts, words=copy)
        assert np.array_equal(copy.cpu().numpy()[:n], voted) and (copy.cpu().numpy()[n:] == -7).all(), n
        want_v = _np_counts(gt, np.where(voted == 251, 2, np.where(voted == 9, 1, 0)))
        assert np.array_equal(v_counts.cpu().numpy(), want_v), (n, v_counts.cpu().numpy(), want_v)


def _make_sequence(root, n, labels=True, crowded=None):
    """n 16x120-point synthetic scans in SemanticKITTI layout; scan `crowded` gets 2100 extra points inside the range box."""
    seq = root / "sequences" / "08"
    (seq / "velodyne").mkdir(parents=True)
    if labels:
        (seq / "labels").mkdir()
    rng = np.random.default_rng(11)
    for k in range(n):
        scan, lab = synth.synthetic_scan(k, 16, 120, with_labels=True)
        if k == crowded:
            extra = np.concatenate((rng.uniform(-20, 20, (2100, 2)), rng.uniform(-1.5, 0.0, (2100, 1)),
                                    rng.random((2100, 1))), axis=1).astype(np.float32)
            scan, lab = np.concatenate((scan, extra)), np.concatenate((lab, np.ones(2100, dtype=lab.dtype)))
            assert int(preprocess.range_mask(scan, preprocess.VoxelSpec()).sum()) >= FPN
        scan.tofile(seq / "velodyne" / ("%06d.bin" % k))
        if labels:
            words = np.where(lab == 2, 252, 40).astype(np.uint32)
            words[rng.random(words.size) < 0.1] = 0                              # unlabeled points are not counted
            (words | (np.uint32(k + 1) << 16)).tofile(seq / "labels" / ("%06d.label" % k))
    kitti.write_poses(seq / "poses.txt", [synth.synthetic_pose(k) for k in range(n)])
    kitti.write_calibration(seq / "calib.txt")
    return seq


def _serial_reference(model, seq, out, vote):
    """The device-preprocessing loop as it stood before the overlapped one: StreamRunner(pipeline=False).step_raw, a
    readback and a capacity check per frame, numpy IoU."""
    files = sorted(f for f in os.listdir(seq / "velodyne") if f.endswith(".bin"))
    n = len(files)
    poses = kitti.read_poses(seq / "poses.txt", kitti.read_calibration(seq / "calib.txt"))
    has_gt = (seq / "labels").is_dir()
    runner = streaming.StreamRunner(model, DEV, vote=vote)
    m_raw, m_ref = kitti.MovingIoU(), kitti.MovingIoU()
    scans = [torch.from_numpy(kitti.read_scan(seq / "velodyne" / f)).to(DEV) for f in files]

    def gt(i):
        return kitti.read_label(seq / "labels" / (files[i][:-4] + ".label"))

    def emit(voted):
        for fid, lab in voted:
            lab = lab.cpu().numpy()
            kitti.write_prediction(os.path.join(out, "refined", files[fid][:-4] + ".label"), lut_labels=lab)
            if has_gt:
                m_ref.add(gt(fid), np.where(lab == 251, 2, np.where(lab == 9, 1, 0)))

    for i in range(n):
        idx = [min(j, n - 1) for j in preprocess.window_indices(i, n, 3)]
        o = runner.step_raw([scans[j] for j in idx], [poses[j] for j in idx], FPN)
        raw = o["raw_labels"].cpu().numpy()
        runner.check_last_raw_sample()
        kitti.write_prediction(os.path.join(out, "predictions", files[i][:-4] + ".label"), labels_012=raw)
        if "bf_raw_labels" in o:
            kitti.write_prediction(os.path.join(out, "predictions_bf", files[i][:-4] + ".label"),
                                   lut_labels=o["bf_raw_labels"].cpu().numpy())
        if has_gt:
            m_raw.add(gt(i), raw)
        emit(o["voted"])
    emit(runner.voter.flush())
    return {"network": m_raw.result(), "voted": m_ref.result()}


def _files(root):
    got = {}
    for dirpath, _, names in os.walk(root):
        for name in names:
            path = os.path.join(dirpath, name)
            got[os.path.relpath(path, root)] = open(path, "rb").read()
    return got


@pytest.mark.parametrize("n", [13, 5])
def test_overlapped_files_equal_the_serial_loop(tmp_path, model, n):
    """13 frames: the window fills, then one vote per frame; 5 frames: every vote comes from flush()."""
    seq = _make_sequence(tmp_path, n)
    want = _serial_reference(model, seq, str(tmp_path / "ref"), True)
    res = run_sequence.run_sequence(model, str(seq), str(tmp_path / "out"), DEV, vote=True, frame_point_num=FPN,
                                    device_preprocess=True)
    ref_files, got_files = _files(tmp_path / "ref"), _files(tmp_path / "out")
    assert sorted(got_files) == sorted(ref_files) and len(ref_files) == 2 * n
    for name in ref_files:
        assert got_files[name] == ref_files[name], name
    assert res["scans"] == n and res["network"] == want["network"] and res["voted"] == want["voted"]


def test_overlapped_instance_voting_files_equal_the_serial_loop(tmp_path, seg_model):
    n = 13
    seq = _make_sequence(tmp_path, n)
    want = _serial_reference(seg_model, seq, str(tmp_path / "ref"), "instance")
    res = run_sequence.run_sequence(seg_model, str(seq), str(tmp_path / "out"), DEV, vote="instance", frame_point_num=FPN,
                                    device_preprocess=True)
    ref_files, got_files = _files(tmp_path / "ref"), _files(tmp_path / "out")
    assert sorted(got_files) == sorted(ref_files) and len(ref_files) == 3 * n
    for name in ref_files:
        assert got_files[name] == ref_files[name], name
    assert res["network"] == want["network"] and res["voted"] == want["voted"]


class _SyncCounter:
    """Counts the host<-device readbacks and stream / device synchronisations the MAIN thread makes.  The runner's one-off
    probe for a concurrent side stream (streaming.concurrent_stream: it times spin kernels, and how many candidates it tries
    varies from run to run) is set-up, not per-frame work, and is left out."""

    def __init__(self, monkeypatch):
        self.n = 0
        self.probing = False
        main = threading.main_thread()

        def counted(fn, test):
            def wrapper(*args, **kwargs):
                out = fn(*args, **kwargs)
                if threading.current_thread() is main and not self.probing and test(args, out):
                    self.n += 1
                return out
            return wrapper

        probe = streaming.concurrent_stream

        def unprobed(*args, **kwargs):
            self.probing = True
            try:
                return probe(*args, **kwargs)
            finally:
                self.probing = False
        monkeypatch.setattr(streaming, "concurrent_stream", unprobed)

        on_gpu = lambda args, out: torch.is_tensor(args[0]) and args[0].is_cuda           # noqa: E731
        for name in ("cpu", "item", "tolist", "__bool__"):
            monkeypatch.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name), on_gpu))
        monkeypatch.setattr(torch.Tensor, "to", counted(torch.Tensor.to, lambda args, out: args[0].is_cuda and
                                                        torch.is_tensor(out) and not out.is_cuda))
        monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize, lambda args, out: True))
        monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted(torch.cuda.Stream.synchronize, lambda args, out: True))


def test_main_thread_syncs_do_not_grow_with_the_sequence(tmp_path, model, monkeypatch):
    seq = _make_sequence(tmp_path, 20)
    run_sequence.run_sequence(model, str(seq), str(tmp_path / "warm"), DEV, vote=True, frame_point_num=FPN, limit=10,
                              device_preprocess=True)
    counts = {}
    for limit in (10, 20):
        with monkeypatch.context() as mp:
            c = _SyncCounter(mp)
            run_sequence.run_sequence(model, str(seq), str(tmp_path / ("out%d" % limit)), DEV, vote=True, frame_point_num=FPN,
                                      limit=limit, device_preprocess=True)
            counts[limit] = c.n
    assert counts[10] == counts[20], counts


def test_over_capacity_scan_raises_and_leaves_the_serial_loops_files(tmp_path, model):
    seq = _make_sequence(tmp_path, 10, crowded=5)
    with pytest.raises(ValueError, match="leaves no padding") as ref_err:
        _serial_reference(model, seq, str(tmp_path / "ref"), True)
    before = threading.active_count()
    with pytest.raises(ValueError, match="leaves no padding") as err:
        run_sequence.run_sequence(model, str(seq), str(tmp_path / "out"), DEV, vote=True, frame_point_num=FPN,
                                  device_preprocess=True)
    assert str(err.value) == str(ref_err.value)
    assert threading.active_count() == before
    ref_files, got_files = _files(tmp_path / "ref"), _files(tmp_path / "out")
    assert sorted(got_files) == sorted(ref_files) and len(ref_files) > 0
    for name in ref_files:
        assert got_files[name] == ref_files[name], name

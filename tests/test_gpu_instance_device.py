"""Device-resident instance voting (ops.instance_cluster / box_vote_dev / instance_apply, InstanceVoter(device_resident=True),
the status word of the overlapped sequence loop) against scikit-learn, the existing per-frame path and the CPU oracle.
Integer / index work: every comparison is array_equal."""
import os
import threading

import numpy as np
import pytest
import torch

from oracle import ops_np
from streammos_amd import kitti, ops, preprocess, run_sequence, streaming, synth
from tests.test_gpu_instance import _cloud, _rank, _sequence

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_POINTS, FLOOR_LIFT = 30, 0.2
PARAMS = [(0, 6, 120, 400, 0.25, 0.3, 5), (1, 12, 60, 1500, 0.4, 0.3, 5), (2, 3, 700, 50, 0.6, 0.3, 5),
          (3, 8, 40, 300, 0.2, 0.5, 3), (4, 5, 90, 0, 0.3, 0.3, 12), (5, 0, 0, 300, 0.3, 0.3, 5)]   # test_dbscan_matches_sklearn's


def _embed(cloud, seed):
    """The cloud as the foreground of a scan: twice as many non-foreground points, every foreground point once more as a
    non-foreground point at the same coordinates, all randomly interleaved.  Returns (scan [4m, 4], bf [4m])."""
    rng = np.random.default_rng(1000 + seed)
    m = len(cloud)
    lo, hi = (cloud.min(0), cloud.max(0)) if m else (np.zeros(3), np.ones(3))
    other = rng.uniform(lo, hi, (2 * m, 3)).astype(np.float32)
    xyz = np.concatenate((cloud, other, cloud)).astype(np.float32)
    bf = np.concatenate((np.full(m, 2), rng.integers(0, 2, 3 * m))).astype(np.uint8)
    order = rng.permutation(len(xyz))
    scan = np.concatenate((xyz[order], np.zeros((len(xyz), 1), np.float32)), axis=1)
    return scan, bf[order]


def _cluster(scan, bf, eps, min_samples, max_boxes=ops.MAX_BOXES, work=None):
    out = ops.instance_cluster(torch.from_numpy(scan).to(DEV), torch.from_numpy(bf).to(DEV), eps, min_samples, MIN_POINTS,
                               FLOOR_LIFT, max_boxes, work=work)
    k = int(out["k"].item())
    boxes = out["boxes"].cpu().numpy()[:k]
    return out["names"].cpu().numpy(), boxes[np.lexsort(boxes.T[::-1])], k, out


def _check_names(scan, bf, eps, min_samples, names):
    """names against scikit-learn and against ops.dbscan on the compacted foreground, mapped back to scan indices"""
    from sklearn.cluster import DBSCAN
    fg = np.nonzero(bf == 2)[0]
    assert (names[bf != 2] == -1).all()
    if len(fg) == 0:
        return
    model = DBSCAN(eps=eps, min_samples=min_samples).fit(scan[fg, :3])
    assert np.array_equal(_rank(names[fg]), model.labels_)
    core = np.zeros(len(scan), dtype=bool)
    core[fg[model.core_sample_indices_]] = True
    for name in np.unique(names[names >= 0]):
        assert core[name] and name == np.where(core & (names == name))[0].min()
    old = ops.dbscan(torch.from_numpy(scan[fg]).to(DEV), eps, min_samples).cpu().numpy()
    assert np.array_equal(names[fg], np.where(old >= 0, fg[np.maximum(old, 0)], -1))


@pytest.mark.parametrize("seed,n_blobs,per,n_noise,sigma,eps,min_samples", PARAMS)
def test_names_equal_sklearn_and_the_existing_kernel(seed, n_blobs, per, n_noise, sigma, eps, min_samples):
    scan, bf = _embed(_cloud(seed, n_blobs, max(per, 1), n_noise, sigma), seed)
    names, boxes, k, out = _cluster(scan, bf, eps, min_samples)
    _check_names(scan, bf, eps, min_samples, names)
    assert int(out["status"].item()) == 0
    # boxes and slots against InstanceVoter.cluster_boxes on the compacted foreground
    fg = np.nonzero(bf == 2)[0]
    voter = streaming.InstanceVoter(DEV)
    voter.EPS, voter.MIN_SAMPLES = eps, min_samples
    member, slot, want = voter.cluster_boxes(torch.from_numpy(scan[fg, :3]).to(DEV))
    want = want.cpu().numpy()
    assert k == len(want) and np.array_equal(boxes, want[np.lexsort(want.T[::-1])])
    slot_of = out["slot_of"].cpu().numpy()
    got_member = np.zeros(len(scan), dtype=bool)
    got_member[names >= 0] = slot_of[names[names >= 0]] >= 0
    assert np.array_equal(got_member[fg], member.cpu().numpy())


@pytest.mark.parametrize("min_samples", [3, 2])
def test_long_chain(min_samples):
    """A 30-row serpentine of points 0.25 apart: one component whose labels need thousands of propagation sweeps."""
    from sklearn.cluster import DBSCAN
    rng = np.random.default_rng(5)
    rows = [np.stack((np.arange(100) * 0.25, np.full(100, 0.5 * r), np.zeros(100)), axis=1) for r in range(30)]
    joints = [np.array([[24.75 if r % 2 == 0 else 0.0, 0.5 * r + 0.25, 0.0]]) for r in range(29)]
    noise = np.stack((rng.uniform(-5, 30, 500), rng.uniform(-5, 20, 500), rng.uniform(3, 8, 500)), axis=1)
    xyz = np.concatenate(rows + joints + [noise]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    scan = np.concatenate((xyz, np.zeros((len(xyz), 1), np.float32)), axis=1)
    bf = np.full(len(scan), 2, dtype=np.uint8)
    want = DBSCAN(eps=0.3, min_samples=min_samples).fit_predict(xyz)
    assert np.bincount(want[want >= 0]).max() == 3029
    names, _, _, _ = _cluster(scan, bf, 0.3, min_samples)
    assert np.array_equal(_rank(names), want)
    _check_names(scan, bf, 0.3, min_samples, names)


@pytest.mark.parametrize("n_fg", [0, 1, 4, 255, 256, 257, 513, 1000])
def test_edge_counts(n_fg):
    rng = np.random.default_rng(n_fg)
    xyz = (rng.uniform(0, 6, (1000, 3)) * np.array([1, 1, 0.08])).astype(np.float32)
    scan = np.concatenate((xyz, np.zeros((1000, 1), np.float32)), axis=1)
    bf = np.ones(1000, dtype=np.uint8)
    bf[rng.permutation(1000)[:n_fg]] = 2
    names, _, k, out = _cluster(scan, bf, 0.3, 5)
    _check_names(scan, bf, 0.3, 5, names)
    if n_fg == 0:
        assert k == 0 and int(out["status"].item()) == 0


def test_coincident_points_and_an_empty_scan():
    scan = np.ones((12, 4), dtype=np.float32)
    bf = np.array([1, 0, 2, 2, 1, 2, 2, 2, 1, 2, 2, 1], dtype=np.uint8)           # 7 coincident foreground points
    names, _, k, _ = _cluster(scan, bf, 0.3, 5)
    assert names.tolist() == [2 if b == 2 else -1 for b in bf] and k == 0
    out = ops.instance_cluster(torch.zeros((0, 4), device=DEV), torch.zeros(0, dtype=torch.uint8, device=DEV), 0.3, 5,
                               MIN_POINTS, FLOOR_LIFT)
    torch.cuda.synchronize()
    assert out["names"].numel() == 0 and int(out["k"].item()) == 0 and int(out["status"].item()) == 0


def test_no_stale_state():
    seed, n_blobs, per, n_noise, sigma, eps, min_samples = PARAMS[0]
    scan, bf = _embed(_cloud(seed, n_blobs, per, n_noise, sigma), seed)
    work = torch.zeros(ops.instance_work_bytes(len(scan)), dtype=torch.uint8, device=DEV)
    first = _cluster(scan, bf, eps, min_samples, work=work)[:3]
    work.fill_(0xFF)
    second = _cluster(scan, bf, eps, min_samples, work=work)[:3]
    big = torch.full((ops.instance_work_bytes(4 * len(scan)),), 0xFF, dtype=torch.uint8, device=DEV)
    third = _cluster(scan, bf, eps, min_samples, work=big)[:3]
    assert first[2] > 0
    for other in (second, third):
        assert np.array_equal(other[0], first[0]) and np.array_equal(other[1], first[1]) and other[2] == first[2]


# ---- the voter ------------------------------------------------------------------------------------------------------
BLOBS = [((10.0, 5.0, -1.0), 30, (1, 1, 1)), ((-12.0, 8.0, -1.0), 31, (1, 1, 1)), ((6.0, -14.0, -1.0), 40, (1, 1, 0)),
         ((-9.0, -11.0, -1.0), 40, (0, 1, 1)), ((15.0, -4.0, -1.0), 5, (1, 1, 1)), ((-18.0, -2.0, -1.0), 1, (1, 1, 1))]
EXTRA = [((20.0, 12.0, -1.0), 31, (1, 1, 1)), ((-22.0, 14.0, -1.0), 31, (1, 1, 1))]


def _steered_frame(k, blobs):
    """synthetic_scan(k, 16, 120) plus foreground blobs (sigma 0.04 per axis, 0 where the mask says so) at fixed places;
    pred of the added points alternates 2 / 1 by frame parity, bf = 2 on them and on the scan's moving points."""
    scan, lab = synth.synthetic_scan(k, 16, 120, with_labels=True)
    rng = np.random.default_rng(500 + k)
    added = np.concatenate([np.asarray(c) + rng.normal(0.0, 0.04, (m, 3)) * np.asarray(mask) for c, m, mask in blobs])
    added = np.concatenate((added, rng.random((len(added), 1))), axis=1).astype(np.float32)
    pred = np.concatenate((lab, np.full(len(added), 2 if k % 2 == 0 else 1))).astype(np.uint8)
    bf = np.concatenate((np.where(lab == 2, 2, 1), np.full(len(added), 2))).astype(np.uint8)
    return np.concatenate((scan, added)), pred, bf


def _steered_sequence(n_frames, blobs=BLOBS):
    frames = [_steered_frame(k, blobs) for k in range(n_frames)]
    return [f[0] for f in frames], [f[1] for f in frames], [f[2] for f in frames], [np.eye(4) for _ in frames]


def _quiet_sequence():
    """3 frames, window 2: frame 1 has no foreground at all, frame 2's foreground is DBSCAN noise only."""
    scans, preds, bfs, poses = _sequence(3)
    scans, preds = [s[:3000] for s in scans], [p[:3000] for p in preds]
    bfs = [bfs[0][:3000].copy(), np.ones(3000, dtype=np.uint8), np.ones(3000, dtype=np.uint8)]
    bfs[2][2100::97] = 2
    return scans, preds, bfs, poses


def _oracle(seq, window):
    scans, preds, bfs, poses = seq
    lut = np.zeros(256, dtype=np.int32)
    lut[1], lut[2] = 9, 251
    want = []
    for fid in range(len(scans)):
        hist_ids = [h for h in streaming.vote_history_ids(fid, window) if h < len(scans)]
        inv_cur = np.linalg.inv(poses[fid])
        hp = np.concatenate([preprocess.pose_align(scans[h], inv_cur.dot(poses[h])) for h in hist_ids], 0)
        hl = np.concatenate([preds[h] for h in hist_ids], 0)
        want.append(lut[ops_np.instance_vote_frame(scans[fid], preds[fid], bfs[fid], hp, hl)])
    return want


def _run_voter(voter, seq):
    scans, preds, bfs, poses = seq
    got = {}
    for k in range(len(scans)):
        for fid, lab in voter.push(torch.from_numpy(scans[k]).to(DEV), torch.from_numpy(preds[k]).to(DEV), poses[k],
                                   torch.from_numpy(bfs[k]).to(DEV)):
            got[fid] = lab.cpu().numpy()
    for fid, lab in voter.flush():
        got[fid] = lab.cpu().numpy()
    return got


@pytest.fixture(scope="module")
def sequences():
    """name -> (sequence, window, oracle labels), computed once"""
    out = {}
    for name, seq, window in (("noisy", _sequence(7), 4), ("steered", _steered_sequence(6), 4), ("quiet", _quiet_sequence(), 2)):
        out[name] = (seq, window, _oracle(seq, window))
    return out


@pytest.mark.parametrize("name", ["noisy", "steered", "quiet"])
def test_voter_equals_the_existing_path_and_the_oracle(sequences, name):
    seq, window, want = sequences[name]
    got = _run_voter(streaming.InstanceVoter(DEV, window=window, device_resident=True), seq)
    old = _run_voter(streaming.InstanceVoter(DEV, window=window), seq)
    plain = streaming.VoxelVoter(DEV, window=window)
    assert sorted(got) == sorted(old) == list(range(len(want)))
    for fid in range(len(want)):
        assert np.array_equal(got[fid], old[fid]), fid
        assert np.array_equal(got[fid], want[fid]), (fid, int((got[fid] != want[fid]).sum()))
    if name == "steered":
        scans, preds, _, poses = seq
        changed = 0
        for k in range(len(scans)):
            for fid, lab in plain.push(torch.from_numpy(scans[k]).to(DEV), torch.from_numpy(preds[k]).to(DEV), poses[k]):
                changed += int((lab.cpu().numpy() != got[fid]).sum())
        assert changed > 0          # the instance stage did overrule the voxel vote somewhere
        n31 = slice(1920 + 30, 1920 + 61)                       # the 31-point cluster is overruled uniformly, by frame parity
        for fid in range(len(scans)):
            assert (got[fid][n31] == (251 if fid % 2 == 0 else 9)).all(), fid


def test_voter_matches_reference_golden(golden):
    """The 10-frame fixture sequence the REFERENCE's post_processing() labelled (tests/golden/instance.npz): bit-exact."""
    from tests import cases
    g = golden("instance")
    frames = cases.instance_sequence()
    voter = streaming.InstanceVoter(DEV, device_resident=True)
    got = {}
    for scan, pred, bf, pose in frames:
        for k, lab in voter.push(torch.from_numpy(scan).to(DEV), torch.from_numpy(pred).to(DEV), pose, torch.from_numpy(bf).to(DEV)):
            got[k] = lab.cpu().numpy()
            assert int(voter.status(k).item()) == 0
    assert sorted(got) == list(range(len(frames)))
    for fid in range(len(frames)):
        want = g["inst_f%d_refined" % fid]
        assert np.array_equal(got[fid], want), (fid, int((got[fid] != want).sum()))


def test_too_many_clusters_set_the_status_bit():
    seq = _steered_sequence(6, BLOBS + EXTRA)
    for scan, pred, bf in zip(*seq[:3]):
        kept = [c for c in ops_np.instance_cluster_stats(scan, pred, bf) if c["points"] > MIN_POINTS]
        assert len(kept) >= 5
    voter = streaming.InstanceVoter(DEV, window=4, device_resident=True, max_boxes=4)
    scans, preds, bfs, poses = seq
    seen = 0
    for k in range(len(scans)):
        for fid, _ in voter.push(torch.from_numpy(scans[k]).to(DEV), torch.from_numpy(preds[k]).to(DEV), poses[k],
                                 torch.from_numpy(bfs[k]).to(DEV)):
            assert int(voter.status(fid).item()) & 1, fid
            seen += 1
    assert seen == len(scans)
    roomy = streaming.InstanceVoter(DEV, window=4, device_resident=True)
    for k in range(4):
        for fid, _ in roomy.push(torch.from_numpy(scans[k]).to(DEV), torch.from_numpy(preds[k]).to(DEV), poses[k],
                                 torch.from_numpy(bfs[k]).to(DEV)):
            assert int(roomy.status(fid).item()) == 0


@pytest.fixture(scope="module")
def seg_model():
    return run_sequence.load_model(None, DEV, seg=True)


def test_run_sequence_raises_on_too_many_clusters(tmp_path, seg_model, monkeypatch):
    """12 frames; frames 10 and 11 carry two more 31-point clusters than a voter of 4 boxes holds.  The foreground labels
    are steered (2 on the added points, which are the scan's last rows) so that the clusters are known."""
    n, bad = 12, 10
    seq = tmp_path / "sequences" / "08"
    (seq / "velodyne").mkdir(parents=True)
    added = {}
    for k in range(n):
        blobs = BLOBS + EXTRA if k >= bad else BLOBS
        scan, _, _ = _steered_frame(k, blobs)
        added[scan.shape[0]] = scan.shape[0] - 1920
        scan.tofile(seq / "velodyne" / ("%06d.bin" % k))
    assert len(added) == 2
    kitti.write_poses(seq / "poses.txt", [np.eye(4) for _ in range(n)])
    kitti.write_calibration(seq / "calib.txt")
    push = streaming.InstanceVoter.push

    def steered_push(self, points, preds, pose, bf=None):
        bf = torch.ones_like(bf)
        bf[1920:] = 2
        return push(self, points, preds, pose, bf)

    monkeypatch.setattr(streaming.InstanceVoter, "push", steered_push)
    monkeypatch.setattr(streaming.InstanceVoter, "MAX_BOXES", 4)
    before = threading.active_count()
    with pytest.raises(RuntimeError, match="instance voting: more than 4 clusters in frame %06d" % bad):
        run_sequence.run_sequence(seg_model, str(seq), str(tmp_path / "out"), DEV, vote="instance", frame_point_num=4096,
                                  device_preprocess=True)
    assert threading.active_count() == before
    assert sorted(os.listdir(tmp_path / "out" / "refined")) == ["%06d.label" % k for k in range(bad)]
    monkeypatch.setattr(streaming.InstanceVoter, "MAX_BOXES", ops.MAX_BOXES)          # room for all: every file is written
    run_sequence.run_sequence(seg_model, str(seq), str(tmp_path / "ok"), DEV, vote="instance", frame_point_num=4096,
                              device_preprocess=True)
    assert sorted(os.listdir(tmp_path / "ok" / "refined")) == ["%06d.label" % k for k in range(n)]


def test_push_does_not_wait_for_the_stream():
    seq, window = _steered_sequence(5), 4
    scans, preds, bfs, poses = seq
    dev = [(torch.from_numpy(scans[k]).to(DEV), torch.from_numpy(preds[k]).to(DEV), poses[k], torch.from_numpy(bfs[k]).to(DEV))
           for k in range(5)]
    want = _run_voter(streaming.InstanceVoter(DEV, window=window), seq)[4]
    a = torch.randn((8192, 8192), device=DEV)
    c = torch.empty_like(a)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(a, a, out=c)
    start.record()
    for _ in range(4):
        torch.mm(a, a, out=c)
    stop.record()
    stop.synchronize()
    reps = int(np.ceil(150.0 / (start.elapsed_time(stop) / 4)))           # at least 100 ms of plain work, with a margin
    voter = streaming.InstanceVoter(DEV, window=window, device_resident=True)
    for k in range(4):
        voter.push(*dev[k])                                                   # fills the window (and allocates the scratch)
    torch.cuda.synchronize()
    for _ in range(reps):
        torch.mm(a, a, out=c)
    busy = torch.cuda.Event()
    busy.record()
    ready = voter.push(*dev[4])                                               # frame 4 votes
    waited = busy.query()
    torch.cuda.synchronize()
    assert not waited
    assert [fid for fid, _ in ready] == [4] and np.array_equal(ready[0][1].cpu().numpy(), want)


class _SyncCounter:
    """Counts the host<-device readbacks and stream / device synchronisations the MAIN thread makes.  The runner's one-off
    probe for a concurrent side stream (streaming.concurrent_stream: it times spin kernels, and how many candidates it tries
    varies from run to run) is set-up, not per-frame work, and is left out.  Beyond the counter of
    tests/test_gpu_sequence_overlap.py this one also counts ``nonzero``: the per-frame voter compacts the foreground with it
    in every voted frame, whether the frame has foreground or not."""

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
        for name in ("cpu", "item", "tolist", "__bool__", "nonzero"):         # nonzero: the host waits for the element count
            monkeypatch.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name), on_gpu))
        monkeypatch.setattr(torch, "nonzero", counted(torch.nonzero, on_gpu))
        monkeypatch.setattr(torch.Tensor, "to", counted(torch.Tensor.to, lambda args, out: args[0].is_cuda and
                                                        torch.is_tensor(out) and not out.is_cuda))
        monkeypatch.setattr(torch.cuda, "synchronize", counted(torch.cuda.synchronize, lambda args, out: True))
        monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted(torch.cuda.Stream.synchronize, lambda args, out: True))


def test_main_thread_syncs_do_not_grow_with_instance_voting(tmp_path, seg_model, monkeypatch):
    from tests.test_gpu_sequence_overlap import FPN, _make_sequence
    seq = _make_sequence(tmp_path, 21)
    run_sequence.run_sequence(seg_model, str(seq), str(tmp_path / "warm"), DEV, vote="instance", frame_point_num=FPN, limit=13,
                              device_preprocess=True)
    counts = {}
    for limit in (13, 21):
        with monkeypatch.context() as mp:
            c = _SyncCounter(mp)
            run_sequence.run_sequence(seg_model, str(seq), str(tmp_path / ("out%d" % limit)), DEV, vote="instance",
                                      frame_point_num=FPN, limit=limit, device_preprocess=True)
            counts[limit] = c.n
    assert counts[13] == counts[21], counts

"""Generate tests/golden/copy_paste.npz by running the reference's own copy-paste augmentation on CPU.

Run in the build container only (needs the reference tree, see oracle/ref_import.py):

    python tests/golden/make_copy_paste_golden.py

``in_range``, ``in_hull``, ``compute_box_3d``, ``rotate_along_z``, ``random_f`` and ``SequenceCutPaste`` are pulled out of the
source text of datasets/copy_paste.py (stage 1) and datasets/copy_paste_seg.py (stage 2) and executed, constructor included: the
object bank of tests/copy_paste_cases.py is written to a temporary directory in the reference's layout and loaded from there.
``scipy.spatial.Delaunay`` is the real one.  What is replaced, and by what:
  * ``random.randint`` / ``random.choice`` / ``random.random`` and ``np.random.normal`` / ``np.random.shuffle``: stand-ins that
    hand out the supplied draws (the velocity as the uniform draw ``random_f`` turns into it);
  * ``cv2.getRotationMatrix2D`` (cv2 is not installed): OpenCV's documented formula, as in make_train_prep_golden.py.
``in_hull`` is wrapped by a counter (one call per trial), which is how the accepted trial of each object is read off.
The fixture is data: inputs (the scans by hash), bank, draws and the reference's outputs -- the rows it removed, the rows it
appended and their labels, plus a hash of each whole output array.  No reference source or bytecode is stored.
"""
import os
import sys
import tempfile

import numpy as np
from scipy.spatial import Delaunay

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import ref_import  # noqa: E402
from streammos_amd import kitti, preprocess  # noqa: E402
from tests import copy_paste_cases as cc  # noqa: E402
from tests import train_prep_cases as tc  # noqa: E402
import make_train_prep_golden as base  # noqa: E402

NAMES = ["in_range", "in_hull", "compute_box_3d", "rotate_along_z", "random_f", "SequenceCutPaste"]


class _NumpyStandIn:
    def __init__(self, noise, orders):
        outer = self

        class _Random:
            @staticmethod
            def normal(mean, std, size=None):
                v = outer.noise.take()
                assert (mean, std) == (0, preprocess.PASTE_NOISE_STD) and tuple(size) == v.shape, (mean, std, size, v.shape)
                return v

            @staticmethod
            def shuffle(theta_list):
                assert theta_list == list(range(0, 360, preprocess.PASTE_STEP_DEG))
                theta_list[:] = [preprocess.PASTE_STEP_DEG * int(a) for a in outer.orders.take()]

        self.noise, self.orders, self.random = base._Queue(noise), base._Queue(orders), _Random

    def __getattr__(self, name):
        return getattr(np, name)


class _RandomStandIn:
    def __init__(self, count, choices, uniforms):
        self.count, self.choices, self.uniforms = count, base._Queue(choices), base._Queue(uniforms)

    def randint(self, lo, hi):
        assert lo <= self.count <= hi
        return self.count

    def choice(self, seq):
        v = self.choices.take()
        assert v in seq, (v, seq)
        return v

    def random(self):
        return self.uniforms.take()


def write_bank(bank, root):
    paths = []
    for c in preprocess.PASTE_CATEGORIES:
        os.makedirs(os.path.join(root, c))
    for i, o in enumerate(bank):
        path = os.path.join(root, o.cate, "00_%04d.npz" % i)
        np.savez(path, pcds=o.pcds, center=o.center, size=o.size, yaw=np.float64(o.yaw), cate=o.cate,
                 cate_id=preprocess.PASTE_CATEGORIES.index(o.cate))
        paths.append(path)
    np.savez(os.path.join(root, bank[0].cate, "08_0000.npz"), pcds=bank[0].pcds)       # a validation-sequence file: skipped
    return paths


def run_stage(fname, s, root, paths, bf=None):
    bank, draws = s["bank"], s["draws"]
    sizes = [bank[i].pcds.shape[0] for i in draws.index]
    np_in = _NumpyStandIn([draws.noise[i][t] for i in range(draws.count) for t in range(5)],
                          [draws.order[i] for i in range(draws.count) if sizes[i] >= preprocess.PASTE_MIN_POINTS])
    choices = []
    for i in draws.index:
        choices += [bank[i].cate, paths[i]]
    uniforms = [cc.reference_velocity(bank[draws.index[n]].cate, v)[0] for n, (_, v, _) in enumerate(cc.SAMPLE_SPEC)]
    rand_in = _RandomStandIn(draws.count, choices, uniforms)
    mod = base._extract(os.path.join(ref_import.REF_ROOT, "datasets", fname), NAMES,
                        dict(np=np_in, random=rand_in, cv2=base._cv2_stand_in(), Delaunay=Delaunay, os=os))
    hull_calls = [0]
    real_in_hull = mod.in_hull

    def counting_in_hull(p, hull):
        hull_calls[0] += 1
        return real_in_hull(p, hull)

    mod.in_hull = counting_in_hull
    aug = mod.SequenceCutPaste(root, preprocess.PASTE_MAX_OBJECTS)
    assert sorted(sum(aug.sub_dirs_dic.values(), [])) == sorted(paths)              # the 08_ file was skipped
    sems = [w & np.uint32(0xFFFF) for w in s["words"]]
    pcds = [a.copy() for a in s["aligned"]]
    labels = [preprocess.relabel_lut(x, kitti.learning_map_lut()) for x in sems]
    road = [a[x == 40] for a, x in zip(s["aligned"], sems)]
    raw = [x.copy() for x in sems]
    # __call__ hides the per-object progress; paste_single_obj is what it loops over (copy_paste.py:247-255)
    assert rand_in.randint(0, aug.paste_max_obj_num) == draws.count
    status = []
    for i in range(draws.count):
        pasted_before, calls = int((raw[0] == preprocess.PASTE_RAW_ID).sum()), hull_calls[0]
        if bf is None:
            pcds, labels, raw = aug.paste_single_obj(pcds, labels, road, raw)
        else:
            pcds, labels, bf, raw = aug.paste_single_obj(pcds, labels, bf, road, raw)
        trials = hull_calls[0] - calls
        # the loop breaks at the accepted trial; after 20 trials nothing may have been appended (no object of this sample is
        # accepted at its last trial)
        if trials in (0, preprocess.PASTE_TRIALS):
            assert int((raw[0] == preprocess.PASTE_RAW_ID).sum()) <= pasted_before
            status.append(-1)
        else:
            assert (raw[0][-sizes[i]:] == preprocess.PASTE_RAW_ID).all()
            status.append(trials - 1)
    assert np_in.noise.at == 5 * draws.count and rand_in.uniforms.at == draws.count
    return pcds, labels, bf, raw, status


def split_output(aligned, out):
    """The reference's array = the kept originals in their order, then the appended rows: (removed row indices, tail)."""
    at, kept = 0, []
    for i in range(aligned.shape[0]):
        if at < out.shape[0] and np.array_equal(aligned[i], out[at]):
            kept.append(i)
            at += 1
    removed = np.setdiff1d(np.arange(aligned.shape[0]), np.array(kept, dtype=np.int64))
    return removed.astype(np.int32), out[at:]


def main():
    s = cc.sample()
    bank, draws = s["bank"], s["draws"]
    with tempfile.TemporaryDirectory() as root:
        paths = write_bank(bank, root)
        pcds, labels, _, raw, status = run_stage("copy_paste.py", s, root, paths)
        bf_in = [preprocess.relabel_lut(w & np.uint32(0xFFFF), tc.second_map()) for w in s["words"]]
        pcds2, labels2, bf2, raw2, status2 = run_stage("copy_paste_seg.py", s, root, paths, bf=list(bf_in))
    assert status == status2 and all(np.array_equal(a, b) for a, b in zip(pcds, pcds2))
    assert all(np.array_equal(a, b) for a, b in zip(labels, labels2))
    out = {"scans_sha": np.array(base.sha(*s["scans"])), "pose": np.stack(s["poses"]), "status": np.array(status, dtype=np.int32),
           "draw_index": np.array(draws.index, dtype=np.int32), "draw_velocity": np.array(draws.velocity, dtype=np.float64),
           "draw_order": draws.order, "bank_cate": np.array([o.cate for o in bank])}
    for i, o in enumerate(bank):
        out["bank_pcds_%d" % i], out["bank_center_%d" % i], out["bank_size_%d" % i] = o.pcds, o.center, o.size
        out["bank_yaw_%d" % i] = np.float64(o.yaw)
    for i in range(draws.count):
        out["draw_noise_%d" % i] = draws.noise[i]
    for k in range(5):
        removed, tail = split_output(s["aligned"][k], pcds[k])
        n_kept = s["aligned"][k].shape[0] - removed.shape[0]
        keep = np.ones(s["aligned"][k].shape[0], dtype=bool)
        keep[removed] = False
        sem = s["words"][k] & np.uint32(0xFFFF)
        assert np.array_equal(pcds[k][:n_kept], s["aligned"][k][keep])
        assert np.array_equal(labels[k][:n_kept], preprocess.relabel_lut(sem[keep], kitti.learning_map_lut()))
        assert np.array_equal(bf2[k][:n_kept], bf_in[k][keep]) and np.array_equal(raw[k][:n_kept], sem[keep])
        assert (raw[k][n_kept:] == preprocess.PASTE_RAW_ID).all()
        out["word_%d" % k] = s["words"][k]
        out["removed_%d" % k], out["tail_%d" % k] = removed, tail
        out["tail_label_%d" % k] = labels[k][n_kept:].astype(np.int8)
        out["tail_bf_%d" % k] = bf2[k][n_kept:].astype(np.int8)
        out["out_sha_%d" % k] = np.array(base.sha(pcds[k], labels[k].astype(np.int64), bf2[k].astype(np.int64)))
    assert tuple(status) == cc.EXPECTED, status
    path = os.path.join(HERE, "copy_paste.npz")
    np.savez_compressed(path, **out)
    print("copy_paste %d arrays %.1f KiB, status %s" % (len(out), os.path.getsize(path) / 1024, status))


if __name__ == "__main__":
    main()

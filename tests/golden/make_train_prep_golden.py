"""Generate tests/golden/train_prep.npz by running the reference's own training-sample arithmetic on CPU.

Run in the build container only (needs the reference tree, see oracle/ref_import.py):

    python tests/golden/make_train_prep_golden.py

``Trans``, ``filter_pcds_mask``, ``relabel``, ``random_float``, ``DataAugmentTemp``, ``Quantize``, ``SphereQuantize``
(datasets/utils.py) and ``make_point_feat`` (datasets/data_StreamMOS.py) are pulled out of the reference's source text and
executed; the BEV label grid goes through the reference's deep_point.VoxelMaxPool.  ``DataloadTrain.__getitem__`` itself cannot
run (``np.long``, the dataset walk, the object bank), so its window loop (data_StreamMOS.py:304-346) is restated around those
functions below.  What is replaced, and by what:
  * ``np.random.normal`` / ``np.random.choice`` / ``random.random``: stand-ins that hand out the supplied draws;
  * ``cv2.getRotationMatrix2D`` (cv2 is not installed): OpenCV's documented formula, alpha = scale cos, beta = scale sin,
    [[alpha, beta, (1 - alpha) cx - beta cy], [-beta, alpha, beta cx + (1 - alpha) cy]].
The fixture is data: inputs (the scans by hash), draws and the reference's outputs.  No reference source or bytecode is stored.
"""
import ast
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import train_prep_cases as tc  # noqa: E402


class _Queue:
    def __init__(self, items):
        self.items, self.at = list(items), 0

    def take(self):
        v = self.items[self.at]
        self.at += 1
        return v


class _NumpyStandIn:
    """numpy with ``random`` replaced: normal() hands out the supplied noise, choice() the supplied resampling words."""

    def __init__(self, noise, words):
        outer = self

        class _Random:
            @staticmethod
            def normal(mean, std, size=None):
                v = outer.noise.take()
                assert tuple(size) == v.shape, (size, v.shape)
                return v

            @staticmethod
            def choice(n, size, replace=True):
                w = outer.words.take()
                assert replace and size == w.shape[0]
                return ((w.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)

        self.noise, self.words, self.random = _Queue(noise), _Queue(words), _Random

    def __getattr__(self, name):
        return getattr(np, name)


def _cv2_stand_in():
    cv2 = types.ModuleType("cv2_stand_in")

    def getRotationMatrix2D(center, angle, scale):
        a = angle * np.pi / 180.0
        alpha, beta = scale * np.cos(a), scale * np.sin(a)
        return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]],
                         [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]], dtype=np.float64)

    cv2.getRotationMatrix2D = getRotationMatrix2D
    return cv2


def _extract(path, names, namespace):
    tree = ast.parse(open(path).read(), path)
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    mod = types.ModuleType("smos_ref_" + os.path.basename(path)[:-3])
    mod.__dict__.update(namespace)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), mod.__dict__)
    return mod


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def inverse_random_float(value, v_range):
    """The uniform draw for which random_float (datasets/utils.py:88-91) returns `value` (up to rounding; the fixture stores
    what the reference actually used)."""
    return (value - v_range[0]) / (v_range[1] - v_range[0])


def main():
    import yaml
    ns = ref_import.import_reference()
    scans, words, poses, draws = tc.fixture_inputs()
    n = tc.FIXTURE_N
    aug_cfg = ns.config.get_config()[1].Train.AugParam
    voxel = ns.config.get_config()[0].Voxel
    task_cfg = yaml.safe_load(open(os.path.join(ref_import.REF_ROOT, "datasets", "semantic-kitti.yaml")))

    np_in = _NumpyStandIn([draws.noise[w] for w in range(3)], [draws.words[w, t] for w in range(3) for t in range(3)])
    # uniform draws in the order DataAugmentTemp consumes them on its first call: shift x, y, z, scale, h_flip, v_flip, theta
    uniforms = [inverse_random_float(draws.shift[d], aug_cfg.shift_range[d]) for d in range(3)]
    uniforms += [inverse_random_float(draws.scale, aug_cfg.size_range), 0.25 if draws.h_flip else 0.75, 0.25 if draws.v_flip else 0.75,
                 inverse_random_float(draws.theta_z, aug_cfg.theta_range)]
    rand_q = _Queue(uniforms)
    random_in = types.SimpleNamespace(random=rand_q.take)
    du = _extract(os.path.join(ref_import.REF_ROOT, "datasets", "utils.py"),
                  ["Trans", "filter_pcds_mask", "relabel", "random_float", "DataAugmentTemp", "Quantize", "SphereQuantize"],
                  dict(np=np_in, random=random_in, cv2=_cv2_stand_in()))
    dm = _extract(os.path.join(ref_import.REF_ROOT, "datasets", "data_StreamMOS.py"), ["make_point_feat"], dict(np=np))
    aug = du.DataAugmentTemp(noise_mean=aug_cfg.noise_mean, noise_std=aug_cfg.noise_std, theta_range=aug_cfg.theta_range,
                             shift_range=aug_cfg.shift_range, size_range=aug_cfg.size_range)

    # form_seq (data_StreamMOS.py:213-237)
    inv0 = np.linalg.inv(poses[0])
    pc_list_all, pc_label_list_all = [], []
    for scan, word, pose in zip(scans, words, poses):
        pc_list_all.append(du.Trans(scan, inv0.dot(pose)))
        pc_label_list_all.append(du.relabel(word & 0xFFFF, task_cfg["learning_map"]))

    out = {"draw_words": draws.words, "draw_noise": draws.noise,
           "draw_scalars": None, "pose": np.stack(poses)}
    # the scans are regenerated by tests/train_prep_cases.py (synthetic scans + steering): only their hash is stored, which
    # keeps the file below the largest existing fixture
    out["scans_sha"] = np.array(sha(*scans))
    for k in range(5):
        out["word_%d" % k] = words[k]
    aug_para = {}
    sample_num = 3
    for w in range(len(pc_list_all) - sample_num + 1):                      # __getitem__ (data_StreamMOS.py:304-346)
        pc_list = [p.copy() for p in pc_list_all[w:w + 3]]
        pc_label_list = [p.copy() for p in pc_label_list_all[w:w + 3]]
        if w > 0:
            pose_diff = np.linalg.inv(poses[w]).dot(poses[0])
            for i in range(sample_num):
                pc_list[i] = du.Trans(pc_list[i], pose_diff)
        for ht in range(len(pc_list)):
            mask = du.filter_pcds_mask(pc_list[ht], range_x=voxel.range_x, range_y=voxel.range_y, range_z=voxel.range_z)
            pc_list[ht] = pc_list[ht][mask]
            pc_label_list[ht] = pc_label_list[ht][mask]
        counts = [p.shape[0] for p in pc_list]
        for ht in range(len(pc_list)):
            choice = np_in.random.choice(pc_list[ht].shape[0], n, replace=True)
            pc_list[ht] = pc_list[ht][choice]
            pc_label_list[ht] = pc_label_list[ht][choice]
        pcds_total = np.concatenate(pc_list, axis=0)
        pcds_target = torch.LongTensor(pc_label_list[0].astype(np.int64)).unsqueeze(-1)
        # form_batch (data_StreamMOS.py:159-184)
        pcds_total = aug(pcds_total.copy(), aug_para)
        xyzi = pcds_total[:, :4]
        coord = du.Quantize(xyzi, range_x=voxel.range_x, range_y=voxel.range_y, range_z=voxel.range_z, size=voxel.bev_shape)
        sphere = du.SphereQuantize(xyzi, phi_range=(-180.0, 180.0), theta_range=voxel.RV_theta, size=voxel.rv_shape)
        feat = dm.make_point_feat(xyzi, coord, sphere, voxel)
        feat = torch.FloatTensor(feat.astype(np.float32)).view(3, n, -1, 1).permute(0, 2, 1, 3).contiguous()
        coord = torch.FloatTensor(coord.astype(np.float32)).view(3, n, -1, 1)
        sphere = torch.FloatTensor(sphere.astype(np.float32)).view(3, n, -1, 1)
        # generate_bev_label (data_StreamMOS.py:284-290)
        size = (np.array(voxel.bev_shape[:2]) / 2).astype("int")
        bev = ns.deep_point.VoxelMaxPool(pcds_feat=pcds_target.clone().unsqueeze(0).unsqueeze(0).float(),
                                         pcds_ind=coord[:1, :, :2, :].clone(), output_size=size, scale_rate=(0.5, 0.5))
        bev = bev.to(pcds_target.dtype).squeeze(0).squeeze(0).unsqueeze(-1)
        out["pcds_xyzi_%d" % w], out["pcds_coord_%d" % w] = feat.numpy(), coord.numpy()
        out["pcds_sphere_coord_%d" % w], out["pcds_target_%d" % w] = sphere.numpy(), pcds_target.numpy()
        nz = np.nonzero(bev.numpy().reshape(-1))[0]
        out["pcds_bev_target_%d_idx" % w], out["pcds_bev_target_%d_val" % w] = nz.astype(np.int32), bev.numpy().reshape(-1)[nz].astype(np.int8)
        out["counts_%d" % w] = np.array(counts, dtype=np.int32)
    # the scalars the reference's augmentation actually used (its aug_para dict after the loop)
    out["draw_scalars"] = np.array(list(aug_para["shift_xyz"]) + [aug_para["scale"], aug_para["h_flip"], aug_para["v_flip"],
                                                                    aug_para["theta_z"]], dtype=np.float64)
    assert rand_q.at == len(uniforms) and np_in.noise.at == 3 and np_in.words.at == 9
    assert min(int(out["counts_%d" % w].min()) for w in range(3)) == 1          # the lone-point frame is in the fixture
    path = os.path.join(HERE, "train_prep.npz")
    np.savez_compressed(path, **out)
    print("train_prep %d arrays %.1f KiB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()

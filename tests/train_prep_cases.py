"""Inputs, draws and independent references for the training sample builder (streammos_amd.preprocess.build_train_sample,
streammos_amd.device_preprocess.DeviceTrainPreprocessor).  Everything here is a pure function of its arguments."""
import numpy as np

from streammos_amd import kitti, preprocess, synth

FIXTURE_N = 512
# (name, beams, azimuth, N, options): every device-against-host case of tests/test_gpu_train_prep.py
DEVICE_CASES = (
    ("n2048", 16, 120, 2048, dict(v_flip=0, h_flip=0, theta_z=37.123, lone=True)),
    ("n1000_pushed_out", 16, 120, 1000, dict(v_flip=1, h_flip=0, theta_z=90.0, shift=(30.0, -40.0, 0.3), scale=1.5, empty=True)),
    ("n1_no_noise", 16, 120, 1, dict(v_flip=0, h_flip=1, theta_z=-180.0, noise_std=0.0, lone=True)),
    ("one_point_scans", 1, 1, 64, dict(v_flip=1, h_flip=1, theta_z=0.0)),
    ("full_size", 64, 1875, 130000, dict(v_flip=1, h_flip=1, theta_z=37.123, lone=True)),
)
# semantic ids of the label words: unlabeled, static and moving ids of the learning map, the last entry of the 360-entry
# table, ids past it (the reference's relabel leaves an id its map does not name at 0)
SEM_IDS = np.array([0, 1, 9, 40, 44, 99, 251, 252, 259, 359, 360, 400, 65535], dtype=np.uint32)


def second_map():
    """A stage-2 style second label map (the movable-object map of data_StreamMOS_seg.py has the same form): distinguishable
    from the learning map, non-zero at the table's last entry."""
    lut = np.zeros(360, dtype=np.int32)
    lut[[9, 40, 251, 252]] = (2, 1, 1, 2)
    lut[359] = 2
    return lut


def label_maps(two=False):
    maps = {"pcds_target": kitti.learning_map_lut()}
    if two:
        maps["pcds_bf_target"] = second_map()
    return maps


def sample_inputs(beams=16, azimuth=120, lone=False, empty=False):
    """Five scans in meta_list_raw order (frames 6, 5, 4, 3, 2 of the synthetic sequence), label words with instance bits in
    the high half, poses.  Steering (scans of at least 64 points):
      * scan 0 (frame 0 of window 0): points exactly on the six faces of the half-open range and one float32 step inside;
      * scan 2 (in all three windows): points that land on or next to a face after window 1's / window 2's second alignment
        (the inverse of the two alignments applied to a face point, rounded to float32);
      * lone: scan 4 (frame 2 of window 2) has exactly one in-range point; empty: it has none."""
    idx = preprocess.train_window_indices(6, 12)
    scans = [synth.synthetic_scan(k, beams, azimuth) for k in idx]
    poses = [synth.synthetic_pose(k) for k in idx]
    rng = np.random.Generator(np.random.PCG64(9100 + beams))
    words = [(SEM_IDS[rng.integers(0, SEM_IDS.shape[0], s.shape[0])] | (rng.integers(0, 1 << 16, s.shape[0]).astype(np.uint32) << np.uint32(16)))
             for s in scans]
    faces = np.array([[-50.0, 0, 0], [50.0, 0, 0], [49.999996, 1, -4.0], [0, -50.0, 1.9999999], [0, 50.0, 0], [0, 49.999996, 0],
                      [1, 1, 2.0], [1, 1, -4.0000005], [-50.000004, 2, 0]], dtype=np.float32)
    if scans[0].shape[0] >= 64:
        scans[0][:faces.shape[0], :3] = faces
        inv0 = np.linalg.inv(poses[0])
        at = faces.shape[0]
        for w in (1, 2):
            both = np.linalg.inv(poses[w]).dot(poses[0]).dot(inv0.dot(poses[2]))
            back = np.linalg.inv(both)
            src = back[:3, :3].dot(faces.astype(np.float64).T).T + back[:3, 3]
            scans[2][at:at + faces.shape[0], :3] = src.astype(np.float32)
            at += faces.shape[0]
        if lone or empty:
            scans[4][:, 2] += np.float32(1000.0)
        if lone:
            scans[4][7, 2] -= np.float32(1000.0)
            scans[4][7, :3] = (3.0, -2.0, -1.0)
    return scans, words, poses


def explicit_draws(n, seed, v_flip=0, h_flip=0, theta_z=37.123, shift=(1.2345678912, -2.7182818284, 0.1414213562), scale=1.0314159265, noise_std=0.0001, noise_mean=0.0):
    """Draws from numpy's generator (nothing to do with the seeded device generator): words cover the whole 32-bit range
    and include both ends.  The default shift and scale are not float32 numbers, like the reference's random doubles: a float64
    shift then rounds differently from the float32 one."""
    rng = np.random.Generator(np.random.PCG64(seed))
    words = rng.integers(0, 1 << 32, (3, 3, n), dtype=np.uint64).astype(np.uint32)
    words[:, :, 0] = 0xFFFFFFFF
    if n > 1:
        words[:, :, 1] = 0
    noise = rng.normal(noise_mean, noise_std, (3, 3 * n, 3)) if noise_std > 0 else np.full((3, 3 * n, 3), float(noise_mean))
    return preprocess.TrainDraws(words, noise, shift, scale, h_flip, v_flip, theta_z)


def device_case(name):
    for cname, beams, azimuth, n, opt in DEVICE_CASES:
        if cname == name:
            opt = dict(opt)
            scans, words, poses = sample_inputs(beams, azimuth, lone=opt.pop("lone", False), empty=opt.pop("empty", False))
            return scans, words, poses, n, explicit_draws(n, 77 + n, **opt)
    raise KeyError(name)


def fixture_inputs():
    """What tests/golden/make_train_prep_golden.py feeds the reference (no empty frame: the reference raises there)."""
    scans, words, poses = sample_inputs(16, 120, lone=True)
    return scans, words, poses, explicit_draws(FIXTURE_N, 4242, v_flip=1, h_flip=0, theta_z=-63.5)


# ---- Philox4x32-10: an independent implementation in Python integers (one counter at a time) -----------------------------
def philox4x32_int(counter, key, rounds=10):
    c, k = [int(v) for v in counter], [int(v) for v in key]
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


# (counter, key) -> output, computed once with philox4x32_int; the first and third are the known-answer vectors of the
# generator's authors (Random123 kat_vectors: zeros, and the digits of pi)
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


# ---- Box-Muller ---------------------------------------------------------------------------------------------------------
# Bound on |z32 - z64| for z = r cos(a), r = sqrt(-2 ln u1), a = 2 pi u2, evaluated in float32 against float64 from the same
# words (u1 = ((w1 >> 8) + 1) 2^-24 and u2 = (w2 >> 8) 2^-24 are exact in both):
#   r <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.77
#   angle: float32(2 pi) is off by 1.7e-7 relative and the product rounds once more: |da| <= 2 pi 2^-24 + 2^-23 (a < 2 pi),
#          and a float32 cos adds a few 2^-24 absolute                              -> |d cos| <= ~7e-7, times r: 4e-6
#   radius: ln, the product with -2 and sqrt each round once; the relative error of r is a few 2^-24 except near u1 = 1,
#          where ln u1 -> 0 loses nothing (u1 exact, ln correctly scaled)            -> |dr| <= ~1e-6
#   the final product rounds once more: 5.77 * 2^-24 = 3.4e-7
# Sum about 6e-6; the bar leaves a factor of three for the libraries' ulp errors.
BOX_MULLER_BOUND = 2e-5


def box_muller_f64(w1, w2):
    u1 = ((np.asarray(w1) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (np.asarray(w2) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def seeded_z64(seed, sample_index, n):
    """float64 Box-Muller of the words the seeded generator uses for its noise: [3, 3*n, 3] in units of noise_std."""
    w = preprocess.seeded_words(seed, sample_index, n)
    z = np.stack((box_muller_f64(w[0, ..., 2], w[0, ..., 3]), box_muller_f64(w[1, ..., 0], w[1, ..., 1]),
                  box_muller_f64(w[1, ..., 2], w[1, ..., 3])), axis=-1)
    return z.reshape(3, 3 * n, 3)


# 99.9 % quantile of chi-square with 15 degrees of freedom (16 bins)
CHI2_15_999 = 37.697


def compare_sample(got, want, n_maps_keys=("pcds_target",)):
    """Mismatch report of two sample dicts: exact keys -> number of differing values; the range-view angles of the whole sample
    (one build: three windows) -> (max abs difference, fraction in the same half cell), the two figures
    tests/test_gpu_preprocess.py takes over the whole output of one build."""
    exact, diff, same = {}, [], []
    for i in range(3):
        for k in ("pcds_xyzi", "pcds_coord", "pcds_bev_target") + tuple(n_maps_keys):
            a, b = np.asarray(got["%s_%d" % (k, i)]), np.asarray(want["%s_%d" % (k, i)])
            assert a.shape == b.shape and a.dtype == b.dtype, (k, i, a.shape, b.shape, a.dtype, b.dtype)
            exact["%s_%d" % (k, i)] = int((a != b).sum())
        a, b = np.asarray(got["pcds_sphere_coord_%d" % i]), np.asarray(want["pcds_sphere_coord_%d" % i])
        assert a.shape == b.shape and a.dtype == b.dtype
        diff.append(np.abs(a - b).reshape(-1))
        same.append((np.floor(a * 0.5) == np.floor(b * 0.5)).reshape(-1))
    return exact, (float(np.concatenate(diff).max()), float(np.concatenate(same).mean()))

MUTANTS = ("single_alignment_rounding", "filter_before_second_alignment", "noise_after_shift", "float64_shift", "flips_swapped",
           "rotation_sign_flipped", "target_from_frame_1", "scalars_redrawn_per_window")


def restated_sample(scans, words, poses, n, spec, draws, mutant=None):
    """A second, compact restatement of the window loop with one deliberate error per `mutant` (None: no error, equal to
    preprocess.build_train_sample).  It shows that the fixture tells each of these orderings and roundings apart."""
    f = np.float32
    inv0 = np.linalg.inv(poses[0])
    lut = kitti.learning_map_lut()
    out = {}
    for w in range(3):
        second = np.linalg.inv(poses[w]).dot(poses[0]) if w > 0 else None
        frames, sems = [], []
        for t in range(3):
            k = w + t
            first = preprocess.pose_align(scans[k], inv0.dot(poses[k]))
            if second is None:
                pts = first
            elif mutant == "single_alignment_rounding":
                pts = preprocess.pose_align(scans[k], second.dot(inv0.dot(poses[k])))
            else:
                pts = preprocess.pose_align(first, second)
            keep = preprocess.range_mask(first if mutant == "filter_before_second_alignment" else pts, spec)
            choice = preprocess.resample_choice(draws.words[w, t], int(keep.sum()))
            frames.append(pts[keep][choice])
            sems.append((words[k] & np.uint32(0xFFFF))[keep][choice])
        p = np.concatenate(frames, axis=0)
        shift, scale, theta = np.array(draws.shift), draws.scale, draws.theta_z
        if mutant == "scalars_redrawn_per_window" and w > 0:
            shift, scale, theta = shift + 0.01 * w, scale + 0.001 * w, theta + 0.5 * w
        xyz = p[:, :3].astype(np.float64)
        if mutant == "noise_after_shift":
            xyz = ((xyz.astype(f) + shift.astype(f)).astype(np.float64) + draws.noise[w]).astype(f)
        elif mutant == "float64_shift":
            xyz = ((xyz + draws.noise[w]).astype(f).astype(np.float64) + shift).astype(f)
        else:
            xyz = (xyz + draws.noise[w]).astype(f) + shift.astype(f)
        xyz = xyz * f(scale)
        flip_x, flip_y = (draws.h_flip, draws.v_flip) if mutant == "flips_swapped" else (draws.v_flip, draws.h_flip)
        x = (-xyz[:, 0] if flip_x else xyz[:, 0]).astype(np.float64)
        y = (-xyz[:, 1] if flip_y else xyz[:, 1]).astype(np.float64)
        c, s = np.cos(theta * np.pi / 180.0), np.sin(theta * np.pi / 180.0)
        if mutant == "rotation_sign_flipped":
            s = -s
        p = p.copy()
        p[:, 0], p[:, 1], p[:, 2] = (x * c + y * s).astype(f), (y * c - x * s).astype(f), xyz[:, 2]
        feat, bev, sph = preprocess.form_batch(p, 3, spec)
        tgt = preprocess.relabel_lut(sems[1 if mutant == "target_from_frame_1" else 0], lut)
        out["pcds_xyzi_%d" % w], out["pcds_coord_%d" % w], out["pcds_sphere_coord_%d" % w] = feat, bev, sph
        out["pcds_target_%d" % w] = tgt[:, None]
        out["pcds_bev_target_%d" % w] = preprocess.bev_label_grid(tgt, bev[0, :, :2, 0], spec)
    return out


def fixture_sample(g):
    """The reference's outputs as stored in tests/golden/train_prep.npz -> a sample dict (BEV grids are stored sparse)."""
    out = {}
    for w in range(3):
        for k in ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord", "pcds_target"):
            out["%s_%d" % (k, w)] = g["%s_%d" % (k, w)]
        grid = np.zeros(256 * 256, dtype=np.int64)
        grid[g["pcds_bev_target_%d_idx" % w]] = g["pcds_bev_target_%d_val" % w]
        out["pcds_bev_target_%d" % w] = grid.reshape(256, 256, 1)
    return out


def fixture_draws(g):
    sc = g["draw_scalars"]
    return preprocess.TrainDraws(g["draw_words"], g["draw_noise"], sc[:3], sc[3], int(sc[4]), int(sc[5]), sc[6])

"""Host-side (numpy) validation/test preprocessing that feeds ``AttNet.infer``.

Restates what ``DataloadVal`` does to a window of scans (reference: datasets/data_StreamMOS.py:397-599
and datasets/utils.py:98-192) without the disk walk: pose-align T scans, range-filter, pad to a fixed
point count, 4 test-time-augmentation flips, BEV / range-view quantisation and the 7-channel point
feature.  All arithmetic is float32 exactly where the reference's numpy is float32, and float64 only in
the pose transform (datasets/utils.py:116-126).

Second half: the training sample of ``DataloadTrain.__getitem__`` (datasets/data_StreamMOS.py:292-364) without copy-paste,
``build_train_sample``, with the random draws as an input, and the host restatement of the seeded draws the device builder
(csrc/train_prep.hip) generates.  It is the host path: there is no C twin.
"""
import numpy as np

PAD_XYZI = -1000.0     # datasets/data_StreamMOS.py:567
PAD_Z = -4000.0        # datasets/data_StreamMOS.py:568
TTA_SIGNS = ((1, 1), (1, -1), (-1, 1), (-1, -1))   # x_sign outer, y_sign inner (data_StreamMOS.py:495-496)


class VoxelSpec:
    """Grid definition = ``General.Voxel`` of the reference config (config/StreamMOS.py:12-19)."""

    def __init__(self, range_x=(-50.0, 50.0), range_y=(-50.0, 50.0), range_z=(-4.0, 2.0),
                 bev_shape=(512, 512, 30), rv_shape=(64, 2048), RV_theta=(-25.0, 3.0)):
        self.range_x, self.range_y, self.range_z = tuple(range_x), tuple(range_y), tuple(range_z)
        self.bev_shape, self.rv_shape, self.RV_theta = tuple(bev_shape), tuple(rv_shape), tuple(RV_theta)

    @classmethod
    def from_config(cls, voxel_cfg):
        return cls(voxel_cfg.range_x, voxel_cfg.range_y, voxel_cfg.range_z,
                   voxel_cfg.bev_shape, voxel_cfg.rv_shape, voxel_cfg.RV_theta)


def pose_align(scan, pose_diff):
    """datasets/utils.py:116-126 (Trans): homogeneous transform in float64 with w forced to 1, result
    stored back as float32; intensity (and any further column) is carried through untouched."""
    homo = np.ones((4, scan.shape[0]), dtype=scan.dtype)
    homo[:3] = scan[:, :3].T
    moved = np.asarray(pose_diff, dtype=np.float64).dot(homo)
    out = scan.copy()
    out[:, :3] = moved[:3].T
    return out


def range_mask(scan, spec):
    """datasets/utils.py:107-113: half-open box lo <= p < hi on x, y, z."""
    keep = np.ones(scan.shape[0], dtype=bool)
    for d, (lo, hi) in enumerate((spec.range_x, spec.range_y, spec.range_z)):
        keep &= (scan[:, d] >= lo) & (scan[:, d] < hi)
    return keep


def pad_scan(scan, frame_point_num):
    """datasets/data_StreamMOS.py:563-572: constant pad with -1000 (z column -4000)."""
    pad = frame_point_num - scan.shape[0]
    if pad <= 0:
        raise ValueError("scan has %d in-range points, frame_point_num=%d leaves no padding "
                         "(the reference asserts pad_length > 0)" % (scan.shape[0], frame_point_num))
    tail = np.full((pad, scan.shape[1]), PAD_XYZI, dtype=scan.dtype)
    tail[:, 2] = PAD_Z
    return np.concatenate((scan, tail), axis=0), pad


def quantize_bev(xyz, spec):
    """datasets/utils.py:151-169: (p - lo) / cell in float32, no floor."""
    cols = []
    for d, (rng, size) in enumerate(zip((spec.range_x, spec.range_y, spec.range_z), spec.bev_shape)):
        cell = (rng[1] - rng[0]) / size
        cols.append((xyz[:, d] - rng[0]) / cell)
    return np.stack(cols, axis=-1)


def quantize_sphere(xyz, spec):
    """datasets/utils.py:172-192: (theta_quan, phi_quan) over a 64 x 2048 range image."""
    h, w = spec.rv_shape
    phi_hi = 180.0 * np.pi / 180.0
    phi_lo = -180.0 * np.pi / 180.0
    th_lo = spec.RV_theta[0] * np.pi / 180.0
    th_hi = spec.RV_theta[1] * np.pi / 180.0
    dphi = (phi_hi - phi_lo) / w
    dtheta = (th_hi - th_lo) / h
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    d = np.sqrt(x ** 2 + y ** 2 + z ** 2) + 1e-12
    phi_q = (phi_hi - np.arctan2(x, y)) / dphi
    theta_q = (th_hi - np.arcsin(z / d)) / dtheta
    return np.stack((theta_q, phi_q), axis=-1)


def point_features(xyzi, bev_coord):
    """datasets/data_StreamMOS.py:25-50: (x, y, z, intensity, dist, frac(x_quan), frac(y_quan))."""
    x, y, z = xyzi[:, 0], xyzi[:, 1], xyzi[:, 2]
    dist = np.sqrt(x ** 2 + y ** 2 + z ** 2) + 1e-12
    fx = bev_coord[:, 0] - np.floor(bev_coord[:, 0])
    fy = bev_coord[:, 1] - np.floor(bev_coord[:, 1])
    return np.stack((x, y, z, xyzi[:, 3], dist, fx, fy), axis=-1)


def form_batch(stacked, seq_num, spec):
    """One TTA variant: stacked = (T*N, 4) float32 -> xyzi (T,7,N,1), coord (T,N,3,1), sphere (T,N,2,1)."""
    n = stacked.shape[0] // seq_num
    xyzi = stacked[:, :4]
    bev = quantize_bev(xyzi, spec)
    sph = quantize_sphere(xyzi, spec)
    feat = point_features(xyzi, bev).astype(np.float32)
    feat = np.ascontiguousarray(feat.reshape(seq_num, n, 7).transpose(0, 2, 1))[..., None]
    bev = bev.astype(np.float32).reshape(seq_num, n, 3, 1)
    sph = sph.astype(np.float32).reshape(seq_num, n, 2, 1)
    return feat, bev, sph


def window_indices(i, n_frames, seq_num):
    """Which scans make up sample i (datasets/data_StreamMOS.py:424-467, ``meta_list_raw``): frames
    i, i-1, ..., except that the first seq_num-1 samples look forward instead."""
    if i < seq_num - 1:
        return [i + ht for ht in range(seq_num)]
    return [i - ht for ht in range(seq_num)]


def build_sample(scans, poses, frame_point_num, spec, tta=True):
    """scans: list of T raw (n_t,4) float32 scans, current first; poses: matching 4x4 float64 poses.

    Returns a dict with the arrays ``AttNet.infer`` consumes *without* the DataLoader's leading
    batch dim: pcds_xyzi (B,T,7,N,1), pcds_coord (B,T,N,3,1), pcds_sphere_coord (B,T,N,2,1) with
    B = 4 TTA variants (or 1), plus valid_mask (current scan) and pad_length.
    """
    seq_num = len(scans)
    inv_cur = np.linalg.inv(poses[0])
    aligned, masks, pads = [], [], []
    for scan, pose in zip(scans, poses):
        moved = pose_align(scan, inv_cur.dot(pose))
        keep = range_mask(moved, spec)
        padded, pad = pad_scan(moved[keep], frame_point_num)
        aligned.append(padded)
        masks.append(keep)
        pads.append(pad)
    stacked = np.concatenate(aligned, axis=0)
    feats, bevs, sphs = [], [], []
    for sx, sy in (TTA_SIGNS if tta else TTA_SIGNS[:1]):
        flipped = stacked.copy()
        flipped[:, 0] *= sx
        flipped[:, 1] *= sy
        f, b, s = form_batch(flipped, seq_num, spec)
        feats.append(f)
        bevs.append(b)
        sphs.append(s)
    return {
        "pcds_xyzi": np.stack(feats, axis=0),
        "pcds_coord": np.stack(bevs, axis=0),
        "pcds_sphere_coord": np.stack(sphs, axis=0),
        "valid_mask": masks[0],
        "pad_length": pads[0],
    }


# ---- training samples (DataloadTrain.__getitem__, datasets/data_StreamMOS.py:292-364) --------------------------------------
TRAIN_FRAMES = 5        # scans of one training sample: config seq_num + 2 (data_StreamMOS.py:79)
TRAIN_WINDOWS = 3       # chained windows of seq_num = 3 frames (data_StreamMOS.py:305-307)
_M32 = 0xFFFFFFFF


class AugParam:
    """``DatasetParam.Train.AugParam`` of the reference config (config/StreamMOS.py:35-40)."""

    def __init__(self, noise_mean=0, noise_std=0.0001, theta_range=(-180.0, 180.0),
                 shift_range=((-3, 3), (-3, 3), (-0.4, 0.4)), size_range=(0.95, 1.05)):
        self.noise_mean, self.noise_std = noise_mean, noise_std
        self.theta_range, self.size_range = tuple(theta_range), tuple(size_range)
        self.shift_range = tuple(tuple(r) for r in shift_range)

    @classmethod
    def from_config(cls, aug_cfg):
        return cls(aug_cfg.noise_mean, aug_cfg.noise_std, aug_cfg.theta_range, aug_cfg.shift_range, aug_cfg.size_range)


class TrainDraws:
    """The random draws of one training sample.

    words uint32 [3, T, N]: slot j of frame t of window w takes kept point ``(words * n_valid) >> 32``;
    noise float64 [3, T*N, 3]: the additive noise of each window's stacked points;
    shift (3 floats), scale, h_flip, v_flip, theta_z (degrees): drawn once per sample, shared by its windows (the
    reference's ``aug_para`` dict lives across the window loop)."""

    def __init__(self, words, noise, shift, scale, h_flip, v_flip, theta_z):
        self.words, self.noise = words, noise
        self.shift = tuple(float(v) for v in shift)
        self.scale, self.theta_z = float(scale), float(theta_z)
        self.h_flip, self.v_flip = int(h_flip), int(v_flip)


def train_window_indices(i, n_frames, seq_num=3):
    """Which scans make up training sample i (``meta_list_raw``, datasets/data_StreamMOS.py:96-138): seq_num + 2 frames,
    i, i-1, ... except that the first seq_num + 1 samples look forward instead."""
    total = seq_num + 2
    if i < total - 1:
        return [i + ht for ht in range(total)]
    return [i - ht for ht in range(total)]


def philox4x32(counter, key, rounds=10):
    """Philox4x32 (Salmon et al., SC'11) on arrays: counter [..., 4] and key [..., 2] of 32-bit words -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask, sh = np.uint64(_M32), np.uint64(32)
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & mask, (p0 >> sh) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(0x9E3779B9)) & mask, (k[1] + np.uint64(0xBB67AE85)) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def box_muller_f32(w1, w2):
    """The kernels' float32 Box-Muller (cosine branch): u1 = ((w1 >> 8) + 1) 2^-24 in (0, 1], u2 = (w2 >> 8) 2^-24."""
    f = np.float32
    u1 = ((w1 >> np.uint32(8)) + np.uint32(1)).astype(f) * f(2.0 ** -24)
    u2 = (w2 >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    return np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(6.2831855) * u2)


def seeded_words(seed, sample_index, frame_point_num, seq_num=3):
    """The two Philox calls per slot (layout: include/smos.h): returns uint32 [2, 3, T, N, 4]."""
    n = int(frame_point_num)
    w, t, j = np.meshgrid(np.arange(TRAIN_WINDOWS, dtype=np.uint64), np.arange(seq_num, dtype=np.uint64),
                          np.arange(n, dtype=np.uint64), indexing="ij")
    key = np.array([int(seed) & _M32, (int(seed) >> 32) & _M32], dtype=np.uint64)
    out = []
    for call in (0, 1):
        c1 = (np.uint64(call) << np.uint64(16)) | (w << np.uint64(8)) | t
        ctr = np.stack((j, c1, np.full_like(j, int(sample_index) & _M32), np.full_like(j, (int(sample_index) >> 32) & _M32)), axis=-1)
        out.append(philox4x32(ctr, key))
    return np.stack(out, axis=0)


def seeded_scalars(seed, sample_index, aug):
    """The five per-sample scalars: ``random.Random`` seeded with (seed, sample index), drawn in the order and with the
    formula of DataAugmentTemp.__call__ / random_float (datasets/utils.py:88-91,291-338)."""
    import random
    rng = random.Random((int(seed) << 64) | int(sample_index))

    def random_float(v_range):
        v = rng.random()
        return v * (v_range[1] - v_range[0]) + v_range[0]

    shift = [random_float(aug.shift_range[i]) for i in range(3)]
    scale = random_float(aug.size_range)
    h_flip = 1 if rng.random() < 0.5 else 0
    v_flip = 1 if rng.random() < 0.5 else 0
    theta_z = random_float(aug.theta_range)
    return shift, scale, h_flip, v_flip, theta_z


def draws_from_seed(seed, sample_index, frame_point_num, aug=None, seq_num=3):
    """Host restatement of the seeded draws: a function of (seed, sample index, window, frame, slot) only.  The words equal
    the kernels' bit for bit; the noise goes through numpy's float32 log / cos, which may differ from the device's in the last
    bits (bound: tests/train_prep_cases.py)."""
    aug = aug or AugParam()
    w = seeded_words(seed, sample_index, frame_point_num, seq_num)
    f = np.float32
    z = np.stack((box_muller_f32(w[0, ..., 2], w[0, ..., 3]), box_muller_f32(w[1, ..., 0], w[1, ..., 1]),
                  box_muller_f32(w[1, ..., 2], w[1, ..., 3])), axis=-1)
    noise = (z * f(aug.noise_std) + f(aug.noise_mean)).astype(np.float64)
    shift, scale, h_flip, v_flip, theta_z = seeded_scalars(seed, sample_index, aug)
    return TrainDraws(np.ascontiguousarray(w[0, ..., 0]), noise.reshape(TRAIN_WINDOWS, seq_num * int(frame_point_num), 3),
                      shift, scale, h_flip, v_flip, theta_z)


def resample_choice(words, n_valid):
    """(uint64(r) * n_valid) >> 32: an index < n_valid for every 32-bit word r."""
    return ((np.asarray(words).astype(np.uint64) * np.uint64(n_valid)) >> np.uint64(32)).astype(np.int64)


def relabel_lut(sem, lut):
    """utils.relabel through a table: an id the table does not reach is 0, as an id the reference's map does not name."""
    sem = np.asarray(sem).astype(np.int64)
    lut = np.asarray(lut)
    return np.where(sem < lut.shape[0], lut[np.minimum(sem, lut.shape[0] - 1)], 0).astype(np.int64)


def augment(stacked, noise, draws):
    """DataAugmentTemp.__call__ (datasets/utils.py:280-343) in explicit elementwise operations; stacked (T*N, 4) float32."""
    f = np.float32
    out = stacked.copy()
    out[:, :3] = (out[:, :3].astype(np.float64) + noise).astype(f)                   # float64 add, one rounding
    for d in range(3):
        out[:, d] = out[:, d] + f(draws.shift[d])                                    # float32 add
    out[:, :3] = out[:, :3] * f(draws.scale)                                         # float32 multiply
    if draws.v_flip == 1:
        out[:, 0] = -out[:, 0]
    if draws.h_flip == 1:
        out[:, 1] = -out[:, 1]
    ang = draws.theta_z * np.pi / 180.0                                              # cv2.getRotationMatrix2D: alpha = cos, beta = sin
    c, s = np.cos(ang), np.sin(ang)
    x, y = out[:, 0].astype(np.float64), out[:, 1].astype(np.float64)
    out[:, 0] = (x * c + y * s).astype(f)
    out[:, 1] = (y * c - x * s).astype(f)
    return out


def bev_label_grid(target, coord_xy, spec):
    """generate_bev_label (data_StreamMOS.py:284-290): VoxelMaxPool of frame 0's labels onto bev_shape / 2 at scale 0.5, with
    the scatter's cell rule (cell = int(float32(coord) * 0.5) truncated toward zero, kept iff 0 <= cell < size); empty = 0."""
    size = (spec.bev_shape[0] // 2, spec.bev_shape[1] // 2)
    p = coord_xy.astype(np.float32) * np.float32(0.5)
    keep = (p[:, 0] > -1) & (p[:, 0] < size[0]) & (p[:, 1] > -1) & (p[:, 1] < size[1])
    cell = p[keep].astype(np.int64)
    grid = np.zeros(size, dtype=np.int64)
    np.maximum.at(grid, (cell[:, 0], cell[:, 1]), np.asarray(target)[keep])
    return grid[..., None]


def build_train_sample(scans, label_words, poses, frame_point_num, spec, aug, draws, label_maps=None, aligned=False):
    """One training sample without copy-paste.  scans: 5 raw (n_k, 4) float32 scans in ``meta_list_raw`` order, label_words:
    their uint32 label words, poses: their 4x4 float64 poses, draws: TrainDraws.  label_maps: name -> LUT, one target per
    entry, the BEV label grid from the first (default: ``pcds_target`` through the SemanticKITTI learning map).

    Returns the reference's dict for one sample, keys ``pcds_xyzi_i`` (T,7,N,1), ``pcds_coord_i`` (T,N,3,1),
    ``pcds_sphere_coord_i`` (T,N,2,1) float32, ``pcds_target_i`` (N,1) and ``pcds_bev_target_i`` (256,256,1) int64 for the
    windows i = 0..2, plus ``in_range_counts`` (3,T).  A frame without in-range points, where the reference raises, is the
    validation padding point with label 0 and a zero count.  ``aug`` supplies nothing the draws do not: it is accepted so that
    the call reads like the device builder's.  aligned=True: the scans already went through the first alignment (float32 in
    frame 0's coordinates, the state in which the reference's copy-paste augmentation edits them); only the windows' second
    alignment is applied."""
    from . import kitti
    if len(scans) != TRAIN_FRAMES or len(label_words) != TRAIN_FRAMES or len(poses) != TRAIN_FRAMES:
        raise ValueError("a training sample is built from %d scans, label arrays and poses" % TRAIN_FRAMES)
    label_maps = label_maps or {"pcds_target": kitti.learning_map_lut()}
    seq_num = TRAIN_FRAMES - TRAIN_WINDOWS + 1
    n_out = int(frame_point_num)
    inv0 = np.linalg.inv(poses[0])
    first = [np.asarray(s, dtype=np.float32) if aligned else pose_align(np.asarray(s, dtype=np.float32), inv0.dot(p))
             for s, p in zip(scans, poses)]                                                                    # float32
    sems = [np.asarray(w).astype(np.uint32) & np.uint32(0xFFFF) for w in label_words]
    out = {"in_range_counts": np.zeros((TRAIN_WINDOWS, seq_num), dtype=np.int32)}
    for w in range(TRAIN_WINDOWS):
        frames, frame_sems = [], []
        second = np.linalg.inv(poses[w]).dot(poses[0]) if w > 0 else None
        for t in range(seq_num):
            pts = first[w + t] if second is None else pose_align(first[w + t], second)                         # second rounding
            keep = range_mask(pts, spec)
            n_valid = int(keep.sum())
            out["in_range_counts"][w, t] = n_valid
            if n_valid == 0:
                pad = np.full((n_out, 4), PAD_XYZI, dtype=np.float32)
                pad[:, 2] = PAD_Z
                frames.append(pad)
                frame_sems.append(None)
                continue
            choice = resample_choice(draws.words[w, t], n_valid)
            frames.append(pts[keep][choice])
            frame_sems.append(sems[w + t][keep][choice])
        stacked = augment(np.concatenate(frames, axis=0), draws.noise[w], draws)
        for t in range(seq_num):
            if frame_sems[t] is None:
                stacked[t * n_out:(t + 1) * n_out] = frames[t]
        feat, bev, sph = form_batch(stacked, seq_num, spec)
        out["pcds_xyzi_%d" % w], out["pcds_coord_%d" % w], out["pcds_sphere_coord_%d" % w] = feat, bev, sph
        for i, (name, lut) in enumerate(label_maps.items()):
            tgt = np.zeros(n_out, dtype=np.int64) if frame_sems[0] is None else relabel_lut(frame_sems[0], lut)
            out["%s_%d" % (name, w)] = tgt[:, None]
            if i == 0:
                out["pcds_bev_target_%d" % w] = bev_label_grid(tgt, bev[0, :, :2, 0], spec)
    return out

"""Host-side (numpy) validation/test preprocessing that feeds ``AttNet.infer``.

Restates what ``DataloadVal`` does to a window of scans (reference: datasets/data_StreamMOS.py:397-599
and datasets/utils.py:98-192) without the disk walk: pose-align T scans, range-filter, pad to a fixed
point count, 4 test-time-augmentation flips, BEV / range-view quantisation and the 7-channel point
feature.  All arithmetic is float32 exactly where the reference's numpy is float32, and float64 only in
the pose transform (datasets/utils.py:116-126).

Second half: the training sample of ``DataloadTrain.__getitem__`` (datasets/data_StreamMOS.py:292-364) behind its copy-paste
step, ``build_train_sample``, with the random draws as an input, and the host restatement of the seeded draws the device builder
(csrc/train_prep.hip) generates.  It is the host path: there is no C twin.

Last part: that copy-paste step (``SequenceCutPaste``, datasets/copy_paste.py), ``copy_paste_sample``, again with explicit
draws; the device stage is csrc/copy_paste.hip.
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
    """One training sample (copy-paste, if any, has been applied before: ``copy_paste_sample``).  scans: 5 raw (n_k, 4) float32 scans in ``meta_list_raw`` order, label_words:
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


# ---- copy-paste augmentation (SequenceCutPaste, datasets/copy_paste.py; stage 2: datasets/copy_paste_seg.py) ------------------
PASTE_TRIALS = 20                   # np.arange(0, 360, 18), shuffled (copy_paste.py:198-199)
PASTE_STEP_DEG = 18
PASTE_RAW_ID = 30                   # raw semantic id of a pasted point (copy_paste.py:236)
PASTE_MIN_POINTS = 10               # copy_paste.py:195
PASTE_MIN_ROAD = 5                  # more than this many road points under the box (copy_paste.py:209)
PASTE_MAX_BLOCKERS = 3              # fewer than this many object-class points inside the view box (copy_paste.py:164)
PASTE_NOISE_STD = 0.001             # copy_paste.py:140
PASTE_BOX_SCALE = 1.05              # copy_paste.py:125
PASTE_SPANS = (8.0, 1.0, 1.0)       # u, phi, theta (copy_paste.py:160)
PASTE_ROAD_ID = 40                  # data_StreamMOS.py:231
PASTE_MAX_OBJECTS = 20              # config/StreamMOS.py:34
PASTE_CATEGORIES = ("other-vehicle", "truck", "car", "motorcyclist", "motorcycle", "person", "bicycle", "bicyclist")
PASTE_VELOCITY = {"other-vehicle": (-15, 15), "truck": (-15, 15), "car": (-15, 15), "motorcyclist": (-8, 8), "motorcycle": (-8, 8),
                  "person": (-3, 3), "bicycle": (-8, 8), "bicyclist": (-8, 8)}
PASTE_PAD = (PAD_XYZI, PAD_XYZI, PAD_Z, PAD_XYZI)


class PasteObject:
    """One entry of the object bank: ``pcds`` float32 [m, 4], box ``center`` [3], ``size`` [3] and ``yaw`` as float64 (a file
    that stores them narrower is widened first: the box is float64 arithmetic from there on), ``cate`` one of PASTE_CATEGORIES."""

    def __init__(self, pcds, center, size, yaw, cate):
        self.pcds = np.ascontiguousarray(pcds, dtype=np.float32)
        self.center = np.asarray(center, dtype=np.float64).reshape(3)
        self.size = np.asarray(size, dtype=np.float64).reshape(3)
        self.yaw = float(np.asarray(yaw, dtype=np.float64).reshape(()))
        self.cate = str(cate)
        if self.pcds.ndim != 2 or self.pcds.shape[1] != 4:
            raise ValueError("an object's pcds are [m, 4] float32, got %s" % (list(self.pcds.shape),))
        if self.cate not in PASTE_CATEGORIES:
            raise ValueError("unknown object category %r" % (self.cate,))


class PasteDraws:
    """The random draws of one sample's copy-paste: ``count`` objects; per object the bank ``index``, the signed ``velocity``
    (m/s), the trial ``order`` (uint8 [count, 20], each row a permutation of 0..19: trial j rotates by 18 * order[j] degrees) and
    the ``noise`` (float64 [5, m, 3] per object, or None: generated in the kernels from (seed, sample index))."""

    def __init__(self, index, velocity, order, noise=None):
        self.index = [int(i) for i in index]
        self.count = len(self.index)
        self.velocity = [float(v) for v in velocity]
        self.order = np.asarray(order, dtype=np.uint8).reshape(self.count, PASTE_TRIALS)
        self.noise = None if noise is None else list(noise)


def paste_label_maps(label_maps, paste_labels):
    """Label maps extended for pasted points: every LUT is zero-filled to the longest one's length (the *label base*), then gets
    the three labels of a pasted point's word label_base + motion label (motion 0 / 1 / 2).  paste_labels: name -> 3 labels,
    e.g. {"pcds_target": (0, 1, 2), "pcds_bf_target": (2, 2, 2)} (copy_paste.py:235, copy_paste_seg.py:237).  Returns
    (maps, label_base)."""
    base = max(int(np.asarray(m).shape[0]) for m in label_maps.values())
    if set(paste_labels) != set(label_maps):
        raise ValueError("paste_labels names %s, the label maps %s" % (sorted(paste_labels), sorted(label_maps)))
    out = {}
    for name, lut in label_maps.items():
        ext = np.zeros(base + 3, dtype=np.asarray(lut).dtype)
        ext[:np.asarray(lut).shape[0]] = np.asarray(lut)
        ext[base:] = np.asarray(paste_labels[name]).reshape(3)
        out[name] = ext
    return out, base


def paste_motion_label(velocity):
    """copy_paste.py:187-193 on |v|."""
    v = abs(float(velocity))
    return 2 if v >= 1 else (1 if v < 0.3 else 0)


def paste_rotations():
    """cos and sin of the 20 trial angles as cv2.getRotationMatrix2D takes them (alpha = cos, beta = sin of angle * pi / 180)."""
    a = np.arange(PASTE_TRIALS, dtype=np.float64) * PASTE_STEP_DEG * np.pi / 180.0
    return np.cos(a), np.sin(a)


def paste_box_footprint(obj):
    """compute_box_3d (copy_paste.py:21-43) of the box scaled by 1.05: its first four corners' x, y (the quadrilateral the road
    test uses), float64 [4, 2]."""
    size = obj.size * PASTE_BOX_SCALE
    c, s = np.cos(obj.yaw), np.sin(obj.yaw)
    xc = np.array([size[0] / 2, size[0] / 2, -size[0] / 2, -size[0] / 2])
    yc = np.array([size[1] / 2, -size[1] / 2, -size[1] / 2, size[1] / 2])
    return np.stack((c * xc - s * yc + obj.center[0], s * xc + c * yc + obj.center[1]), axis=1)


def paste_velocity_xy(obj, velocity):
    return -1 * velocity * np.sin(obj.yaw), velocity * np.cos(obj.yaw)


def view_angles(x, y, z):
    """get_fov / occlusion_process (copy_paste.py:93-115) in float32: u, phi = arctan2(x, y), theta = arcsin(z / d)."""
    f = np.float32
    x, y, z = x.astype(f), y.astype(f), z.astype(f)
    d = np.sqrt(x * x + y * y + z * z) + f(1e-12)
    u = np.sqrt(x * x + y * y) + f(1e-12)
    return u, np.arctan2(x, y), np.arcsin(z / d)


def inside_quad(p, quad):
    """in_hull of a convex quadrilateral whose corners are given in order: p [n, 2] -> (inside [n], distance to the boundary
    [n]); the sign of the four edge cross products decides, in float64."""
    p = np.asarray(p, dtype=np.float64)
    a, b = quad, np.roll(quad, -1, axis=0)
    e = b - a
    rel = p[:, None, :] - a[None, :, :]
    cross = e[None, :, 0] * rel[..., 1] - e[None, :, 1] * rel[..., 0]
    inside = (cross >= 0).all(axis=1) | (cross <= 0).all(axis=1)
    along = np.clip((rel * e[None]).sum(axis=2) / (e * e).sum(axis=1)[None, :], 0.0, 1.0)
    gap = rel - along[..., None] * e[None]
    return inside, np.sqrt((gap * gap).sum(axis=2)).min(axis=1)


def seeded_paste_scalars(seed, sample_index, bank_categories, max_objects=PASTE_MAX_OBJECTS):
    """The host side of seeded copy-paste draws: ``random.Random`` keyed on (seed, sample index) like ``seeded_scalars`` (under a
    tag of its own, so the two streams differ), drawn in the reference's order: the count, then per object category, file,
    velocity and the trial order.  bank_categories: per category the list of bank indices.  Returns (index, velocity, order)."""
    import random
    rng = random.Random((1 << 128) | (int(seed) << 64) | int(sample_index))
    count = rng.randint(0, int(max_objects))
    index, velocity, order = [], [], []
    filled = [c for c in range(len(PASTE_CATEGORIES)) if len(bank_categories[c]) > 0]
    for _ in range(count):
        c = filled[rng.randrange(len(filled))]
        index.append(int(bank_categories[c][rng.randrange(len(bank_categories[c]))]))
        lo, hi = PASTE_VELOCITY[PASTE_CATEGORIES[c]]
        velocity.append(lo + (hi - lo) * rng.random())
        perm = list(range(PASTE_TRIALS))
        rng.shuffle(perm)
        order.append(perm)
    return index, velocity, np.asarray(order, dtype=np.uint8).reshape(count, PASTE_TRIALS)


def seeded_paste_noise(seed, sample_index, obj, m):
    """Host restatement of the kernels' seeded noise of object number `obj` with m points: float64 [5, m, 3] (Philox counter
    layout: include/smos.h).  numpy's float32 log / cos may differ from the device's in the last bits."""
    f = np.float32
    t, p = np.meshgrid(np.arange(TRAIN_FRAMES, dtype=np.uint64), np.arange(int(m), dtype=np.uint64), indexing="ij")
    key = np.array([int(seed) & _M32, (int(seed) >> 32) & _M32], dtype=np.uint64)
    w = []
    for call in (0, 1):
        c1 = np.uint64(1 << 24) | (np.uint64(call) << np.uint64(16)) | (np.uint64(int(obj)) << np.uint64(8)) | t
        ctr = np.stack((p, c1, np.full_like(p, int(sample_index) & _M32), np.full_like(p, (int(sample_index) >> 32) & _M32)), axis=-1)
        w.append(philox4x32(ctr, key))
    z = np.stack((box_muller_f32(w[0][..., 2], w[0][..., 3]), box_muller_f32(w[1][..., 0], w[1][..., 1]),
                  box_muller_f32(w[1][..., 2], w[1][..., 3])), axis=-1)
    return (z * f(PASTE_NOISE_STD) + f(0.0)).astype(np.float64)


PASTE_VARIANTS = ("non_accumulating_rotation", "road_refreshed", "road_ge_5", "closed_upper_bound", "any_frame",
                  "pasted_not_object_class")


def copy_paste_sample(scans_aligned, label_words, road_points, objects, draws, label_base=360, variant=None, trace=None):
    """SequenceCutPaste.__call__ with explicit draws, on scans that went through the first alignment.

    scans_aligned: 5 float32 [n_k, 4]; label_words: their uint32 words; road_points: scan 0's points with semantic id 40 as
    form_seq takes them (before any paste, never updated); objects: the bank (list of PasteObject); draws: PasteDraws with noise.
    Returns (scans', words', status): frame k has n_k + sum(m_i) rows, the originals in their order, then one slot range per
    object in paste order.  A removed point, and the slot of an object that was skipped (fewer than 10 points) or found no valid
    trial, holds the validation padding point; every row keeps its word.  A pasted point's word is label_base + its motion label
    (0 / 1 / 2).  status [count] int32: the accepted trial, or -1.

    Types follow the reference under numpy's current promotion rules: the per-frame shift and the noise are float64 sums rounded
    once to float32, every rotation is a float64 product rounded to float32 (so the rotations accumulate their roundings), the
    road lift and the view angles are float32, the box footprint stays float64.  variant: one deliberate error (tests only).
    trace: a list that receives one dict per trial (road count, edge distances, spans, boxes, counts)."""
    f, d = np.float32, np.float64
    if variant is not None and variant not in PASTE_VARIANTS:
        raise ValueError("unknown variant %r" % (variant,))
    if len(scans_aligned) != TRAIN_FRAMES or len(label_words) != TRAIN_FRAMES:
        raise ValueError("copy-paste edits the %d scans of a training sample" % TRAIN_FRAMES)
    sizes = [objects[i].pcds.shape[0] for i in draws.index]
    total = int(sum(sizes))
    n = [int(s.shape[0]) for s in scans_aligned]
    pts, words, raw, alive, phi, theta = [], [], [], [], [], []
    for k in range(TRAIN_FRAMES):
        p = np.empty((n[k] + total, 4), dtype=f)
        p[:] = np.array(PASTE_PAD, dtype=f)
        p[:n[k]] = scans_aligned[k]
        w = np.zeros(n[k] + total, dtype=np.uint32)
        w[:n[k]] = np.asarray(label_words[k]).astype(np.uint32)
        pts.append(p)
        words.append(w)
        raw.append((w & np.uint32(0xFFFF)).astype(np.int64))
        alive.append(np.arange(n[k] + total) < n[k])
        _, ph, th = view_angles(p[:, 0], p[:, 1], p[:, 2])
        phi.append(ph)
        theta.append(th)
    road = np.asarray(road_points, dtype=f)
    rot_c, rot_s = paste_rotations()
    status = np.full(draws.count, -1, dtype=np.int32)
    upper = (lambda v, hi: v <= hi) if variant == "closed_upper_bound" else (lambda v, hi: v < hi)
    slot = 0
    for i in range(draws.count):
        obj, m = objects[draws.index[i]], sizes[i]
        at, slot = slot, slot + m
        if m < PASTE_MIN_POINTS:
            continue
        v = draws.velocity[i]
        noise = np.asarray(draws.noise[i], dtype=d)
        if noise.shape != (TRAIN_FRAMES, m, 3):
            raise ValueError("object %d: noise of shape %s, expected %s" % (i, list(noise.shape), [TRAIN_FRAMES, m, 3]))
        vx, vy = paste_velocity_xy(obj, v)
        frames = []
        for t in range(TRAIN_FRAMES):
            p = obj.pcds.copy()
            p[:, 0] = (p[:, 0].astype(d) - vx * t * 0.1).astype(f)
            p[:, 1] = (p[:, 1].astype(d) - vy * t * 0.1).astype(f)
            p[:, :3] = (p[:, :3].astype(d) + noise[t]).astype(f)
            frames.append(p)
        quad = paste_box_footprint(obj)                  # frame 0: t * 0.1 = 0, the footprint of the road test
        start = ([p.copy() for p in frames], quad.copy())
        motion = paste_motion_label(v)
        for j in range(PASTE_TRIALS):
            c, s = rot_c[draws.order[i, j]], rot_s[draws.order[i, j]]
            if variant == "non_accumulating_rotation":
                for t in range(TRAIN_FRAMES):
                    frames[t][:, :2] = start[0][t][:, :2]
                quad = start[1].copy()
            for p in frames:
                x, y = p[:, 0].astype(d), p[:, 1].astype(d)
                p[:, 0], p[:, 1] = (x * c + y * s).astype(f), (y * c - x * s).astype(f)
            quad = np.stack((quad[:, 0] * c + quad[:, 1] * s, quad[:, 1] * c - quad[:, 0] * s), axis=1)
            if variant == "road_refreshed":
                road = pts[0][alive[0] & ((raw[0] == PASTE_ROAD_ID) | (raw[0] == PASTE_RAW_ID))]
            under, edge = inside_quad(road[:, :2], quad)
            n_road = int(under.sum())
            rec = {"object": i, "trial": j, "road_count": n_road, "road_edge": float(edge.min()) if edge.size else np.inf}
            if trace is not None:
                trace.append(rec)
            if not (n_road >= PASTE_MIN_ROAD if variant == "road_ge_5" else n_road > PASTE_MIN_ROAD):
                continue
            road_mean = f(road[under][:, 2].mean())
            for p in frames:
                p[:, 2] = p[:, 2] + (road_mean - p[:, 2].min())
            ok, masks = [], []
            rec["frames"] = []
            for t in range(TRAIN_FRAMES):
                u, ph, th = view_angles(frames[t][:, 0], frames[t][:, 1], frames[t][:, 2])
                spans = (abs(u.max() - u.min()), abs(ph.max() - ph.min()), abs(th.max() - th.min()))
                fits = spans[0] < PASTE_SPANS[0] and spans[1] < PASTE_SPANS[1] and spans[2] < PASTE_SPANS[2]
                fr = {"spans": tuple(float(v_) for v_ in spans), "fits": bool(fits)}
                rec["frames"].append(fr)
                if not fits:
                    ok.append(False)
                    masks.append(None)
                    continue
                box = (ph.min(), ph.max(), th.min(), th.max())
                mask = alive[t] & (phi[t] >= box[0]) & upper(phi[t], box[1]) & (theta[t] >= box[2]) & upper(theta[t], box[3])
                cls = ((raw[t] >= 10) & (raw[t] < 33)) | ((raw[t] >= 252) & (raw[t] < 260))
                if variant == "pasted_not_object_class":
                    cls = cls & (np.arange(cls.shape[0]) < n[t])
                blockers = int((mask & cls).sum())
                if trace is not None:
                    e = 1e-4
                    wide = alive[t] & (phi[t] >= box[0] - e) & (phi[t] <= box[1] + e) & (theta[t] >= box[2] - e) & (theta[t] <= box[3] + e)
                    deep = alive[t] & (phi[t] >= box[0] + e) & (phi[t] < box[1] - e) & (theta[t] >= box[2] + e) & (theta[t] < box[3] - e)
                    fr.update(box=tuple(float(b) for b in box), blockers=blockers, removed=int(mask.sum()),
                              removed_pasted=int((mask & (np.arange(mask.shape[0]) >= n[t])).sum()), near=np.nonzero(wide & ~deep)[0])
                ok.append(blockers < PASTE_MAX_BLOCKERS)
                masks.append(mask)
            rec["valid"] = ok
            if not (any(ok) and all(mk is not None for mk in masks) if variant == "any_frame" else all(ok)):
                continue
            for t in range(TRAIN_FRAMES):
                pts[t][masks[t]] = np.array(PASTE_PAD, dtype=f)
                alive[t][masks[t]] = False
                rows = slice(n[t] + at, n[t] + at + m)
                pts[t][rows] = frames[t]
                words[t][rows] = np.uint32(label_base + motion)
                raw[t][rows] = PASTE_RAW_ID
                alive[t][rows] = True
                _, phi[t][rows], theta[t][rows] = view_angles(frames[t][:, 0], frames[t][:, 1], frames[t][:, 2])
            status[i] = j
            break
    return pts, words, status

"""The scan-to-label path -- csrc/preprocess.hip (with csrc/prep_point.h), the voting kernels of csrc/vote.hip and
csrc/labels.hip: named, seeded cases and their numpy references, shared by tests/test_host_stream_reference.py (no GPU) and
tests/test_gpu_stream_path.py.

References.  The project's restatements that tests/test_oracle_golden.py pins to the reference: preprocess.build_sample /
pose_align / range_mask, oracle.ops_np.vote_crop_mask / vote_quantize / vote_voxel_labels / vote_point_labels / vote_frame and
kitti.MovingIoU.  What they do not cover is restated here in explicit numpy and held against them by the host tests wherever both
apply: ``emit_rows`` (the compaction of prep_emit as a row model, with the guard that drops surplus points), ``vote_table`` (the
packed words c0 | c1 << 21 | c2 << 42), ``vote_resolve_ref`` (the argmax at the point's voxel, the own label outside the crop, the
LUT), ``vote_quantize_recip`` (the ``recip_quantize`` variant) and ``label_ref`` (words and moving-IoU counts).  Everything is
integers or copies of float32 values: EVERY comparison built on this module is np.array_equal, except the two range-view angles.

Sizes.  SWEEP = 2048 * 256: grid_for caps a launch at 2048 blocks of 256 threads, a grid-stride loop over more points takes a
second trip.  LABEL_SWEEP = 1024 * 256 * 4: frame_labels has 1024 blocks of 256 lanes with four points a lane.

Preprocessing cases (PREP_CASES; T scans, V flip variants, N = frame_point_num):
    tta_off           V = 1: one variant, the sign arrays of prep_emit padded with 1
    tiny              n = 5, T = 3
    n_gt_N            700 raw points, about 200 in range, N = 256: span = max(n, N) = n
    n_lt_N            40 raw points, N = 512: span = N, the padding loop runs past the scan
    all_out           no point in range: prefix[-1] = 0, every row is padding
    empty_history     a history scan of 0 points (null pointers, count = 0)
    empty_current     the current scan has 0 points: unpad_labels returns an empty tensor
    identity_none     history with pose difference None ...
    identity_eye      ... and with exactly eye(4), same scans: both take the shortcut past the float64 product
    faces             each of the six range faces at the face value, its float32 neighbour inside, its neighbour outside and well
                      inside (lower faces kept, upper faces dropped); NaN, +inf, -inf in every coordinate (dropped); a history
                      scan under a translation-only pose that lands x = 49 + 1 on the upper face (dropped) and x = -51 + 1 on the
                      lower one (kept)
    axes              the angle edge points in all four flips: the origin, the vertical (0, 0, +-1.5), the branch cut of
                      atan2(x, y) at (+-0, -3, 0) (column 0 against 2048), (+-3, 0, 0), (1e-20, 1e-20, -1e-20) and the padding point.
                      The pose alignment ends in "+ translation", so a raw -0 leaves it as +0 (column 0, for the identity too:
                      build_sample multiplies by it); the flip x * -1 then makes both -0 (column 2048).  ``same_bits`` compares the
                      float32 outputs as bit patterns, so that the sign of a zero counts.
    second_sweep      T = 1, V = 1, n = SWEEP + 300 with about half in range, N = 300 000: prep_transform_mask, prep_emit and
                      prep_unpad_labels take a second trip
    overflow          scan 0 holds c = N + 37 in-range points, scan 1 (the last) about N + 5: rows [0, N) are the first N kept points,
                      no padding row, the surplus is dropped.  (Without the guard scan 0's surplus lands in scan 1's rows, which the
                      next launch overwrites; the surplus of the LAST scan lands in the next flip variant's scan 0.)
    overflow_exact    c == N in scan 0, scan 1 fits
The expected outputs come from ``prep_want``: preprocess.build_sample with frame_point_num = max(N, max c + 1), cut to the rows
[0, N) -- for c < N that IS build_sample at N.

Range-view angles.  theta_q = (th_hi - asin(z / d)) / dtheta and phi_q = (phi_hi - atan2(x, y)) / dphi are the only values of this
path that go through a library routine whose last bit is not fixed.  ``angle_ref`` computes both in float64 from the float32 x, y,
z the kernel emits (after the flip) and the float32 constants it holds ((float)rv4[i]); ``angle_bounds`` bounds the kernel's
float32 result per element.  With u = 2^-24 (a float32 operation's relative rounding error) and t = z / d:
    t       x^2, y^2, z^2, two additions, the square root, the addition of 1e-12 and the division: the additions of positive terms
            carry the squares' errors through unamplified and the root halves them, so five roundings bound it with room:
            dt = 5 u |t|.  (The float64 d adds the same 1e-12; where d < 1e-11 -- the origin cases -- t is 0 or 1e-8 on both
            sides and dt covers the difference.)
    asin    monotone, so the effect of dt is max |asin(clip(t +- dt)) - asin t| EXACTLY, with no derivative term that would blow
            up at t -> +-1, plus the routine's own error ASIN_ULP u |asin t|:  dasin.
    theta   the subtraction th_hi - a rounds once, u |th_hi - asin t|; the division by dtheta rounds once, u |theta_q|, and carries
            the numerator's error over, (1 + u) / dtheta:
                bound_theta = (dasin + u |th_hi - asin t|) / dtheta (1 + u) + u |theta_q|
    phi     atan2f sees exact inputs:
                bound_phi = (ATAN2_ULP u |atan2| + u |phi_hi - atan2|) / dphi (1 + u) + u |phi_q|
The two allowances ASIN_ULP and ATAN2_ULP cannot be derived: the ROCm tree this was written against documents no accuracy figure
for the device library's asinf / atan2f.  They are measured as point_head_cases.TTA_EXP_ULP was, and NOT on the kernel:
tests/test_host_stream_reference.py takes the worst distance, in ulps, of numpy's float32 arcsin / arctan2 from the float64 value
rounded to float32 over the inputs of ANGLE_CASES, doubles it, raises it to the next power of two and asserts that the constant
is that number.  The bound is about 1e-4 cells away from the vertical; at the vertical itself (|t| = 1) dt moves asin by
sqrt(10 u) = 7.7e-4 rad = 0.1 cell.

Voting cases (VOTE_CASES; frames of (points, labels, pose difference) go through accumulate, the probe through resolve):
    recip             the 29 interior z boundaries float32(-4 + 0.2 k) and their two float32 neighbours, each point in an x / y cell
                      of its own: trunc((p - lo) * (float32(1) / float32(cell))) against the true division.  In x / y (cell
                      25 / 128, exact in binary after scaling) the two never differ; in z at least 8 of the 87 points do.
    strides_labels    labels 0, 1, 2, 3, 7, 255 on a cloud that reaches past the crop: labels > 2 cast no vote; outside the crop a
                      point keeps its label (lut[label] under a 256-entry LUT); inside it takes the voxel's argmax whatever its own
    ties              one voxel per count pattern (1,1,0) (0,1,1) (1,0,1) (2,2,2) (1,2,2) (2,1,2) (0,0,1) (0,3,0): ties go to the
                      lowest class, TIES_WANT
    faces             the six crop faces float32(lo + 1e-4) / float32(hi - 1e-4) at the face value, both neighbours and well
                      inside: the interval is open, both face values are dropped
    non_finite        NaN, +inf and -inf in every coordinate, without and with a pose: never counted, resolve keeps the own label
    second_sweep      one frame of SWEEP + 300 points through accumulate and resolve
    counter_width     2^21 - 1 points of class 0 in ONE voxel (the most the ABI admits), then 3 of class 1 and 2 of class 2:
                      the word is 0x1FFFFF | 3 << 21 | 2 << 42, the argmax 0
    ragged13/25       13 and 25 non-empty frames -- two and three launches of at most 12 -- of lengths cycling through 1, 63, 0,
                      257, 9 000 (the empty frames come on top: the launcher skips them before it counts to 12) with one frame of
                      SWEEP + 300 points, poses mixed with None

Label tail (LABEL_SIZES): n = 2, 3, 4, 5, 255, 256, 257 and LABEL_SWEEP + 4 * 64 + 3 (a second trip plus the tail); label bytes
0, 1, 2, 3, 255; ground-truth ids inside a 260-entry map, at its length (260) and at 0xFFFF, instance bits above.
"""
import functools
import hashlib
import types

import numpy as np

from oracle import ops_np
from streammos_amd import kitti, preprocess

U = 2.0 ** -24
F32 = np.float32
SWEEP = 2048 * 256
LABEL_SWEEP = 1024 * 256 * 4
SPEC = preprocess.VoxelSpec()
VOTE_CELLS = 512 * 512 * 30
VOTE_MAX_POINTS = (1 << 21) - 1
VOTE_MAX_FRAMES = 12                 # csrc/vote.hip: kMaxFrames
FIELD = (1 << 21) - 1
ASIN_ULP = 4.0      # measured worst 2 ulp (tests/test_host_stream_reference.py, case faces) -> doubled, next power of two
ATAN2_ULP = 4.0     # measured worst 2 ulp (tests/test_host_stream_reference.py, case tiny) -> doubled, next power of two


def _rng(name):
    return np.random.Generator(np.random.PCG64(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")))


def _pose(angle_deg, shift):
    """A rigid 4x4 float64: rotation about z, then the translation."""
    a = np.deg2rad(angle_deg)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = shift
    return m


def _neighbours(v, inside):
    """(v, its float32 neighbour towards `inside`, its neighbour away from it) as float32."""
    v = F32(v)
    return v, np.nextafter(v, F32(inside)), np.nextafter(v, F32(2.0) * v - F32(inside))


NON_FINITE = (np.nan, np.inf, -np.inf)


def _non_finite_points(base):
    """Nine rows: `base` with NaN, +inf, -inf put into x, y and z in turn."""
    rows = []
    for d in range(3):
        for bad in NON_FINITE:
            p = list(base)
            p[d] = bad
            rows.append(p)
    return np.array(rows, dtype=F32)


# ---------------------------------------------------------------------------------------------
# A. preprocessing
# ---------------------------------------------------------------------------------------------
RANGES = (SPEC.range_x, SPEC.range_y, SPEC.range_z)
INSIDE = (1.25, -2.5, -0.75)            # a point well inside the range box and the voting crop


def _cloud(rng, n, frac_in=0.5):
    """n points [n, 4] float32, about `frac_in` of them inside the range box (the others miss it in one coordinate at least)."""
    lo = np.array([r[0] for r in RANGES])
    hi = np.array([r[1] for r in RANGES])
    p = rng.uniform(lo + 0.5, hi - 0.5, (n, 3))
    out = rng.random(n) >= frac_in
    axis = rng.integers(0, 3, n)
    far = np.where(rng.random(n) < 0.5, lo[axis] - rng.uniform(0.01, 30.0, n), hi[axis] + rng.uniform(0.0, 30.0, n))
    p[out, axis[out]] = far[out]
    return np.concatenate((p, rng.random((n, 1))), axis=1).astype(F32)


def face_points(faces_lo, faces_hi):
    """Per axis and face: the face value, the neighbour inside, the neighbour outside, a value well inside; the other two
    coordinates from INSIDE.  Returns ([24, 3] float32, keep [24] under lo <= p < hi on the given faces)."""
    rows, keep = [], []
    for d in range(3):
        for face, other, is_lo in ((faces_lo[d], faces_hi[d], True), (faces_hi[d], faces_lo[d], False)):
            on, inner, outer = _neighbours(face, other)
            for v, k in ((on, is_lo), (inner, True), (outer, False), (F32(INSIDE[d]), True)):
                p = list(INSIDE)
                p[d] = v
                rows.append(p)
                keep.append(k)
    return np.array(rows, dtype=F32), np.array(keep)


def _with_intensity(xyz, rng):
    return np.concatenate((xyz, rng.random((xyz.shape[0], 1)).astype(F32)), axis=1).astype(F32)


def _prep(name, scans, diffs, N, tta=True):
    c = types.SimpleNamespace(name=name, scans=[np.ascontiguousarray(s, dtype=F32) for s in scans], diffs=list(diffs), N=int(N),
                              tta=bool(tta))
    c.T, c.V = len(scans), 4 if tta else 1
    return c


def _build_prep(name):
    rng = _rng("prep_" + ("identity" if name.startswith("identity") else name))      # the two identity cases share their scans
    hist = [_pose(2.0, (0.8, -0.3, 0.02)), _pose(-3.5, (-1.5, 0.6, -0.04))]
    if name == "tta_off":
        return _prep(name, [_cloud(rng, n) for n in (90, 70, 130)], [None] + hist, 96, tta=False)
    if name == "tiny":
        return _prep(name, [_cloud(rng, 5, 0.8) for _ in range(3)], [None] + hist, 64)
    if name == "n_gt_N":
        return _prep(name, [_cloud(rng, 700, 0.29), _cloud(rng, 300, 0.5)], [None, hist[0]], 256)
    if name == "n_lt_N":
        return _prep(name, [_cloud(rng, 40, 0.6), _cloud(rng, 700, 0.5)], [None, hist[1]], 512)
    if name == "all_out":
        far = _cloud(rng, 150, 0.0)
        return _prep(name, [far, _cloud(rng, 60, 0.0)], [None, hist[0]], 64)
    if name == "empty_history":
        return _prep(name, [_cloud(rng, 100), np.zeros((0, 4), dtype=F32), _cloud(rng, 80)], [None] + hist, 128)
    if name == "empty_current":
        return _prep(name, [np.zeros((0, 4), dtype=F32), _cloud(rng, 100)], [None, hist[0]], 128)
    if name in ("identity_none", "identity_eye"):
        ident = None if name == "identity_none" else np.eye(4)
        return _prep(name, [_cloud(rng, 100), _cloud(rng, 90), _cloud(rng, 110)], [None, ident, hist[1]], 128)
    if name == "faces":
        xyz, _ = face_points([r[0] for r in RANGES], [r[1] for r in RANGES])
        cur = np.concatenate((xyz, _non_finite_points(INSIDE)))
        # translation by exactly +1 in x: 49 -> 50 (upper face, dropped), -51 -> -50 (lower face, kept); the float64 sum is exact
        h = np.array([[49.0, 1.0, 0.5], [-51.0, 2.0, 0.25], [48.999996, -1.0, 0.0], [-51.000004, 3.0, -1.0], [7.0, 7.0, 0.0]])
        return _prep(name, [_with_intensity(cur, rng), _with_intensity(h, rng)], [None, _pose(0.0, (1.0, 0.0, 0.0))], 64)
    if name == "axes":
        pts = [[0, 0, 0], [0, 0, 1.5], [0, 0, -1.5], [0.0, -3, 0], [-0.0, -3, 0], [3, 0, 0], [-3, 0, 0],
               [1e-20, 1e-20, -1e-20]]
        return _prep(name, [_with_intensity(np.array(pts, dtype=F32), rng)], [None], 64)
    if name == "second_sweep":
        return _prep(name, [_cloud(rng, SWEEP + 300, 0.5)], [None], 300000, tta=False)
    if name in ("overflow", "overflow_exact"):
        N = 192
        c = N + 37 if name == "overflow" else N
        scan = np.concatenate((_cloud(rng, c, 1.0), _cloud(rng, 150, 0.0)))[rng.permutation(c + 150)]
        c1 = N + 5 if name == "overflow" else N // 2
        last = np.concatenate((_cloud(rng, c1, 1.0), _cloud(rng, 90, 0.0)))[rng.permutation(c1 + 90)]
        return _prep(name, [scan, preprocess.pose_align(last, np.linalg.inv(hist[0]))], [None, hist[0]], N)
    raise KeyError(name)


PREP_CASES = ("tta_off", "tiny", "n_gt_N", "n_lt_N", "all_out", "empty_history", "empty_current", "identity_none", "identity_eye",
              "faces", "axes", "second_sweep", "overflow", "overflow_exact")
PREP_OVERFLOW = ("overflow", "overflow_exact")
ANGLE_CASES = ("tiny", "faces", "axes")


@functools.lru_cache(maxsize=None)
def prep_case(name):
    return _build_prep(name)


def moved_scans(case):
    """The scans after pose alignment (preprocess.pose_align; where the kernel skips the transform, the scan with +0 added to
    x, y, z, which is all the identity does to float32 values: -0 becomes +0) and their range masks."""
    moved = []
    for s, d in zip(case.scans, case.diffs):
        if d is None or np.array_equal(d, np.eye(4)):
            m = s.copy()
            m[:, :3] = s[:, :3] + F32(0.0)
        else:
            m = preprocess.pose_align(s, d)
        moved.append(m)
    with np.errstate(invalid="ignore"):
        masks = [preprocess.range_mask(m, SPEC) for m in moved]
    return moved, masks


def host_poses(case):
    """Absolute poses whose differences inv(P_0) P_t are the case's pose differences bit for bit: P_0 = eye."""
    assert case.diffs[0] is None
    return [np.eye(4) if d is None else np.asarray(d, dtype=np.float64) for d in case.diffs]


@functools.lru_cache(maxsize=None)
def prep_want(name):
    """The expected outputs of DevicePreprocessor.build for a case, through preprocess.build_sample (see the module docstring
    for the overflow cases): mask, counts, pcds_coord, pcds_xyzi, pcds_sphere_coord (numpy's float32 angles: not a reference,
    see angle_ref)."""
    case = prep_case(name)
    _, masks = moved_scans(case)
    counts = np.array([int(m.sum()) for m in masks], dtype=np.int32)
    n_host = max(case.N, int(counts.max()) + 1)
    with np.errstate(invalid="ignore"):
        host = preprocess.build_sample(case.scans, host_poses(case), n_host, SPEC, tta=case.tta)
    w = types.SimpleNamespace(mask=masks[0], counts=counts, n_host=n_host)
    w.xyzi = np.ascontiguousarray(host["pcds_xyzi"][:, :, :, :case.N])
    w.coord = np.ascontiguousarray(host["pcds_coord"][:, :, :case.N])
    w.sphere = np.ascontiguousarray(host["pcds_sphere_coord"][:, :, :case.N])
    assert np.array_equal(host["valid_mask"], masks[0])
    return w


def emit_rows(case, guard=True):
    """prep_emit as a row model: float32 [V, T, N, 4], the flipped points in the kernel's flat order (variant v, scan t: rows
    [(v T + t) N, (v T + t + 1) N)), one launch per scan in scan order.  Kept point i goes to row prefix[i] - 1 of its scan, the
    rows from count = min(prefix[-1], N) on are the padding point.  guard=False is the kernel without `j < N` and without the
    min: a surplus point is stored past its scan's rows -- into the next scan's, which that scan's later launch overwrites, or,
    from the last scan, into the next variant's scan 0, where it races with that launch's own stores and is taken to win here
    (past the last variant it is out of bounds: dropped)."""
    moved, masks = moved_scans(case)
    V, T, N = case.V, case.T, case.N
    rows = np.full((V * T * N, 4), np.nan, dtype=F32)
    pad = np.array([preprocess.PAD_XYZI, preprocess.PAD_XYZI, preprocess.PAD_Z, preprocess.PAD_XYZI], dtype=F32)
    signs = preprocess.TTA_SIGNS if case.tta else preprocess.TTA_SIGNS[:1]
    for t in range(T):
        c = int(masks[t].sum())
        kept = moved[t][masks[t]]
        for surplus in (False, True):
            for v, (sx, sy) in enumerate(signs):
                at = (v * T + t) * N
                flipped = kept * np.array([sx, sy, 1, 1], dtype=F32)
                assert flipped.dtype == F32
                if not surplus:
                    rows[at + (min(c, N) if guard else c):at + N] = pad * np.array([sx, sy, 1, 1], dtype=F32)
                    rows[at:at + min(c, N)] = flipped[:N]
                elif not guard:
                    spill = flipped[N:][:max(0, rows.shape[0] - at - N)]
                    rows[at + N:at + N + spill.shape[0]] = spill
    return rows.reshape(V, T, N, 4)


def form_rows(case, rows):
    """The rows of emit_rows through preprocess.form_batch: (xyzi, coord, sphere) in build_sample's shapes."""
    out = [preprocess.form_batch(rows[v].reshape(case.T * case.N, 4), case.T, SPEC) for v in range(case.V)]
    return tuple(np.stack([o[k] for o in out], axis=0) for k in range(3))


def same_bits(got, want):
    """Equality of float32 arrays as bit patterns: -0 is not +0, a NaN equals only the same NaN."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    return got.shape == want.shape and bool(np.array_equal(got.view(np.int32), want.view(np.int32)))


def unpad_want(case, labels):
    """labels [N] uint8 of the padded sample -> [n_raw] uint8: labels[j] for the j-th kept point while j < N, 0 for the surplus
    and for the points out of range."""
    mask = prep_want(case.name).mask
    raw = np.zeros(case.scans[0].shape[0], dtype=np.uint8)
    kept = np.flatnonzero(mask)[:case.N]
    raw[kept] = np.asarray(labels)[:kept.size]
    return raw


def rv_constants():
    """The four float32 range-view constants as DevicePreprocessor hands them over and fill_geom rounds them."""
    h, w = SPEC.rv_shape
    phi_hi, phi_lo = 180.0 * np.pi / 180.0, -180.0 * np.pi / 180.0
    th_lo, th_hi = SPEC.RV_theta[0] * np.pi / 180.0, SPEC.RV_theta[1] * np.pi / 180.0
    return tuple(float(F32(v)) for v in (phi_hi, (phi_hi - phi_lo) / w, th_hi, (th_hi - th_lo) / h))


def angle_inputs(xyzi):
    """pcds_xyzi [V, T, 7, N, 1] -> float64 x, y, z [V, T, N] of the emitted (flipped) points."""
    a = np.asarray(xyzi)[..., 0].astype(np.float64)
    return a[:, :, 0], a[:, :, 1], a[:, :, 2]


def angle_terms(x, y, z):
    """t = z / d and atan2(x, y) in float64 (d = sqrt(x^2 + y^2 + z^2) + float32(1e-12))."""
    d = np.sqrt(x * x + y * y + z * z) + float(F32(1e-12))
    return z / d, np.arctan2(x, y)


def angle_ref(x, y, z, swap=False):
    """(theta_q, phi_q) in float64; swap=True is the deliberate error atan2(y, x)."""
    phi_hi, dphi, th_hi, dth = rv_constants()
    t, a = angle_terms(x, y, z)
    if swap:
        a = np.arctan2(y, x)
    return (th_hi - np.arcsin(np.clip(t, -1.0, 1.0))) / dth, (phi_hi - a) / dphi


def angle_bounds(x, y, z):
    """Per-element bounds on |kernel - angle_ref| for (theta_q, phi_q): the derivation in the module docstring."""
    phi_hi, dphi, th_hi, dth = rv_constants()
    t, a = angle_terms(x, y, z)
    t = np.clip(t, -1.0, 1.0)
    s = np.arcsin(t)
    dt = 5.0 * U * np.abs(t)
    dasin = np.maximum(np.abs(np.arcsin(np.clip(t + dt, -1.0, 1.0)) - s), np.abs(np.arcsin(np.clip(t - dt, -1.0, 1.0)) - s))
    dasin = dasin + ASIN_ULP * U * np.abs(s)
    th_q, phi_q = (th_hi - s) / dth, (phi_hi - a) / dphi
    b_th = (dasin + U * np.abs(th_hi - s)) / dth * (1.0 + U) + U * np.abs(th_q)
    b_phi = (ATAN2_ULP * U * np.abs(a) + U * np.abs(phi_hi - a)) / dphi * (1.0 + U) + U * np.abs(phi_q)
    return b_th, b_phi


def angle_ratios(sphere, xyzi):
    """Worst |sphere - angle_ref| / bound over the elements, (theta, phi); a NaN anywhere gives inf."""
    x, y, z = angle_inputs(xyzi)
    (r_th, r_phi), (b_th, b_phi) = angle_ref(x, y, z), angle_bounds(x, y, z)
    sp = np.asarray(sphere)[..., 0].astype(np.float64)
    out = []
    for got, want, bound in ((sp[..., 0], r_th, b_th), (sp[..., 1], r_phi, b_phi)):
        err = np.abs(got - want)
        ratio = np.where(err == 0, 0.0, err / bound)
        out.append(float("inf") if not np.isfinite(ratio).all() else float(ratio.max()))
    return tuple(out)


def ulp_distance(f32_values, f64_values):
    """Worst distance, in float32 ulps of the rounded float64 value, of float32 results from those rounded values."""
    want = np.asarray(f64_values, dtype=np.float64).astype(F32)
    got = np.asarray(f32_values, dtype=F32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp).max())


def ulp_allowance(worst):
    """The measured worst ulp distance -> the constant: doubled, raised to the next power of two (at least 1)."""
    return float(2.0 ** np.ceil(np.log2(max(2.0 * worst, 1.0))))


# ---------------------------------------------------------------------------------------------
# B. voting
# ---------------------------------------------------------------------------------------------
VOTE_LO = tuple(F32(ops_np.VOTE_FOV[0][d]) for d in range(3))
VOTE_CELL = tuple(F32((ops_np.VOTE_FOV[1][d] - ops_np.VOTE_FOV[0][d]) / ops_np.VOTE_SIZE[d]) for d in range(3))
CROP_LO = tuple(F32(ops_np.VOTE_FOV[0][d] + ops_np.CROP_EPS) for d in range(3))
CROP_HI = tuple(F32(ops_np.VOTE_FOV[1][d] - ops_np.CROP_EPS) for d in range(3))
TIES = ((1, 1, 0), (0, 1, 1), (1, 0, 1), (2, 2, 2), (1, 2, 2), (2, 1, 2), (0, 0, 1), (0, 3, 0))
TIES_WANT = (0, 1, 0, 0, 1, 0, 2, 1)
RAGGED_CYCLE = (1, 63, 0, 257, 9000)


def vote_quantize_recip(points):
    """The ``recip_quantize`` variant of ops_np.vote_quantize: what torch computes on a GPU for `tensor / python_scalar`, a
    multiplication by the float32 reciprocal of the float32 cell: trunc((p - lo) * (float32(1) / float32(cell)))."""
    points = np.asarray(points, dtype=F32)
    cols = []
    for d in range(3):
        r = F32(1.0) / VOTE_CELL[d]
        q = (points[:, d] - VOTE_LO[d]) * r
        assert q.dtype == F32
        cols.append(np.trunc(q).astype(np.int64))
    return np.stack(cols, axis=-1)


def crop_closed(points):
    """The deliberate error `>=` / `<=` in the crop."""
    points = np.asarray(points, dtype=F32)
    keep = np.ones(points.shape[0], dtype=bool)
    for d in range(3):
        keep &= (points[:, d] >= CROP_LO[d]) & (points[:, d] <= CROP_HI[d])
    return keep


def linear_voxel(points, recip=False, true_division_under_recip=False, crop=None):
    """int64 [n]: the linear voxel (x * 512 + y) * 30 + z of a point inside the crop, -1 outside (non-finite included)."""
    points = np.asarray(points, dtype=F32)[:, :3]
    with np.errstate(invalid="ignore"):
        keep = (crop or ops_np.vote_crop_mask)(points)
    safe = np.where(keep[:, None], points, F32(0))
    q = vote_quantize_recip(safe) if recip and not true_division_under_recip else ops_np.vote_quantize(safe)
    size = ops_np.VOTE_SIZE
    assert ((q >= 0) & (q < np.array(size))).all()            # inside the crop the kernel's clamp never acts
    return np.where(keep, (q[:, 0] * size[1] + q[:, 1]) * size[2] + q[:, 2], -1)


def aligned(points, pose):
    points = np.asarray(points, dtype=F32)
    if pose is None:
        return points
    with np.errstate(invalid="ignore"):
        return preprocess.pose_align(points, pose)


def vote_table(frames, recip=False, skip_above_2=True, **kw):
    """frames of (points, labels, pose or None) -> the dense table, int64 [VOTE_CELLS]: c0 | c1 << 21 | c2 << 42 per voxel.
    skip_above_2=False is the deliberate error of counting every label: 1 << (21 * label) modulo 2^64."""
    table = np.zeros(VOTE_CELLS, dtype=np.uint64)
    for points, labels, pose in frames:
        lin = linear_voxel(aligned(points, pose), recip, **kw)
        lab = np.asarray(labels).astype(np.int64)
        keep = lin >= 0
        if skip_above_2:
            keep &= lab <= 2
        inc = np.array([(1 << (21 * int(l))) & 0xFFFFFFFFFFFFFFFF for l in range(256)], dtype=np.uint64)
        np.add.at(table, lin[keep], inc[lab[keep]])
    return table.view(np.int64)


def table_counts(words):
    w = np.asarray(words).view(np.uint64)
    return np.stack([(w >> np.uint64(21 * k)) & np.uint64(FIELD) for k in range(3)], axis=-1).astype(np.int64)


def vote_resolve_ref(points, labels, table, recip=False, lut=None, ties_high=False, **kw):
    """int32 [n]: the argmax of the point's voxel (ties to the lowest class; ties_high=True is the deliberate error) inside the
    crop, the point's own label outside; through lut[label & 0xFF] when a LUT is given."""
    lin = linear_voxel(points, recip, **kw)
    out = np.asarray(labels).astype(np.int64).copy()
    inside = lin >= 0
    c = table_counts(np.asarray(table)[lin[inside]])
    out[inside] = 2 - c[:, ::-1].argmax(axis=-1) if ties_high else c.argmax(axis=-1)
    if lut is not None:
        out = np.asarray(lut)[out & 0xFF]
    return out.astype(np.int32)


def frame_launches(lengths):
    """How smos_vote_accumulate_frames groups frames: empty ones are skipped, at most VOTE_MAX_FRAMES go into a launch.
    Returns the list of launches, each the list of its frame lengths."""
    live = [int(n) for n in lengths if n > 0]
    return [live[i:i + VOTE_MAX_FRAMES] for i in range(0, len(live), VOTE_MAX_FRAMES)]


def _vote_cloud(rng, n, layout=4):
    """[n, layout] float32: x, y in -56 .. 56, z in -5 .. 3 (about a quarter outside the crop), clustered on a 0.4 m lattice
    with jitter so that voxels hold several points."""
    p = np.stack((rng.uniform(-56, 56, n), rng.uniform(-56, 56, n), rng.uniform(-5, 3, n)), axis=1)
    p = np.round(p / 0.4) * 0.4 + rng.normal(0, 0.05, (n, 3))
    extra = rng.random((n, layout - 3))
    return np.ascontiguousarray(np.concatenate((p, extra), axis=1), dtype=F32)


def _vote(name, frames, probe, probe_labels, recip=False):
    f = [(np.ascontiguousarray(p, dtype=F32), np.ascontiguousarray(l, dtype=np.uint8), d) for p, l, d in frames]
    return types.SimpleNamespace(name=name, frames=f, probe=np.ascontiguousarray(probe, dtype=F32),
                                 probe_labels=np.ascontiguousarray(probe_labels, dtype=np.uint8), recip=recip)


def _column(i):
    """x, y of a voxel column of its own for index i (0.5 m apart: more than a cell of 25 / 128 m)."""
    return -20.0 + 0.5 * (i % 80), 3.1 + 0.5 * (i // 80)


def recip_points():
    z = []
    for k in range(1, 30):
        b = F32(-4.0 + 0.2 * k)
        z += [np.nextafter(b, F32(-10)), b, np.nextafter(b, F32(10))]
    pts = np.array([[_column(i)[0], _column(i)[1], v] for i, v in enumerate(z)], dtype=F32)
    assert pts.shape == (87, 3)
    return pts


def _build_vote(name):
    rng = _rng("vote_" + name)
    if name == "recip":
        pts = recip_points()
        own = (np.arange(87) % 3).astype(np.uint8)
        other = ((own + 1) % 3).astype(np.uint8)
        # two history votes for another class, then the point's own: where the conventions part, the probe finds its voxel empty
        # but for itself
        return _vote(name, [(pts, other, None), (pts, other, None), (pts, own, None)], pts, own, recip=True)
    if name == "strides_labels":
        n = 400
        pts = _vote_cloud(rng, n)
        lab = np.array([0, 1, 2, 3, 7, 255], dtype=np.uint8)[rng.integers(0, 6, n)]
        hist = _vote_cloud(rng, 600)
        hist[:n // 2, :3] = pts[:n // 2, :3]                       # half of the probe's voxels hold history votes
        hlab = np.array([0, 1, 2, 2, 1, 3, 7, 255], dtype=np.uint8)[rng.integers(0, 8, 600)]
        # a point with label 255 on top of counted votes, one with label 7 alone in its voxel, both inside the crop
        pts[0, :3], lab[0], hist[0, :3], hlab[0] = (1.0, 1.0, 0.0), 255, (1.0, 1.0, 0.0), 2
        pts[n - 1, :3], lab[n - 1] = (-30.3, 12.7, -1.1), 7
        return _vote(name, [(hist, hlab, _pose(0.0, (0.0, 0.0, 0.0))), (pts, lab, None)], pts, lab)
    if name == "ties":
        pts, lab = [], []
        for v, pattern in enumerate(TIES):
            for cls, count in enumerate(pattern):
                pts += [[_column(v)[0], _column(v)[1], 0.1]] * count
                lab += [cls] * count
        order = rng.permutation(len(lab))
        probe = np.array([[_column(v)[0], _column(v)[1], 0.1] for v in range(len(TIES))], dtype=F32)
        return _vote(name, [(np.array(pts, dtype=F32)[order], np.array(lab)[order], None)], probe, np.full(len(TIES), 2))
    if name == "faces":
        pts, _ = face_points(CROP_LO, CROP_HI)
        lab = (np.arange(pts.shape[0]) % 3).astype(np.uint8)
        return _vote(name, [(pts, (lab + 1) % 3, None), (pts, (lab + 1) % 3, None), (pts, lab, None)], pts, lab)
    if name == "non_finite":
        pts = np.concatenate((_non_finite_points(INSIDE), _vote_cloud(rng, 40, 3)))
        lab = rng.integers(0, 3, pts.shape[0]).astype(np.uint8)
        other = np.concatenate((_non_finite_points((4.0, 5.0, 0.5)), _vote_cloud(rng, 40, 3)))
        olab = rng.integers(0, 3, other.shape[0]).astype(np.uint8)
        return _vote(name, [(other, olab, _pose(11.0, (0.7, -0.2, 0.05))), (pts, lab, _pose(-4.0, (0.1, 0.3, 0.0))), (pts, lab, None)],
                     pts, lab)
    if name == "second_sweep":
        n = SWEEP + 300
        pts = _vote_cloud(rng, n, 3)
        lab = rng.integers(0, 3, n).astype(np.uint8)
        return _vote(name, [(pts, lab, None)], pts, lab)
    if name in ("ragged13", "ragged25"):
        want, lengths, i = int(name[6:]), [], 0
        while sum(1 for n in lengths if n > 0) < want:
            lengths.append(RAGGED_CYCLE[i % len(RAGGED_CYCLE)])
            i += 1
        lengths[3] = SWEEP + 300
        frames = []
        for f, n in enumerate(lengths):
            pose = None if f % 3 == 0 else _pose(1.5 * f - 9.0, (0.3 * f - 2.0, 0.1 * f, 0.01 * f))
            frames.append((_vote_cloud(rng, n), rng.integers(0, 3, n).astype(np.uint8), pose))
        return _vote(name, frames, frames[3][0][:5000], frames[3][1][:5000])
    raise KeyError(name)


VOTE_CASES = ("recip", "strides_labels", "ties", "faces", "non_finite", "second_sweep", "ragged13", "ragged25")
COUNTER_POINT = (1.0, 1.0, 0.0)
COUNTER_WORD = 0x1FFFFF | 3 << 21 | 2 << 42


@functools.lru_cache(maxsize=None)
def vote_case(name):
    return _build_vote(name)


def vote_want(name):
    """(table int64 [VOTE_CELLS], resolved int32 [n]) of a case (63 MB: not cached)."""
    c = vote_case(name)
    table = vote_table(c.frames, c.recip)
    return table, vote_resolve_ref(c.probe, c.probe_labels, table, c.recip)


def wide_lut():
    """A 256-entry LUT whose entries all differ from their index and from each other."""
    return (1000 + 3 * np.arange(256)).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# C. label tail
# ---------------------------------------------------------------------------------------------
LABEL_SIZES = (2, 3, 4, 5, 255, 256, 257, LABEL_SWEEP + 4 * 64 + 3)
LABEL_BYTES = (0, 1, 2, 3, 255)
GT_MAP_LEN = 260
GT_IDS = (0, 1, 52, 99, 258, 259, 260, 0xFFFF) + kitti.STATIC_IDS[:6] + kitti.MOVING_IDS[:4]
VOTED_WORDS = (0, 9, 251, 5, 1, 2, -1, 255)
WORD_LUT = np.array([0, 9, 251], dtype=np.int32)


def gt_map():
    return np.ascontiguousarray(kitti.learning_map_lut()[:GT_MAP_LEN])


@functools.lru_cache(maxsize=None)
def label_case(n):
    """labels uint8 [n] over LABEL_BYTES, voted int32 [n] over VOTED_WORDS, gt uint32 [n] over GT_IDS with instance bits on top;
    the first entries run through the special values so that the smallest sizes hold them too."""
    rng = _rng("labels_%d" % n)
    labels = np.array(LABEL_BYTES, dtype=np.uint8)[rng.integers(0, len(LABEL_BYTES), n)]
    voted = np.array(VOTED_WORDS, dtype=np.int32)[rng.integers(0, len(VOTED_WORDS), n)]
    ids = np.array(GT_IDS, dtype=np.uint32)[rng.integers(0, len(GT_IDS), n)]
    head = min(n, 5)
    labels[:head] = np.array([3, 255, 1, 2, 0], dtype=np.uint8)[:head]
    ids[:head] = np.array([252, 40, 0xFFFF, 260, 252], dtype=np.uint32)[:head]
    gt = ids | (rng.integers(0, 1 << 16, n).astype(np.uint32) << np.uint32(16))
    return types.SimpleNamespace(n=n, labels=labels, voted=voted, gt=gt)


def mapped_gt(gt, table=None):
    """The class of a ground-truth word: table[word & 0xFFFF], 0 (unlabeled) for an id the table does not reach."""
    return preprocess.relabel_lut(np.asarray(gt).astype(np.uint32) & np.uint32(0xFFFF), gt_map() if table is None else table)


def iou_counts(gt_cls, pred_cls):
    """tp[1:3], pred[1:3], gt[1:3] of kitti.MovingIoU.add as int64 [6]."""
    m = kitti.MovingIoU()
    m.add(gt_cls, pred_cls)
    return np.concatenate((m.tp, m.pred, m.gt)).astype(np.int64)


def label_ref(case, mode):
    """(words int32 [n], counts int64 [6]) of a mode: "lut" (0 / 9 / 251, 0 for a byte above 2), "raw" (the byte), "voted" (a copy;
    251 counts as class 2, 9 as class 1, anything else as class 0).  A label byte above 2 is a prediction of neither class."""
    if mode == "voted":
        words = case.voted.copy()
        pred = np.where(words == 251, 2, np.where(words == 9, 1, 0))
    else:
        pred = case.labels.astype(np.int64)
        words = np.where(pred <= 2, WORD_LUT[np.minimum(pred, 2)], 0).astype(np.int32) if mode == "lut" else pred.astype(np.int32)
    return words, iou_counts(mapped_gt(case.gt), pred)

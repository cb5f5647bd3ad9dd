"""Inputs for the copy-paste augmentation (streammos_amd.preprocess.copy_paste_sample, device_preprocess.DeviceCopyPaste): five
designed scans, an object bank and one sample's draws, chosen so that the reference itself takes every branch listed in
EXPECTED below, each with margin in its own arithmetic (the asserts of ``sample()``).  A pure function of nothing.

The scene lives in frame 0's coordinates.  Twenty *slots* are the azimuths 270 - 18 j degrees: a trial angle 18 a moves an object
from slot s to slot s + a, so every position a trial can reach is one of twenty per object.  Slot 0 is the -y axis, where
phi = arctan2(x, y) wraps.  Each object stands on a *ring* (a radius) of its own and moves radially, so it stays in its slot over
the five frames.  Road points (semantic id 40) exist only in small patches at chosen (ring, slot) places; the background carries
no id 40 and, below 0.2 rad of elevation, no object-class id.
"""
import functools

import numpy as np

from streammos_amd import preprocess, synth

F = np.float32
LABEL_BASE = 360
BACKGROUND_IDS = np.array([0, 1, 9, 33, 44, 48, 50, 70, 72, 99, 251, 260, 359, 400], dtype=np.uint32)   # none in [10,33) or [252,260)
HIGH_IDS = np.array([10, 18, 30, 32, 252, 259], dtype=np.uint32)      # object classes, only far above every view box
ROAD_Z = -1.73
BACKGROUND_COUNTS = (3001, 3777, 4502, 5219, 5801)


def slot_azimuth(slot):
    return np.deg2rad(270.0 - 18.0 * slot)


def place(ring, slot, tangential=0.0, radial=0.0):
    """x, y of the point `radial` further out and `tangential` clockwise of (ring, slot)."""
    a = slot_azimuth(slot)
    return ((ring + radial) * np.cos(a) + tangential * np.sin(a), (ring + radial) * np.sin(a) - tangential * np.cos(a))


# name -> (points, category, ring, first slot, (tangential, radial, height) extents)
BANK_SPEC = (
    ("tiny", 9, "person", 12.0, 1, (0.6, 0.6, 1.0)),
    ("low", 10, "person", 12.0, 3, (0.8, 0.8, 0.5)),
    ("chained", 33, "bicycle", 13.0, 5, (0.8, 0.9, 1.0)),
    ("road_count", 64, "car", 18.0, 9, (1.2, 1.0, 1.5)),
    ("one_frame", 65, "car", 21.0, 13, (1.2, 1.0, 1.5)),
    ("wrap", 47, "motorcycle", 25.0, 0, (1.0, 1.0, 1.2)),
    ("long", 300, "truck", 35.0, 17, (1.6, 9.0, 2.0)),
    ("behind_low", 20, "bicyclist", 15.0, 2, (1.4, 0.9, 1.5)),
    ("behind_chained", 40, "other-vehicle", 16.0, 10, (1.6, 1.0, 1.6)),
)
# the sample: (bank name, velocity, first trial angles in units of 18 degrees); the rest of each order is filled in ascending order
SAMPLE_SPEC = (
    ("tiny", 0.5, (0,)),
    ("low", 0.2, (0,)),                       # accepted at trial 0 in slot 3
    ("chained", 2.5, (2, 1, 3)),              # slot 7: road, blocked; slot 8: no road; slot 11: accepted at trial 2
    ("road_count", -0.6, (1, 2)),             # slot 10: exactly 5 road points; slot 12: exactly 6, accepted at trial 1
    ("one_frame", 5.0, (1, 2)),               # slot 14: blocked in frame 3 only; slot 16: accepted at trial 1
    ("wrap", 1.3, (0,)),                      # slot 0: across the phi wrap; no road on its ring elsewhere
    ("long", 0.1, (0, 1)),                    # slots 17, 18: road, radial extent 8.8
    ("behind_low", -1.5, (1,)),               # slot 3, behind `low`: its view box holds the two top points of `low`
    ("behind_chained", 0.25, (1, 2)),         # slot 11, behind `chained`: blocked by pasted points; slot 13: accepted at trial 1
)
EXPECTED = (-1, 0, 2, 1, 1, -1, -1, 0, 1)
# (ring, slot, road points)
ROAD_PATCHES = ((12.0, 3, 12), (13.0, 7, 12), (13.0, 11, 12), (18.0, 10, 5), (18.0, 12, 6), (21.0, 14, 12), (21.0, 16, 12), (25.0, 0, 12),
                (35.0, 17, 12), (35.0, 18, 12), (15.0, 3, 12), (16.0, 11, 12), (16.0, 13, 12))


def make_bank():
    rng = np.random.Generator(np.random.PCG64(4100))
    bank = []
    for name, m, cate, ring, slot, (lt, wr, h) in BANK_SPEC:
        local = rng.uniform(-0.5, 0.5, (m, 3)) * np.array([lt, wr, h]) * 0.96
        local[:, 2] += 0.5 * h
        if name == "low":                       # eight points up to 0.2 m, two at the top
            local[:8, 2] = rng.uniform(0.0, 0.2, 8)
            local[8:, 2] = (0.5, 0.49)
        if name == "long":                      # the radial extent is carried by four points at the two ends
            local[:2, 1], local[2:4, 1] = -4.4, 4.4
        local[0, 2], local[1 % m, 0], local[2 % m, 0] = 0.0, -0.48 * lt, 0.48 * lt
        x, y = place(ring, slot, local[:, 0], local[:, 1])
        pcds = np.stack((x, y, -0.9 + local[:, 2], rng.random(m)), axis=1).astype(F)
        cx, cy = place(ring, slot)
        yaw = slot_azimuth(slot) - 0.5 * np.pi                # heading clockwise: the velocity is radial
        bank.append(preprocess.PasteObject(pcds, (cx, cy, -0.9 + 0.5 * h), (lt, wr, h), yaw, cate))
    return bank


def reference_velocity(cate, nominal):
    """(uniform draw, velocity): what random_f (copy_paste.py:52-53) makes of the uniform draw that aims at `nominal`."""
    lo, hi = preprocess.PASTE_VELOCITY[cate]
    u = (nominal - lo) / (hi - lo)
    return u, lo + (hi - lo) * u


def _names():
    return [s[0] for s in BANK_SPEC]


def make_draws(bank):
    rng = np.random.Generator(np.random.PCG64(4200))
    index, velocity, order, noise = [], [], [], []
    for name, v, head in SAMPLE_SPEC:
        i = _names().index(name)
        index.append(i)
        velocity.append(reference_velocity(bank[i].cate, v)[1])
        order.append(list(head) + [a for a in range(preprocess.PASTE_TRIALS) if a not in head])
        noise.append(rng.normal(0.0, preprocess.PASTE_NOISE_STD, (preprocess.TRAIN_FRAMES, bank[i].pcds.shape[0], 3)))
    return preprocess.PasteDraws(index, velocity, order, noise)


def _centre(name, v, slot, t, height):
    """Where the object's centre stands in frame t when a trial has brought it to `slot` (it moves inwards for v > 0)."""
    ring = dict((s[0], s[3]) for s in BANK_SPEC)[name]
    x, y = place(ring, slot, 0.0, -v * t * 0.1)
    return (x, y, ROAD_Z + height)


def designed_points(k):
    """Points every scan carries (xyz, id): road patches, victims inside accepted boxes, blockers."""
    rng = np.random.Generator(np.random.PCG64(4300))           # the same in every frame
    xyz, ids = [], []
    for n_patch, (ring, slot, count) in enumerate(ROAD_PATCHES):
        for _ in range(count):
            x, y = place(ring, slot, rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25))
            xyz.append((x, y, ROAD_Z + 0.01 * n_patch + rng.uniform(-0.02, 0.02)))
            ids.append(40)
    # inside the box `low` is accepted with: four ids next to the class ranges and two inside them (2 < 3: still valid)
    for j, sem in enumerate((9, 33, 251, 260, 32, 252)):
        x, y = place(12.0, 3, -0.1 + 0.04 * j, 0.05)
        xyz.append((x, y, ROAD_Z + 0.05 + 0.01 * j))
        ids.append(sem)
    # `chained` in slot 7: three object-class points inside its box in every frame
    for j, sem in enumerate((10, 18, 259)):
        c = _centre("chained", 2.5, 7, k, 0.4 + 0.1 * j)
        xyz.append((c[0] + 0.01 * j, c[1], c[2]))
        ids.append(sem)
    # `one_frame` in slot 14: three of them in frame 3 only (two in the other frames)
    for j, sem in enumerate((252, 20, 31)):
        if j < 2 or k == 3:
            c = _centre("one_frame", 5.0, 14, k, 0.5 + 0.1 * j)
            xyz.append((c[0], c[1] + 0.01 * j, c[2]))
            ids.append(sem)
    return np.array(xyz, dtype=np.float64), np.array(ids, dtype=np.uint32)


def designed_scans():
    """The five scans in frame 0's coordinates (float64), their label words and which of their points are designed ones."""
    scans, words, designed = [], [], []
    for k, n_back in enumerate(BACKGROUND_COUNTS):
        rng = np.random.Generator(np.random.PCG64(4400 + k))
        az, r = rng.uniform(0, 2 * np.pi, n_back), rng.uniform(4.0, 48.0, n_back)
        ground = rng.random(n_back) < 0.6
        z = np.where(ground, ROAD_Z + rng.normal(0, 0.02, n_back), rng.uniform(-1.5, 1.5, n_back))
        ids = BACKGROUND_IDS[rng.integers(0, BACKGROUND_IDS.shape[0], n_back)]
        high = rng.random(n_back) < 0.05                      # object classes at 0.5 rad of elevation and more
        z = np.where(high, r * rng.uniform(0.6, 1.0, n_back), z)
        ids = np.where(high, HIGH_IDS[rng.integers(0, HIGH_IDS.shape[0], n_back)], ids)
        xyz = np.stack((r * np.cos(az), r * np.sin(az), z), axis=1)
        dxyz, dids = designed_points(k)
        at = rng.permutation(n_back + dxyz.shape[0])          # the designed points are spread through the scan
        xyz, ids = np.concatenate((xyz, dxyz))[at], np.concatenate((ids, dids))[at]
        designed.append(at >= n_back)
        inten = rng.random(xyz.shape[0])
        scans.append(np.concatenate((xyz, inten[:, None]), axis=1))
        words.append(ids | (rng.integers(0, 1 << 16, ids.shape[0]).astype(np.uint32) << np.uint32(16)))
    return scans, words, designed


def poses():
    return [synth.synthetic_pose(k) for k in preprocess.train_window_indices(6, 12)]


def _raw_from_designed(designed, pose_list):
    """The raw scan whose first alignment lands next to the designed points (the alignment rounds once more)."""
    inv0 = np.linalg.inv(pose_list[0])
    raw = []
    for s, p in zip(designed, pose_list):
        back = np.linalg.inv(inv0.dot(p))
        xyz = s[:, :3].dot(back[:3, :3].T) + back[:3, 3]
        raw.append(np.concatenate((xyz, s[:, 3:]), axis=1).astype(F))
    return raw


def align(raw, pose_list):
    inv0 = np.linalg.inv(pose_list[0])
    return [preprocess.pose_align(s, inv0.dot(p)) for s, p in zip(raw, pose_list)]


def road_of(aligned0, words0):
    return aligned0[(words0 & np.uint32(0xFFFF)) == preprocess.PASTE_ROAD_ID]


def _steer(raw, words, designed, pose_list, bank, draws):
    """Delete the background points that sit within the margin of a tested box bound (a handful) and lift the designed ones
    among them by 5 mm, until none is left."""
    for _ in range(8):
        aligned = align(raw, pose_list)
        trace = []
        preprocess.copy_paste_sample(aligned, words, road_of(aligned[0], words[0]), bank, draws, LABEL_BASE, trace=trace)
        drop = [set() for _ in raw]
        for rec in trace:
            for t, fr in enumerate(rec.get("frames", ())):
                drop[t].update(int(i) for i in fr.get("near", ()) if i < raw[t].shape[0])
        if not any(drop):
            return raw, words
        for t, rows in enumerate(drop):
            keep = np.ones(raw[t].shape[0], dtype=bool)
            keep[list(rows)] = False
            keep |= designed[t]
            raw[t][[i for i in rows if designed[t][i]], 2] += F(0.005)      # the poses turn about z: a raw z is an aligned z
            raw[t], words[t], designed[t] = raw[t][keep], words[t][keep], designed[t][keep]
    raise AssertionError("the steering did not converge")


@functools.lru_cache(maxsize=None)
def sample():
    """dict: scans (raw), words, poses, aligned, road, bank, draws, and the twin's outputs out_scans / out_words / status / trace.
    Asserts the margin condition and that every case of EXPECTED is taken for the reason it is meant to be."""
    bank, pose_list = make_bank(), poses()
    draws = make_draws(bank)
    scene, words, designed = designed_scans()
    raw = _raw_from_designed(scene, pose_list)
    raw, words = _steer(raw, words, designed, pose_list, bank, draws)
    # a scan-0 point with exactly the x, y of the phi-max point of `road_count` as it is pasted in frame 0: it sits on the
    # box's upper phi bound, which is open.  (Frame 0's alignment is the identity up to 1e-16, so the raw x, y survive it.)
    aligned = align(raw, pose_list)
    out, _, status = preprocess.copy_paste_sample(aligned, words, road_of(aligned[0], words[0]), bank, draws, LABEL_BASE)
    first = aligned[0].shape[0] + sum(bank[i].pcds.shape[0] for i in draws.index[:3])
    rows = out[0][first:first + 64]
    _, phi, theta = preprocess.view_angles(rows[:, 0], rows[:, 1], rows[:, 2])
    top = int(np.argmax(phi))
    assert status[3] == 1 and theta.min() + 1e-3 < theta[top] < theta.max() - 1e-3
    tie_row = raw[0].shape[0]
    raw[0] = np.concatenate((raw[0], np.array([[rows[top, 0], rows[top, 1], rows[top, 2], 0.5]], dtype=F)))
    words[0] = np.concatenate((words[0], np.array([72 | (7 << 16)], dtype=np.uint32)))
    # unequal lengths, none a multiple of the wave size
    assert all(s.shape[0] % 64 for s in raw) and len(set(s.shape[0] for s in raw)) == 5, [s.shape[0] for s in raw]

    aligned = align(raw, pose_list)
    assert np.array_equal(aligned[0][tie_row, :2], rows[top, :2])
    road = road_of(aligned[0], words[0])
    trace = []
    out_scans, out_words, status = preprocess.copy_paste_sample(aligned, words, road, bank, draws, LABEL_BASE, trace=trace)

    # ---- the margin condition ----
    for v in draws.velocity:
        assert min(abs(abs(v) - 0.3), abs(abs(v) - 1.0)) > 1e-6
    ties = 0
    for rec in trace:
        assert rec["road_edge"] > 1e-6, rec
        for t, fr in enumerate(rec.get("frames", ())):
            for span, limit in zip(fr["spans"], preprocess.PASTE_SPANS):
                assert abs(span - limit) > 1e-4, (rec["object"], rec["trial"], t, fr["spans"])
            near = [int(i) for i in fr.get("near", ())]
            if near:                         # only the designed tie, which sits on the bound itself
                assert near == [tie_row] and t == 0 and rec["object"] == 3, (rec["object"], rec["trial"], t, near)
                _, p, _ = preprocess.view_angles(*aligned[0][tie_row:tie_row + 1, :3].T)
                assert float(p[0]) == fr["box"][1]
                ties += 1
    assert ties == 1

    # ---- every case is taken, for its reason ----
    assert tuple(status) == EXPECTED, status
    by = {}
    for rec in trace:
        by[(rec["object"], rec["trial"])] = rec
    assert not any(o == 0 for o, _ in by)                                            # under 10 points: never tried
    assert by[(1, 0)]["frames"][0]["blockers"] == 2                                  # ids 32 and 252 count, 9 / 33 / 251 / 260 do not
    assert by[(2, 0)]["road_count"] > 5 and not any(by[(2, 0)]["valid"])             # road passed, view failed: the lift stays
    assert by[(2, 1)]["road_count"] == 0 and by[(2, 2)]["road_count"] > 5
    assert by[(3, 0)]["road_count"] == 5 and by[(3, 1)]["road_count"] == 6
    assert by[(4, 0)]["valid"] == [True, True, True, False, True]                    # the all-frames AND
    assert all(by[(5, j)]["road_count"] == 0 or by[(5, j)]["frames"][0]["spans"][1] > 6.0 for j in range(20))
    assert sum(by[(5, j)]["road_count"] > 5 for j in range(20)) >= 1
    assert sum(by[(6, j)]["road_count"] > 5 for j in range(20)) >= 2
    assert all(by[(6, j)]["road_count"] == 0 or by[(6, j)]["frames"][0]["spans"][0] >= 8.0 for j in range(20))
    taken = [fr["removed_pasted"] for fr in by[(7, 0)]["frames"]]                    # takes the top points of `low` away
    assert max(taken) <= 2 and taken[0] in (1, 2), taken
    assert by[(8, 0)]["road_count"] > 5 and all(fr["blockers"] >= 3 for fr in by[(8, 0)]["frames"])
    removed = [int((o[:a.shape[0], 0] == F(preprocess.PAD_XYZI)).sum()) for o, a in zip(out_scans, aligned)]
    assert min(removed) > 0
    return dict(scans=raw, words=words, poses=pose_list, aligned=aligned, road=road, bank=bank, draws=draws, out_scans=out_scans,
                out_words=out_words, status=status, trace=trace, tie_row=tie_row)


def lift_count(s, obj):
    """How many road lifts object number `obj` of the sample went through up to and including its accepted trial."""
    return sum(1 for rec in s["trace"] if rec["object"] == obj and rec["road_count"] > preprocess.PASTE_MIN_ROAD)


def z_bound(road_z, count, lifts):
    """Bound on |z_a - z_b| of a pasted point between two implementations that differ only in the order in which they sum the
    float32 road heights of a trial.  For n road points the two means differ by at most (ceil(log2 n) + 2) 2^-24 max|z_road|.
    A lift is z += mean - min(z) in float32: the difference of the means enters once, and the subtraction and the sum round once
    each on either side; two roundings of values below 2 m (asserted by the comparison) differ by at most one ulp, 2^-23, each.
    The lifts of the road-passing trials up to the accepted one accumulate."""
    zmax = float(np.abs(road_z).max())
    per_lift = (np.ceil(np.log2(max(count, 2))) + 2) * 2.0 ** -24 * zmax + 2.0 ** -22
    return lifts * per_lift


def layout(s):
    """(sizes, slot starts) of the sample's objects: object i owns rows n_k + start_i .. + size_i of every frame."""
    sizes = [s["bank"][i].pcds.shape[0] for i in s["draws"].index]
    return sizes, np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64).tolist()


def fixture_sample(g):
    """sample() checked against the fixture's inputs (tests/golden/copy_paste.npz): the fixture was made from these very arrays."""
    import hashlib
    s = sample()
    h = hashlib.sha256()
    for a in s["scans"]:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    assert h.hexdigest() == str(g["scans_sha"]), "the fixture was generated from other scans: regenerate it"
    for k in range(5):
        assert np.array_equal(s["words"][k], g["word_%d" % k])
    assert np.array_equal(np.stack(s["poses"]), g["pose"])
    bank = [preprocess.PasteObject(g["bank_pcds_%d" % i], g["bank_center_%d" % i], g["bank_size_%d" % i], g["bank_yaw_%d" % i],
                                   str(g["bank_cate"][i])) for i in range(len(g["bank_cate"]))]
    assert len(bank) == len(s["bank"]) and all(np.array_equal(a.pcds, b.pcds) and np.array_equal(a.center, b.center)
                                               and np.array_equal(a.size, b.size) and a.yaw == b.yaw for a, b in zip(bank, s["bank"]))
    draws = preprocess.PasteDraws(g["draw_index"], g["draw_velocity"], g["draw_order"],
                                  [g["draw_noise_%d" % i] for i in range(len(g["draw_index"]))])
    assert draws.index == s["draws"].index and draws.velocity == s["draws"].velocity
    assert np.array_equal(draws.order, s["draws"].order) and all(np.array_equal(a, b) for a, b in zip(draws.noise, s["draws"].noise))
    return s


def reference_arrays(s, g):
    """What the reference left behind: per frame the points, the label word of each (originals: their word; appended rows:
    LABEL_BASE + motion label) and the stage-2 label of the appended rows."""
    pts, words = [], []
    for k in range(5):
        keep = np.ones(s["aligned"][k].shape[0], dtype=bool)
        keep[g["removed_%d" % k]] = False
        pts.append(np.concatenate((s["aligned"][k][keep], g["tail_%d" % k])))
        words.append(np.concatenate((s["words"][k][keep], (LABEL_BASE + g["tail_label_%d" % k].astype(np.int64)).astype(np.uint32))))
    return pts, words


def compare_with_reference(out_scans, out_words, status, s, g):
    """(mismatch counts, z ratios): everything but the z of a pasted point is compared for equality, that z against z_bound of
    its object (ratios = |dz| / bound, one array per object that was pasted)."""
    sizes, starts = layout(s)
    bad = {"status": int((np.asarray(status) != g["status"]).sum()), "removed": 0, "kept_rows": 0, "slot_state": 0, "xyi": 0, "word": 0}
    ratios = {}
    road_z = s["road"][:, 2]
    pad = np.array(preprocess.PASTE_PAD, dtype=F)
    for k in range(5):
        n = s["aligned"][k].shape[0]
        got, words = np.asarray(out_scans[k]), np.asarray(out_words[k])
        assert got.shape == (n + sum(sizes), 4) and words.shape == (n + sum(sizes),) and got.dtype == F
        gone = (got[:n] == pad).all(axis=1)
        bad["removed"] += int(not np.array_equal(np.nonzero(gone)[0], g["removed_%d" % k]))
        bad["kept_rows"] += int((got[:n][~gone] != s["aligned"][k][~gone]).sum()) + int((words[:n] != s["words"][k]).sum())
        tail, tail_label, at = g["tail_%d" % k], g["tail_label_%d" % k], 0
        for i, (m, start) in enumerate(zip(sizes, starts)):
            rows, w = got[n + start:n + start + m], words[n + start:n + start + m]
            live = ~(rows == pad).all(axis=1)
            if g["status"][i] < 0:
                bad["slot_state"] += int(live.sum()) + int((w != 0).sum())
                continue
            # a later object may have taken some of these rows away again: the reference's tail holds the survivors in order
            want = tail[at:at + int(live.sum())]
            ok = want.shape[0] == int(live.sum()) and want.shape[0] > 0
            bad["slot_state"] += int(not ok)
            if not ok:
                continue
            at += want.shape[0]
            bad["xyi"] += int((rows[live][:, [0, 1, 3]] != want[:, [0, 1, 3]]).sum())
            bad["word"] += int((w[live].astype(np.int64) - LABEL_BASE != tail_label[at - want.shape[0]:at]).sum())
            assert max(np.abs(want[:, 2]).max(), np.abs(road_z).max()) < 2.0
            bound = z_bound(road_z, 12, lift_count(s, i))
            ratios.setdefault(i, []).append(np.abs(rows[live][:, 2].astype(np.float64) - want[:, 2]) / bound)
        bad["slot_state"] += int(at != tail.shape[0])
    return bad, dict((i, np.concatenate(r)) for i, r in ratios.items())

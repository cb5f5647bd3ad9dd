"""The references and cases of tests/stream_cases.py, checked without a GPU: every restatement there against the project's pinned
ones (preprocess.build_sample / pose_align / range_mask, oracle.ops_np.vote_*, kitti.MovingIoU) wherever both apply, the size
conditions the cases are named for, the two measured ulp allowances of the angle bound, and -- "the cases can tell" -- that each
deliberately wrong restatement changes the expected result of the case built against it."""
import numpy as np
import pytest

from oracle import ops_np
from streammos_amd import device_preprocess, preprocess
from tests import stream_cases as cases

F32 = np.float32


# ---- A. preprocessing -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.PREP_CASES)
def test_row_model_equals_build_sample(name):
    """emit_rows + form_batch against build_sample: at N where the scan fits, at max c + 1 cut to N rows where it does not."""
    c, w = cases.prep_case(name), cases.prep_want(name)
    with np.errstate(invalid="ignore"):
        xyzi, coord, sphere = cases.form_rows(c, cases.emit_rows(c))
    assert xyzi.shape == (c.V, c.T, 7, c.N, 1) and coord.shape == (c.V, c.T, c.N, 3, 1)
    # the angles are left out: numpy's float32 arcsin / arctan2 give another last bit in the vector body than in the tail of an
    # array, so two numpy runs over arrays of different lengths need not agree (the angles have their own reference below)
    assert sphere.shape == w.sphere.shape == (c.V, c.T, c.N, 2, 1)
    assert cases.same_bits(xyzi, w.xyzi) and cases.same_bits(coord, w.coord)
    assert not np.isnan(xyzi).any()                                           # every row was written
    if name not in cases.PREP_OVERFLOW:
        assert w.n_host == c.N and (w.counts < c.N).all()
        host = preprocess.build_sample(c.scans, cases.host_poses(c), c.N, cases.SPEC, tta=c.tta)
        assert np.array_equal(host["pcds_xyzi"], w.xyzi) and host["pad_length"] == c.N - w.counts[0]
        device_preprocess.check_in_range_counts(w.counts.tolist(), c.N)
    else:
        with pytest.raises(ValueError):
            preprocess.build_sample(c.scans, cases.host_poses(c), c.N, cases.SPEC, tta=c.tta)
        with pytest.raises(ValueError):
            device_preprocess.check_in_range_counts(w.counts.tolist(), c.N)


def test_prep_cases_hold_what_they_are_named_for():
    want = {n: cases.prep_want(n) for n in cases.PREP_CASES}
    case = {n: cases.prep_case(n) for n in cases.PREP_CASES}
    assert case["tta_off"].V == 1 and all(case[n].V == 4 for n in ("tiny", "faces", "axes", "overflow"))
    assert case["tiny"].scans[0].shape[0] == 5
    c = case["n_gt_N"]
    assert c.scans[0].shape[0] == 700 > c.N == 256 and 150 <= want["n_gt_N"].counts[0] <= 250
    assert case["n_lt_N"].scans[0].shape[0] < case["n_lt_N"].N and case["n_lt_N"].scans[1].shape[0] > case["n_lt_N"].N
    assert not want["all_out"].counts.any() and case["all_out"].scans[0].shape[0] > 0
    assert (want["all_out"].xyzi[:, :, 2] == preprocess.PAD_Z).all()
    assert case["empty_history"].scans[1].shape[0] == 0 and want["empty_history"].counts.tolist()[1] == 0
    assert case["empty_current"].scans[0].shape[0] == 0 and want["empty_current"].counts[1] > 0
    assert case["identity_none"].diffs[1] is None and np.array_equal(case["identity_eye"].diffs[1], np.eye(4))
    assert np.array_equal(want["identity_none"].xyzi, want["identity_eye"].xyzi)
    for n in cases.PREP_CASES:
        if n not in ("second_sweep",):
            assert 64 <= case[n].N <= 512, n
    # second trips: grid_for caps at SWEEP threads; transform_mask and unpad_labels walk n, emit walks max(n, N)
    c = case["second_sweep"]
    n = c.scans[0].shape[0]
    assert (c.T, c.V, n, c.N) == (1, 1, 2048 * 256 + 300, 300000) and n > cases.SWEEP
    assert 0.45 * n < want["second_sweep"].counts[0] < 0.55 * n and want["second_sweep"].counts[0] < c.N
    assert np.flatnonzero(want["second_sweep"].mask).max() >= cases.SWEEP     # a kept point is met on the second trip
    assert all(case[k].scans[0].shape[0] < cases.SWEEP for k in cases.PREP_CASES if k != "second_sweep")
    # overflow
    c = case["overflow"]
    assert want["overflow"].counts[0] == c.N + 37 and c.N < want["overflow"].counts[1] <= c.N + 5 and c.T == 2
    assert want["overflow_exact"].counts[0] == case["overflow_exact"].N > want["overflow_exact"].counts[1] > 0
    assert (want["overflow"].xyzi[:, :, 2] != preprocess.PAD_Z).all()         # no padding row in an overflowing scan
    assert (want["overflow_exact"].xyzi[:, 0, 2] != preprocess.PAD_Z).all()
    assert (want["overflow_exact"].xyzi[:, 1, 2] == preprocess.PAD_Z).any()   # scan 1 keeps its own


def test_faces_case_keeps_the_lower_faces_and_drops_the_upper_ones():
    c, w = cases.prep_case("faces"), cases.prep_want("faces")
    lo, hi = [r[0] for r in cases.RANGES], [r[1] for r in cases.RANGES]
    xyz, keep = cases.face_points(lo, hi)
    assert xyz.shape == (24, 3) and np.array_equal(c.scans[0][:24, :3], xyz)
    assert np.array_equal(w.mask[:24], keep) and keep.sum() == 15
    for d in range(3):
        on_lo, in_lo, out_lo, mid = xyz[8 * d:8 * d + 4, d]
        on_hi, in_hi, out_hi, _ = xyz[8 * d + 4:8 * d + 8, d]
        assert on_lo == F32(lo[d]) and out_lo < on_lo < in_lo < mid < in_hi < on_hi < out_hi and on_hi == F32(hi[d])
        assert np.nextafter(out_lo, F32(np.inf)) == on_lo and np.nextafter(on_lo, F32(np.inf)) == in_lo
        assert np.nextafter(in_hi, F32(np.inf)) == on_hi and np.nextafter(on_hi, F32(np.inf)) == out_hi
    assert not w.mask[24:].any() and np.isnan(c.scans[0][24:, :3]).sum() == 3 and np.isinf(c.scans[0][24:, :3]).sum() == 6
    moved, masks = cases.moved_scans(c)
    assert moved[1][:2, 0].tolist() == [50.0, -50.0] and masks[1].tolist() == [False, True, True, False, True]


def test_unpad_reference_is_the_numpy_scatter():
    for name in cases.PREP_CASES:
        c, w = cases.prep_case(name), cases.prep_want(name)
        labels = np.arange(1, c.N + 1, dtype=np.int64).astype(np.uint8)
        got = cases.unpad_want(c, labels)
        assert got.shape == (c.scans[0].shape[0],)
        if name not in cases.PREP_OVERFLOW:
            want = np.zeros(c.scans[0].shape[0], dtype=np.uint8)              # as tests/test_gpu_preprocess.py states it
            want[w.mask] = labels[:int(w.mask.sum())]
            assert np.array_equal(got, want), name
        else:
            kept = np.flatnonzero(w.mask)
            assert np.array_equal(got[kept[:c.N]], labels) and not got[kept[c.N:]].any() and not got[~w.mask].any()


# ---- range-view angles ----------------------------------------------------------------------------------------------------

def test_angle_allowances_are_the_measured_ones_and_numpy_float32_is_inside_the_bound():
    worst_asin = worst_atan = 0.0
    for name in cases.ANGLE_CASES:
        w = cases.prep_want(name)
        x, y, z = cases.angle_inputs(w.xyzi)
        # numpy's float32 path on the float32 inputs, as preprocess.quantize_sphere runs it
        xf, yf, zf = x.astype(F32), y.astype(F32), z.astype(F32)
        t32 = zf / (np.sqrt(xf ** 2 + yf ** 2 + zf ** 2) + F32(1e-12))
        d_asin = cases.ulp_distance(np.arcsin(t32), np.arcsin(t32.astype(np.float64)))
        d_atan = cases.ulp_distance(np.arctan2(xf, yf), np.arctan2(x, y))
        r_th, r_phi = cases.angle_ratios(w.sphere, w.xyzi)
        print("stream-angles host %-6s numpy float32: arcsin %.1f ulp, arctan2 %.1f ulp from the rounded float64; error / bound "
              "theta %.4f phi %.4f" % (name, d_asin, d_atan, r_th, r_phi))
        assert r_th <= 1.0 and r_phi <= 1.0, (name, r_th, r_phi)
        worst_asin, worst_atan = max(worst_asin, d_asin), max(worst_atan, d_atan)
    assert cases.ulp_allowance(worst_asin) == cases.ASIN_ULP, worst_asin
    assert cases.ulp_allowance(worst_atan) == cases.ATAN2_ULP, worst_atan


def test_axes_case_holds_its_points_and_tells_atan2_y_x_apart():
    c, w = cases.prep_case("axes"), cases.prep_want("axes")
    assert w.counts[0] == 8 and c.V == 4
    x, y, z = cases.angle_inputs(w.xyzi)
    th, phi = cases.angle_ref(x, y, z)
    b_th, b_phi = cases.angle_bounds(x, y, z)
    # the branch cut: the raw -0 is +0 after the pose alignment, so (+-0, -3) are both column 0; flipped to -0, both 2048
    assert np.signbit(c.scans[0][4, 0]) and not np.signbit(c.scans[0][3, 0])
    assert not np.signbit(w.xyzi[0, 0, 0, 3:5, 0]).any() and np.signbit(w.xyzi[2, 0, 0, 3:5, 0]).all()
    assert (np.abs(phi[0, 0, 3:5]) < 1e-3).all() and (np.abs(phi[2, 0, 3:5] - 2048) < 1e-3).all()      # y = -3: the cut
    assert (np.abs(phi[1, 0, 3:5] - 1024) < 1e-3).all() and (np.abs(phi[3, 0, 3:5] - 1024) < 1e-3).all()  # y = +3: atan2(+-0, 3)
    assert not cases.same_bits(w.xyzi[0], w.xyzi[2]) and np.array_equal(w.xyzi[0, 0, 0, 3:5], w.xyzi[2, 0, 0, 3:5])
    # the vertical: asin(+-1), a tenth of a cell of room and no more
    assert 0.05 < b_th[0, 0, 1] < 0.2 and 0.05 < b_th[0, 0, 2] < 0.2
    away = np.ones(b_th.shape, dtype=bool)
    away[:, :, 1:3] = False
    assert b_th[away].max() < 2e-4 and b_phi.max() < 1.5e-3
    assert (w.xyzi[:, 0, 2, 8:, 0] == preprocess.PAD_Z).all()                  # the padding point is among the inputs
    # a wrong branch or swapped arguments are far outside: on every point off the diagonal
    _, wrong = cases.angle_ref(x, y, z, swap=True)
    assert (np.abs(wrong - phi) > b_phi)[:, :, 3:7].all()
    assert float((np.abs(wrong - phi) / b_phi).max()) > 1e3


# ---- B. voting ------------------------------------------------------------------------------------------------------------

def _frame_reference(c):
    """oracle.ops_np.vote_frame on a case whose labels are all <= 2 and whose probe is its last frame."""
    hist = [(cases.aligned(p, d)[:, :3], l) for p, l, d in c.frames[:-1]]
    return ops_np.vote_frame(c.frames[-1][0], c.frames[-1][1], np.concatenate([h[0] for h in hist]) if hist else np.zeros((0, 3), F32),
                             np.concatenate([h[1] for h in hist]) if hist else np.zeros(0, np.uint8))


@pytest.mark.parametrize("name", ["faces", "non_finite", "second_sweep"])
def test_vote_references_equal_vote_frame(name):
    """Where the pinned pipeline applies -- true division, labels 0..2, the probe is the last frame -- table + resolve equal it."""
    c = cases.vote_case(name)
    assert c.frames[-1][2] is None and np.array_equal(c.frames[-1][0], c.probe, equal_nan=True) and not c.recip
    table, resolved = cases.vote_want(name)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(resolved, _frame_reference(c))
    counts = cases.table_counts(table)
    kept = sum(int((cases.linear_voxel(cases.aligned(p, d)) >= 0).sum()) for p, _, d in c.frames)
    assert counts.sum() == kept > 0


def test_vote_table_equals_the_dense_histogram():
    """The packed words against ops_np.vote_voxel_labels' histogram (its argmax, and the counts through np.bincount)."""
    c = cases.vote_case("ragged13")
    table, _ = cases.vote_want("ragged13")
    pts = np.concatenate([cases.aligned(p, d)[:, :3] for p, _, d in c.frames])
    lab = np.concatenate([l for _, l, _ in c.frames]).astype(np.int64)
    keep = ops_np.vote_crop_mask(pts)
    q = ops_np.vote_quantize(pts[keep])
    lin = (q[:, 0] * 512 + q[:, 1]) * 30 + q[:, 2]
    counts = np.bincount(lin * 3 + lab[keep], minlength=3 * cases.VOTE_CELLS).reshape(-1, 3)
    assert np.array_equal(cases.table_counts(table), counts)
    assert np.array_equal(counts.argmax(-1), ops_np.vote_voxel_labels(q, lab[keep]).reshape(-1))


def test_recip_case_parts_the_two_conventions():
    c = cases.vote_case("recip")
    pts = cases.recip_points()
    assert ops_np.vote_crop_mask(pts).all()
    a, b = ops_np.vote_quantize(pts), cases.vote_quantize_recip(pts)
    assert np.array_equal(a[:, :2], b[:, :2])                                  # x / y: never
    differ = int((a[:, 2] != b[:, 2]).sum())
    print("recip: %d of 87 points land in another voxel under the reciprocal" % differ)
    assert differ >= 8
    assert len(set(map(tuple, a[:, :2].tolist()))) == 87                        # every point in an x / y cell of its own
    assert np.array_equal(pts[1::3, 2], np.array([F32(-4.0 + 0.2 * k) for k in range(1, 30)]))
    # the x / y claim on the boundaries themselves: every cell boundary of x and its two neighbours
    edge = (np.arange(1, 512, dtype=np.float64) * (25.0 / 128.0) - 50.0).astype(F32)
    col = np.concatenate((edge, np.nextafter(edge, F32(-100)), np.nextafter(edge, F32(100))))
    probe = np.stack((col, col, np.zeros_like(col)), axis=1)
    assert np.array_equal(ops_np.vote_quantize(probe)[:, :2], cases.vote_quantize_recip(probe)[:, :2])
    # D: true division under the flag changes table and labels
    table, resolved = cases.vote_want("recip")
    wrong = cases.vote_table(c.frames, recip=True, true_division_under_recip=True)
    assert not np.array_equal(table, wrong)
    assert int((table != wrong).sum()) == 2 * differ
    assert np.array_equal(cases.vote_resolve_ref(c.probe, c.probe_labels, table, recip=True), resolved)
    assert np.array_equal(resolved, (c.probe_labels + 1) % 3)


def test_vote_faces_are_open_and_a_closed_crop_is_told_apart():
    c = cases.vote_case("faces")
    pts, keep_half_open = cases.face_points(cases.CROP_LO, cases.CROP_HI)
    inside = ops_np.vote_crop_mask(pts)
    assert inside.sum() == 12 and keep_half_open.sum() == 15                    # both face values are out: 4 x 6 - 2 x 6
    for d in range(3):
        assert not inside[8 * d] and inside[8 * d + 1] and not inside[8 * d + 2] and inside[8 * d + 3]
        assert not inside[8 * d + 4] and inside[8 * d + 5] and not inside[8 * d + 6]
    table, resolved = cases.vote_want("faces")
    near = np.arange(24) % 4 != 3                                               # the six copies of INSIDE share one voxel
    assert np.array_equal(resolved[~inside], c.probe_labels[~inside])
    assert np.array_equal(resolved[inside & near], (c.probe_labels[inside & near] + 1) % 3)
    wrong = cases.vote_table(c.frames, crop=cases.crop_closed)
    assert not np.array_equal(table, wrong)
    assert not np.array_equal(cases.vote_resolve_ref(c.probe, c.probe_labels, wrong, crop=cases.crop_closed), resolved)


def test_ties_case_goes_to_the_lowest_class():
    c = cases.vote_case("ties")
    table, resolved = cases.vote_want("ties")
    pts, lab, _ = c.frames[0]
    voxel_labels = ops_np.vote_voxel_labels(ops_np.vote_quantize(pts), lab.astype(np.int64))
    assert np.array_equal(ops_np.vote_point_labels(ops_np.vote_quantize(c.probe), voxel_labels), resolved)
    assert resolved.tolist() == list(cases.TIES_WANT)
    lin = cases.linear_voxel(c.probe)
    assert len(set(lin.tolist())) == len(cases.TIES) and [tuple(r) for r in cases.table_counts(table[lin]).tolist()] == list(cases.TIES)
    high = cases.vote_resolve_ref(c.probe, c.probe_labels, table, ties_high=True)
    assert high.tolist() != resolved.tolist() and high.tolist() == [1, 2, 2, 2, 2, 2, 2, 1]


def test_strides_labels_case_and_the_skip_of_labels_above_two():
    c = cases.vote_case("strides_labels")
    table, resolved = cases.vote_want("strides_labels")
    lut = cases.wide_lut()
    assert lut.shape == (256,) and len(set(lut.tolist())) == 256 and not set(lut.tolist()) & set(range(256))
    inside = cases.linear_voxel(c.probe) >= 0
    lab = c.probe_labels
    for v in (0, 1, 2, 3, 7, 255):
        assert (lab[inside] == v).any() and (lab[~inside] == v).any(), v       # every label on both sides of the crop
    assert np.array_equal(resolved[~inside], lab[~inside]) and resolved[inside].max() <= 2
    mapped = cases.vote_resolve_ref(c.probe, lab, table, lut=lut)
    assert np.array_equal(mapped, lut[resolved]) and (mapped[~inside & (lab == 255)] == lut[255]).all()
    assert lab[0] == 255 and resolved[0] == 2 and lab[-1] == 7 and resolved[-1] == 0 and inside[0] and inside[-1]
    # labels <= 2 alone give the same table: labels above 2 cast no vote ...
    low = [(p[l <= 2], l[l <= 2], d) for p, l, d in c.frames]
    assert np.array_equal(cases.vote_table(low), table)
    counted = sum(int(((cases.linear_voxel(cases.aligned(p, d)) >= 0) & (l <= 2)).sum()) for p, l, d in c.frames)
    assert cases.table_counts(table).sum() == counted
    # ... and D: with the skip removed the table changes (label 3 lands in bit 63)
    wrong = cases.vote_table(c.frames, skip_above_2=False)
    assert not np.array_equal(wrong, table) and (wrong < 0).any()


def test_non_finite_case():
    c = cases.vote_case("non_finite")
    table, resolved = cases.vote_want("non_finite")
    assert not np.isfinite(c.probe[:9]).all(axis=1).any() and np.isfinite(c.probe[9:]).all()
    assert np.array_equal(resolved[:9], c.probe_labels[:9])
    assert [d is None for _, _, d in c.frames] == [False, False, True]
    for p, l, d in c.frames:
        assert (cases.linear_voxel(cases.aligned(p, d))[:9] == -1).all()


def test_vote_size_conditions():
    assert cases.SWEEP == 2048 * 256 and cases.VOTE_MAX_POINTS == 2 ** 21 - 1 and cases.LABEL_SWEEP == 1024 * 256 * 4
    c = cases.vote_case("second_sweep")
    assert c.frames[0][0].shape == (cases.SWEEP + 300, 3) and cases.SWEEP < c.probe.shape[0] < 2 ** 21
    assert (cases.linear_voxel(c.probe[cases.SWEEP:]) >= 0).any()
    for name, n_frames, launches in (("ragged13", 13, 2), ("ragged25", 25, 3)):
        c = cases.vote_case(name)
        lengths = [p.shape[0] for p, _, _ in c.frames]
        assert sum(1 for n in lengths if n > 0) == n_frames and 0 in lengths
        assert set(lengths) == {1, 63, 0, 257, 9000, cases.SWEEP + 300} and lengths.count(cases.SWEEP + 300) == 1
        groups = cases.frame_launches(lengths)
        assert len(groups) == launches and [len(g) for g in groups] == [12] * (launches - 1) + [1]
        assert all(len(set(g)) >= 4 for g in groups[:-1])                              # uneven lengths inside a launch
        assert sum(lengths) < 2 ** 21
        poses = [d is None for _, _, d in c.frames]
        assert any(poses) and not all(poses)
    for name in cases.VOTE_CASES:
        if name not in ("second_sweep", "ragged13", "ragged25"):
            assert all(p.shape[0] < cases.SWEEP for p, _, _ in cases.vote_case(name).frames)
    assert cases.COUNTER_WORD == 0x1FFFFF | 3 << 21 | 2 << 42
    assert cases.linear_voxel(np.array([cases.COUNTER_POINT], dtype=F32))[0] >= 0
    word = np.array([cases.COUNTER_WORD], dtype=np.int64)
    assert cases.table_counts(word).tolist() == [[2 ** 21 - 1, 3, 2]]


# ---- C. label tail --------------------------------------------------------------------------------------------------------

def test_label_cases_and_reference():
    assert cases.LABEL_SIZES[:7] == (2, 3, 4, 5, 255, 256, 257)
    big = cases.LABEL_SIZES[-1]
    assert big == 1024 * 256 * 4 + 4 * 64 + 3 and big // 4 > cases.LABEL_SWEEP // 4 and big % 4 == 3
    assert all(n <= cases.LABEL_SWEEP for n in cases.LABEL_SIZES[:-1])
    gmap = cases.gt_map()
    assert gmap.shape == (260,) and gmap.dtype == np.int32 and set(gmap.tolist()) == {0, 1, 2}
    for n in cases.LABEL_SIZES:
        c = cases.label_case(n)
        sem = c.gt & 0xFFFF
        g = cases.mapped_gt(c.gt)
        assert not g[sem >= 260].any() and np.array_equal(g[sem < 260], gmap[sem[sem < 260]])
        if n >= 255:
            assert {260, 0xFFFF} <= set(sem.tolist()) and set(c.labels.tolist()) == set(cases.LABEL_BYTES)
            assert (c.gt >> 16).max() > 0
        words, counts = cases.label_ref(c, "lut")
        raw, counts_raw = cases.label_ref(c, "raw")
        assert np.array_equal(counts, counts_raw) and np.array_equal(raw, c.labels.astype(np.int32))
        assert not words[c.labels > 2].any() and np.array_equal(words[c.labels <= 2], cases.WORD_LUT[c.labels[c.labels <= 2]])
        # a byte above 2 predicts neither class; its ground truth is counted as usual
        low = c.labels <= 2
        assert np.array_equal(counts[:4], cases.iou_counts(g[low], c.labels[low])[:4])
        assert counts[4] == (g == 1).sum() and counts[5] == (g == 2).sum()
        # where the labels are 0..2 and the ids inside the map: the statement of tests/test_gpu_sequence_overlap.py
        ok = low & (sem < 260)
        assert np.array_equal(cases.iou_counts(gmap[sem[ok]], c.labels[ok])[:4], cases.iou_counts(g[ok], c.labels[ok])[:4])
        vw, vc = cases.label_ref(c, "voted")
        assert np.array_equal(vw, c.voted)
        assert np.array_equal(vc, cases.iou_counts(g, np.where(c.voted == 251, 2, np.where(c.voted == 9, 1, 0))))
    c = cases.label_case(5)
    assert c.labels.tolist() == [3, 255, 1, 2, 0] and (c.gt & 0xFFFF).tolist() == [252, 40, 0xFFFF, 260, 252]
    assert cases.label_ref(c, "lut")[1].tolist() == [0, 0, 0, 0, 1, 2]           # gt: 252 (twice) moving, 40 static; no prediction hits


# ---- D. overflow: the guard ----------------------------------------------------------------------------------------------

def test_overflow_case_tells_the_missing_guard():
    """Without count = min(prefix[-1], N) and `j < N` the surplus of the last scan lands in the next variant's scan 0."""
    c, w = cases.prep_case("overflow"), cases.prep_want("overflow")
    good, bad = cases.emit_rows(c), cases.emit_rows(c, guard=False)
    spill = int(w.counts[1]) - c.N
    assert 0 < spill <= 5
    differ = (good != bad).any(axis=-1)
    assert differ[1:, 0, :spill].all() and differ.sum() == 3 * spill
    moved, masks = cases.moved_scans(c)
    assert np.array_equal(np.abs(bad[1:, 0, :spill]), np.abs(np.broadcast_to(moved[1][masks[1]][c.N:], (3, spill, 4))))
    assert not cases.same_bits(cases.form_rows(c, bad)[0], w.xyzi)
    e = cases.prep_case("overflow_exact")
    assert np.array_equal(cases.emit_rows(e), cases.emit_rows(e, guard=False))   # c == N: nothing to drop, nothing to pad

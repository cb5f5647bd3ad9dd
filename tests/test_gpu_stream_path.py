"""The scan-to-label path on the GPU -- csrc/preprocess.hip through DevicePreprocessor, the voting kernels of csrc/vote.hip through
ops.vote_*, csrc/labels.hip through ops.label_words / voted_label_counts -- against the references of tests/stream_cases.py
(cases and derivations there; tests/test_host_stream_reference.py holds them to the pinned restatements without a GPU).

EVERYTHING IS EXACT except the two range-view angles: masks, counts, table words and labels with array_equal / torch.equal, the
float32 outputs of the preprocessor as bit patterns (stream_cases.same_bits: the sign of a zero counts, it picks the branch of
atan2f).  The angles are held element by element inside the bound derived in stream_cases (ratio = error / bound <= 1).

Case -> kernel path reached:
    prep tta_off / tiny / n_gt_N / n_lt_N / all_out / empty_* / identity_*   prep_emit with V = 1 and 4, span = n and = N, count = 0,
                                                                             n = 0 (null scan pointers), the identity shortcut
    prep faces                                                               every face of the half-open range test, non-finite
                                                                             input, a face reached through the float64 pose product
    prep axes / tiny / faces                                                 asinf at 0 and +-1, atan2f on its cut and axes
    prep second_sweep                                                        second trip of prep_transform_mask / prep_emit /
                                                                             prep_unpad_labels
    prep overflow / overflow_exact                                           count = min(prefix, N), the j < N guards of prep_emit
                                                                             and prep_unpad_labels
    vote recip                                                               the recip_quantize branch of voxel_of
    vote strides_labels                                                      strides 3 / 4 / 6, the label > 2 skip, lut[label & 0xFF]
    vote ties / faces / non_finite                                           the argmax, the open crop, NaN / inf through load_xyz
    vote second_sweep / ragged13 / ragged25                                  second trips; blockIdx.y frames of uneven lengths in
                                                                             two and three launches
    vote counter_width                                                       a full 21-bit field beside two small ones; the n < 2^21
                                                                             refusals
    labels 2 .. 257, LABEL_SWEEP + 259                                       tail only, body + tail, a second trip; three modes

With SMOS_STREAM_RATIOS_FILE set, the angle ratios and the time of the single-voxel run are appended to that file
(profiles/stream_path_error_ratios.txt is made from it)."""
import os
import time

import numpy as np
import pytest
import torch

from streammos_amd import _lib, device_preprocess, ops
from tests import stream_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = -7


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _record(line):
    print(line)
    path = os.environ.get("SMOS_STREAM_RATIOS_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- A. preprocessing -----------------------------------------------------------------------------------------------------

def _poison(c):
    """NaN into the allocator's free blocks of the sizes the build is about to take (as
    test_look_ahead_orders_the_side_stream_behind_uploads_pending_on_main does): an element the kernels leave unwritten shows."""
    sizes = [c.V * c.T * k * c.N for k in (7, 3, 2)]
    for s in c.scans:
        sizes += [4 * s.shape[0], s.shape[0], s.shape[0]]
    junk = [torch.full((max(n, 1),), float("nan"), device=DEV) for n in sizes for _ in range(2)]
    del junk


def _build(name, strict=False):
    c = cases.prep_case(name)
    pre = device_preprocess.DevicePreprocessor(DEV, cases.SPEC, c.N, tta=c.tta)
    scans = [_t(s) for s in c.scans]
    torch.cuda.synchronize()
    _poison(c)
    return c, pre, pre.build(scans, c.diffs, strict=strict)


@pytest.mark.parametrize("name", cases.PREP_CASES)
def test_preprocessor_equals_build_sample(name):
    c, pre, built = _build(name)
    w = cases.prep_want(name)
    n_raw = c.scans[0].shape[0]
    assert built["n_raw"] == n_raw and pre.V == c.V
    assert np.array_equal(built["mask"].cpu().numpy().astype(bool), w.mask)
    if n_raw:
        assert int(built["prefix"][-1]) == int(w.counts[0])
    assert np.array_equal(built["in_range_counts"].cpu().numpy(), w.counts)
    xyzi, coord, sphere = (built[k].cpu().numpy() for k in ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord"))
    assert cases.same_bits(coord, w.coord), int((coord.view(np.int32) != w.coord.view(np.int32)).sum())
    assert cases.same_bits(xyzi, w.xyzi), int((xyzi.view(np.int32) != w.xyzi.view(np.int32)).sum())
    assert sphere.shape == w.sphere.shape and not np.isnan(sphere).any()
    if name in cases.PREP_OVERFLOW:
        # rows [0, N) are those of the host build at c + 1 (prep_want), none of them padding; both checks raise like the host path
        assert w.n_host > c.N and (xyzi[:, 0, 2] != device_preprocess.preprocess.PAD_Z).all()
        with pytest.raises(ValueError):
            pre.check_capacity(built)
        with pytest.raises(ValueError):
            pre.build([_t(s) for s in c.scans], c.diffs, strict=True)
    else:
        pre.check_capacity(built)
    # labels back to the raw scan: nonzero everywhere, inside a longer buffer whose tail a read past N would bring in
    rng = np.random.default_rng(5)
    labels = rng.integers(1, 4, c.N).astype(np.uint8)
    buf = torch.full((c.N + 64,), 99, dtype=torch.uint8, device=DEV)
    buf[:c.N] = _t(labels)
    raw = pre.unpad_labels(buf[:c.N], built)
    assert raw.shape == (n_raw,) and raw.dtype == torch.uint8
    assert np.array_equal(raw.cpu().numpy(), cases.unpad_want(c, labels))


@pytest.mark.parametrize("name", cases.ANGLE_CASES)
def test_range_view_angles_inside_the_float64_bound(name):
    c, pre, built = _build(name)
    w = cases.prep_want(name)
    xyzi, sphere = built["pcds_xyzi"].cpu().numpy(), built["pcds_sphere_coord"].cpu().numpy()
    assert cases.same_bits(xyzi, w.xyzi)                    # the reference is computed from the x, y, z the kernel emitted
    r_th, r_phi = cases.angle_ratios(sphere, xyzi)
    _record("stream-angles %-6s %5d values: error / bound theta %.4f phi %.4f" % (name, sphere.size // 2, r_th, r_phi))
    assert r_th <= 1.0 and r_phi <= 1.0, (name, r_th, r_phi)


# ---- B. voting ------------------------------------------------------------------------------------------------------------

def _table():
    table = torch.empty(cases.VOTE_CELLS, dtype=torch.int64, device=DEV)
    ops.vote_clear(table)
    return table


def _device_frames(frames):
    """An empty frame is made on the device: the copy of an empty host tensor comes back with strides the wrappers refuse."""
    return [(_t(p) if p.shape[0] else torch.zeros((0, p.shape[1]), device=DEV), _t(l), d) for p, l, d in frames]


def _accumulate(frames, recip):
    table = _table()
    for p, l, d in frames:
        ops.vote_accumulate(p, l, table, pose_diff=d, recip_quantize=recip)
    return table


def _check_table(table, want):
    assert table.dtype == torch.int64
    same = torch.equal(table, _t(want))
    assert same, int((table.cpu().numpy() != want).sum())


@pytest.mark.parametrize("name", cases.VOTE_CASES)
def test_vote_table_and_labels(name):
    """Per-frame launches and the one-call frame set give the numpy table word for word; resolve gives the labels, plain and
    through a 256-entry LUT."""
    c = cases.vote_case(name)
    want_table, want = cases.vote_want(name)
    frames = _device_frames(c.frames)
    table = _accumulate(frames, c.recip)
    _check_table(table, want_table)
    batched = _table()
    ops.vote_accumulate_frames(frames, batched, recip_quantize=c.recip)
    assert torch.equal(batched, table)
    probe, own = _t(c.probe), _t(c.probe_labels)
    got = ops.vote_resolve(probe, own, table, recip_quantize=c.recip)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    lut = cases.wide_lut()
    mapped = ops.vote_resolve(probe, own, table, lut=_t(lut), recip_quantize=c.recip)
    assert np.array_equal(mapped.cpu().numpy(), lut[want])
    if name == "ties":
        assert want.tolist() == list(cases.TIES_WANT)


def test_recip_flag_selects_the_reciprocal_and_equals_torch_on_the_device():
    c = cases.vote_case("recip")
    want_table, _ = cases.vote_want("recip")
    frames = _device_frames(c.frames)
    # the flag off: the true division, another table and other labels -- a kernel that ignored the flag would fail above
    plain = _accumulate(frames, False)
    _check_table(plain, cases.vote_table(c.frames, recip=False))
    assert not torch.equal(plain, _t(want_table))
    got = ops.vote_resolve(_t(c.probe), _t(c.probe_labels), plain, recip_quantize=False).cpu().numpy()
    assert np.array_equal(got, cases.vote_resolve_ref(c.probe, c.probe_labels, plain.cpu().numpy()))
    # the reference's Quantize in torch ops on the device tensor: tensor / Python double.  What torch computes here is what
    # the variant exists to reproduce
    p = _t(c.probe)
    lo, hi, size = cases.ops_np.VOTE_FOV[0], cases.ops_np.VOTE_FOV[1], cases.ops_np.VOTE_SIZE
    q = [((p[:, d] - lo[d]) / ((hi[d] - lo[d]) / size[d])).to(torch.int64) for d in range(3)]
    lin = ((q[0] * size[1] + q[1]) * size[2] + q[2]).cpu().numpy()
    assert np.array_equal(lin, cases.linear_voxel(c.probe, recip=True)), int((lin != cases.linear_voxel(c.probe, recip=True)).sum())
    from_torch = np.zeros(cases.VOTE_CELLS, dtype=np.int64)
    for _, labels, _ in c.frames:
        np.add.at(from_torch, lin, np.int64(1) << (21 * labels.astype(np.int64)))
    _check_table(_accumulate(frames, True), from_torch)


def test_point_strides_and_labels_above_two():
    c = cases.vote_case("strides_labels")
    want_table, want = cases.vote_want("strides_labels")
    lut = cases.wide_lut()

    def layout(points, kind):
        xyz = _t(points[:, :3])
        if kind == 3:
            return xyz.contiguous()
        wide = torch.full((points.shape[0], kind), float("nan"), device=DEV)
        wide[:, :3] = xyz
        return wide if kind == 4 else wide[:, :4]

    for kind in (3, 4, 6):
        frames = [(layout(p, kind), _t(l), d) for p, l, d in c.frames]
        assert all(p.stride(0) == kind and p.stride(1) == 1 for p, _, _ in frames)
        table = _accumulate(frames, False)
        _check_table(table, want_table)
        batched = _table()
        ops.vote_accumulate_frames(frames, batched)
        assert torch.equal(batched, table)
        probe, own = layout(c.probe, kind), _t(c.probe_labels)
        assert np.array_equal(ops.vote_resolve(probe, own, table).cpu().numpy(), want), kind
        assert np.array_equal(ops.vote_resolve(probe, own, table, lut=_t(lut)).cpu().numpy(), lut[want]), kind


def test_counter_width_and_the_refusals():
    n = cases.VOTE_MAX_POINTS
    point = torch.tensor([cases.COUNTER_POINT], dtype=torch.float32, device=DEV)
    pts = point.expand(n + 1, 3).contiguous()
    zeros = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
    table = _table()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.vote_accumulate(pts[:n], zeros[:n], table)
    torch.cuda.synchronize()
    _record("stream-counter_width: %d atomic adds on one voxel in %.1f ms" % (n, 1e3 * (time.perf_counter() - t0)))
    ops.vote_accumulate(pts[:5], _t(np.array([1, 1, 1, 2, 2], dtype=np.uint8)), table)
    lin = int(cases.linear_voxel(np.array([cases.COUNTER_POINT], dtype=np.float32))[0])
    assert int(table[lin]) == cases.COUNTER_WORD and int(torch.count_nonzero(table)) == 1
    assert ops.vote_resolve(pts[:3], _t(np.array([2, 1, 0], dtype=np.uint8)), table).tolist() == [0, 0, 0]
    # 2^21 points could carry a field into its neighbour: refused, in one frame and as the total of a frame set
    before = table.clone()
    with pytest.raises(RuntimeError):
        ops.vote_accumulate(pts, zeros, table)
    half = (n + 1) // 2
    with pytest.raises(RuntimeError):
        ops.vote_accumulate_frames([(pts[:half], zeros[:half], None), (pts[half:], zeros[half:], None)], table)
    torch.cuda.synchronize()
    assert torch.equal(table, before)
    ops.vote_accumulate_frames([(pts[:half], zeros[:half], None), (pts[half:n], zeros[half:n], None)], _table())   # 2^21 - 1 passes


# ---- C. label tail --------------------------------------------------------------------------------------------------------

def _label_inputs(n):
    c = cases.label_case(n)
    return c, _t(c.labels), _t(c.voted), _t(c.gt.view(np.int32)), _t(cases.gt_map())


def _run_mode(mode, lab, voted, words, gt=None, gt_map=None, counts=None):
    if mode == "voted":
        return ops.voted_label_counts(voted, gt, gt_map, counts, words=words)
    return ops.label_words(lab, words=words, lut=mode == "lut", gt=gt, gt_map=gt_map, counts=counts)


@pytest.mark.parametrize("n", cases.LABEL_SIZES)
def test_label_words_and_counts(n):
    c, lab, voted, gt, gt_map = _label_inputs(n)
    assert gt_map.numel() == cases.GT_MAP_LEN
    for mode in ("lut", "raw", "voted"):
        want_words, want_counts = cases.label_ref(c, mode)
        words = torch.full((n + 9,), FILL, dtype=torch.int32, device=DEV)
        counts = torch.zeros(6, dtype=torch.int64, device=DEV)
        _run_mode(mode, lab, voted, words, gt, gt_map, counts)
        got = words.cpu().numpy()
        assert np.array_equal(got[:n], want_words), (mode, int((got[:n] != want_words).sum()))
        assert (got[n:] == FILL).all(), mode                                   # a longer buffer keeps its fill beyond n
        assert np.array_equal(counts.cpu().numpy(), want_counts), (mode, counts.tolist(), want_counts.tolist())
        if mode != "voted":                                                    # without counting: the same words
            plain = torch.full((n + 9,), FILL, dtype=torch.int32, device=DEV)
            _run_mode(mode, lab, voted, plain)
            assert torch.equal(plain, words)


def test_misaligned_label_inputs_are_refused_and_nothing_is_written():
    n = 257
    c, lab, voted, gt, gt_map = _label_inputs(n)
    shifted = lambda t: torch.cat((t[:1], t))[1:]                              # the same values, one element further on
    lab1, voted1, gt1 = shifted(lab), shifted(voted), shifted(gt)
    assert lab1.data_ptr() % 4 == 1 and voted1.data_ptr() % 16 == 4 and gt1.data_ptr() % 16 == 4 and torch.equal(lab1, lab)
    wide = torch.full((n + 9,), FILL, dtype=torch.int32, device=DEV)
    words, words1 = wide[:n + 4], wide[1:]
    counts = torch.zeros(6, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    attempts = []
    for mode in ("lut", "raw", "voted"):
        attempts += [lambda m=mode: _run_mode(m, lab1, voted1, words, gt, gt_map, counts),                 # labels / voted
                     lambda m=mode: _run_mode(m, lab, voted, words1, gt, gt_map, counts),                   # words
                     lambda m=mode: _run_mode(m, lab, voted, words, gt1, gt_map, counts)]                   # gt
    # the same through the C entries, past the wrapper's own checks
    for lut in (1, 0):
        for l, w, g in ((lab1, words, gt), (lab, words1, gt), (lab, words, gt1)):
            attempts.append(lambda lut=lut, l=l, w=w, g=g: _lib.call(
                "smos_label_words", l.data_ptr(), n, lut, w.data_ptr(), g.data_ptr(), gt_map.data_ptr(), gt_map.numel(),
                counts.data_ptr(), stream))
    for v, w, g in ((voted1, words, gt), (voted, words1, gt), (voted, words, gt1)):
        attempts.append(lambda v=v, w=w, g=g: _lib.call(
            "smos_label_count_voted", v.data_ptr(), n, w.data_ptr(), g.data_ptr(), gt_map.data_ptr(), gt_map.numel(),
            counts.data_ptr(), stream))
    assert len(attempts) == 18
    for attempt in attempts:
        with pytest.raises(RuntimeError):
            attempt()
    torch.cuda.synchronize()
    assert (wide == FILL).all() and not counts.any()
    # the aligned call on the same tensors goes through
    _run_mode("lut", lab, voted, words, gt, gt_map, counts)
    assert np.array_equal(words.cpu().numpy()[:n], cases.label_ref(c, "lut")[0])

"""The references and case generators behind tests/test_gpu_stem.py, checked on the host (tests/util.py).

(a) the weight packing: what stem_gemm and stem_epilogue compute from ops.stem_prepare_weights' four tensors -- the
    documented (mt, s, lane) operand layout, the nine taps with their class / slot, the pooled maximum with 0 for an empty
    cell inside the grid and nothing for a tap outside it -- emulated in float64 numpy equals stem_dense_ref to 1e-12 of
    the output range;
(b) stem_plan_ref satisfies the invariants of a plan: rows numbered exactly once, class order non-decreasing,
    row_of[row_cell] == arange, the class bounds partition the rows;
(c) stem_dense_ref evaluated in float32 on the CPU stays inside the tolerance the GPU tests use against the float64 run,
    for every case: the tolerance is one a correct fp32 implementation meets;
(d) the ReLU hides neither run: the lifted bias clips fewer than 1 % of the reference's outputs, the plain one fewer
    than 35 % -- for every case with an occupied cell (without one the output is relu(bias) and there is nothing to hide);
(e) pointnet_rows_ref against a per-point loop, and the walk generators against their stated coverage.
"""
import numpy as np
import pytest
import torch

from tests import util


def _emulated_stem(x, plan, wprep, bias):
    """stem_gemm + stem_epilogue in float64: x [B, H, W, Cin] channels-last, wprep = ops.stem_prepare_weights(wa, wp)."""
    from streammos_amd import ops
    b, h, w = plan.b, plan.h, plan.w
    cin, c = x.shape[-1], bias.shape[0]
    cells = x.reshape(b * h * w, cin)
    ys = []
    for cls in range(4):
        p = wprep[cls].double().numpy()                        # [kM, Cin/2, 64], (mt, s, lane) = W[mt*32 + (lane & 31)][(lane >> 5) * Cin/2 + s]
        km = p.shape[0]
        assert km == ops.STEM_TAPS[cls] + 1 and p.shape[1:] == (cin // 2, 64)
        wmat = np.zeros((km * 32, cin))
        for mt in range(km):
            for s in range(cin // 2):
                for lane in range(64):
                    wmat[mt * 32 + (lane & 31), (lane >> 5) * (cin // 2) + s] = p[mt, s, lane]
        rows = plan.row_cell[plan.bounds[cls]:plan.bounds[4 + cls]]
        ys.append(cells[rows] @ wmat.T)                        # Y_cls[r][mt*32 + c] = sum_k W[mt*32 + c][k] X[row][k]
    ho_n, wo_n = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    out = np.zeros((b, c, ho_n, wo_n))
    for s in range(b):
        for ho in range(ho_n):
            for wo in range(wo_n):
                acc, qmax = np.zeros(c), np.full(c, -np.inf)
                for t9 in range(9):
                    ky, kx = t9 // 3, t9 % 3
                    y, xx = 2 * ho - 1 + ky, 2 * wo - 1 + kx
                    if not (0 <= y < h and 0 <= xx < w):
                        continue                               # outside the grid: nothing
                    rid = plan.row_of[(s * h + y) * w + xx]
                    if rid < 0:
                        qmax = np.maximum(qmax, 0.0)           # an empty cell inside the grid: 0 for the pooled branch
                        continue
                    ey, ex = (ky & 1) ^ 1, (kx & 1) ^ 1
                    cls, taps = ey * 2 + ex, (1 + ey) * (1 + ex)
                    slot = (ky >> 1 if ey else 0) * (1 + ex) + (kx >> 1 if ex else 0)
                    assert cls == (y & 1) * 2 + (xx & 1) and taps == ops.STEM_TAPS[cls]
                    row = ys[cls][rid - plan.bounds[cls]]
                    acc = acc + row[slot * c:(slot + 1) * c]
                    qmax = np.maximum(qmax, row[taps * c:(taps + 1) * c])
                out[s, :, ho, wo] = np.maximum((acc + qmax) + bias, 0.0)
    return out


@pytest.mark.parametrize("name", ["6x10_half", "2x2_full"])
@pytest.mark.parametrize("variant", util.STEM_VARIANTS)
def test_weight_packing_and_slot_rule_reproduce_the_dense_block(name, variant):
    from streammos_amd import ops
    c = util.stem_case(name)
    wprep = ops.stem_prepare_weights(torch.tensor(c.wa), torch.tensor(c.wp).float())      # float64 in, float32 out: exact
    for which in util.STEM_BIASES:
        got = _emulated_stem(c.x[variant], c.plan, wprep, c.bias[variant][which])
        want = c.want[variant][which]
        scale = np.abs(want).max()
        assert got.shape == want.shape and scale > 0
        assert np.abs(got - want).max() <= 1e-12 * scale


@pytest.mark.parametrize("name", sorted(util.STEM_CASES) + ["pns/" + n for n in sorted(util.PNS_CASES)])
def test_plan_reference_invariants(name):
    plan = util.pns_case(name[4:]).plan if name.startswith("pns/") else util.stem_case(name).plan
    b, h, w, n = plan.b, plan.h, plan.w, plan.rows
    occupied = plan.row_of >= 0
    assert occupied.sum() == n == plan.occ.sum() and len(plan.row_cell) == n
    assert np.array_equal(occupied.reshape(b, h, w), plan.occ)
    assert np.array_equal(np.sort(plan.row_of[occupied]), np.arange(n))                    # numbered exactly once
    assert np.array_equal(plan.row_of[plan.row_cell], np.arange(n))
    cy, cx = (plan.row_cell // w) % h, plan.row_cell % w
    cls = (cy & 1) * 2 + (cx & 1)
    assert (cls[1:] >= cls[:-1]).all()
    first, last = plan.bounds[:4], plan.bounds[4:]
    assert first[0] == 0 and last[3] == n and np.array_equal(first[1:], last[:3])
    for k in range(4):
        assert (cls[first[k]:last[k]] == k).all() and last[k] - first[k] == (cls == k).sum()
        key = plan.row_cell[first[k]:last[k]].astype(np.int64)                             # sample, then y >> 1, then x >> 1
        assert (np.diff(key) > 0).all()


def test_plan_reference_cell_rule_at_the_borders():
    """-1 < c < size, cell = trunc(c): (-1, 0) lands in cell 0, size - 2^-10 in the last cell, -1.0 and size are outside."""
    e = 2.0 ** -10
    coord = np.full((1, 1, 6, 3), -100.0)
    coord[0, 0, :, :2] = [(-0.5, -e), (4 - e, 6 - e), (-1.0, 1.5), (1.5, -1.0), (4.0, 1.5), (1.5, 6.0)]
    plan = util.stem_plan_ref(coord, 1, 4, 6)
    assert np.array_equal(np.flatnonzero(plan.occ.reshape(-1)), [0, 23])
    assert np.array_equal(plan.row_cell, [0, 23]) and np.array_equal(plan.bounds, [0, 1, 1, 1, 1, 1, 1, 2])


def test_cases_reach_what_they_are_named_for():
    c = util.stem_case
    assert [c(n).plan.rows for n in ("2x2_no_points", "6x10_no_points")] == [0, 0]
    assert np.array_equal(c("2x2_full").plan.bounds, [0, 1, 2, 3, 1, 2, 3, 4])
    half = c("6x10_half").plan
    assert 4 * (2 * 3 * 5) < util.STEM_SCAN_TILE and (2 * 3 * 5) % 8 and half.occ[0, 0, 0] and half.occ[0, 5, 9]
    assert c("6x10_half").b * c("6x10_half").t * c("6x10_half").n < 2 * 6 * 10            # the row table's capacity is the point count
    for k in range(4):
        n_c = np.diff(c("8x8_class%d" % k).plan.bounds.reshape(2, 4), axis=0)[0]
        assert n_c[k] > 0 and n_c.sum() == n_c[k]
    for rows in (31, 32, 33):
        assert np.array_equal(np.diff(c("16x16_rows%d" % rows).plan.bounds.reshape(2, 4), axis=0)[0], [1, 0, 0, rows])
    full = c("46x46_full").plan
    assert full.occ.all() and util.STEM_SCAN_TILE < 46 * 46 < 2 * util.STEM_SCAN_TILE
    mixed = c("64x96_mixed").plan
    per = 3 * 32 * 48
    flags = np.concatenate([mixed.occ[:, k >> 1::2, k & 1::2].reshape(-1) for k in range(4)])
    assert len(flags) == 4 * per == 9 * util.STEM_SCAN_TILE and per % util.STEM_SCAN_TILE
    tiles = flags.reshape(9, -1).sum(1)
    empty = np.flatnonzero(tiles == 0)
    assert len(empty) and 0 < empty[0] and tiles[empty[0] + 1:].any() and not mixed.occ[1].any()   # an empty tile inside the look-back chain
    assert mixed.occ[2].any() and not mixed.occ[2, 1::2].any() and not mixed.occ[2, :, 1::2].any()


@pytest.mark.parametrize("name", sorted(util.STEM_CASES))
def test_float32_cpu_run_meets_the_gpu_tolerance(name):
    c = util.stem_case(name)
    for variant in util.STEM_VARIANTS:
        for which in util.STEM_BIASES:
            want = c.want[variant][which]
            got = util.stem_dense_ref(c.x[variant].transpose(0, 3, 1, 2), c.wa, c.wp, c.bias[variant][which], dtype=np.float32)
            scale = np.abs(want).max()
            err = np.abs(got.astype(np.float64) - want).max() / scale
            print("stem-host %s %s %s float32-cpu %.3e of range, clipped %.3f" % (name, variant, which, err, c.clipped[variant][which]))
            assert scale > 0 and err <= util.STEM_TOL


@pytest.mark.parametrize("name", sorted(n for n in util.STEM_CASES if util.STEM_CASES[n][3] != ("none",)))
def test_relu_does_not_hide_the_outputs(name):
    c = util.stem_case(name)
    assert c.plan.rows > 0
    for variant in util.STEM_VARIANTS:
        assert c.clipped[variant]["lifted"] < 0.01 and c.clipped[variant]["plain"] < 0.35, c.clipped[variant]


@pytest.mark.parametrize("name", ["n33", "t1_b3"])
def test_point_rows_reference_against_a_per_point_loop(name):
    c = util.pns_case(name)
    table = np.zeros((c.plan.rows, c.t, 64))
    for s in range(c.b):
        for f in range(c.t):
            for i in range(c.n):
                py, px = c.coord[s, f, i, :2]
                if -1.0 < py < c.h and -1.0 < px < c.w:
                    hid = np.maximum(c.w1 @ c.xyzi[s, f, :, i] + c.b1, 0.0)
                    out = np.maximum(c.w2 @ hid + c.b2, 0.0).astype(np.float32)
                    row = c.plan.row_of[(s * c.h + int(py)) * c.w + int(px)]
                    table[row, f] = np.maximum(table[row, f], out)
    # (the matrix product of the reference and the loop's matrix-vector products may round differently in float64)
    assert np.abs(table.reshape(c.plan.rows, -1) - c.rows).max() <= 2.0 ** -22 * c.rows.max()
    assert (c.rows > 0).any(1).mean() > 0.9


def test_capped_walks_reach_every_path():
    """The preconditions of the grid-cap GPU tests, from the reference plan (the GPU tests assert them again from the device's
    own counts)."""
    n_c = np.diff(util.stem_case("64x64_cap").plan.bounds.reshape(2, 4), axis=0)[0]
    paths, per_wave, crossings = util.stem_gemm_split(n_c, 1)
    want = {(km, "tile", km) for km in (2, 3, 5)} | {(km, part, cnt) for km in (2, 3, 5) for part in ("head", "tail") for cnt in range(1, km)}
    assert paths == want and min(per_wave) >= 2 * 5 + 2 and crossings == [3]
    _, per_wave, crossings = util.stem_gemm_split(n_c, 3)
    assert min(per_wave) >= 2 * 5 + 2 and crossings[0] >= 1 and crossings[1] >= 1
    c = util.pns_case("n1013")
    kinds = util.pns_tile_kinds(c.coord, c.h, c.w)
    for blocks, trips in ((1, 48), (2, 24)):
        walks = util.pns_wave_walks(kinds, blocks)
        assert len(walks) == 4 * blocks and all(len(wk) == trips for wk in walks)
        pairs = {wk[i:i + 2] for wk in walks for i in range(len(wk) - 1)}
        assert pairs == {a + z for a in "LOP" for z in "LOP"} - {"PP"}                     # frame 0 never follows frame 0 on a wave
        assert any("LOL" in wk for wk in walks) and any("LOOL" in wk for wk in walks)

"""The float64 reference, the bound and the cases of tests/gather_cases.py without a GPU: the reference gather against
torch's float64 CPU F.grid_sample, the reference scatter against oracle.ops_np.voxel_maxpool_fwd, a float32 numpy emulation of
the kernels' expression inside the bound, and the cases checked to be what they are named for."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops_np
from tests import gather_cases as cases

ALL_GS = [(s, n, sc) for s in cases.STRUCTURES for n in cases.NS for sc in cases.SCALES]


def _positions(case):
    iy, ix = ops_np.bilinear_pixel_coords(case.gcoord[..., :2], case.scale, cases.HG, cases.WG)
    return iy.astype(np.float64), ix.astype(np.float64)


@pytest.mark.parametrize("c", cases.GS_CHANNELS)
def test_reference_gather_equals_float64_grid_sample(c):
    """On the float32 positions the kernels use.  torch is not asked about positions that are not finite: those rows are
    sampled at the padding position instead and must be 0 in the reference."""
    worst = 0.0
    for struct in ("runs", "lone0", "notap_runs"):
        for n in cases.NS:
            for sc in cases.SCALES:
                case = cases.gs_case(struct, c, n, sc)
                iy, ix = _positions(case)
                fin = np.isfinite(iy) & np.isfinite(ix)
                iy, ix = np.where(fin, iy, -500.0), np.where(fin, ix, -500.0)
                norm = torch.tensor(np.stack((2.0 * ix / (cases.WG - 1) - 1.0, 2.0 * iy / (cases.HG - 1) - 1.0), -1)).view(case.b, n, 1, 2)
                grid = torch.tensor(case.grid).permute(0, 3, 1, 2)
                want = F.grid_sample(grid, norm, mode="bilinear", padding_mode="zeros", align_corners=True)[..., 0].permute(0, 2, 1).numpy()
                assert not case.S[~fin].any() and not case.A[~fin].any()
                err = np.abs(case.S - want).max()
                worst = max(worst, err / np.abs(want).max()) if np.abs(want).max() > 0 else worst
                assert err <= 1e-12 * max(np.abs(want).max(), 1e-300)
                assert (case.A >= np.abs(case.S) - 1e-12).all()
    print("reference vs grid_sample: worst relative difference %.2e" % worst)


def test_reference_scatter_equals_voxel_maxpool_on_non_negative_rows():
    for struct in cases.STRUCTURES:
        for n in (33, 130):
            case = cases.gs_case(struct, 32, n, "nondyadic")
            rng = np.random.default_rng(n)
            rows = np.abs(rng.standard_normal((case.b, n, 32))).astype(np.float32)
            want, _ = ops_np.voxel_maxpool_fwd(rows.transpose(0, 2, 1), case.scoord, (cases.HO, cases.WO), np.asarray(case.scale, dtype=np.float32))
            got = cases.scatter_max0(rows, case.cell)
            assert got.dtype == np.float32
            assert np.array_equal(got.transpose(0, 2, 1).reshape(want.shape).view(np.int32), want.view(np.int32))


def test_scatter_keeps_zero_where_every_member_is_negative():
    """The contract the kernels have and VoxelMaxPool does not: max(0, members)."""
    for n in cases.NS:
        case = cases.gs_case("negative_grid", 32, n, "dyadic")
        assert (case.grid < 0).all() and (case.S <= 0).all() and (case.S < 0).any() and not case.T.any()
        true_max, _ = ops_np.voxel_maxpool_fwd(case.S.transpose(0, 2, 1), case.scoord, (cases.HO, cases.WO), np.asarray(case.scale, dtype=np.float32))
        assert (true_max < 0).any()


@pytest.mark.parametrize("c", cases.GS_CHANNELS + (3, 71))
def test_float32_emulation_of_the_kernel_expression_stays_inside_the_bound(c):
    worst = {False: 0.0, True: 0.0}
    todo = [cases.gs_case(*k[:1], c, *k[1:]) for k in ALL_GS] if c in cases.GS_CHANNELS else \
           [cases.bil_case(c, n, sc) for n in cases.NS for sc in cases.SCALES]
    if c in cases.GS_CHANNELS:
        todo.append(cases.loop_case(c))
    for case in todo:
        for fused in (False, True):
            got = cases.emulate_f32(case.grid, case.gcoord, case.scale, fused)
            ok, ratio = cases.worst_ratio(got, case.S, case.lim)
            worst[fused] = max(worst[fused], ratio)
            assert ok, (case.name, fused, ratio)
            tgt = cases.scatter_max0(got, case.cell)
            ok, ratio = cases.worst_ratio(tgt, case.T, case.T_lim)
            assert ok, (case.name, fused, ratio)
    print("float32 emulation, C = %d: worst error / bound %.4f un-contracted, %.4f fused" % (c, worst[False], worst[True]))
    assert 0 < worst[False] <= 1 and 0 < worst[True] <= 1


def test_gather_coordinates_reach_every_border_and_every_special():
    for sc in cases.SCALES:
        case = cases.gs_case("lone0", 64, 130, sc)
        iy, ix = _positions(case)
        h, w = cases.HG, cases.WG
        with np.errstate(invalid="ignore"):
            assert ((iy > -1) & (iy < 0)).any() and ((iy > h - 1) & (iy < h)).any() and ((ix > -1) & (ix < 0)).any() and ((ix > w - 1) & (ix < w)).any()
            assert (iy < -1).any() and (iy > h).any() and (ix < -1).any() and (ix > w).any()      # wholly outside
        for py, px in cases.special_pos(h, w):
            # (to a few ulp: W - 1 = 6 is no power of two, and the float32 position chain divides by it)
            assert (np.isclose(iy, py, rtol=0, atol=2e-6) & np.isclose(ix, px, rtol=0, atol=2e-6)).any(), (py, px)
        assert (iy == np.floor(iy))[np.isfinite(iy)].any() and (iy == h - 1).any() and (ix == w - 1).any()
        gy, gx = case.gcoord[..., 0], case.gcoord[..., 1]
        for v in cases.PAD_COORDS:
            assert ((gy == v) & (gx == v)).any()
        assert (np.isnan(gy) & ~np.isnan(gx)).any() and (~np.isnan(gy) & np.isnan(gx)).any() and (np.isnan(gy) & np.isnan(gx)).any()
        assert np.isposinf(case.gcoord).any() and np.isneginf(case.gcoord).any()
        tap = cases.taps(case.gcoord, case.scale, h, w)[3]
        assert set(tap.sum(0).reshape(-1).tolist()) == {0, 1, 2, 4}          # no tap, a corner, an edge, all four
        assert not case.A[~tap.any(0)].any()


def _runs_of(cell_row):
    """Maximal runs of equal cells of one sample: (start, stop, cell)."""
    edges = np.flatnonzero(np.diff(cell_row)) + 1
    starts = np.concatenate(([0], edges))
    stops = np.concatenate((edges, [len(cell_row)]))
    return [(int(a), int(b), int(cell_row[a])) for a, b in zip(starts, stops)]


@pytest.mark.parametrize("sc", list(cases.SCALES))
@pytest.mark.parametrize("n", cases.NS)
def test_scatter_cases_are_what_they_are_named_for(n, sc):
    c = 32
    get = lambda s: cases.gs_case(s, c, n, sc)
    scale = np.asarray(cases.SCALES[sc])
    i = np.arange(n)

    case = get("onecell_neg")
    p = case.scoord * scale
    assert (case.cell == 0).all() and ((p[..., 0] > -1) & (p[..., 0] < 0)).all() and ((p[..., 1] > -1) & (p[..., 1] < 1)).all()
    assert n == 1 or (p[..., 1] < 0).any()
    case = get("onecell_pos")
    p = case.scoord * scale
    assert (case.cell == 0).all() and ((p >= 0) & (p < 1)).all()

    case = get("alternate")
    assert (case.cell >= 0).all() and (np.diff(case.cell, axis=1) != 0).all() and (n < 2 or (case.cell[1, 1::2] == 0).all())

    case = get("straddle")
    for edge in range(32, n, 32):                               # every 31|32 and 63|64 border lies inside one cell
        assert (case.cell[:, edge - 1] == case.cell[:, edge]).all() and (case.cell[:, edge] >= 0).all()
    assert case.cell[0, -1] == case.cell[1, 0]                  # and so does the sample boundary
    assert n < 17 or (np.diff(case.cell, axis=1) != 0).any()

    case = get("holes")
    a = case.cell.max()
    assert set(np.unique(case.cell).tolist()) <= {-1, int(a)}
    assert (case.cell[0, i % 32 == 0] == -1).all() and case.cell[0, n - 1] == -1      # position 0 of every run, the last valid position
    if n >= 3:
        assert case.cell[1, :3].tolist() == [a, -1, a]

    case = get("lone0")
    for s in range(cases.B):
        at = np.flatnonzero(case.cell[s] == 0)
        assert at.tolist() == [j for j in range(n) if j % 64 in cases.LONE0[s]]
        for j in at:                                            # lone: both neighbours are in other cells
            assert (j == 0 or case.cell[s, j - 1] > 0) and (j == n - 1 or case.cell[s, j + 1] > 0)
        p = case.scoord[s, at] * scale
        assert len(at) < 2 or ((p[:, 0] < 0).any() and (p[:, 0] >= 0).any())          # both ways into cell 0
    if n == 130:
        assert {int(j) % 64 for s in range(cases.B) for j in np.flatnonzero(case.cell[s] == 0)} == {0, 1, 15, 30, 31, 32, 33, 62, 63}

    case = get("tailchange")
    if n > 1:
        assert (case.cell[:, :-1] == case.cell[:, :1]).all() and (case.cell[:, -1] != case.cell[:, 0]).all() and case.cell[1, -1] == 0
    assert n in (32, 64) or n % 64                              # the ragged last runs of the list

    case = get("runs")
    tap = cases.has_tap(case)
    assert tap.all()
    if n >= 31:                                                 # a run whose largest member is neither its first nor its last point
        inner = 0
        for s in range(cases.B):
            for a0, a1, cl in _runs_of(case.cell[s]):
                if a1 - a0 >= 3:
                    arg = case.S[s, a0:a1].argmax(0)
                    inner += int(((arg > 0) & (arg < a1 - a0 - 1)).sum())
        assert inner > 0

    case = get("ties")
    for s, d, src in case.dups:
        assert np.array_equal(case.gcoord[s, d], case.gcoord[s, src], equal_nan=True) and np.array_equal(case.scoord[s, d], case.scoord[s, src])
        assert np.array_equal(case.S[s, d], case.S[s, src]) and case.cell[s, d] == case.cell[s, src]
    assert n < 8 or len(case.dups) > 0

    case = get("cell_notap")
    tap = cases.has_tap(case)
    assert (case.cell >= 0).all() and not tap[:, i % 3 == 1].any() and not case.S[:, i % 3 == 1].any()
    assert n < 3 or tap.any()

    for name, run, s in (("notap_runs", 64, 0), ("notap_runs", 32, 1), ("nocell_runs", 64, 0), ("nocell_runs", 32, 1)):
        case = get(name)
        kinds = cases.run_kinds(cases.has_tap(case)[s:s + 1], case.cell[s:s + 1], run)
        want = "Z" if name == "notap_runs" else "S"
        which = [r for r in range(len(kinds)) if (r % 2 == 0 if run == 64 else r % 2 == 1)]
        assert all(kinds[r] == want for r in which) and (which or n <= 32)
        if name == "notap_runs":                               # without a tap, but with cells
            assert (case.cell[s] >= 0).all()


@pytest.mark.parametrize("c", cases.GS_CHANNELS)
def test_run_loop_case_walks_every_pair_of_run_kinds(c):
    case = cases.loop_case(c)
    b, n = case.b, case.n
    assert (b, n) == (3, 394) and n % 64 and n % 32
    tap = cases.has_tap(case)
    k64, k32 = cases.run_kinds(tap, case.cell, 64), cases.run_kinds(tap, case.cell, 32)
    assert len(k64) == 21 and len(k32) == 39
    w64, w32 = cases.walks(k64, 4), cases.walks(k32, 8)         # one block: 4 waves of gather_scatter_cl4 / 8 groups of gather_scatter_cl<32>
    assert [len(w) for w in w64] == [6, 5, 5, 5]
    assert [len(w) for w in w32] == [5, 5, 5, 5, 5, 5, 5, 4]    # groups 6 and 7 share the last wave
    assert cases.walk_pairs(w64) == cases.PAIRS and cases.walk_pairs(w32) == cases.PAIRS
    # every walker crosses a sample boundary, and the last run of every sample is ragged
    per64 = len(k64) // b
    for first in range(4):
        assert len({r // per64 for r in range(first, len(k64), 4)}) > 1
    assert n - (per64 - 1) * 64 == 10
    # two blocks: the walks are still several runs long
    assert min(len(w) for w in cases.walks(k64, 8)) >= 2 and min(len(w) for w in cases.walks(k32, 16)) >= 2
    # Z runs have no tap, S runs no cell, G runs both
    for r, kind in enumerate(k32):
        s, lo = divmod(r, len(k32) // b)
        sl = slice(lo * 32, min(lo * 32 + 32, n))
        assert tap[s, sl].any() == (kind != "Z") and (case.cell[s, sl] >= 0).any() == (kind == "G")
    assert (case.cell == 0).any() and case.neg0.any()

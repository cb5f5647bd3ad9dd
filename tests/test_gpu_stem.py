"""The sparse first stage (csrc/stem.hip: stem_mark, stem_scan, stem_gemm, stem_epilogue) and the compact-row point scatter
(csrc/point_fused.hip: pointnet_scatter with row_of, and its n_live entry point) against float64 references, at shapes small
enough that every branch can be steered.

What reaches what (the cases are built and checked on the host in tests/util.py / tests/test_host_stem_reference.py):
  stem_scan   tile == 0 only, no look-back              2x2_*, 6x10_*, 8x8_*, 16x16_*
              ragged last tile (i0 + k < total)          6x10_* (60 of 2048 cells), 46x46_full (2048 + 68)
              class bounds inside a thread's 8 items     6x10_* (per = 15), 2x2_* (per = 1)
              classes without rows                       *_no_points, 8x8_class*, 16x16_rows*
              look-back over full and over empty tiles   64x96_mixed (9 tiles, per = 2.25 tiles), 64x64_cap
  stem_gemm   total == 0                                 *_no_points
              `valid` false in a tile's tail lanes       16x16_rows31 / 32 / 33, 46x46_full (529 = 16 * 32 + 17 rows per class)
              whole tiles at kM = 2 / 3 / 5, heads and   64x64_cap under grid cap 1 and 3 (the test asserts the split from the
              tails of every count, a block that         device's own row counts)
              crosses class boundaries
  epilogue    Ho = Wo = 1, every tap the cell or outside 2x2_full
              empty in-grid cell -> 0, outside -> nothing every case with SIGNED cell values: pool-branch products are negative,
                                                         so a border window without an empty cell has a negative maximum
                                                         (46x46_full) and one with an empty cell has 0
  scatter     second and later trips of the persistent   n1013 under grid cap 1 (48 trips per wave) and 2 (24), with live,
              loop, the two-deep rotation, the skip path all-outside and all-outside-but-wanted (frame 0) tiles in every order
  n_live      counts 0 .. N + 7                          test_point_scatter_rows_n_live

Bounds: 1e-5 of the reference's output range for the stem (the bound of test_sparse_stem_equals_dense_downsample; a plain
float32 CPU run of the same block stays below 1e-6, tests/test_host_stem_reference.py) and 1e-5 of the reference's maximum
for the scatter (the bound of test_pointnet_scatter_against_unfused_ops).  Everything that is the same arithmetic twice --
compact against dense source, capped against uncapped grid, reused against fresh scratch, with against without n_live -- is
compared bit for bit.  Every test prints its worst error / range (pytest -s); the figures of the MI355X run are kept in
profiles/stem_error_ratios.txt.
"""
import numpy as np
import pytest
import torch

from streammos_amd import ops, scratch
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0


def _t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _flags_all_zero():
    bufs = [buf for _, buf in scratch.entries("stem_flags")]
    return len(bufs) > 0 and not any(bool(buf.any()) for buf in bufs)


def _plan_arrays(plan):
    n_rows = int(plan.meta[11])
    return plan.row_of.cpu().numpy().copy(), plan.row_cell[:n_rows].cpu().numpy().copy(), plan.meta[4:12].cpu().numpy().copy()


def _assert_plan(c, arrays):
    row_of, row_cell, bounds = arrays
    assert row_of.dtype == np.int32 and np.array_equal(row_of, c.plan.row_of)
    assert np.array_equal(row_cell, c.plan.row_cell)
    assert np.array_equal(bounds, c.plan.bounds)


def _run_stem(c, variant, which, wprep=None):
    """stem_plan, then sparse_downsample from the dense grid and from the compact row table -> (plan arrays, dense, compact)."""
    coord = _t(c.coord)
    plan = ops.stem_plan(coord, c.h, c.w, row_floats=util.STEM_CIN)
    arrays = _plan_arrays(plan)
    assert _flags_all_zero()
    x = _t(c.x[variant])                                                  # [B, H, W, 192], zeros at the empty cells
    occupied = plan.row_of.long() >= 0
    plan.rows[plan.row_of.long()[occupied]] = x.view(-1, util.STEM_CIN)[occupied]
    if wprep is None:
        wprep = ops.stem_prepare_weights(_t(c.wa), _t(c.wp))
    bias = _t(c.bias[variant][which])
    dense = ops.sparse_downsample(x, plan, wprep, bias, compact=False)
    compact = ops.sparse_downsample(plan.rows, plan, wprep, bias, compact=True)
    return arrays, dense, compact


def _ratio(label, got, want):
    want = torch.tensor(want, device=DEV)
    assert tuple(got.shape) == tuple(want.shape), (label, got.shape, want.shape)
    scale = want.abs().max().item()
    assert scale > 0
    ratio = (got.double() - want).abs().max().item() / scale
    print("stem-ratio %-58s %.3e" % (label, ratio))
    return ratio


@pytest.mark.parametrize("variant", util.STEM_VARIANTS)
@pytest.mark.parametrize("name", sorted(n for n in util.STEM_CASES if n != "64x64_cap"))
def test_stem_against_float64_reference(name, variant):
    c = util.stem_case(name)
    wprep = ops.stem_prepare_weights(_t(c.wa), _t(c.wp))
    for which in util.STEM_BIASES:
        if c.plan.rows:                                                    # the ReLU hides neither run (else: relu(bias) everywhere)
            assert c.clipped[variant]["lifted"] < 0.01 and c.clipped[variant]["plain"] < 0.35
        arrays, dense, compact = _run_stem(c, variant, which, wprep)
        _assert_plan(c, arrays)
        want = c.want[variant][which]
        assert _ratio("%s %s %s" % (name, variant, which), dense, want) <= util.STEM_TOL
        assert torch.equal(compact, dense)
        if not c.plan.rows:
            bias = _t(c.bias[variant][which]).clamp_min(0.0).view(1, -1, 1, 1)
            assert torch.equal(dense, bias.expand_as(dense))


@pytest.mark.parametrize("variant", util.STEM_VARIANTS)
def test_stem_gemm_work_split_is_invisible(variant):
    """2x64x64 at 60 %: about 507 units.  Grid cap 1: one block, 8 waves of about 63 units -- whole tiles at kM = 2 / 3 / 5,
    heads and tails of every count, all three class boundaries inside the block; cap 3: boundaries inside blocks 0 and 1; cap
    0: the device's own grid, at most a few units per wave.  One accumulator per output block and a fixed k order: same bits."""
    c = util.stem_case("64x64_cap")
    wprep = ops.stem_prepare_weights(_t(c.wa), _t(c.wp))
    outs = {}
    for cap in (0, 1, 3):
        with util.conv_grid_cap(cap):
            arrays, dense, compact = _run_stem(c, variant, "plain", wprep)
        _assert_plan(c, arrays)
        if cap:
            n_c = (arrays[2][4:] - arrays[2][:4]).tolist()                 # plan.class_rows(), as read from the device
            paths, per_wave, crossings = util.stem_gemm_split(n_c, cap)
            assert min(per_wave) >= 2 * 5 + 2                              # a wave's share holds a whole tile of the largest class
            assert {(km, "tile", km) for km in (2, 3, 5)} <= paths
            if cap == 1:
                assert crossings == [3]
                assert {(km, part, cnt) for km in (2, 3, 5) for part in ("head", "tail") for cnt in range(1, km)} <= paths
            else:
                assert crossings[0] >= 1 and crossings[1] >= 1
        assert _ratio("64x64_cap %s grid cap %d" % (variant, cap), dense, c.want[variant]["plain"]) <= util.STEM_TOL
        assert torch.equal(compact, dense)
        outs[cap] = dense
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[3], outs[0])


def test_stem_scratch_reuse_across_geometries():
    """The per-stream scratch (flags, row_of, row_cell, rows, the four Y tables) is grown to the largest request and reused:
    a small grid after a large one sees the large one's leftovers beyond (and inside) its own extent.  Every frame of the
    sequence must equal the same frame run alone on fresh scratch, bit for bit, and every plan the reference."""
    names = ["64x96_mixed", "6x10_half", "2x2_full", "64x96_mixed#again"]
    assert not np.array_equal(util.stem_case(names[0]).plan.row_of, util.stem_case(names[3]).plan.row_of)
    ops.release_stream_workspaces()
    chained = [_run_stem(util.stem_case(n), "signed", "plain") for n in names]
    assert _flags_all_zero()
    for n, (arrays, dense, compact) in zip(names, chained):
        c = util.stem_case(n)
        _assert_plan(c, arrays)
        ops.release_stream_workspaces()
        alone_arrays, alone_dense, alone_compact = _run_stem(c, "signed", "plain")
        for a, b in zip(arrays, alone_arrays):
            assert np.array_equal(a, b)
        assert torch.equal(dense, alone_dense) and torch.equal(compact, alone_compact) and torch.equal(compact, dense)
        assert _ratio("reuse %s" % n, dense, c.want["signed"]["plain"]) <= util.STEM_TOL


# ---------------------------------------------------------------------------------------------------------------------------
# compact-row point scatter
# ---------------------------------------------------------------------------------------------------------------------------
def _run_scatter(c, coord=None, n_live=None, cap=0, dense=False):
    """-> (rows [meta[11], T*64], point-row buffer [B, N, 192] whose columns 64:128 are pts_out, plan arrays).  dense=True: through
    ops.pointnet_scatter into a zero grid, read back in the plan's row order."""
    coord = _t(c.coord if coord is None else coord)
    xyzi = _t(c.xyzi)
    weights = [_t(a) for a in (c.w1, c.b1, c.w2, c.b2)]
    plan = ops.stem_plan(coord, c.h, c.w, row_floats=c.t * 64)
    arrays = _plan_arrays(plan)
    n_rows = len(arrays[1])
    pts = torch.full((c.b, c.n, 192), SENTINEL, device=DEV)
    with util.conv_grid_cap(cap):
        if dense:
            bev = torch.zeros((c.b, c.h, c.w, c.t * 64), device=DEV)
            ops.pointnet_scatter(xyzi, coord, *weights, bev, pts_out=pts[:, :, 64:128])
            cells = bev.view(-1, c.t * 64)
            occupied = plan.row_of.long() >= 0
            assert not bool(cells[~occupied].any())                       # nothing outside the marked cells
            rows = cells[plan.row_cell[:n_rows].long()]
            assert torch.equal(cells[occupied], rows[plan.row_of.long()[occupied]])
        else:
            cnt = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=DEV)
            rows = ops.pointnet_scatter_rows(xyzi, coord, *weights, plan, pts_out=pts[:, :, 64:128], n_live=cnt)[:n_rows].clone()
    return rows, pts, arrays


def _assert_scatter(label, c, rows, pts, want_rows=None, want_pts=None):
    want_rows = torch.tensor(c.rows if want_rows is None else want_rows, device=DEV)
    want_pts = torch.tensor((c.pts if want_pts is None else want_pts)[:, 0], device=DEV)      # frame 0: [B, N, 64]
    assert tuple(rows.shape) == tuple(want_rows.shape)
    r_rows = (rows.double() - want_rows).abs().max().item() / want_rows.max().item() if want_rows.numel() else 0.0
    r_pts = (pts[:, :, 64:128].double() - want_pts).abs().max().item() / want_pts.max().item()
    print("stem-ratio %-58s %.3e" % (label + " rows", r_rows))
    print("stem-ratio %-58s %.3e" % (label + " point rows", r_pts))
    assert r_rows <= util.PNS_TOL and r_pts <= util.PNS_TOL
    assert bool((pts[:, :, :64] == SENTINEL).all()) and bool((pts[:, :, 128:] == SENTINEL).all())


@pytest.mark.parametrize("name", sorted(util.PNS_CASES))
def test_point_scatter_rows_against_float64_reference(name):
    c = util.pns_case(name)
    rows, pts, arrays = _run_scatter(c)
    _assert_plan(c, arrays)
    assert _flags_all_zero()
    _assert_scatter(name, c, rows, pts)
    dense_rows, dense_pts, _ = _run_scatter(c, dense=True)
    assert torch.equal(rows, dense_rows) and torch.equal(pts, dense_pts)


@pytest.mark.parametrize("cap,trips", [(1, 48), (2, 24)])
def test_point_scatter_persistent_loop(cap, trips):
    """N = 1013 -> 32 tiles per scan, 192 in all.  Under grid cap 1 four waves make 48 trips each (cap 2: eight waves, 24): the
    fetch(nt + 2 step) / cell_request(nt + step) rotation runs, and the 32-point blocks of the case are live (L), wholly outside
    (O: skipped) or wholly outside in frame 0 (P: no atomics, point rows still written) in every order two consecutive tiles of
    a wave can have.  A max of non-negative floats: the same bits as the uncapped launch."""
    c = util.pns_case("n1013")
    walks = util.pns_wave_walks(util.pns_tile_kinds(c.coord, c.h, c.w), cap)
    assert len(walks) == 4 * cap and all(len(wk) == trips for wk in walks)
    pairs = {wk[i:i + 2] for wk in walks for i in range(len(wk) - 1)}
    assert pairs == {a + z for a in "LOP" for z in "LOP"} - {"PP"}           # frame 0 never follows frame 0 on a wave
    assert any("LOL" in wk for wk in walks) and any("LOOL" in wk for wk in walks)
    rows, pts, arrays = _run_scatter(c, cap=cap)
    _assert_plan(c, arrays)
    _assert_scatter("n1013 grid cap %d" % cap, c, rows, pts)
    free_rows, free_pts, _ = _run_scatter(c)
    assert torch.equal(rows, free_rows) and torch.equal(pts, free_pts)
    dense_rows, dense_pts, _ = _run_scatter(c, cap=cap, dense=True)
    assert torch.equal(rows, dense_rows) and torch.equal(pts, dense_pts)


@pytest.mark.parametrize("cap", [0, 1])
@pytest.mark.parametrize("n_live", [0, 1, 31, 32, 33, 1012, 1013, 1020])
def test_point_scatter_rows_n_live(n_live, cap):
    """smos_pointnet_scatter_rows: a DEVICE count of the real points at the front of the current (t == 0) scans; the tail
    [k, N) of those scans sits at -4864.0 (outside every grid: the runner's contract).  The row table does not depend on the
    count; the point rows of the real points are the same bits; and a 32-point tile that starts at or after k -- whose points
    are all outside -- is skipped even in frame 0, so its point rows are not written (point_fused.hip: a tile is skipped unless
    `pts_out && t == 0 && n0 < n_live`, or a point of it falls into the grid)."""
    c = util.pns_case("n1013")
    k = min(n_live, c.n)
    coord = c.coord.copy()
    coord[:, 0, k:, :2] = -4864.0
    plan_ref = util.stem_plan_ref(coord, c.b, c.h, c.w)
    want_rows = util.pointnet_rows_ref(c.xyzi, coord, c.w1, c.b1, c.w2, c.b2, plan_ref)
    full_rows, full_pts, arrays = _run_scatter(c, coord=coord, cap=cap)
    assert np.array_equal(arrays[0], plan_ref.row_of) and np.array_equal(arrays[1], plan_ref.row_cell)
    _assert_scatter("n1013 tail from %d grid cap %d" % (k, cap), c, full_rows, full_pts, want_rows=want_rows)
    rows, pts, _ = _run_scatter(c, coord=coord, n_live=n_live, cap=cap)
    assert torch.equal(rows, full_rows)
    assert torch.equal(pts[:, :k], full_pts[:, :k])
    first_skipped = (k + util.PNS_TILE - 1) // util.PNS_TILE * util.PNS_TILE
    assert bool((pts[:, first_skipped:] == SENTINEL).all())
    assert bool((pts[:, :, :64] == SENTINEL).all()) and bool((pts[:, :, 128:] == SENTINEL).all())
    if cap:                                                                   # the capped launch really loops: 48 trips per wave
        assert all(len(wk) == 48 for wk in util.pns_wave_walks(util.pns_tile_kinds(coord, c.h, c.w), cap))


# ---------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_op_and_launch_nothing():
    c = util.stem_case("6x10_half")
    coord = _t(c.coord)
    ops.release_stream_workspaces()
    for h, w in ((5, 10), (6, 9)):
        with pytest.raises(RuntimeError, match="stem_mark"):
            ops.stem_plan(coord, h, w)
    with pytest.raises(RuntimeError, match="stem_plan"):
        ops.stem_plan(coord[:, :, :, ::2], c.h, c.w)                          # not contiguous
    with pytest.raises(RuntimeError, match="stem_plan"):
        ops.stem_plan(coord.double(), c.h, c.w)
    assert _flags_all_zero()                                                  # stem_mark did not run

    p = util.pns_case("n33")
    xyzi, pcoord = _t(p.xyzi), _t(p.coord)
    weights = [_t(a) for a in (p.w1, p.b1, p.w2, p.b2)]
    pts = torch.full((p.b, p.n, 64), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="pointnet_scatter_rows"):
        ops.pointnet_scatter_rows(xyzi, pcoord, *weights, ops.stem_plan(pcoord, p.h, p.w), pts_out=pts)
    with pytest.raises(RuntimeError, match="pointnet_scatter_rows"):
        ops.pointnet_scatter_rows(xyzi, pcoord, *weights, ops.stem_plan(pcoord, p.h, p.w, row_floats=64), pts_out=pts)
    plan = ops.stem_plan(pcoord, p.h, p.w, row_floats=p.t * 64)
    for bad in (torch.tensor([5], device=DEV), torch.tensor([5.0], device=DEV)):
        with pytest.raises(RuntimeError, match="pointnet_scatter_rows"):
            ops.pointnet_scatter_rows(xyzi, pcoord, *weights, plan, pts_out=pts, n_live=bad)
    assert bool((pts == SENTINEL).all()) and not bool(plan.rows[:int(plan.meta[11])].any())

    plan = ops.stem_plan(coord, c.h, c.w)
    wprep = ops.stem_prepare_weights(_t(c.wa), _t(c.wp))
    out = ops.empty_cl(c.b, 32, c.h // 2, c.w // 2, DEV)
    out.fill_(SENTINEL)
    with pytest.raises(RuntimeError, match="stem_gemm"):                      # Cin = 64
        ops.sparse_downsample(torch.zeros((c.b, c.h, c.w, 64), device=DEV), plan, wprep, torch.zeros(32, device=DEV), compact=False, out=out)
    out16 = ops.empty_cl(c.b, 16, c.h // 2, c.w // 2, DEV)
    out16.fill_(SENTINEL)
    with pytest.raises(RuntimeError, match="stem_gemm"):                      # Cout = 16
        ops.sparse_downsample(_t(c.x["signed"]), plan, wprep, torch.zeros(16, device=DEV), compact=False, out=out16)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out16 == SENTINEL).all())

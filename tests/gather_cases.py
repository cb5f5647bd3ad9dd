"""Grid -> point bilinear gather and the max scatter behind it (csrc/cl_kernels.hip: gather_scatter_cl / gather_scatter_cl4;
csrc/bilinear_gather.hip: bil_points / bil_rows): the float64 reference, the per-element bound and the case builders shared by
tests/test_host_gather_reference.py (no GPU) and tests/test_gpu_gather_scatter.py.  numpy only.

Reference.  The sampling positions are the float32 numbers the kernels use (oracle.ops_np.bilinear_pixel_coords: the normalise /
un-normalise chain of BilinearSample + grid_sample, operation by operation); from there on everything is float64.  Per point and
channel, over the taps of the point that lie inside the map (whatever their weight),

    S = sum_k w_k g_k,        A = sum_k |w_k g_k|;

a position that is not finite, or that has no tap inside the map, gives S = A = 0.  The target cell of a point is
oracle.ops_np.voxel_cell_index: the float32 product coordinate * scale truncated toward zero, kept iff -1 < p < size on both
axes (a coordinate in (-1, 0) lands in cell 0).

Bound for a gathered value: |got - S| <= 12 * 2^-24 * A, and exactly 0 where A = 0.  A float32 weight is the product of two
float32 differences: three roundings; the product with g: one more (none if the compiler contracts it into the addition); at
most three additions while the four terms are summed: seven roundings touch a term, and 12 = m + 8 at m = 4 taps is the
convention of tests/bilinear_bwd_cases.py::bound, whose margin covers the second-order terms.  Nothing in it is fitted to a
kernel: a float32 numpy emulation of the kernels' expression (emulate_f32: their tap order, un-contracted and with the product
fused) stays inside it on every case (tests/test_host_gather_reference.py prints the worst ratio).

Scatter target.  gather_scatter_cl keeps max(0, .) per cell: the target is zero-filled and the running maximum starts at 0.
It is checked (a) bit for bit against scatter_max0 of the device's own point rows, and (b) against the float64 reference:
|got - max(0, max_p S_p)| <= max_p bound_p over the members p of the cell -- a maximum is 1-Lipschitz in every argument, so
the per-point bound carries over.

Cases.  Source map 5 x 7, target map 4 x 6, two samples, N in NS, both scales; grids are signed randn.  The gather coordinates
of every case are uniform positions up to one cell beyond every border with the special positions of SPECIAL_POS / SPECIAL_COORD
dealt over them (integer positions, the last row and column, -0.5 and size - 0.5, two cells outside, the padding rows at -1000
and -4864, NaN in one or both coordinates, +-inf).  The scatter coordinates follow one of STRUCTURES: what the run loop of the
kernels branches on, laid against the 64-point runs of gather_scatter_cl4 / gather_scatter_cl<64> and against the 32-point runs
of gather_scatter_cl<32> = the half runs of gather_scatter_cl4<32, true>'s second sweep.
"""
import functools
import hashlib
import types

import numpy as np

from oracle import ops_np

U = 2.0 ** -24
FACTOR = 12.0
HG, WG = 5, 7                # source map
HO, WO = 4, 6                # scatter target
B = 2
KG, KS = 3, 2                # coordinate columns (the gather's third is not a coordinate)
SCALES = {"dyadic": (0.5, 0.5), "nondyadic": (0.5, 0.25)}
NS = (1, 31, 32, 33, 63, 64, 65, 130)
GS_CHANNELS = (32, 64)
# bil_points chunks the channels over blockIdx.y for C >= 16 (17 -> 9 + 8, 71 -> 7 x 9 + 8); bil_rows takes a group of 8 (C = 8),
# 16 (C = 12), 32 (C = 17, 20, 32) or 64 lanes (C = 64; C = 71: a second trip of 7)
BIL_CHANNELS = (3, 8, 12, 17, 20, 32, 64, 71)
LONE0 = ((0, 15, 30, 32, 62), (1, 31, 33, 63))        # positions of the lone cell-0 points in a 64-point run, per sample
PAD_COORDS = (-1000.0, -4864.0)

STRUCTURES = (
    "onecell_neg",      # every point in cell 0, from coordinates in (-1, 0)
    "onecell_pos",      # every point in cell 0, from coordinates in [0, 1)
    "alternate",        # A, B, A, B, ...: a flush at every step (sample 1: B = cell 0)
    "straddle",         # cells change at 16 mod 32 only: one cell across every 31|32 and 63|64 border, and across the sample boundary
    "holes",            # one cell with points without a target cell inside: A, -1, A; at position 0 of a run; at the last valid position
    "lone0",            # lone cell-0 points at LONE0 between other cells
    "tailchange",       # one cell, the last valid point in another (sample 1: in cell 0)
    "runs",             # runs of 3..9 points per cell: the largest member in the middle of a run
    "ties",             # runs with duplicated coordinates: exact ties inside a run and across runs
    "cell_notap",       # every third point has a cell but no tap: its value is 0
    "notap_runs",       # whole 64-point runs (sample 0) and 32-point runs (sample 1) without a tap, with cells
    "nocell_runs",      # whole 64-point runs (sample 0) and 32-point runs (sample 1) with taps, without a cell
    "negative_grid",    # "runs" on a grid that is negative everywhere: the rows are negative, the target stays 0
)

NO_CELL = ((-1.0, 2.5), (2.5, -1.0), (float(HO), 2.5), (2.5, float(WO)), (-100.0, -100.0), (np.nan, 1.0), (1.5, np.inf), (-2000.0, 1.0))


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


# ---------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------
def taps(coord, scale, h, w):
    """coord [B, N, >= 2] -> (y [4, B, N] int64, x [4, B, N] int64, wgt [4, B, N] float64, inside [4, B, N] bool) in the tap
    order of the kernels (k = 2 dy + dx); the weights are float64 expressions of the float32 positions."""
    iy, ix = ops_np.bilinear_pixel_coords(np.asarray(coord)[..., :2], scale, h, w)
    iy, ix = iy.astype(np.float64), ix.astype(np.float64)
    fin = np.isfinite(iy) & np.isfinite(ix) & (np.abs(iy) < 2.0 ** 30) & (np.abs(ix) < 2.0 ** 30)
    iy, ix = np.where(fin, iy, -10.0), np.where(fin, ix, -10.0)
    y0, x0 = np.floor(iy), np.floor(ix)
    wy = ((y0 + 1.0) - iy, iy - y0)
    wx = ((x0 + 1.0) - ix, ix - x0)
    ys, xs, ws, ins = [], [], [], []
    for k in range(4):
        yy, xx = y0 + (k >> 1), x0 + (k & 1)
        ok = fin & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
        ys.append(np.where(ok, yy, 0).astype(np.int64))
        xs.append(np.where(ok, xx, 0).astype(np.int64))
        ws.append(np.where(ok, wy[k >> 1] * wx[k & 1], 0.0))
        ins.append(ok)
    return np.stack(ys), np.stack(xs), np.stack(ws), np.stack(ins)


def gather_ref(grid, coord, scale):
    """grid [B, H, W, C] (channels-last), coord [B, N, >= 2] -> S, A [B, N, C] float64."""
    grid = np.asarray(grid, dtype=np.float64)
    b, h, w, c = grid.shape
    ys, xs, ws, ins = taps(coord, scale, h, w)
    bi = np.arange(b)[:, None]
    s = np.zeros((b, coord.shape[1], c))
    a = np.zeros_like(s)
    for k in range(4):
        term = ws[k][..., None] * grid[bi, ys[k], xs[k]] * ins[k][..., None]
        s += term
        a += np.abs(term)
    return s, a


def emulate_f32(grid, coord, scale, fused):
    """The kernels' expression in float32 numpy: the differences, the four weight products and the sum over the taps that
    exist in tap order, each operation rounded to float32; `fused`: the product and the addition rounded once (one float64
    multiply-add rounded to float32 models the fma: the float64 product of two float32 numbers is exact)."""
    f = np.float32
    grid = np.asarray(grid).astype(f)
    b, h, w, c = grid.shape
    iy, ix = ops_np.bilinear_pixel_coords(np.asarray(coord)[..., :2], scale, h, w)
    with np.errstate(invalid="ignore"):
        fy, fx = np.floor(iy), np.floor(ix)
        wx1, wx0 = (ix - fx).astype(f), ((fx + f(1)) - ix).astype(f)
        wy1, wy0 = (iy - fy).astype(f), ((fy + f(1)) - iy).astype(f)
        w4 = [(wx0 * wy0).astype(f), (wx1 * wy0).astype(f), (wx0 * wy1).astype(f), (wx1 * wy1).astype(f)]
        fin = (iy > -2) & (iy < h + 1) & (ix > -2) & (ix < w + 1)
    y0 = np.where(fin, fy, -5).astype(np.int64)
    x0 = np.where(fin, fx, -5).astype(np.int64)
    bi = np.arange(b)[:, None]
    v = np.zeros((b, coord.shape[1], c), dtype=f)
    for k in range(4):
        yy, xx = y0 + (k >> 1), x0 + (k & 1)
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        g = grid[bi, np.where(ok, yy, 0), np.where(ok, xx, 0)]
        wk = np.where(ok, w4[k], f(0))[..., None].astype(f)
        if fused:
            nxt = (g.astype(np.float64) * wk.astype(np.float64) + v.astype(np.float64)).astype(f)
        else:
            nxt = (v + (g * wk).astype(f)).astype(f)
        v = np.where(ok[..., None], nxt, v)
    assert v.dtype == f
    return v


def cell_index(scoord, scale, ho=HO, wo=WO):
    """[B, N] flat target cell per point, -1: none."""
    return ops_np.voxel_cell_index(np.asarray(scoord)[..., :2], (ho, wo), np.asarray(scale, dtype=np.float32))


def scatter_max0(rows, cell, ncell=HO * WO):
    """rows [B, N, C] (any float dtype, kept), cell [B, N] -> [B, ncell, C]: max(0, members) per cell, 0 for an empty cell."""
    rows = np.asarray(rows)
    b, n, c = rows.shape
    out = np.zeros((b, ncell, c), dtype=rows.dtype)
    for s in range(b):
        keep = cell[s] >= 0
        np.maximum.at(out[s], cell[s][keep], rows[s][keep])
    return out


def bound(a):
    return FACTOR * U * np.asarray(a)


def worst_ratio(got, want, lim):
    """-> (every element inside its bound, worst error / bound).  Where the bound is 0 the error has to be 0; a NaN is outside
    every bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    ok = bool((err <= lim).all())
    pos = lim > 0
    return ok, (float((err[pos] / lim[pos]).max()) if pos.any() else 0.0)


# ---------------------------------------------------------------------------------------------
# coordinates
# ---------------------------------------------------------------------------------------------
def special_pos(h, w):
    """Pixel positions (y, x): integer positions, the last row / column, half a cell outside (one row / column of taps
    absent), on the validity border and two cells outside (no tap)."""
    return [(0.0, 0.0), (1.0, 2.0), (2.0, 3.0), (h - 1.0, 1.65), (0.85, w - 1.0), (h - 1.0, w - 1.0),
            (-0.5, 1.5), (1.5, -0.5), (h - 0.5, 2.5), (2.5, w - 0.5), (-0.5, w - 0.5),
            (-1.0, 2.5), (2.5, float(w)), (-1.25, 1.5), (1.5, w + 0.25), (-2.0, 2.5), (2.5, w + 1.0), (h + 1.0, -2.0)]


SPECIAL_COORD = [(-1000.0, -1000.0), (-4864.0, -4864.0), (np.nan, 3.0), (3.0, np.nan), (np.nan, np.nan), (np.inf, 3.0),
                 (3.0, -np.inf), (-np.inf, np.inf)]


def gather_coords(rng, b, n, scale, h=HG, w=WG, special=True):
    """[B, N, KG] float32-valued coordinates: position / scale (both scales are powers of two: the product is the position
    again), uniform up to 1.5 cells beyond the first and half a cell beyond the last row / column, the specials at (7 j) mod n."""
    pos = np.stack((rng.uniform(-1.5, h + 0.5, (b, n)), rng.uniform(-1.5, w + 0.5, (b, n))), -1)
    coord = np.empty((b, n, KG))
    coord[..., :2] = pos / np.asarray(scale)
    coord[..., 2] = rng.random((b, n))
    if special:
        both = [tuple(np.asarray(p) / np.asarray(scale)) for p in special_pos(h, w)] + SPECIAL_COORD
        for j, p in enumerate(both):
            coord[j % b, (7 * j) % n, :2] = p
    return coord


def interior_coords(rng, shape, scale, h=HG, w=WG):
    """Coordinates strictly inside the source map: all four taps."""
    pos = np.stack((rng.uniform(0.05, h - 1.05, shape), rng.uniform(0.05, w - 1.05, shape)), -1)
    return pos / np.asarray(scale)


def _cell_runs(rng, n, lo, hi, cells=None):
    """[n] cells in runs of lo..hi points, consecutive runs in different cells, never cell 0."""
    out = np.empty(n, dtype=np.int64)
    i, prev = 0, -1
    while i < n:
        c = int(rng.integers(1, HO * WO)) if cells is None else cells[int(rng.integers(0, len(cells)))]
        if c == prev:
            continue
        ln = int(rng.integers(lo, hi + 1))
        out[i:i + ln] = c
        i, prev = i + ln, c
    return out


def scatter_coords(rng, cell, neg0, scale):
    """cell [B, N] (-1: a point without a target cell), neg0 [B, N] (a cell-0 point from coordinates in (-1, 0)) -> [B, N, KS]."""
    b, n = cell.shape
    u = rng.uniform(0.05, 0.95, (b, n, 2))
    pos = np.stack((cell // WO, cell % WO), -1) + u
    idx = np.arange(n)[None, :, None]
    flip = np.stack((np.ones((b, n), dtype=bool), np.broadcast_to(idx[..., 0] % 2 == 0, (b, n))), -1)     # y < 0 always, x < 0 on even points
    pos = np.where(neg0[..., None] & flip, -u, pos)
    none = np.asarray(NO_CELL)[(np.arange(b)[:, None] * 3 + np.arange(n)[None, :]) % len(NO_CELL)]
    pos = np.where((cell < 0)[..., None], none, pos)
    return pos / np.asarray(scale)


def structure(name, rng, n):
    """-> cell [B, N], neg0 [B, N], notap [B, N] (gather coordinate at a padding value), interior [B, N] (all four taps),
    dups: (sample, dst, src) points that copy both coordinate rows."""
    cell = np.zeros((B, n), dtype=np.int64)
    neg0 = np.zeros((B, n), dtype=bool)
    notap = np.zeros((B, n), dtype=bool)
    interior = np.zeros((B, n), dtype=bool)
    dups = []
    i = np.arange(n)
    a, b_ = (int(v) for v in rng.permutation(np.arange(1, HO * WO))[:2])
    if name == "onecell_neg":
        neg0[:] = True
    elif name == "onecell_pos":
        pass
    elif name == "alternate":
        cell[0] = np.where(i % 2 == 0, a, b_)
        cell[1] = np.where(i % 2 == 0, a, 0)
        neg0[1] = (i % 4 == 1)
    elif name == "straddle":
        order = rng.permutation(np.arange(HO * WO))
        k = (i + 16) // 32
        cell[0] = order[k]
        cell[1] = order[k.max() - k]                       # starts in the cell sample 0 ends in
    elif name == "holes":
        cell[:] = a
        cell[0, i % 32 == 0] = -1
        cell[0, n - 1] = -1
        cell[1, np.isin(i, (1, 33, 47))] = -1
    elif name == "lone0":
        for s in range(B):
            cell[s] = _cell_runs(rng, n, 2, 5)
            at = np.isin(i % 64, LONE0[s])
            cell[s, at] = 0
            neg0[s, at] = (np.cumsum(at)[at] % 2 == 1)     # every other lone point from (-1, 0)
    elif name == "tailchange":
        cell[:] = a
        cell[0, n - 1] = b_
        cell[1, n - 1] = 0
    elif name in ("runs", "ties", "negative_grid", "cell_notap"):
        for s in range(B):
            cell[s] = _cell_runs(rng, n, 3, 9)
        interior[:] = name in ("runs", "negative_grid")    # every member has a value
        if name == "ties":
            # in ascending order of the copy, so that a source is final when it is copied
            dups = [(s, d, d - 3 if d % 11 == 7 else d - 1) for s in range(B) for d in range(n) if d % 5 == 2 or d % 11 == 7]
        if name == "cell_notap":
            notap[:] = i % 3 == 1
    elif name in ("notap_runs", "nocell_runs"):
        for s in range(B):
            cell[s] = _cell_runs(rng, n, 3, 9)
        mask = np.stack(((i // 64) % 2 == 0, (i // 32) % 2 == 1))
        if name == "notap_runs":
            notap[:] = mask
        else:
            cell[mask] = -1
            interior[:] = True
    else:
        raise KeyError(name)
    return cell, neg0, notap, interior, dups


def make_case(name, c, n, scale, cell, neg0, notap, interior, dups, b=B, negative=False, special=True):
    rng = np.random.default_rng(_seed("gather/" + name))
    case = types.SimpleNamespace(name=name, b=b, c=c, n=n, scale=tuple(scale), hg=HG, wg=WG, ho=HO, wo=WO)
    gcoord = gather_coords(rng, b, n, scale, special=special)
    gcoord[..., :2] = np.where(interior[..., None], interior_coords(rng, (b, n), scale), gcoord[..., :2])
    pad = np.asarray(PAD_COORDS)[(np.arange(n)[None, :] + np.arange(b)[:, None]) % 2]
    gcoord[..., :2] = np.where(notap[..., None], pad[..., None], gcoord[..., :2])
    scoord = scatter_coords(rng, cell, neg0, scale)
    cell, neg0 = cell.copy(), neg0.copy()
    for s, d, src in dups:
        gcoord[s, d], scoord[s, d], cell[s, d], neg0[s, d] = gcoord[s, src], scoord[s, src], cell[s, src], neg0[s, src]
    grid = rng.standard_normal((b, HG, WG, c))
    if negative:
        grid = -np.abs(grid) - 0.01
    case.grid, case.gcoord, case.scoord = _f32(grid), _f32(gcoord), _f32(scoord)
    case.want_cell, case.neg0, case.dups = cell, neg0, tuple(dups)
    case.cell = cell_index(case.scoord, scale)
    assert np.array_equal(case.cell, cell), name             # the coordinates say what the structure asked for
    case.S, case.A = gather_ref(case.grid, case.gcoord, scale)
    case.lim = bound(case.A)
    case.T = scatter_max0(case.S, case.cell)                 # [B, HO * WO, C]
    case.T_lim = scatter_max0(case.lim, case.cell)           # bounds are >= 0: max_p bound_p, 0 for an empty cell
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def gs_case(struct, c, n, scale_name):
    rng = np.random.default_rng(_seed("gather-structure/%s/%d/%s" % (struct, n, scale_name)))
    parts = structure(struct, rng, n)
    return make_case("%s/c%d/n%d/%s" % (struct, c, n, scale_name), c, n, SCALES[scale_name], *parts,
                     negative=struct == "negative_grid")


@functools.lru_cache(maxsize=None)
def bil_case(c, n, scale_name):
    """ops.bilinear_gather: the gather coordinates alone (the scatter side is one cell per point and not used)."""
    z = np.zeros((B, n), dtype=bool)
    return make_case("bilinear/c%d/n%d/%s" % (c, n, scale_name), c, n, SCALES[scale_name], np.zeros((B, n), dtype=np.int64), z, z, z, [])


def has_tap(case):
    return taps(case.gcoord, case.scale, HG, WG)[3].any(0)


# ---------------------------------------------------------------------------------------------
# the run loop under the grid cap (tests/util.py::conv_grid_cap)
# ---------------------------------------------------------------------------------------------
LOOP_B, LOOP_N = 3, 394      # 7 runs of 64 and 13 runs of 32 per sample, the last one of 10 points
PAIRS = {x + y for x in "GZS" for y in "GZS"}


def run_kinds(tap, cell, run):
    """Per run of `run` points, [B * runs per sample] in the kernels' run order: "Z" no tap inside the source map (the early
    `continue`: the rows are zeros), "S" taps but no target cell (a scatter-only launch skips it; a launch with rows sweeps
    the tile without an atomic), "G" taps and cells."""
    b, n = tap.shape
    per = -(-n // run)
    pad_t = np.zeros((b, per * run), dtype=bool)
    pad_c = np.zeros((b, per * run), dtype=bool)
    pad_t[:, :n], pad_c[:, :n] = tap, cell >= 0
    t = pad_t.reshape(b * per, run).any(1)
    cc = pad_c.reshape(b * per, run).any(1)
    return np.where(~t, "Z", np.where(cc, "G", "S"))


def walks(kinds, walkers):
    """The run sequence of every walker (a wave of gather_scatter_cl4 / a lane group of gather_scatter_cl: walker v of `walkers`
    takes runs v, v + walkers, ...) as strings of run kinds -- util.pns_wave_walks on one row of runs."""
    return ["".join(kinds[first::walkers]) for first in range(min(walkers, len(kinds)))]


def walk_pairs(ws):
    return {w[i:i + 2] for w in ws for i in range(len(w) - 1)}


def _loop_kinds32():
    """Kinds per 32-point run (halves of a 64-point run mostly alike) such that a one-block launch meets all nine ordered
    pairs on the walks over 64-point runs (4 walkers) and over 32-point runs (8 walkers): the first seed that does."""
    per64, per32 = -(-LOOP_N // 64), -(-LOOP_N // 32)
    for seed in range(10000):
        rng = np.random.default_rng(seed)
        k64 = rng.choice(list("GZS"), (LOOP_B, per64))
        k32 = np.repeat(k64, 2, axis=1)[:, :per32].copy()
        flip = rng.random(k32.shape) < 0.25
        k32[flip] = rng.choice(list("GZS"), int(flip.sum()))
        halves = np.full((LOOP_B, per64 * 2), "Z")
        halves[:, :per32] = k32
        halves = halves.reshape(LOOP_B, per64, 2)
        # a 64-point run is Z when both halves are, G when a half is (a Z half of loop_case has no cell either), else S
        got64 = np.where((halves == "Z").all(2), "Z", np.where((halves == "G").any(2), "G", "S"))
        if walk_pairs(walks(got64.reshape(-1), 4)) == PAIRS and walk_pairs(walks(k32.reshape(-1), 8)) == PAIRS:
            return k32
    raise AssertionError("no kind assignment found")


@functools.lru_cache(maxsize=None)
def loop_case(c):
    """B = 3, N = 394: 21 runs of 64 points (under a cap of one block wave 0 makes six trips, the others five) and 39 runs of
    32 points (the two lane groups of the last wave of gather_scatter_cl<32> make five and four), the run sequence crosses both
    sample boundaries and the last run of every sample is ragged.  Every 32-point run is G, Z or S (a Z run has no cell
    either, so that the halves decide the kind of the 64-point run)."""
    k32 = _loop_kinds32()
    n = LOOP_N
    rng = np.random.default_rng(_seed("gather-loop"))
    per_point = np.repeat(k32, 32, axis=1)[:, :n]
    cell = np.stack([_cell_runs(rng, n, 1, 9) for _ in range(LOOP_B)])
    zero = rng.random((LOOP_B, n)) < 0.05
    cell[zero] = 0
    cell[per_point != "G"] = -1
    notap = per_point == "Z"
    interior = (per_point != "Z") & (rng.random((LOOP_B, n)) < 0.7)          # the rest: the uniform mix, some without a tap
    first = np.arange(n) % 32 == 0
    interior |= (per_point != "Z") & first[None]                             # at least one tap in every G / S run
    return make_case("loop/c%d" % c, c, n, SCALES["nondyadic"], cell, (cell == 0) & (np.arange(n) % 2 == 0), notap, interior, [], b=LOOP_B,
                     special=False)

"""The fused training transfer grid -> point -> grid (csrc/gather_scatter_train.hip, ops.gather_scatter_train): shapes, case
generators, the float64 reference and the per-element bound shared by tests/test_host_cross_view_train.py (no GPU) and
tests/test_gpu_cross_view_train.py.

A transfer is BilinearSample followed by VoxelMaxPool.  Its backward has two parts:

  x[b,c,n] = grad_out[b,c,cell(n)] if point n is kept and its gathered value equals out[b,c,cell(n)], else 0
             (+ grad_pts[b,c,n] where the point values were handed on),
  grad_grid = the bilinear gather's backward of x.

The first part is a selection: given the winner mask it is exact (and one float32 addition with grad_pts).  The second is the
sum tests/bilinear_bwd_cases.py bounds.  So the reference takes the winner mask as given -- from the numpy chain on the host,
from the device's own forward results on the GPU -- forms x in float64 and takes S, A, m from
bilinear_bwd_cases.backward_ref(x).  Bound per grid element:

    |got - S| <= (m + 8) * 2^-24 * A            without grad_pts (bilinear_bwd_cases: three roundings in a weight, one in
                                                the product, m - 1 additions in any order, the rest for second-order terms)
    |got - S| <= (m + 9) * 2^-24 * A            with grad_pts: x = fl(g + p) carries one more relative rounding 2^-24, which
                                                every term w * x of the element inherits, so A * 2^-24 more in the sum

and exactly 0 where m = 0.  Neither depends on the order of the additions, so they hold for the float atomics.
"""
import functools
import hashlib
import types

import numpy as np

from oracle import ops_np
from tests import bilinear_bwd_cases as bcases

U = bcases.U

# name -> B, C, Hg, Wg, N, Ho, Wo
SHAPES = {
    "c3": (2, 3, 5, 7, 37, 4, 6),                # C < 8: the points form
    "c8": (2, 8, 4, 16, 129, 3, 8),              # four tiles + 1 point
    "c32": (1, 32, 8, 8, 257, 4, 16),
    "c64": (2, 64, 6, 10, 300, 5, 5),
    "c71_ragged": (1, 71, 5, 5, 65, 2, 9),       # a second channel chunk of 7
    "empty": (1, 32, 8, 8, 0, 4, 16),            # N = 0
}
# name -> (gather coordinates: a kind of bilinear_bwd_cases.positions, scatter coordinates: a kind of scatter_positions),
# drawn independently of each other
KINDS = {"uniform": ("uniform", "uniform"), "onecell": ("onecell", "onecell"), "runs": ("runs", "mix"), "mix": ("mix", "mix"),
         "dropped": ("uniform", "dropped")}
# what a steered case of each kind has to contain (self_check)
EXPECT = {"uniform": ("multi", "zero", "dropped", "loser"), "onecell": ("multi", "zero", "loser"),
          "runs": ("multi", "zero", "dropped", "loser"), "mix": ("multi", "zero", "dropped", "loser"), "dropped": ("dropped",)}
GSCALE = bcases.SCALE
SSCALE = (0.25, 0.5)
KG, KS = bcases.K, 2         # coordinate columns: the gather's third is not a coordinate; VoxelMaxPool wants exactly D = 2


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def scatter_positions(rng, kind, b, ho, wo, n):
    """[B, N, 2] positions (y, x) in units of target cells; cell = trunc toward zero, kept iff 0 <= cell < size."""
    if kind == "onecell":
        return np.array([ho // 2, wo // 2]) + rng.uniform(0.05, 0.95, (b, n, 2))
    if kind == "dropped":                                       # beyond a border on at least one axis, or not a number
        pos = np.stack((rng.uniform(-3.0, ho + 3.0, (b, n)), rng.uniform(wo + 0.5, wo + 3.0, (b, n))), -1)
        pick = rng.random((b, n))
        pos[pick < 0.3] = np.stack((rng.uniform(-3.0, -1.0, (b, n)), rng.uniform(-3.0, wo + 3.0, (b, n))), -1)[pick < 0.3]
        pos[(pick >= 0.3) & (pick < 0.4), 0] = np.nan
        pos[(pick >= 0.4) & (pick < 0.5)] = -1000.0 * np.array(SSCALE)
        return pos
    pos = np.stack((rng.uniform(-1.5, ho + 0.5, (b, n)), rng.uniform(-1.5, wo + 0.5, (b, n))), -1)    # one cell beyond every border
    special = [(-1.0, 1.5), (1.5, -1.0), (float(ho), 1.5), (1.5, float(wo)), (0.0, 0.0), (ho - 0.5, wo - 0.5), (-0.5, -0.5)]
    for j, p in enumerate(special[:n]):
        pos[j % b, (j * 5) % n] = p
    if kind == "mix":
        bad = rng.random((b, n))
        pos[bad < 0.08] = -1000.0 * np.array(SSCALE)
        pos[(bad >= 0.08) & (bad < 0.12), 0] = np.nan
        pos[(bad >= 0.12) & (bad < 0.16), 1] = np.nan
    return pos


def winners(pts, cell, out):
    """[B, C, N] bool: the point is kept and its value equals its cell's entry of out [B, C, Ho, Wo]."""
    b, c, n = pts.shape
    flat = out.reshape(b, c, -1)
    at = np.take_along_axis(flat, np.broadcast_to(np.maximum(cell, 0)[:, None, :], (b, c, n)), axis=2) if n else pts
    return (cell >= 0)[:, None, :] & (pts == at)


def at_cells(maps, cell):
    """[B, C, N]: maps [B, C, Ho, Wo] at every point's cell (cell 0 for a dropped point)."""
    b, c = maps.shape[:2]
    n = cell.shape[1]
    return np.take_along_axis(maps.reshape(b, c, -1), np.broadcast_to(np.maximum(cell, 0)[:, None, :], (b, c, n)), axis=2)


def point_grad(case, win, with_pts, dtype=np.float64):
    """x [B, C, N] for a winner mask: the selection, then one addition in `dtype` (float32: the bits the kernels produce)."""
    x = np.where(win, at_cells(case.grad_out, case.cell), 0.0).astype(dtype)
    return x + case.grad_pts.astype(dtype) if with_pts else x


def reference(case, win, with_pts):
    """S, A, m of the grid gradient for a winner mask."""
    s, a, m = bcases.backward_ref(point_grad(case, win, with_pts), case.gcoord, GSCALE, case.hg, case.wg)
    return types.SimpleNamespace(S=s, A=a, m=m, extra=1 if with_pts else 0)


def bound(ref):
    return (ref.m + 8 + ref.extra) * U * ref.A


def worst_ratio(got, ref):
    """-> (every element inside the bound, worst error / bound).  Where the bound is 0 the error has to be 0; a NaN is
    outside every bound."""
    got = np.asarray(got, dtype=np.float64)
    lim = bound(ref)
    err = np.abs(got - ref.S)
    pos = lim > 0
    return bool((err <= lim).all()), (float((err[pos] / lim[pos]).max()) if pos.any() else 0.0)


def self_check(case):
    """The coverage a steered case promises (EXPECT), counted on the host chain: {property: count}."""
    win = case.win_np
    per_cell = np.zeros((case.b, case.c, case.ho * case.wo), dtype=np.int64)
    for s in range(case.b):
        keep = case.cell[s] >= 0
        for ch in range(case.c):
            np.add.at(per_cell[s, ch], case.cell[s][keep], win[s, ch][keep])
    kept = (case.cell >= 0)[:, None, :]
    return {"multi": int((per_cell > 1).sum()), "zero": int((win & (case.pts_np == 0)).sum()),
            "dropped": int((case.cell < 0).sum()), "loser": int((kept & ~win).sum()), "kept": int((case.cell >= 0).sum()),
            "winner": int(win.sum())}


def make_case(name, shape, kind, signed=False):
    b, c, hg, wg, n, ho, wo = SHAPES[shape]
    gkind, skind = KINDS[kind]
    rng = np.random.default_rng(_seed("cross_view/" + name))
    gpos = bcases.positions(rng, gkind, b, hg, wg, n)
    spos = scatter_positions(rng, skind, b, ho, wo, n)
    dup = np.arange(9, n, 10)                                    # every tenth point repeats its neighbour: exact ties
    gpos[:, dup], spos[:, dup] = gpos[:, dup - 1], spos[:, dup - 1]
    gcoord = np.empty((b, n, KG))
    gcoord[..., :2] = gpos / np.asarray(GSCALE)
    gcoord[..., 2] = rng.random((b, n))
    grid = rng.standard_normal((b, c, hg, wg))
    if not signed:
        grid = np.maximum(grid, 0.0)                             # what the model scatters: post-ReLU maps
    grid[:, 1] = 0.0                                             # a channel of zeros: every kept point wins with the value 0
    grid[:, 1::2, :(hg + 1) // 2] = 0.0                          # a zero region: cells whose maximum is 0 next to positive ones
    case = types.SimpleNamespace(name=name, shape=shape, kind=kind, signed=signed, b=b, c=c, hg=hg, wg=wg, n=n, ho=ho, wo=wo)
    case.gcoord, case.scoord, case.grid = _f32(gcoord), _f32(spos / np.asarray(SSCALE)), _f32(grid)
    case.grad_out = _f32(rng.standard_normal((b, c, ho, wo)))
    case.grad_pts = _f32(rng.standard_normal((b, c, n)))
    # the host chain: float32 values of oracle.ops_np (not the kernels' bits: the GPU tests take their mask from the device)
    case.cell = ops_np.voxel_cell_index(case.scoord, (ho, wo), SSCALE)
    case.pts_np = ops_np.bilinear_sample(case.grid, case.gcoord[..., :2].astype(np.float32), GSCALE)
    case.out_np = ops_np.voxel_maxpool_fwd(case.pts_np, case.scoord, (ho, wo), SSCALE)[0]
    case.win_np = winners(case.pts_np, case.cell, case.out_np)
    for v in vars(case).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def case_of(shape, kind):
    return make_case("%s/%s" % (shape, kind), shape, kind)


@functools.lru_cache(maxsize=None)
def signed_case():
    """A grid of both signs: cells whose maximum is negative, the scatter's exact path."""
    return make_case("c8/mix/signed", "c8", "mix", signed=True)


ALL = [(s, k) for s in SHAPES for k in KINDS]

"""Backward of the grid -> point bilinear gather (csrc/bilinear_gather.hip, smos_bilinear_gather_bwd): the float64 reference,
the case generators and the per-element bound shared by tests/test_host_bilinear_backward.py (no GPU) and
tests/test_gpu_bilinear_backward.py.

Reference: the sampling positions are the float32 numbers the forward uses (oracle.ops_np.bilinear_pixel_coords: the
normalise / un-normalise chain of BilinearSample + grid_sample, operation by operation); from there on everything is
float64.  Per grid element it returns

    S = sum of w * g        over the (point, tap) pairs that reach the element,
    A = sum of |w * g|      over the same pairs,
    m = their number        (a tap inside the map counts, whatever its weight).

Bound: |got - S| <= (m + 8) * 2^-24 * A.  A float32 weight is a product of two differences: three roundings; the product
with g: one; m - 1 additions in any order, each touching a term at most once; the rest of the margin covers second-order
terms.  The bound does not depend on the order of the additions, so it also holds for float atomics.  Where m = 0 it is 0:
the element has to be exactly 0.
"""
import functools
import hashlib
import types

import numpy as np

from oracle import ops_np

U = 2.0 ** -24
TILE = 32            # points per wave tile of bil_bwd_rows (kBt)
BLOCK_TILES = 4      # waves = tiles per block

# name -> B, C, H, W, N
SHAPES = {
    "c3_points": (2, 3, 5, 7, 37),          # C < 8: the points form
    "c8": (2, 8, 4, 16, 129),               # 4 full tiles + 1 point: a second block
    "c32": (1, 32, 8, 8, 257),              # 8 tiles + 1: two blocks and a third
    "c64": (2, 64, 6, 10, 300),
    "c71_ragged": (1, 71, 5, 5, 65),        # a second channel chunk of 7
    "empty": (1, 32, 8, 8, 0),
}
COORD_SETS = ("uniform", "onecell", "runs", "mix")
SCALE = (0.5, 0.25)
K = 3                # coord columns (the third is not a coordinate)


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def positions(rng, kind, b, h, w, n):
    """[B, N, 2] pixel positions (y, x)."""
    if kind == "onecell":                                      # largest m, every atomic on four rows, one run per tile
        pos = np.array([h // 2, w // 2]) + rng.uniform(0.05, 0.95, (b, n, 2))
        return pos
    if kind == "runs":                                         # sorted scan lines: runs of 1..9 points in one cell
        cy, cx = np.zeros((b, n), dtype=np.int64), np.zeros((b, n), dtype=np.int64)
        for s in range(b):
            i = 0
            while i < n:
                ln = int(rng.integers(1, 10))
                cy[s, i:i + ln], cx[s, i:i + ln] = rng.integers(-1, h), rng.integers(-1, w)
                i += ln
            for edge in range(TILE, n, TILE):                  # a run across every tile border (every 4th is a block border)
                cy[s, edge - 1:edge + 1], cx[s, edge - 1:edge + 1] = cy[s, edge - 1], cx[s, edge - 1]
        return np.stack((cy, cx), -1) + rng.uniform(0.05, 0.95, (b, n, 2))
    pos = np.stack((rng.uniform(-1.5, h + 0.5, (b, n)), rng.uniform(-1.5, w + 0.5, (b, n))), -1)   # one cell over every border
    special = [(-1.0, 2.5), (2.5, -1.0), (float(h), 2.5), (2.5, float(w)), (0.0, 0.0), (h - 1.0, w - 1.0), (-0.5, -0.5),
               (h - 0.5, w - 0.5), (-0.25, w - 0.75), (h - 0.75, -0.25), (1.0, 2.0)]
    for j, p in enumerate(special[:n]):
        pos[j % b, (j * 7) % n] = p
    if kind == "mix":
        bad = rng.random((b, n))
        pos[bad < 0.10] = -1000.0 * np.array(SCALE)           # the padding rows: coordinate -1000 on both axes
        pos[(bad >= 0.10) & (bad < 0.15), 0] = np.nan
        pos[(bad >= 0.15) & (bad < 0.20), 1] = np.nan
        pos[(bad >= 0.20) & (bad < 0.23)] = np.nan
    return pos


def backward_ref(grad_out, coord, scale, h, w):
    """grad_out [B, C, N], coord [B, N, K] -> S, A [B, C, H, W] float64 and m [B, 1, H, W] int64."""
    grad_out = np.asarray(grad_out, dtype=np.float64)
    b, c, n = grad_out.shape
    iy, ix = ops_np.bilinear_pixel_coords(np.asarray(coord)[..., :2], scale, h, w)
    iy, ix = iy.astype(np.float64), ix.astype(np.float64)
    fin = np.isfinite(iy) & np.isfinite(ix)
    iy, ix = np.where(fin, iy, -10.0), np.where(fin, ix, -10.0)
    y0, x0 = np.floor(iy), np.floor(ix)
    wy = ((y0 + 1.0) - iy, iy - y0)
    wx = ((x0 + 1.0) - ix, ix - x0)
    s = np.zeros((b * h * w, c))
    a = np.zeros((b * h * w, c))
    m = np.zeros(b * h * w, dtype=np.int64)
    g_rows = grad_out.transpose(0, 2, 1)                       # [B, N, C]
    batch = np.broadcast_to(np.arange(b)[:, None], (b, n))
    for k in range(4):
        yy, xx = y0 + (k >> 1), x0 + (k & 1)
        ok = fin & (yy >= 0) & (yy <= h - 1) & (xx >= 0) & (xx <= w - 1)
        cell = ((batch[ok] * h + yy[ok].astype(np.int64)) * w + xx[ok].astype(np.int64))
        term = (wy[k >> 1] * wx[k & 1])[ok][:, None] * g_rows[ok]
        np.add.at(s, cell, term)
        np.add.at(a, cell, np.abs(term))
        np.add.at(m, cell, 1)
    to_map = lambda v: np.ascontiguousarray(v.reshape(b, h, w, -1).transpose(0, 3, 1, 2))
    return to_map(s), to_map(a), to_map(m)


def bound(case):
    return (case.m + 8) * U * case.A


def worst_ratio(got, case, factor=1.0):
    """-> (every element inside factor * bound, worst error / bound).  Where the bound is 0 the error has to be 0, and a NaN
    is outside every bound."""
    got = np.asarray(got, dtype=np.float64)
    lim = factor * bound(case)
    err = np.abs(got - case.S)
    ok = bool((err <= lim).all())
    pos = lim > 0
    return ok, (float((err[pos] / lim[pos]).max()) if pos.any() else 0.0)


def make_case(name, b, c, h, w, n, kind, scale=SCALE, pos=None):
    rng = np.random.default_rng(_seed("bilinear_bwd/" + name))
    if pos is None:
        pos = positions(rng, kind, b, h, w, n)
    coord = np.empty((b, n, K))
    coord[..., :2] = pos / np.asarray(scale)
    coord[..., 2] = rng.random((b, n))
    case = types.SimpleNamespace(name=name, b=b, c=c, h=h, w=w, n=n, scale=scale)
    case.coord = _f32(coord)
    case.grad_out = _f32(rng.standard_normal((b, c, n)))
    case.S, case.A, case.m = backward_ref(case.grad_out, case.coord, scale, h, w)
    for v in vars(case).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def case_of(shape, kind):
    b, c, h, w, n = SHAPES[shape]
    return make_case("%s/%s" % (shape, kind), b, c, h, w, n, kind)


@functools.lru_cache(maxsize=None)
def sparse_case():
    """Nine points on 2 x 8 x 8 cells: most elements receive nothing."""
    return make_case("sparse", 2, 32, 8, 8, 9, "uniform")


GRID_WAVES = 2048 * BLOCK_TILES      # waves of the largest grid bil_bwd_rows is launched with (kMaxGrid blocks)


@functools.lru_cache(maxsize=None)
def grid_stride_case():
    """The regime training runs in: more 32-point tiles (2 x 4375) than the largest grid has waves (8192), so waves walk a
    second tile, and the tile sequence crosses the sample boundary (N is no multiple of the tile).  Sorted runs with a mix
    of NaN rows, and in the middle of every sample a stretch of padding rows at -1000 that spans whole tiles: those
    tiles take the kernel's early `continue`, among them second tiles of waves and first tiles of waves that go on."""
    b, c, h, w, n = 2, 8, 12, 20, 139987
    rng = np.random.default_rng(_seed("bilinear_bwd/grid-stride-pos"))
    pos = positions(rng, "runs", b, h, w, n)
    bad = rng.random((b, n))
    pos[bad < 0.02] = np.nan
    pos[(bad >= 0.02) & (bad < 0.04)] = -1000.0 * np.array(SCALE)
    pos[0, 3203:9605] = -1000.0 * np.array(SCALE)             # tiles 101..299: first tiles of waves that have a second one
    pos[0, 60011:75003] = -1000.0 * np.array(SCALE)           # tiles 1876..2342: the only tiles of their waves
    pos[1, 120005:131009] = -1000.0 * np.array(SCALE)         # tiles 8126..8468 overall: around the wrap at tile 8192
    return make_case("grid_stride", b, c, h, w, n, None, pos=pos)


@functools.lru_cache(maxsize=None)
def dyadic_case():
    """Positions j / 32 on a 9 x 17 map with scale (0.5, 0.5): size - 1 is a power of two, so the float32 position chain is
    exact however a division by size - 1 is carried out (a true division, or a product with the reciprocal as torch's GPU
    kernels do for a scalar divisor), and every weight is exact too.  Two formulations then differ by the rounding of the sums alone."""
    b, c, h, w, n = 2, 32, 9, 17, 211
    rng = np.random.default_rng(_seed("bilinear_bwd/dyadic-pos"))
    pos = np.stack((rng.integers(-48, (h + 1) * 32, (b, n)), rng.integers(-48, (w + 1) * 32, (b, n))), -1) / 32.0
    return make_case("dyadic", b, c, h, w, n, None, scale=(0.5, 0.5), pos=pos)


def grid_sample_formulation(torch, grid_feat, grid_coord, scale):
    """BilinearSample's F.grid_sample path (networks/backbone.py:453-475), for tensors of any device / dtype."""
    import torch.nn.functional as F
    h, w = grid_feat.shape[2], grid_feat.shape[3]
    gx = (2 * grid_coord[:, :, 1] * scale[1] / (w - 1)) - 1
    gy = (2 * grid_coord[:, :, 0] * scale[0] / (h - 1)) - 1
    return F.grid_sample(grid_feat, torch.stack((gx, gy), dim=-1), mode="bilinear", padding_mode="zeros", align_corners=True)

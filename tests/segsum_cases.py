"""The fixed-order backward sums of csrc/segsum.hip (smos_bilinear_gather_bwd_det, smos_msda_bwd_det) restated in numpy
float32, shared by tests/test_host_segsum.py (no GPU) and tests/test_gpu_deterministic_backward.py.

Both gradients have one structure: a destination row is the sum, over the (source, tap) pairs that reach it, of a scalar
weight times a source row of grad_out.  The result is a defined float32 number.  For a destination with terms
t_0 .. t_{m-1} in ascending pair index:

    t_j[c] = w_j * src_j[c]                       one float32 product
    chunks of L consecutive terms                 L = smos_segsum_chunk(), a parameter here
    a chunk: left to right from its first term    float32 additions, no FMA
    the chunk partials: left to right in chunk order
    no term: exactly 0

``chunked_sum`` does this for all destinations at once: the terms are ordered by their rank inside their destination, and
one loop over the rank (the rank inside a chunk, chunk after chunk) adds one term to every destination that has one of that
rank.  The kernels have to return these bits; the restatement itself is held to the float64 references' bounds in
tests/test_host_segsum.py.

Bilinear: pair (b * N + n) * 4 + k, k = nw, ne, sw, se; positions from oracle.ops_np.bilinear_pixel_coords, weights in
float32 as make_taps (csrc/bilinear_taps.h) forms them; a padding row, a NaN coordinate or a tap outside the map is absent.
MSDA: pair ((((b * Lq + q) * M + m) * L + l) * P + p) * 4 + corner, weight (w_y * w_x) * attn; util.MSDA_BWD_CASES have
dyadic locations, so loc * size - 0.5 and the corner fractions are exact in float32 and the restatement is bit-determined
however the position arithmetic is contracted.
"""
import functools

import numpy as np

from oracle import ops_np
from tests import bilinear_bwd_cases as bcases
from tests import util

F = np.float32
OTHER_L = 512                    # a second chunk length for the host checks (the kernels have one, smos_segsum_chunk())
ONECELL_SHAPE = (1, 32, 8, 8)    # B, C, H, W of the chunk-edge cases


def chunked_sum(keys, weights, src_row, src, n_rows, chunk):
    """keys [P] (destination row, >= n_rows: absent), weights [P] float32, src_row [P] (row of src [rows, C] float32)
    -> (sums [n_rows, C] float32, m [n_rows] terms per destination)."""
    keys = np.asarray(keys, dtype=np.int64)
    src = np.asarray(src, dtype=F)
    idx = np.flatnonzero(keys < n_rows)
    idx = idx[np.argsort(keys[idx], kind="stable")]            # what the stable radix sort leaves: ascending pair index per key
    k = keys[idx]
    m = np.bincount(k, minlength=n_rows).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(m)[:-1]))
    rank = np.arange(len(k)) - first[k]
    by_rank = np.argsort(rank, kind="stable")
    k, idx, rank = k[by_rank], idx[by_rank], rank[by_rank]
    total = np.zeros((n_rows, src.shape[1]), dtype=F)
    part = np.zeros_like(total)
    top = int(m.max()) if len(k) else 0
    edge = np.searchsorted(rank, np.arange(top + 1))
    for q in range(top):
        sel = slice(edge[q], edge[q + 1])
        d, pi = k[sel], idx[sel]                                # every destination at most once
        term = np.asarray(weights, dtype=F)[pi][:, None] * src[np.asarray(src_row)[pi]]
        assert term.dtype == F
        part[d] = term if q % chunk == 0 else part[d] + term
        de = d[(q % chunk == chunk - 1) | (q == m[d] - 1)]      # the chunk, or the list, ends here
        total[de] = part[de] if q < chunk else total[de] + part[de]
    return total, m


def bilinear_pairs(coord, scale, h, w):
    """coord [B, N, K] -> keys [B*N*4] int64 (B*H*W: absent) and weights [B*N*4] float32 in pair order."""
    coord = np.asarray(coord)
    b, n = coord.shape[:2]
    iy, ix = ops_np.bilinear_pixel_coords(coord[..., :2], scale, h, w)
    with np.errstate(invalid="ignore"):
        fy, fx = np.floor(iy), np.floor(ix)
        wx1, wx0 = ix - fx, (fx + F(1)) - ix
        wy1, wy0 = iy - fy, (fy + F(1)) - iy
        near = (iy > F(-2)) & (iy < F(h + 1)) & (ix > F(-2)) & (ix < F(w + 1))
        y0 = np.where(near, fy, -5).astype(np.int64)
        x0 = np.where(near, fx, -5).astype(np.int64)
        wt = np.stack((wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1), -1)
    assert wt.dtype == F
    batch = np.arange(b)[:, None]
    keys = np.empty((b, n, 4), dtype=np.int64)
    for k in range(4):
        y, x = y0 + (k >> 1), x0 + (k & 1)
        inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        keys[..., k] = np.where(inside, (batch * h + y) * w + x, b * h * w)
    wt = np.where(keys < b * h * w, wt, F(0))
    return keys.reshape(-1), wt.reshape(-1)


@functools.lru_cache(maxsize=None)
def bilinear_restated(case_key, chunk):
    """-> (grad_grid [B, C, H, W] float32, m [B, 1, H, W]) of a case named by ``bilinear_case``'s key."""
    case = bilinear_case(case_key)
    b, c, h, w, n = case.b, case.c, case.h, case.w, case.n
    keys, wt = bilinear_pairs(case.coord, case.scale, h, w)
    rows = np.ascontiguousarray(case.grad_out.astype(F).transpose(0, 2, 1)).reshape(b * n, c)
    total, m = chunked_sum(keys, wt, np.arange(b * n * 4) // 4, rows, b * h * w, chunk)
    out = np.ascontiguousarray(total.reshape(b, h, w, c).transpose(0, 3, 1, 2))
    out.setflags(write=False)
    return out, m.reshape(b, 1, h, w)


@functools.lru_cache(maxsize=None)
def onecell_case(n):
    b, c, h, w = ONECELL_SHAPE
    return bcases.make_case("segsum/onecell/%d" % n, b, c, h, w, n, "onecell")


def onecell_sizes(chunk):
    return (chunk - 1, chunk, chunk + 1, 2 * chunk + 3)


def bilinear_case(key):
    """key: ("shape", shape, kind) | ("sparse",) | ("dyadic",) | ("grid_stride",) | ("onecell", n)."""
    if key[0] == "shape":
        return bcases.case_of(key[1], key[2])
    if key[0] == "onecell":
        return onecell_case(key[1])
    return {"sparse": bcases.sparse_case, "dyadic": bcases.dyadic_case, "grid_stride": bcases.grid_stride_case}[key[0]]()


def bilinear_keys(chunks):
    """The cases of the issue: every SHAPES x COORD_SETS case, the three special ones and the chunk-edge cases of every
    chunk length in ``chunks``."""
    keys = [("shape", s, k) for s in bcases.SHAPES for k in bcases.COORD_SETS]
    keys += [("sparse",), ("dyadic",), ("grid_stride",)]
    seen = set()
    for chunk in chunks:
        for n in onecell_sizes(chunk):
            if n not in seen:
                seen.add(n)
                keys.append(("onecell", n))
    return keys


def key_id(key):
    return "-".join(str(v) for v in key)


def msda_pairs(c):
    """A case of util.msda_bwd_case -> keys [pairs] int64 (N*S*M: absent), weights [pairs] float32, in pair order."""
    loc, attn = c.loc.astype(F), c.attn.astype(F)
    assert np.array_equal(loc.astype(np.float64), c.loc)           # dyadic: nothing is lost
    n_rows = c.n * c.s * c.m
    keys = np.empty((c.n, c.lq, c.m, c.l, c.p, 4), dtype=np.int64)
    wt = np.empty(keys.shape, dtype=F)
    b = np.arange(c.n)[:, None, None, None]
    head = np.arange(c.m)[None, None, :, None]
    for l in range(c.l):
        h, w = int(c.shapes[l, 0]), int(c.shapes[l, 1])
        w_im = loc[:, :, :, l, :, 0] * F(w) - F(0.5)
        h_im = loc[:, :, :, l, :, 1] * F(h) - F(0.5)
        valid = (h_im > -1) & (w_im > -1) & (h_im < h) & (w_im < w)
        h_low, w_low = np.floor(h_im), np.floor(w_im)
        lh, lw = h_im - h_low, w_im - w_low
        hh, hw = F(1) - lh, F(1) - lw
        y0, x0 = h_low.astype(np.int64), w_low.astype(np.int64)
        for corner, (wy, wx) in enumerate(((hh, hw), (hh, lw), (lh, hw), (lh, lw))):
            y, x = y0 + (corner >> 1), x0 + (corner & 1)
            inside = valid & (y >= 0) & (y <= h - 1) & (x >= 0) & (x <= w - 1)
            keys[:, :, :, l, :, corner] = np.where(inside, (b * c.s + int(c.lsi[l]) + y * w + x) * c.m + head, n_rows)
            weight = (wy * wx) * attn[:, :, :, l, :]
            assert weight.dtype == F
            wt[:, :, :, l, :, corner] = np.where(inside, weight, F(0))
    return keys.reshape(-1), wt.reshape(-1)


@functools.lru_cache(maxsize=None)
def msda_restated(name, chunk):
    """-> (grad_value [N, S, M, D] float32, m [N, S, M]) of util.msda_bwd_case(name)."""
    c = util.msda_bwd_case(name)
    keys, wt = msda_pairs(c)
    rows = c.grad_out.astype(F).reshape(c.n * c.lq * c.m, c.d)
    total, m = chunked_sum(keys, wt, np.arange(len(keys)) // (c.l * c.p * 4), rows, c.n * c.s * c.m, chunk)
    out = total.reshape(c.n, c.s, c.m, c.d)
    out.setflags(write=False)
    return out, m.reshape(c.n, c.s, c.m)

"""Point -> grid max-pool scatter (csrc/voxel_maxpool.hip, csrc/voxel_cell.h): the float64 reference, the restatement of the host's
kernel choice and the case builders shared by tests/test_host_voxel_maxpool_reference.py (no GPU) and
tests/test_gpu_voxel_maxpool.py.

Reference.  ``pool_ref``: the cell of a point comes from the FLOAT32 product float32(coord) * float32(scale) (what the reference
computes, point_deep_cuda_kernel.cu:39-47): kept iff -1 < p < size on every axis, then truncated toward zero (a product in
(-1, 0) lands in cell 0; NaN and +-inf fail both comparisons).  The kept points of a sample are put in cell order by a stable
sort and every run of equal cells is reduced by np.maximum.reduceat in float64; an empty cell keeps 0.  Nothing is shared with
oracle.ops_np.voxel_maxpool_fwd (np.maximum.at on a -inf buffer); the host tests hold the two against each other.
``grad_ref``: every kept point whose value equals the maximum of its cell receives the cell's gradient (ties all do), every
other point 0.  ``winners`` is the mask behind it.

A maximum returns one of its inputs, so every comparison built on this module is EXACT (``same``: np.array_equal on the values
as float64, NaN equal to NaN); there is no tolerance anywhere.  Values are compared, not bit patterns: whether an all-zero cell
ends as +0 or -0 depends on the order of racing stores on the exact path.

Kernel choice.  ``launch_path`` restates the dispatch of smos_voxel_maxpool_fwd (csrc/voxel_maxpool.hip: the dtype split at
:300-301, the rows condition and its lane-group size at :308-310, the channel chunks of the points kernel at :328-336).  The
flag-gated exact path (vmp_fwd_signed, :343-345) depends on the data: ``Case.signed`` says whether a kept point carries a value
that raises the flag.

Cases.  ``make`` draws coordinates from -0.2 ... 1.2 of the grid's extent and features as multiples of 1/8 (exact in float16,
exact ties are common), shapes the signs by the mode, and then plants what a draw cannot promise: the points of one cell are
sent to the reference's padding coordinate (an empty cell), and two points are moved onto a third, one of them with the cell's
maximum in every channel (a cell of >= 3 members with an exact tie for its maximum).  ``check_properties`` asserts the four
properties -- an empty cell, a cell of >= 3 members, an exact tie for a maximum, a dropped point -- for every case; the
one-point case (N = 1) cannot hold the last three and says so in its ``lacks``.
"""
import functools
import hashlib
import types

import numpy as np
import torch

PAD = -4864.0                               # the reference's padding coordinate
SIGNS = ("relu", "mixed", "neg", "neg_in_last_chunk")
LAYOUTS = ("nchw", "cl", "pm_nchw", "sliced")
# (a) nchw:    contiguous [BS,C,N] features into a contiguous NCHW grid                          -> points kernel
# (b) cl:      point-major features ([BS,N,C] buffer) into a channels-last grid                  -> rows kernel for C >= 8
# (c) pm_nchw: point-major features into a contiguous NCHW grid                                  -> points kernel, fs_c == 1
# (d) sliced:  a channel slice and an every-other-point slice of a wider [BS,C+3,2N+5] buffer    -> points kernel, no tight stride
C_POINTS_ONE = (1, 7, 8, 9)
C_POINTS_CHUNKED = (16, 17, 20, 71)
C_ROWS = (8, 12, 16, 17, 32, 33, 64, 71, 130)
C_ALL = tuple(sorted(set(C_POINTS_ONE + C_POINTS_CHUNKED + C_ROWS)))
C_GENERIC = (1, 20, 71)
NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64, torch.float16: np.float16}


# ---------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------
def cell_of(ind, out_size, scale):
    """int64 [BS,N]: row-major flat cell over the spatial dims, -1 for a dropped point."""
    ind = np.asarray(ind)
    bs, n, d = ind.shape
    assert d == len(out_size) == len(scale)
    cell = np.zeros((bs, n), dtype=np.int64)
    keep = np.ones((bs, n), dtype=bool)
    for k in range(d):
        p = ind[:, :, k].astype(np.float32) * np.float32(scale[k])
        assert p.dtype == np.float32
        with np.errstate(invalid="ignore"):
            ok = (p > np.float32(-1.0)) & (p < np.float32(out_size[k]))
        keep &= ok
        cell = cell * int(out_size[k]) + np.trunc(np.where(ok, p, np.float32(0))).astype(np.int64)
    return np.where(keep, cell, -1)


def pool_ref(feat, ind, out_size, scale):
    """feat [BS,C,N], ind [BS,N,D] -> (out float64 [BS,C,*out_size], cell int64 [BS,N])."""
    feat = np.asarray(feat)
    bs, c, n = feat.shape
    cell = cell_of(ind, out_size, scale)
    cells = int(np.prod(out_size))
    out = np.zeros((bs, c, cells), dtype=np.float64)
    for b in range(bs):
        kept = np.flatnonzero(cell[b] >= 0)
        if kept.size == 0:
            continue
        order = kept[np.argsort(cell[b, kept], kind="stable")]
        run = cell[b, order]
        starts = np.flatnonzero(np.concatenate(([True], run[1:] != run[:-1])))
        out[b][:, run[starts]] = np.maximum.reduceat(feat[b][:, order].astype(np.float64), starts, axis=1)
    return out.reshape((bs, c) + tuple(int(s) for s in out_size)), cell


def winners(feat, cell, out):
    """bool [BS,C,N]: the point is kept and its value equals the maximum of its cell."""
    feat = np.asarray(feat)
    bs, c, n = feat.shape
    flat = np.asarray(out).reshape(bs, c, -1)
    win = np.zeros(feat.shape, dtype=bool)
    for b in range(bs):
        kept = np.flatnonzero(cell[b] >= 0)
        win[b][:, kept] = flat[b][:, cell[b, kept]] == feat[b][:, kept].astype(np.float64)
    return win


def grad_ref(feat, cell, out, grad_out):
    """float64 [BS,C,N]: the cell's gradient for every winner, 0 for everything else."""
    bs, c, n = np.asarray(feat).shape
    go = np.asarray(grad_out).reshape(bs, c, -1).astype(np.float64)
    win = winners(feat, cell, out)
    grad = np.zeros(win.shape, dtype=np.float64)
    for b in range(bs):
        grad[b] = np.where(win[b], go[b][:, np.maximum(cell[b], 0)], 0.0)
    return grad


def same(got, want):
    """Exact equality of the values (NaN equal to NaN, +0 equal to -0)."""
    return np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), equal_nan=True)


# ---------------------------------------------------------------------------------------------
# the host's kernel choice
# ---------------------------------------------------------------------------------------------
def launch_path(dtype, C, points, fs_c, out_c):
    """(kernel, G or chunks, c_chunk) of smos_voxel_maxpool_fwd: ("generic", 1, C) for float16 / float64,
    ("rows", G, None) or ("points", chunks, c_chunk) for float32."""
    if dtype != torch.float32:
        return ("generic", 1, C)                                    # voxel_maxpool.hip:300-301
    if fs_c == 1 and out_c == 1 and C >= 8:                         # :308
        G = 8
        while G < 64 and G < C:                                     # :309-310
            G <<= 1
        return ("rows", G, None)
    chunks = 1
    if points < (1 << 20) and C >= 16:                              # :328-333
        chunks = ((1 << 20) + points - 1) // points
        chunks = max(1, min(chunks, C // 8))
    c_chunk = (C + chunks - 1) // chunks                            # :334-336
    c_chunk = (c_chunk + 7) // 8 * 8
    chunks = (C + c_chunk - 1) // c_chunk
    return ("points", chunks, c_chunk)


def points_per_sweep(kernel, G=None):
    """Points one grid-stride sweep of a kernel covers: the rows and points kernels cap their grid at 4096 blocks
    (voxel_maxpool.hip:312,337), the signed, generic and backward kernels at 2048 (csrc/smos_common.h: kMaxGrid)."""
    if kernel == "rows":
        return 4096 * (256 // G)
    return (4096 if kernel == "points" else 2048) * 256


# ---------------------------------------------------------------------------------------------
# tensors of a case in a layout
# ---------------------------------------------------------------------------------------------
def place(feat, size, layout, dtype, device):
    """(feat view [BS,C,N], out view [BS,C,*size] zero-filled) of ``layout`` on ``device``; ``feat`` is a numpy array already
    rounded to ``dtype``."""
    bs, c, n = feat.shape
    f = torch.from_numpy(np.ascontiguousarray(feat)).to(device=device, dtype=dtype)
    if layout in ("cl", "pm_nchw"):
        f = f.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    elif layout == "sliced":
        wide = torch.full((bs, c + 3, 2 * n + 5), 77.0, dtype=dtype, device=device)
        wide[:, 2:2 + c, 3:3 + 2 * n:2] = f
        f = wide[:, 2:2 + c, 3:3 + 2 * n:2]
    else:
        assert layout == "nchw"
    if layout == "cl":
        out = torch.zeros((bs,) + tuple(size) + (c,), dtype=dtype, device=device).movedim(-1, 1)
    else:
        out = torch.zeros((bs, c) + tuple(size), dtype=dtype, device=device)
    return f, out


def cell_offsets(cell, size, out):
    """voxel_max_idx as the kernels define it: b * out.stride(0) + sum_d cell_d * out.stride(2 + d) from the real strides of
    ``out``, -1 for a dropped point."""
    bs, n = cell.shape
    off = np.arange(bs, dtype=np.int64)[:, None] * int(out.stride(0)) + np.zeros((bs, n), dtype=np.int64)
    rest = np.maximum(cell, 0)
    for d in range(len(size) - 1, -1, -1):
        off += (rest % int(size[d])) * int(out.stride(2 + d))
        rest = rest // int(size[d])
    return np.where(cell >= 0, off, -1)


def layout_strides(layout, n, size):
    """(fs_c, out_c) of the tensors ``place`` builds."""
    fs_c = {"nchw": n, "cl": 1, "pm_nchw": 1, "sliced": 2 * n + 5}[layout]
    return fs_c, (1 if layout == "cl" else int(np.prod(size)))


def path_of(case, layout, dtype=torch.float32):
    """launch_path of a case in a layout."""
    fs_c, out_c = layout_strides(layout, case.n, case.size)
    return launch_path(dtype, case.c, case.bs * case.n, fs_c, out_c)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.Generator(np.random.PCG64(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")))


def _signed(sign, base):
    """base: multiples of 1/8 [BS,C,N] -> the features of a sign mode."""
    if sign == "relu":
        return np.maximum(base, 0.0) + 0.0                            # (+ 0.0: no -0 in an all-non-negative tensor)
    if sign == "mixed":
        return base
    if sign == "neg":
        return -np.abs(base)                                          # -0.0 included: the largest "negative" a cell can hold
    assert sign == "neg_in_last_chunk" and base.shape[1] > 16
    out = np.maximum(base, 0.0) + 0.0
    out[:, 16:] = -np.abs(base[:, 16:]) - 0.125                       # strictly negative, in channels >= 16 only
    return out


def _finish(name, sign, feat, ind, size, scale, layout, lacks=(), npdt=np.float32):
    feat = np.ascontiguousarray(feat, dtype=npdt)
    ind = np.ascontiguousarray(ind, dtype=np.float32)
    bs, c, n = feat.shape
    out, cell = pool_ref(feat, ind, size, scale)
    kept = np.broadcast_to((cell >= 0)[:, None, :], feat.shape)
    with np.errstate(invalid="ignore"):
        signed = bool((~(feat == 0) & ~(feat > 0) & kept).any())     # a kept negative or NaN raises the flag
    case = types.SimpleNamespace(name=name, sign=sign, feat=feat, ind=ind, size=tuple(size), scale=tuple(scale), layout=layout,
                                 bs=bs, c=c, n=n, d=len(size), out=out, cell=cell, signed=signed, lacks=tuple(lacks))
    check_properties(case)
    return case


def properties(case):
    """The four properties of a case as booleans: (empty cell, cell of >= 3 members, exact tie for a maximum, dropped point)."""
    cells = int(np.prod(case.size))
    empty = members3 = tie = False
    win = winners(case.feat, case.cell, case.out)
    for b in range(case.bs):
        kept = case.cell[b] >= 0
        count = np.bincount(case.cell[b][kept], minlength=cells)
        empty |= bool((count == 0).any())
        members3 |= bool((count >= 3).any())
        for ch in range(case.c):
            if tie:
                break
            tie |= bool((np.bincount(case.cell[b][win[b, ch]], minlength=cells) >= 2).any())
    return empty, members3, tie, bool((case.cell < 0).any())


PROPERTY_NAMES = ("empty_cell", "cell_of_3", "tie", "dropped")


def check_properties(case):
    for name, holds in zip(PROPERTY_NAMES, properties(case)):
        assert holds or name in case.lacks, "case %s lacks %s" % (case.name, name)


def make(name, sign, C, N, BS, D, size, scale, layout="nchw", lacks=(), edit=None, hole=None):
    """The case builder: uniform coordinates over -0.2 ... 1.2 of the extent, features in multiples of 1/8 shaped by ``sign``,
    then the planted empty cell and the planted tie (module docstring).  ``edit(feat, ind, rng)`` may overwrite points before
    the planting."""
    assert len(size) == len(scale) == D and sign in SIGNS
    rng = _rng(name)
    extent = np.asarray(size, dtype=np.float64) / np.asarray(scale, dtype=np.float64)
    ind = (rng.uniform(-0.2, 1.2, (BS, N, D)) * extent).astype(np.float32)
    feat = _signed(sign, np.round(rng.normal(0.0, 1.5, (BS, C, N)) * 8.0) / 8.0).astype(np.float32)
    if edit is not None:
        edit(feat, ind, rng)
    cell = cell_of(ind, size, scale)
    hole = int(np.prod(size)) // 2 if hole is None else hole
    ind[cell == hole] = PAD                                            # an empty cell, and its points dropped
    cell = cell_of(ind, size, scale)
    if N >= 3:                                                         # sample 0: two points moved onto a kept third
        kept = np.flatnonzero(cell[0] >= 0)
        assert kept.size, "case %s keeps no point of sample 0" % name
        i0 = int(kept[0])
        i1, i2 = [i for i in range(N - 1, -1, -1) if i != i0][:2]
        ind[0, i1] = ind[0, i0]
        ind[0, i2] = ind[0, i0]
        members = np.flatnonzero(cell_of(ind, size, scale)[0] == cell[0, i0])
        top = feat[0][:, members].max(axis=1)
        feat[0, :, i0] = top                                           # the tie: the cell's maximum twice, in every channel
        feat[0, :, i1] = top
    return _finish(name, sign, feat, ind, size, scale, layout, lacks)


def _rounding_seeds(size, scale, kmax=15):
    """Coordinates x next to k / scale whose float32 product x * scale and the float64 product of the same two float32 numbers
    truncate to different cells, or whose float32 product is exactly ``size`` (dropped; the float64 product is kept)."""
    s32 = np.float32(scale)
    found = []
    for k in range(1, kmax + 1):
        x = np.float32(k / float(s32))
        near = {float(x)}
        lo = hi = x
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            near.update((float(lo), float(hi)))
        for v in sorted(near):
            p32 = np.float32(v) * s32
            p64 = float(np.float32(v)) * float(s32)
            if np.trunc(float(p32)) != np.trunc(p64) or (float(p32) == size and p64 < size):
                found.append((np.float32(v), float(p32), p64))
    return found


@functools.lru_cache(maxsize=None)
def scale_rounding(sign="mixed"):
    """size (7, 9), scale (0.7, 0.3): points on which a product in float64 (or a fused one) picks another cell than the float32
    product does.  Every seeded point carries the largest feature of the tensor, so moving it changes the output."""
    size, scale = (7, 9), (0.7, 0.3)
    seeds = [_rounding_seeds(size[0], scale[0]), _rounding_seeds(size[1], scale[1])]
    planted = []

    def edit(feat, ind, rng):
        i = 5
        for b in range(feat.shape[0]):
            for d in (0, 1):
                for x, p32, p64 in seeds[d]:
                    other = np.float32((1.5 + (i % 3)) / scale[1 - d])             # the middle of a cell on the other axis
                    ind[b, i, d], ind[b, i, 1 - d] = x, other
                    feat[b, :, i] = 8.0 + (i % 4)
                    planted.append((b, i, d, p32, p64))
                    i += 1

    case = make("scale_rounding_" + sign, sign, 9, 257, 2, 2, size, scale, edit=edit, hole=8)       # (hole: cell (0, 8), which no seed can reach)
    far = 0
    for b, i, d, p32, p64 in planted:
        assert np.float32(case.ind[b, i, d]) * np.float32(scale[d]) == np.float32(p32)
        assert np.trunc(p32) != np.trunc(p64) or p32 == size[d]
        if p32 == size[d] and p64 < size[d]:
            far += 1
            assert case.cell[b, i] == -1
    assert len(planted) >= 2 * 8 and far >= 2, (len(planted), far)
    assert len(seeds[0]) >= 8 and len(seeds[1]) >= 4                               # (0.7: e.g. 10.0; 0.3: e.g. 23.333332)
    case.planted = planted
    return case


EDGE_PRODUCTS = (-1.0, float(np.nextafter(np.float32(-1), np.float32(0))), -0.0, "size", "below_size", float("nan"), float("inf"),
                 float("-inf"), 1e30, -1e30, PAD)


@functools.lru_cache(maxsize=None)
def edge_coords(sign="mixed"):
    """Every edge of the keep rule on either axis: the listed values are products (coordinate = value / scale, exact for the
    dyadic scales used), the other axis sits in the middle of a cell."""
    size, scale = (5, 6), (1.0, 0.5)
    expect = []

    def edit(feat, ind, rng):
        i = 3
        for d in (0, 1):
            for v in EDGE_PRODUCTS:
                if v == "size":
                    v = float(size[d])
                elif v == "below_size":
                    v = float(np.nextafter(np.float32(size[d]), np.float32(0)))
                ind[0, i, d] = np.float32(v) / np.float32(scale[d])
                ind[0, i, 1 - d] = np.float32(2.5) / np.float32(scale[1 - d])
                feat[0, :, i] = feat[0, :, i] + 8.0 if sign != "neg" else -0.125      # visible where it lands
                expect.append((i, d, v))
                i += 1

    case = make("edge_coords_" + sign, sign, 9, 130, 2, 2, size, scale, edit=edit)
    for i, d, v in expect:
        landed = case.cell[0, i]
        if v in (-1.0, float(size[d])) or not np.isfinite(v) or abs(v) > 100:
            assert landed == -1, (i, d, v)
        else:
            want_d = 0 if v <= 0 else size[d] - 1
            assert landed == (want_d * size[1] + 2 if d == 0 else 2 * size[1] + want_d), (i, d, v, landed)
    return case


@functools.lru_cache(maxsize=None)
def special_values(sign, dtype=torch.float32):
    """Hand-placed special values in a 6 x 6 grid (scale 1), each in a cell of its own AND as the maximum of a shared cell:
    +inf, the largest finite number and the smallest positive denormal of ``dtype`` (the denormal also as the only positive
    member of a cell of zeros); with sign "mixed" also -inf, the most negative finite number and a negative denormal, and -0.0
    above negatives.  A NaN is the sole member of a cell.  With sign "relu" no value of the tensor is negative."""
    assert sign in ("relu", "mixed")
    fi = np.finfo(NP_DTYPE[dtype])
    big, tiny, inf, nan = float(fi.max), float(fi.smallest_subnormal), float("inf"), float("nan")
    groups = [[inf], [big], [tiny], [nan],
              [inf, 1.0, big], [big, 1.0, 0.5], [tiny, 0.0, 0.0], [2.0, 2.0, 1.0], [0.0, 0.0]]
    if sign == "mixed":
        groups += [[-inf], [-big], [-tiny], [-inf, -inf], [-big, -inf, -inf], [-tiny, -1.0, -big], [-0.0, -1.0, -2.0, -3.0, -0.5],
                   [tiny, -1.0, 0.0], [-1.0, 3.0, -2.0]]
    size, scale = (6, 6), (1.0, 1.0)
    c = 9
    rows, coords = [], []
    for k, members in enumerate(groups):                            # group k -> cell k (cells 0 .. len - 1), the rest stays empty
        for j, v in enumerate(members):
            rows.append(v)
            coords.append((k // 6 + 0.25 + 0.1 * j, k % 6 + 0.5))
    rows.append(5.0)                                                # a dropped point that would win anywhere
    coords.append((PAD, PAD))
    n = len(rows)
    feat = np.empty((2, c, n), dtype=np.float64)
    feat[:] = np.asarray(rows)[None, None, :]
    feat[1] = feat[1][:, ::-1]                                      # sample 1: the same members in the opposite order
    ind = np.empty((2, n, 2), dtype=np.float32)
    ind[0] = np.asarray(coords, dtype=np.float32)
    ind[1] = ind[0][::-1]
    case = _finish("special_values_%s_%s" % (sign, str(dtype).split(".")[-1]), sign, feat, ind, size, scale, "nchw", npdt=NP_DTYPE[dtype])
    nan_cell = 3
    assert np.isnan(case.out[0, :, 0, nan_cell]).all() and (np.bincount(case.cell[0][case.cell[0] >= 0])[nan_cell] == 1)
    assert np.isnan(case.out).sum() == 2 * c                        # the sole-member cells only
    assert case.signed                                              # the NaN has to take the exact path
    return case


def _matrix_name(sign, C):
    return "m_%s_c%d" % (sign, C)


@functools.lru_cache(maxsize=None)
def matrix_case(sign, C):
    """N = 257, BS = 2 into 5 x 6 at scales (0.5, 0.25): the shape of the forward matrix (sign mode x C x layout)."""
    return make(_matrix_name(sign, C), sign, C, 257, 2, 2, (5, 6), (0.5, 0.25))


def matrix_keys():
    return [(sign, C) for sign in SIGNS for C in C_ALL if sign != "neg_in_last_chunk" or C > 16]


SHAPE_CASES = {
    # name: (sign, C, N, BS, D, size, scale, lacks)
    "d1": ("mixed", 9, 257, 2, 1, (11,), (0.5,), ()),
    "d3": ("mixed", 9, 257, 1, 3, (4, 5, 3), (1.0, 0.5, 0.25), ()),
    "d4": ("mixed", 17, 300, 3, 4, (3, 4, 2, 3), (0.5, 1.0, 0.25, 0.5), ()),
    "d4_relu": ("relu", 8, 300, 1, 4, (3, 4, 2, 3), (0.5, 1.0, 0.25, 0.5), ()),
    "n1": ("mixed", 9, 1, 3, 2, (5, 6), (0.5, 0.25), ("cell_of_3", "tie", "dropped")),
    "n63": ("mixed", 20, 63, 1, 2, (5, 6), (0.5, 0.25), ()),
    "n64": ("relu", 20, 64, 1, 2, (5, 6), (0.5, 0.25), ()),
    "n65": ("neg", 20, 65, 3, 2, (5, 6), (0.5, 0.25), ()),
    "sparse": ("mixed", 16, 300, 2, 2, (24, 24), (0.5, 0.25), ()),      # most cells empty, most occupied cells with one member
}
SWEEP_CASES = {
    # a second grid-stride sweep of vmp_fwd_points (1 048 576 points per sweep), vmp_fwd_signed, vmp_fwd_generic and the
    # backward kernels (524 288)
    "sweep_points": ("mixed", 2, 1100000, 1, 2, (16, 16), (0.5, 0.5), "nchw"),
    # vmp_fwd_rows<64>: 16 384 points per sweep, 40 000 points
    "sweep_rows": ("neg", 33, 20000, 2, 2, (8, 8), (0.5, 0.5), "cl"),
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    sign, C, N, BS, D, size, scale, lacks = SHAPE_CASES[name]
    if name == "n1":                                                   # one point per sample: placed, not drawn
        feat = _signed(sign, np.round(_rng(name).normal(0.0, 1.5, (BS, C, N)) * 8.0) / 8.0)
        ind = np.asarray([[[3.0, 9.0]], [[-1.5, -3.5]], [[9.75, 23.5]]], dtype=np.float32)     # cells (1, 2), (0, 0), (4, 5)
        return _finish(name, sign, feat, ind, size, scale, "nchw", lacks)
    return make(name, sign, C, N, BS, D, size, scale, lacks=lacks)


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    sign, C, N, BS, D, size, scale, layout = SWEEP_CASES[name]
    return make(name, sign, C, N, BS, D, size, scale, layout=layout)


def small_cases():
    """name -> case for every case but the two sweeps (built on demand, cached)."""
    todo = {_matrix_name(s, c): functools.partial(matrix_case, s, c) for s, c in matrix_keys()}
    todo.update({n: functools.partial(shape_case, n) for n in SHAPE_CASES})
    for sign in ("relu", "mixed"):
        todo["scale_rounding_" + sign] = functools.partial(scale_rounding, sign)
        todo["special_values_" + sign] = functools.partial(special_values, sign)
        todo["special_values_%s_f64" % sign] = functools.partial(special_values, sign, torch.float64)
    for sign in ("relu", "mixed", "neg"):
        todo["edge_coords_" + sign] = functools.partial(edge_coords, sign)
    return todo


def rounded(case, dtype):
    """(feat, ind, out, cell) of a case with its inputs rounded to ``dtype`` first and the reference run on the rounded values
    (float16 moves coordinates: the cells are recomputed)."""
    npdt = NP_DTYPE[dtype]
    if case.feat.dtype == npdt:
        return case.feat, case.ind, case.out, case.cell
    feat, ind = case.feat.astype(npdt), case.ind.astype(npdt)
    out, cell = pool_ref(feat, ind, case.size, case.scale)
    return feat, ind, out, cell

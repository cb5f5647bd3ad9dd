"""The fused point head (csrc/point_head.hip: point_head<false> / point_head<true>, through ops.point_head) and the TTA reduce
(csrc/vote.hip: tta_argmax): the float64 references, the per-element bounds, float32 restatements of the kernels' order, mutants,
steered row groups, exact twins and the walk geometry under the grid cap, shared by tests/test_host_point_head.py (no GPU) and
tests/test_gpu_point_head.py.  numpy only.

Arrays.  Every array is a float64 array whose entries are float32 numbers, seeded by the case name, built once and read-only.

Reference (head_ref).  relu(W1 x + b1) -> relu(W2 . + b2) -> W3 . + b3 in float64, logits [B, M3, N].  The gather form
("gather": ops.point_head(..., gather=(grid, coord, scale))) takes channels [64, 128) of x from
gather_cases.gather_ref(grid, coord, scale)[0]: float32 positions, float64 taps.

Bound, u = 2^-24, per element; nothing in it is fitted to a kernel.  Roundings counted in csrc/point_head.hip: layer l adds
K_l products, one at a time, to a float32 accumulator that starts at the bias (K1 = 192, K2 = 96, K3 = 64; layer 3 starts at 0
and adds b3 with one float32 addition behind the sum): a term passes at most K_l roundings, K3 + 1 in layer 3.  C_EXTRA = 2
more: one for a product rounded on its own and one for the second-order terms ((1 + u)^n - 1 <= (n + 1) u while n^2 u <= 1;
n <= 195 here).  fmaxf(., 0) is exact and 1-Lipschitz, so the error of a layer's input passes through |W|:

    f1 = u (K1 + 2),  f2 = u (K2 + 2),  f3 = u (K3 + 1 + 2)
    e1 = f1 (|W1| |x| + |b1|)  [+ (1 + f1) |W1[:, 64:128]| gather_cases.bound(A)   in the gather form, where |x| of that third is A]
    e2 = (1 + f2) |W2| e1 + f2 (|W2| relu(z1) + |b2|)
    e3 = (1 + f3) |W3| e2 + f3 (|W3| relu(z2) + |b3|)

Float32 restatement (head_f32), the kernel's order read from csrc/point_head.hip.  The accumulator starts at the bias; layer 1
walks the k-steps of k_order() (= ops.point_head_k_order(): step s, lane half h -> channel 64 (s >> 5) + 32 h + (s & 31)),
layers 2 and 3 walk their input in accumulator order (step s, lane half h -> channel 32 (s >> 4) + 8 ((s & 15) >> 2) + 4 h +
(s & 3)); the two products of one v_mfma_f32_32x32x2_f32 are taken as an fma chain over h = 0, 1 onto the accumulator (the ISA
document does not specify their order; RMS_FACTOR covers the other one).  Layer 3 starts at 0, b3 is added at the end.  The
gather form's BEV third is gather_cases.emulate_f32(..., fused=True): bilinear_sum_cl is contracted under -ffp-contract=on.

Row groups of the steered cases (N = 300: 27 points each, one_hot 192), judged separately as tfusion_cases.GROUPS are:

    randn      standard normal rows                                                                  baseline
    all_dead   every layer-1 pre-activation is negative: the logits are the constant W3 relu(b2) + b3 to the bound
    cancel     the layer-1 sums cancel to 1e-3 of |W1| |x| + |b1|
    one_hot    one nonzero input channel per row, stepping through all 192: every W1 column is seen alone
    big        |x| about 1e3

Exact twins.  Inputs are integers in [-3, 3], weights k / 4 with |k| <= 2, biases multiples of 1 / 4 in [-2, 2]; the gather form
takes an integer map (5 x 9: size - 1 a power of two, so that the float32 position chain is exact) at integer and half positions
under scale (0.5, 0.5), which makes its BEV third multiples of 1 / 4.  The numbers of layer l are multiples of 1 / d_l with
d = (4, 16, 64), (16, 64, 256) in the gather form; as long as (|W| |input| + |b|) d_l < 2^24 at every layer (exact_condition,
asserted per case and form) every partial sum in any order is a float32 number, and the kernel must return float32(reference)
bit for bit.

Walks.  The grid of point_head is min(ceil(tiles / 8), CUs) blocks of 8 waves, capped by tests/util.py::conv_grid_cap; wave v
of `waves` takes tiles v, v + waves, ... of the B * ceil(n_live / 32) live tiles.  walk_tiles() states that; WALKS lists the
shapes and caps.  With 8 waves in a block a cap of c blocks needs more than 16 c tiles for a third trip: B = 2, N = 300 (20
tiles) has one under a cap of 1 (2 trips under a cap of 2), B = 3, N = 70 (9 tiles) never has more than two trips, and
B = 3, N = 360 (36 tiles) has three and more under both caps.  WALK_FULL names the (case, cap) pairs on which some wave takes
>= 3 tiles AND some wave's consecutive tiles lie in different samples.

tta_argmax.  Reference: softmax over K and the mean over B in float64.  Restatement (tta_f32): float32 in the kernel's order
with numpy's float32 exp.  Bound on a probability, absolute (every term is <= 1): (K + B + 2 + TTA_EXP_ULP) u.  Counted from
the kernel: v - max, 1 (|x| e^x <= 1 / e: a relative error of the argument is an absolute one of the term); the sum over K,
K - 1; the division, 1; the sum over B (partial sums <= b, divided by B afterwards), B - 1; the division by B, 1; second order,
1.  An error of the exponentials moves p_k = e_k / sum_j e_j by p_k (1 - p_k) 2 max|delta| <= max|delta| / 2, so the error of
expf counts once.  The ROCm tree this was written against documents no ulp figure for the device library's expf (its headers
and documents were searched for one), so that term is measured as tfusion_cases.MAX_FACTOR was: the worst
|restatement - reference| / u over TTA_SPECS, doubled and rounded up to a power of two (tests/test_host_point_head.py prints the
figures and asserts that the constant is that number).
"""
import functools
import hashlib
import os
import types

import numpy as np

from tests import gather_cases
from tests import tfusion_cases

U = 2.0 ** -24
F32 = np.float32
K1, M1, M2 = 192, 96, 64
C_EXTRA = 2                   # a product rounded on its own + second order
F1, F2, F3 = U * (K1 + C_EXTRA), U * (M1 + C_EXTRA), U * (M2 + 1 + C_EXTRA)
RMS_FACTOR = tfusion_cases.RMS_FACTOR
MUTANT_MARGIN = tfusion_cases.MUTANT_MARGIN
SCALE = (0.5, 0.5)
KG = gather_cases.KG
HG, WG = gather_cases.HG, gather_cases.WG
XH, XW = 5, 9                 # the exact twins' map
FORMS = ("rows", "gather")
GROUPS = ("randn", "all_dead", "cancel", "big", "one_hot")
GROUP_SIZES = (27, 27, 27, 27, 192)
A1_FLOATS, A2_FLOATS, A3_FLOATS = 3 * 96 * 64, 2 * 48 * 64, 32 * 64
BLOCK_FLOATS = A1_FLOATS + A2_FLOATS + A3_FLOATS + M1 + M2 + 32
WAVES = 8                     # per block of point_head
TTA_EXP_ULP = 8.0             # measured worst 2.850 u (tests/test_host_point_head.py: tta case k8_b1_n257) -> doubled, next power of two


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


_f32 = gather_cases._f32
_freeze = gather_cases._freeze
worst_ratio = gather_cases.worst_ratio
rms = tfusion_cases.rms
ratio = tfusion_cases.ratio


def relu(x):
    return np.maximum(x, 0.0)


def k_order():
    """[96, 2]: the input channel k-step s of layer 1 feeds to lane half h (ops.point_head_k_order)."""
    s, h = np.arange(96)[:, None], np.arange(2)[None, :]
    return 64 * (s >> 5) + 32 * h + (s & 31)


def acc_order(steps):
    """[steps, 2]: the input channel of k-step s, lane half h of layers 2 / 3: register s & 15 of tile s >> 4."""
    s, h = np.arange(steps)[:, None], np.arange(2)[None, :]
    return 32 * (s >> 4) + 8 * ((s & 15) >> 2) + 4 * h + (s & 3)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def _spec(b, n, m3, pitch, steered=False, coords="special", exact=False):
    return dict(b=b, n=n, m3=m3, pitch=pitch, steered=steered, coords=coords, exact=exact)


BOUND_SPECS = {
    "n1_m1": _spec(1, 1, 1, 192),
    "n31_m3": _spec(2, 31, 3, 200),
    "n32_m8": _spec(3, 32, 8, 192),
    "n33_m9": _spec(2, 33, 9, 200),
    "n70_m20": _spec(3, 70, 20, 192),
    "n70_m32": _spec(1, 70, 32, 200),
    "n300_m3": _spec(1, 300, 3, 192, steered=True),
    "n300_m32": _spec(2, 300, 32, 200, steered=True),
}
# name -> caps
WALKS = {"walk_b2_n300": (1, 2), "walk_b3_n70": (1, 2), "walk_b3_n360": (1, 2)}
WALK_SPECS = {"walk_b2_n300": _spec(2, 300, 9, 200, coords="interior"), "walk_b3_n70": _spec(3, 70, 3, 192, coords="interior"),
              "walk_b3_n360": _spec(3, 360, 20, 192, coords="interior")}
WALK_FULL = (("walk_b2_n300", 1), ("walk_b3_n360", 1), ("walk_b3_n360", 2))
WALK_N_LIVE = (None, 0, 1, 45, 64, 290, "N")
SPECS = dict(BOUND_SPECS)
SPECS.update(WALK_SPECS)
EXACT_NAMES = tuple(k + "/x" for k in SPECS)
SPECS.update({k + "/x": dict(v, exact=True, steered=False, coords="exact") for k, v in list(SPECS.items())})


def _steer(rng, c, x):
    """Fills the row groups of x [B, N, 192] in place -> {group: slice of points}."""
    assert c.n == sum(GROUP_SIZES)
    rows, at = {}, 0
    for g, k in zip(GROUPS, GROUP_SIZES):
        rows[g] = slice(at, at + k)
        at += k
    pinv = np.linalg.pinv(c.w1)                                       # [192, 96]: W1 pinv = 1
    mag_w = np.abs(c.w1)
    for s in range(c.b):
        k = GROUP_SIZES[1]
        want = -(0.5 + rng.random((k, M1))) - c.b1                    # W1 x = want: the pre-activation is in [-1.5, -0.5]
        x[s, rows["all_dead"]] = want @ pinv.T
        x0 = rng.standard_normal((k, K1))
        sign = rng.choice((-1.0, 1.0), (k, M1))
        for _ in range(3):                                            # (the magnitude moves with x: settle it)
            delta = 1e-3 * (np.abs(x0) @ mag_w.T + np.abs(c.b1)) * sign
            x0 = x0 - (x0 @ c.w1.T + c.b1 - delta) @ pinv.T
        x[s, rows["cancel"]] = x0
        x[s, rows["big"]] = 1e3 * rng.standard_normal((k, K1))
        hot = np.zeros((K1, K1))
        hot[np.arange(K1), (np.arange(K1) + 61 * s) % K1] = rng.choice((-1.0, 1.0), K1) * (1.0 + rng.random(K1))
        x[s, rows["one_hot"]] = hot
    return rows


@functools.lru_cache(maxsize=None)
def case(name):
    sp = SPECS[name]
    rng = np.random.default_rng(_seed("point_head/" + name))
    b, n, m3 = sp["b"], sp["n"], sp["m3"]
    c = types.SimpleNamespace(name=name, b=b, n=n, m3=m3, pitch=sp["pitch"], exact=sp["exact"], steered=sp["steered"], scale=SCALE)
    rn = rng.standard_normal
    if sp["exact"]:
        c.hg, c.wg = XH, XW
        c.w1, c.b1 = rng.integers(-2, 3, (M1, K1)) / 4.0, rng.integers(-8, 9, M1) / 4.0
        c.w2, c.b2 = rng.integers(-2, 3, (M2, M1)) / 4.0, rng.integers(-8, 9, M2) / 4.0
        c.w3, c.b3 = rng.integers(-2, 3, (m3, M2)) / 4.0, rng.integers(-8, 9, m3) / 4.0
        c.x = rng.integers(-3, 4, (b, n, K1)).astype(np.float64)
        c.grid = rng.integers(-3, 4, (b, XH, XW, 64)).astype(np.float64)
        # positions in halves from one cell outside to one cell outside; every ninth point a padding row
        pos = np.stack((rng.integers(-2, 2 * XH + 1, (b, n)), rng.integers(-2, 2 * XW + 1, (b, n))), -1) / 2.0
        pos[:, 4::9] = -500.0
        coord = np.empty((b, n, KG))
        coord[..., :2] = pos / np.asarray(SCALE)
        coord[..., 2] = rng.random((b, n))
        c.rows = {"all": slice(0, n)}
    else:
        c.hg, c.wg = HG, WG
        # the weight scales of tests/test_gpu_ops.py::test_point_head_against_float64_reference
        c.w1, c.b1 = _f32(0.1 * rn((M1, K1))), _f32(0.2 * rn(M1))
        c.w2, c.b2 = _f32(0.15 * rn((M2, M1))), _f32(0.2 * rn(M2))
        c.w3, c.b3 = _f32(0.2 * rn((m3, M2))), _f32(rn(m3))
        x = rn((b, n, K1))
        c.rows = _steer(rng, c, x) if sp["steered"] else {"randn": slice(0, n)}
        c.x = _f32(x)
        c.grid = _f32(rn((b, HG, WG, 64)))
        if sp["coords"] == "special":
            coord = gather_cases.gather_coords(rng, b, n, SCALE, special=True)
        else:
            coord = np.empty((b, n, KG))
            coord[..., :2] = gather_cases.interior_coords(rng, (b, n), SCALE)
            coord[..., 2] = rng.random((b, n))
    c.gcoord = _f32(coord)
    c.S, c.A = gather_cases.gather_ref(c.grid, c.gcoord, SCALE)
    c.ref = {f: head_ref(c, x_of(c, f)) for f in FORMS}
    c.lim = {f: bound(c, f) for f in FORMS}
    if sp["exact"]:
        iy, ix = gather_cases.ops_np.bilinear_pixel_coords(c.gcoord[..., :2], SCALE, XH, XW)
        assert np.array_equal(iy * 2, np.round(iy * 2)) and np.array_equal(ix * 2, np.round(ix * 2)), name
        for f in FORMS:
            assert exact_condition(c, f), (name, f)
    if sp["steered"]:
        z1 = c.x @ c.w1.T + c.b1
        mag = np.abs(c.x) @ np.abs(c.w1).T + np.abs(c.b1)
        assert (z1[:, c.rows["all_dead"]] < -0.25).all() and (F1 * mag[:, c.rows["all_dead"]] < 0.01).all(), name
        const = relu(c.b2) @ c.w3.T + c.b3
        assert np.allclose(c.ref["rows"][:, :, c.rows["all_dead"]], const[None, :, None], rtol=0, atol=1e-12), name
        r = np.abs(z1[:, c.rows["cancel"]]) / mag[:, c.rows["cancel"]]
        assert 5e-4 < r.min() and r.max() < 2e-3, (name, r.min(), r.max())
        assert ((c.x[:, c.rows["one_hot"]] != 0).sum(-1) == 1).all() and ((c.x[:, c.rows["one_hot"]] != 0).sum(1) == 1).all(), name
    if sp["coords"] == "interior":
        # the gathered rows of the tiles that one lane column meets are pairwise different: a tile computed from another
        # tile's coordinates cannot coincide
        flat = c.S.reshape(b * n, 64)
        assert len(np.unique(flat, axis=0)) == b * n and gather_cases.taps(c.gcoord, SCALE, HG, WG)[3].all(), name
    return _freeze(c)


def x_of(c, form, mag=False):
    """The 192 input channels [B, N, 192] of a form; mag: their magnitudes (A for the gathered third)."""
    x = np.abs(c.x) if mag else c.x
    if form == "rows":
        return x
    return np.concatenate((x[..., :64], c.A if mag else c.S, x[..., 128:]), -1)


def head_ref(c, x, mutant=None):
    """x [B, N, 192] float64 -> logits [B, M3, N].  Mutants of the chain: see MUTANTS."""
    if mutant == "drop_last_kstep":                   # k-step 32 t + 31 of third t = 1: channels 64 t + 31 and 64 t + 63
        x = x.copy()
        x[..., [64 + 31, 64 + 63]] = 0.0
    z1 = x @ c.w1.T + c.b1
    h1 = relu(z1)
    if mutant == "relu_missing":
        h1[..., 37] = z1[..., 37]
    if mutant == "swap_l2":                           # group of 8 at channel 40: accumulator order pairs (0, 4), natural order (0, 1)
        h1[..., [41, 44]] = h1[..., [44, 41]]
    h2 = relu(h1 @ c.w2.T + c.b2)
    acc = h2 @ c.w3.T
    b3 = c.b3
    if mutant == "b3_xor4":
        b3p = np.zeros(32)
        b3p[:c.m3] = c.b3
        b3 = b3p[np.arange(c.m3) ^ 4]
    out = acc + b3
    if mutant == "rows16_half0":
        ch = np.arange(c.m3)
        out = out[..., np.where(ch >= 16, ch & ~4, ch)]
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def stale_coords(c):
    """The coordinates a lane would use if tile t (of the B * ceil(N / 32) tiles) took those of tile t - 1 (tile 0: its own)."""
    tiles = -(-c.n // 32)
    out = np.array(c.gcoord)
    for s in range(c.b):
        for nn in range(c.n):
            lt = max(s * tiles + nn // 32 - 1, 0)
            bb, n2 = lt // tiles, (lt % tiles) * 32 + nn % 32
            out[s, nn] = c.gcoord[bb, n2 if n2 < c.n else 0]
    return out


# name -> (case, form)
MUTANTS = {"swap_l2": ("n70_m20", "rows"), "relu_missing": ("n33_m9", "rows"), "drop_last_kstep": ("n300_m3", "rows"),
           "rows16_half0": ("n70_m32", "gather"), "b3_xor4": ("n32_m8", "rows"), "stale_coord": ("n70_m20", "gather")}


def mutant_out(mutant):
    name, form = MUTANTS[mutant]
    c = case(name)
    if mutant == "stale_coord":
        s, _ = gather_cases.gather_ref(c.grid, stale_coords(c), SCALE)
        return head_ref(c, np.concatenate((c.x[..., :64], s, c.x[..., 128:]), -1))
    return head_ref(c, x_of(c, form), mutant)


def _layers_mag(c, form):
    """(|W1| |x| + |b1|, |W2| relu(z1) + |b2|, |W3| relu(z2) + |b3|), [B, N, .] each."""
    x = x_of(c, form)
    h1 = relu(x @ c.w1.T + c.b1)
    h2 = relu(h1 @ c.w2.T + c.b2)
    return (x_of(c, form, mag=True) @ np.abs(c.w1).T + np.abs(c.b1), h1 @ np.abs(c.w2).T + np.abs(c.b2),
            h2 @ np.abs(c.w3).T + np.abs(c.b3))


def bound(c, form):
    m1, m2, m3 = _layers_mag(c, form)
    e1 = F1 * m1
    if form == "gather":
        e1 = e1 + (1.0 + F1) * gather_cases.bound(c.A) @ np.abs(c.w1[:, 64:128]).T
    e2 = (1.0 + F2) * e1 @ np.abs(c.w2).T + F2 * m2
    e3 = (1.0 + F3) * e2 @ np.abs(c.w3).T + F3 * m3
    return np.ascontiguousarray(e3.transpose(0, 2, 1))


def exact_condition(c, form):
    """Sufficient for every partial sum of the three layers (and of the tap sum) to be a float32 number on the case's data."""
    for a in (c.x, c.grid, c.w1 * 4, c.w2 * 4, c.w3 * 4, c.b1 * 4, c.b2 * 4, c.b3 * 4, c.S * 4):
        if not np.array_equal(a, np.round(a)):
            return False
    d = 4.0 if form == "rows" else 16.0
    if c.A.max() * 4.0 >= 2.0 ** 24:
        return False
    for m in _layers_mag(c, form):
        if m.max() * d >= 2.0 ** 24:
            return False
        d *= 4.0
    return True


# ---------------------------------------------------------------------------------------------
# float32 restatement
# ---------------------------------------------------------------------------------------------
_fma32 = tfusion_cases._fma32


def _chain(acc, x, w, order):
    """acc [P, O] float32 += over the k-steps of `order` [steps, 2]: two rounded fmas per step (h = 0, then h = 1)."""
    for s in range(order.shape[0]):
        for h in range(2):
            k = order[s, h]
            acc = _fma32(acc, x[:, k:k + 1], w[None, :, k])
    return acc


def head_f32(c, form):
    """The kernel's order in float32 -> logits [B, M3, N] float32."""
    x = c.x.astype(F32)
    if form == "gather":
        x = np.concatenate((x[..., :64], gather_cases.emulate_f32(c.grid, c.gcoord, SCALE, fused=True), x[..., 128:]), -1)
    x = x.reshape(c.b * c.n, K1)
    w1, w2, w3 = c.w1.astype(F32), c.w2.astype(F32), c.w3.astype(F32)
    z1 = _chain(np.broadcast_to(c.b1.astype(F32), (x.shape[0], M1)).copy(), x, w1, k_order())
    h1 = np.where(z1 > 0, z1, F32(0))
    z2 = _chain(np.broadcast_to(c.b2.astype(F32), (x.shape[0], M2)).copy(), h1, w2, acc_order(48))
    h2 = np.where(z2 > 0, z2, F32(0))
    out = _chain(np.zeros((x.shape[0], c.m3), dtype=F32), h2, w3, acc_order(32)) + c.b3.astype(F32)
    assert out.dtype == F32
    return np.ascontiguousarray(out.reshape(c.b, c.n, c.m3).transpose(0, 2, 1))


@functools.lru_cache(maxsize=None)
def restatement(name, form):
    out = head_f32(case(name), form)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# the prepared weight block (ops.point_head_prepare) walked on the host
# ---------------------------------------------------------------------------------------------
def walk_block(flat, m3, h1, h2):
    """flat: the prepared block (float64 view of it); h1 [96], h2 [64] -> (W2 h1 [64], W3 h2 [32]) by walking the A2 and A3
    blocks as the kernel does: k-step s, lane 32 h + m holds the weight of output row m (of tile mt) and channel
    acc_order[s, h]."""
    a2 = flat[A1_FLOATS:A1_FLOATS + A2_FLOATS].reshape(2, 48, 2, 32)                 # (mt, s, h, m)
    a3 = flat[A1_FLOATS + A2_FLOATS:A1_FLOATS + A2_FLOATS + A3_FLOATS].reshape(32, 2, 32)
    o2, o3 = acc_order(48), acc_order(32)
    return np.einsum("tshm,sh->tm", a2, h1[o2]).reshape(64), np.einsum("shm,sh->m", a3, h2[o3])


# ---------------------------------------------------------------------------------------------
# walks under the grid cap
# ---------------------------------------------------------------------------------------------
def launch_honours_cap():
    """(point_head, tta_argmax): the launch takes its block count from conv_grid_cap(...).  Read from the sources, the one
    place where a test can see it (the results do not depend on the grid): a walk test computes its trips with the cap only
    where the launch has it, and fails its own trip count otherwise."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "streammos_amd", "csrc")
    with open(os.path.join(csrc, "point_head.hip")) as f:
        head = f.read().split("static int launch_point_head")[1].split("static bool fits_int")[0]
    with open(os.path.join(csrc, "vote.hip")) as f:
        tta = f.read().split('extern "C" int smos_tta_argmax')[1]
    return ("blocks = conv_grid_cap(" in head and "dim3((unsigned)blocks)" in head,
            "hipLaunchKernelGGL(tta_argmax, dim3((unsigned)conv_grid_cap(grid_for(N)))" in tta)


def head_blocks(b, n, cus, cap):
    """launch_point_head's grid: min(ceil(B ceil(N / 32) / 8), CUs), capped (cap 0 / None: no cap)."""
    want = -(-(b * -(-n // 32)) // WAVES)
    g = min(want, cus)
    return min(g, cap) if cap else g


def walk_tiles(b, n, n_live, blocks):
    """-> per wave that has a tile, the list of (sample, tile in the sample) it takes."""
    live = n if n_live is None else min(max(n_live, 0), n)
    per = -(-live // 32)
    waves = blocks * WAVES
    return [[(lt // per, lt % per) for lt in range(v, b * per, waves)] for v in range(min(waves, b * per))]


def walk_facts(walks):
    """-> (most tiles of one wave, some wave's consecutive tiles lie in different samples)."""
    most = max((len(w) for w in walks), default=0)
    cross = any(w[i][0] != w[i + 1][0] for w in walks for i in range(len(w) - 1))
    return most, cross


# ---------------------------------------------------------------------------------------------
# tta_argmax
# ---------------------------------------------------------------------------------------------
def _tta(k, b, n, kind="randn"):
    return dict(k=k, b=b, n=n, kind=kind)


TTA_SPECS = {
    "k1_b1_n1": _tta(1, 1, 1), "k1_b2_n257": _tta(1, 2, 257), "k2_b2_n255": _tta(2, 2, 255), "k3_b4_n1000": _tta(3, 4, 1000),
    "k8_b5_n256": _tta(8, 5, 256), "k8_b1_n257": _tta(8, 1, 257), "k2_b5_n1": _tta(2, 5, 1),
    "k3_b5_n256_big": _tta(3, 5, 256, "big"), "k8_b4_n1000_big": _tta(8, 4, 1000, "big"), "k2_b1_n255_big": _tta(2, 1, 255, "big"),
    "k3_b4_n1000_ties": _tta(3, 4, 1000, "ties"), "k8_b5_n1000_ties": _tta(8, 5, 1000, "ties"), "k2_b2_n1000_ties": _tta(2, 2, 1000, "ties"),
}
TIE_POINTS = (0, 100, 255, 256, 257, 511, 512, 700, 998, 999)       # every trip of the grid-stride loop under a cap of one block
MAX_LEFT_OUT = 0.01


def left_out(c):
    """The share of a case's points that the gap rule leaves undecided."""
    return float((~c.decided).sum()) / c.n


def tta_bound(k, b):
    return (k + b + 2 + TTA_EXP_ULP) * U


def tta_ref(pred):
    """pred [B, K, N] float64 -> (prob [N, K], labels [N])."""
    e = np.exp(pred - pred.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).mean(0).T
    return np.ascontiguousarray(p), p.argmax(1)


def tta_f32(pred):
    """The kernel's order in float32 with numpy's float32 exp -> (prob [N, K] float32, labels [N])."""
    pred = np.asarray(pred).astype(F32)
    b, k, n = pred.shape
    acc = np.zeros((k, n), dtype=F32)
    for s in range(b):
        v = pred[s]
        mx = v.max(0)
        e = np.exp((v - mx).astype(F32))
        tot = np.zeros(n, dtype=F32)
        for j in range(k):
            tot = tot + e[j]
        acc = acc + e / tot
    m = acc / F32(b)
    assert m.dtype == F32 and e.dtype == F32
    return np.ascontiguousarray(m.T), m.argmax(0)                   # argmax: the first maximum, as `m > best` keeps it


@functools.lru_cache(maxsize=None)
def tta_case(name):
    sp = TTA_SPECS[name]
    rng = np.random.default_rng(_seed("tta/" + name))
    b, k, n = sp["b"], sp["k"], sp["n"]
    c = types.SimpleNamespace(name=name, b=b, k=k, n=n, kind=sp["kind"])
    pred = 3.0 * rng.standard_normal((b, k, n))
    c.ties = {}
    if sp["kind"] == "big":
        # classes at about 80 and about -80 (the same ones in every variant: with a choice per variant the float64 means tie
        # exactly too often): exp(v) overflows, exp(v - max) of the low ones flushes
        pred = pred + 80.0 * rng.choice((-1.0, 1.0), (1, k, n))
    pred = _f32(pred)
    if sp["kind"] == "ties":
        for i, p in enumerate(TIE_POINTS):
            if p >= n:
                continue
            width = 2 if k == 2 or i % 2 == 0 else 3
            cls = np.sort(rng.permutation(k)[:width]) if i % 3 else np.arange(k - width, k)
            pred[:, cls, p] = _f32(pred[:, :, p].max(1, keepdims=True) + 2.0)     # bitwise equal in every variant, and on top
            c.ties[p] = tuple(int(v) for v in cls)
    c.pred = pred
    c.prob, c.labels = tta_ref(pred)
    c.lim = tta_bound(k, b)
    top = np.sort(c.prob, axis=1)
    c.gap = top[:, -1] - top[:, -2] if k > 1 else np.ones(n)
    c.decided = c.gap > 2.0 * c.lim
    return _freeze(c)

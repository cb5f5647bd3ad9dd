"""The fused training loss (csrc/seg_loss.hip, ops.seg_loss): OHEM cross-entropy + lovasz_weight * Lovasz-softmax.  The float64
reference of value and gradient, a float32 restatement of the kernels' arithmetic, the error bounds and the case builder
shared by tests/test_host_seg_loss.py (no GPU) and tests/test_gpu_seg_loss.py.

Reference (``reference``): the logits are the float32 numbers the kernel reads; from there on everything is float64.  The
Lovasz coefficients come from the integer counts in closed form (with G the foreground total, F_i the foreground count
among the sorted elements 0..i, I_i = G - F_i, U_i = G + (i + 1 - F_i)):

    foreground  d_i = 1 / U_i            background  d_i = I_i / ((U_i - 1) * U_i)

which equals jac_i - jac_{i-1} of the reference's ``_lovasz_grad`` for every i, i = 0 included (I_{-1} = U_{-1} = G).  Ties
between equal errors (and equal CE values in the top-k) are broken by position: a stable sort.

Bounds.  u = 2^-24.  A = the largest |x_c - max x| of a position.

  softmax     x_c - m: one rounding, which the exponential turns into a relative error u * A; expf itself <= 2 u; C - 1
              additions; the reciprocal; the product.  Relative error of p_c:  rho = u * (2 A + C + 6); absolute error
              dp = rho * p_c + 2^-126 (float32 underflows where float64 does not: exp(-400) is 0 there).
  err_c       |[y == c] - p_c|: absolute error  delta = dp + u * err_c.
  CE          m + log(s) - x_y: s carries u * (2 A + C + 2); logf <= 2 u |log s|; the addition u |lse|; the subtraction
              u * ce.  delta_ce is their sum.
  value       the Lovasz extension is 1-Lipschitz in its errors with weights d_i >= 0, sum d_i = J <= 1: class c moves by at
              most max(delta) * J + 2 u L_c (d_i is rounded to float32 once; the products and sums are float64).  The mean CE
              moves by at most mean(delta_ce), the top-k mean by at most max(delta_ce); the result is rounded once.
  gradient    the coefficient of a position depends on its RANK, which is not continuous in the logits: two errors closer
              than 2 max(delta) may come out in either order in float32.  For every element the reference therefore
              returns, besides d, the interval [d_lo, d_hi] of the closed form over every rank and every foreground count
              the elements inside that window allow; where the whole window holds one exact value the order is the
              position order and the interval is the point d.  Likewise the top-k flag of an element within 2 max(delta_ce)
              of the k-th value, unless the values are exactly equal.  The per-element bound is the formula of
              smos_seg_loss_bwd differentiated term by term with these widths, plus u per float32 operation of the kernel
              (``grad_bound``).
Nothing in the bounds is tuned to what the kernel returns.
"""
import functools
import hashlib
import types

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126    # smallest normal float32: the absolute error of a result that underflows (or is flushed) in float32
TILE = 2048           # smos_seg_loss_tile(): elements per block of the scan kernels (the GPU test checks the number)
TOP_RATIO, TOP_WEIGHT, LOVASZ_WEIGHT = 0.2, 4.0, 3.0


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def top_k(n, top_ratio=TOP_RATIO):
    return max(int(top_ratio * n), 1)           # losses.ohem_cross_entropy


def closed_form(fg_sorted):
    """Lovasz coefficients of a sorted 0/1 foreground sequence from the integer counts, float64."""
    fg = np.asarray(fg_sorted).astype(np.int64)
    g = int(fg.sum())
    if g == 0 or fg.size == 0:
        return np.zeros(fg.shape, dtype=np.float64)
    f = np.cumsum(fg)
    u = (g + (np.arange(1, fg.size + 1) - f)).astype(np.float64)
    i = (g - f).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(fg == 1, 1.0 / u, i / ((u - 1.0) * u))


def _intervals(e, fg, tol):
    """Sorted errors e (descending), their foreground flags -> (d, d_lo, d_hi) per sorted element: the closed form, and its
    range over the orders that errors closer than tol allow."""
    d = closed_form(fg)
    n = e.size
    g = int(fg.sum())
    if g == 0 or n == 0:
        return d, d, d
    lo = np.searchsorted(-e, -(e + tol), side="left")
    hi = np.searchsorted(-e, -(e - tol), side="right") - 1
    pure = e[lo] == e[hi]                                    # one exact value in the window: position order decides
    fc = np.concatenate(([0], np.cumsum(fg)))
    f0 = fc[lo]
    nf = fc[hi + 1] - f0
    nb = (hi - lo + 1) - nf
    b0 = lo - f0
    gb = (g + b0).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        fg_lo, fg_hi = 1.0 / (gb + nb), 1.0 / gb
        bg_hi = (g - f0) / (gb * (gb + 1.0))
        bg_lo = np.maximum(g - f0 - nf, 0) / ((gb + nb - 1.0) * (gb + nb))
    d_lo = np.where(pure, d, np.where(fg == 1, fg_lo, bg_lo))
    d_hi = np.where(pure, d, np.where(fg == 1, fg_hi, bg_hi))
    return d, np.minimum(d_lo, d), np.maximum(d_hi, d)


def _flat(pred, target):
    """pred [B,C,P(,1)], target [B,P(,1)] -> x [n, C] float64, t [n] int64 in the kernel's position order b * P + p."""
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 4:
        pred = pred[..., 0]
    b, c, p = pred.shape
    return pred.transpose(0, 2, 1).reshape(b * p, c).astype(np.float64), target.reshape(b * p).astype(np.int64)


def reference(pred, target, top_ratio=TOP_RATIO, top_weight=TOP_WEIGHT, ignore_index=0, lovasz_weight=LOVASZ_WEIGHT):
    """-> namespace of float64 results: ohem, lovasz, value, grad [n, C] (for grad_out = 1), the bounds value_bound and
    grad_bound [n, C], and what the bounds are made of."""
    x, t = _flat(pred, target)
    n, c = x.shape
    k = top_k(n, top_ratio)
    valid = (t != ignore_index) & (t >= 0) & (t < c)
    y = np.where(valid, t, 0)
    m = x.max(1)
    a = x - m[:, None]
    e = np.exp(a)
    s = e.sum(1)
    p = e / s[:, None]
    lse = m + np.log(s)
    ce = np.where(valid, lse - x[np.arange(n), y], 0.0)
    onehot = (np.arange(c)[None, :] == y[:, None]) & valid[:, None]
    amax = np.abs(a).max(1)
    rho = U * (2.0 * amax + c + 6.0)
    delta_ce = np.where(valid, U * (2.0 * amax + c + 2.0) + 2.0 * U * np.abs(np.log(s)) + U * np.abs(lse) + U * np.abs(ce), 0.0)

    # OHEM: mean + top_weight * mean of the k largest; ties by position
    order = np.argsort(-ce, kind="stable")
    top = np.zeros(n, dtype=bool)
    top[order[:k]] = True
    ohem = ce.mean() + top_weight * ce[order[:k]].mean()
    top_open = np.zeros(n, dtype=bool)                         # whose flag float32 may decide the other way
    if k < n:
        hi_v, lo_v = ce[order[k - 1]], ce[order[k]]
        tol = 2.0 * delta_ce.max()
        if hi_v - lo_v <= tol:
            near = (ce >= lo_v - tol) & (ce <= hi_v + tol)
            if not (ce[near] == hi_v).all():
                top_open = near

    # Lovasz-softmax over the valid positions, classes present
    coef = np.zeros((c, n))
    width = np.zeros((c, n))
    class_loss, class_bound, present = [], [], []
    vidx = np.flatnonzero(valid)
    for cls in range(c):
        fg = onehot[vidx, cls].astype(np.int64)
        if fg.sum() == 0:
            continue
        err = np.abs(fg - p[vidx, cls])
        delta = rho[vidx] * p[vidx, cls] + TINY + U * err
        srt = np.argsort(-err, kind="stable")
        d, d_lo, d_hi = _intervals(err[srt], fg[srt], 2.0 * delta.max())
        coef[cls, vidx[srt]] = d
        width[cls, vidx[srt]] = np.maximum(d_hi - d, d - d_lo) + U * d
        loss = float((err[srt] * d).sum())
        present.append(cls)
        class_loss.append(loss)
        class_bound.append(delta.max() * d.sum() + 2.0 * U * loss)
    lovasz = sum(class_loss) / len(class_loss) if class_loss else 0.0
    value = ohem + lovasz_weight * lovasz
    value_bound = (delta_ce.mean() + top_weight * delta_ce.max() + (lovasz_weight * sum(class_bound) / len(class_bound) if class_bound else 0.0)
                   + 2.0 * U * abs(value))

    # gradient for grad_out = 1 and its bound
    w_ce = 1.0 / n + top_weight / k * top
    w_lov = lovasz_weight / len(present) if present else 0.0
    sgn = np.where(onehot, -1.0, 1.0)
    tc = sgn * coef.T * p                                       # [n, C]
    grad = w_ce[:, None] * (p - onehot) + w_lov * (tc - p * tc.sum(1, keepdims=True))
    grad = np.where(valid[:, None], grad, 0.0)
    dp = rho[:, None] * p + TINY
    pm = np.abs(p - onehot)
    b_ce = (top_weight / k * top_open)[:, None] * pm + w_ce[:, None] * dp + 6.0 * U * w_ce[:, None] * pm
    wt, ct = width.T, coef.T
    # sum_c s_c d_c p_c ([c == j] - p_j) = t_j - p_j * T: the widths of d, of p_c and of p_j, then u per operation on the
    # magnitudes the kernel actually adds (it forms t_j and p_j * T separately)
    tabs = ct * p
    b_lov = (wt * p + ct * dp) + p * (wt * p + ct * dp).sum(1, keepdims=True) + dp * tabs.sum(1, keepdims=True)
    b_lov = b_lov + 10.0 * U * (tabs + p * tabs.sum(1, keepdims=True))
    grad_bound = np.where(valid[:, None], b_ce + w_lov * b_lov + 2.0 * U * np.abs(grad), 0.0)
    return types.SimpleNamespace(n=n, c=c, k=k, ohem=float(ohem), lovasz=float(lovasz), value=float(value), grad=grad,
                                 value_bound=float(value_bound), grad_bound=grad_bound, coef=coef, top=top, top_open=top_open,
                                 present=present, valid=valid, p=p, ce=ce)


# ---- the kernels' arithmetic in float32 ------------------------------------------------------------------------------
ONE_BITS, INF_BITS = 0x3F800000, 0x7F800000


def sort_key(v, top):
    """seg_key of csrc/seg_loss.hip: float32 values -> the value field of the sort key (uint32): larger values first, NaN,
    Inf and anything above the segment's largest value clamped to its first key."""
    bits = np.asarray(v, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.uint32(top) - np.minimum(bits, np.uint32(top))


def key_value(key, top):
    return (np.uint32(top) - np.asarray(key, dtype=np.uint32)).view(np.float32)


def restate_f32(pred, target, top_ratio=TOP_RATIO, top_weight=TOP_WEIGHT, ignore_index=0, lovasz_weight=LOVASZ_WEIGHT):
    """The kernels step by step with numpy float32 (numpy's exp / log for the device's): prep, a stable sort of the 33-bit
    keys, the tile-free scan, finish, backward.  -> value (float32), grad [n, C] float32, the full keys [C + 1, n] uint64."""
    x64, t = _flat(pred, target)
    x = x64.astype(np.float32)
    n, c = x.shape
    k = top_k(n, top_ratio)
    f32 = np.float32
    with np.errstate(all="ignore"):
        valid = (t != ignore_index) & (t >= 0) & (t < c)
        y = np.where(valid, t, 0)
        m = x[:, 0].copy()
        for j in range(1, c):
            m = np.fmax(m, x[:, j])
        e = np.exp(x - m[:, None]).astype(f32)
        s = e[:, 0].copy()
        for j in range(1, c):
            s = (s + e[:, j]).astype(f32)
        inv = (f32(1.0) / s).astype(f32)
        p = (e * inv[:, None]).astype(f32)
        lse = (m + np.log(s).astype(f32)).astype(f32)
        ce = np.where(valid, (lse - x[np.arange(n), y]).astype(f32), f32(0.0)).astype(f32)
        onehot = (np.arange(c)[None, :] == y[:, None]) & valid[:, None]
        err = np.abs(onehot.astype(f32) - p).astype(f32)
    keys = np.empty((c + 1, n), dtype=np.uint64)
    for cls in range(c):
        low = np.where(valid, sort_key(err[:, cls], ONE_BITS), np.uint32(ONE_BITS + 1))
        keys[cls] = (np.uint64(cls) << np.uint64(31)) | low.astype(np.uint64)
    keys[c] = (np.uint64(c) << np.uint64(31)) | sort_key(ce, INF_BITS).astype(np.uint64)
    flat = keys.reshape(-1)
    order = np.argsort(flat, kind="stable")
    skeys, spos = flat[order].reshape(c + 1, n), (order % n).reshape(c + 1, n)
    assert ((skeys >> np.uint64(31)) == np.arange(c + 1, dtype=np.uint64)[:, None]).all()      # every segment holds its n keys
    coef = np.zeros((c + 1, n), dtype=f32)
    sums, present = [], 0
    for cls in range(c):
        low = (skeys[cls] & np.uint64(0x7FFFFFFF)).astype(np.uint32)
        ok = low <= ONE_BITS
        fg = ok & (y[spos[cls]] == cls) & valid[spos[cls]]
        d = np.where(ok, closed_form(fg), 0.0).astype(f32)              # the ignored tail adds neither foreground nor rank
        v = key_value(np.where(ok, low, np.uint32(ONE_BITS)), ONE_BITS)
        coef[cls, spos[cls]] = d
        if fg.any():
            present += 1
            sums.append(float((v.astype(np.float64) * d.astype(np.float64)).sum()))
    low = (skeys[c] & np.uint64(0x7FFFFFFF)).astype(np.uint32)
    v = key_value(low, INF_BITS).astype(np.float64)
    coef[c, spos[c][:k]] = 1.0
    with np.errstate(all="ignore"):
        inv_present = 1.0 / present if present else 0.0
        value = f32(ce.astype(np.float64).sum() / n + float(f32(top_weight)) * v[:k].sum() / k + float(f32(lovasz_weight)) * sum(sums) * inv_present)
        # backward, grad_out = 1
        w_mean, w_top = f32(1.0 / n), f32(float(f32(top_weight)) / k)
        w_lov = (f32(1.0) * f32(lovasz_weight) * f32(inv_present)).astype(f32)
        w_ce = (f32(1.0) * (w_mean + w_top * coef[c]).astype(f32)).astype(f32)
        tc = (np.where(onehot, -coef[:c].T, coef[:c].T) * p).astype(f32)
        tsum = tc[:, 0].copy()
        for j in range(1, c):
            tsum = (tsum + tc[:, j]).astype(f32)
        left = (w_ce[:, None] * (p - onehot.astype(f32)).astype(f32)).astype(f32)
        right = (w_lov * (tc - (p * tsum[:, None]).astype(f32)).astype(f32)).astype(f32)
        grad = np.where(valid[:, None], (left + right).astype(f32), f32(0.0)).astype(f32)
    return value, grad, keys


# ---- cases -----------------------------------------------------------------------------------------------------------
def worst_ratio(got_value, got_grad, ref, factor=1.0):
    """-> (inside the bounds, worst value error / bound, worst gradient error / bound).  got_grad [n, C] in position order;
    where a bound is 0 the error has to be 0 and a NaN is outside every bound."""
    ev = abs(float(got_value) - ref.value)
    eg = np.abs(np.asarray(got_grad, dtype=np.float64) - ref.grad)
    lim = factor * ref.grad_bound
    ok = bool(ev <= factor * ref.value_bound) and bool((eg <= lim).all())
    pos = lim > 0
    rv = ev / (factor * ref.value_bound) if ref.value_bound > 0 else (0.0 if ev == 0 else float("inf"))
    return ok, rv, (float((eg[pos] / lim[pos]).max()) if pos.any() else 0.0)


def grad_rows(grad):
    """[B,C,P(,1)] -> [n, C] in position order."""
    g = np.asarray(grad)
    if g.ndim == 4:
        g = g[..., 0]
    return g.transpose(0, 2, 1).reshape(-1, g.shape[1])


LOGITS = ("normal", "equal", "pm200", "ce_ties")
LABELS = ("random", "all_ignored", "one_valid", "absent", "last_tile_fg", "ignored_border")


def make_case(name, b, c, p, logits="normal", labels="random", ignore_index=0):
    """One case: pred [B, C, P, 1] float32 numbers, target [B, P, 1] int64, its float64 reference (computed once)."""
    rng = np.random.default_rng(_seed("seg_loss/" + name))
    n = b * p
    if logits == "normal":
        x = 2.0 * rng.standard_normal((b, c, p))
    elif logits == "equal":                                     # every key ties
        x = np.full((b, c, p), 0.5)
    elif logits == "pm200":                                     # p exactly 0 or 1, CE 0 or 400
        x = np.where(np.arange(c)[None, :, None] == rng.integers(0, c, (b, 1, p)), 200.0, -200.0)
    elif logits == "ce_ties":                                   # four distinct logit rows: CE ties across the k boundary
        rows = rng.standard_normal((4, c))
        x = rows[rng.integers(0, 4, (b, p))].transpose(0, 2, 1)
    else:
        raise ValueError(logits)
    other = [v for v in range(c) if v != ignore_index]
    if labels == "random":
        pool = np.array(sorted(set(range(c)) | {ignore_index}))
        t = pool[rng.integers(0, len(pool), (b, p))]
    elif labels == "all_ignored":
        t = np.full((b, p), ignore_index)
    elif labels == "one_valid":
        t = np.full((b, p), ignore_index)
        t.reshape(-1)[n // 2] = other[-1]
    elif labels == "absent":                                    # with ignore_index outside the classes: class 1 never occurs
        pool = np.array([v for v in other if v != 1] + [ignore_index])
        t = pool[rng.integers(0, len(pool), (b, p))]
    elif labels == "last_tile_fg":
        # no ignored position; class `fgc` on five positions whose error is the smallest of its segment (p = 0.98 there, 0.5
        # elsewhere): the foreground of that segment sits in the last tile alone
        fgc, bgc = other[-1], other[0]
        t = np.full((b, p), bgc)
        spots = rng.choice(n, size=min(5, n), replace=False)
        t.reshape(-1)[spots] = fgc
        x = 0.05 * rng.standard_normal((b, c, p)) - 8.0
        x[:, fgc] += 8.0
        x[:, bgc] += 8.0
        xv = x.transpose(0, 2, 1).reshape(n, c)                 # a copy: write back below
        xv[spots, fgc] += 4.0
        x = xv.reshape(b, p, c).transpose(0, 2, 1)
    elif labels == "ignored_border":
        # ignored positions on both sides of position TILE, and TILE + 1 valid ones: the valid prefix of every sorted
        # segment ends one element behind a tile border
        assert b == 1 and p == TILE + 42
        t = np.array(other)[rng.integers(0, len(other), (b, p))]
        t[0, TILE - 20:TILE + 21] = ignore_index
    else:
        raise ValueError(labels)
    case = types.SimpleNamespace(name=name, b=b, c=c, p=p, n=n, ignore_index=ignore_index, logits=logits, labels=labels)
    case.pred = np.ascontiguousarray(x, dtype=np.float32).reshape(b, c, p, 1)
    case.target = np.ascontiguousarray(t, dtype=np.int64).reshape(b, p, 1)
    case.ref = reference(case.pred, case.target, ignore_index=ignore_index)
    case.k = case.ref.k
    for v in (case.pred, case.target, case.ref.grad, case.ref.grad_bound, case.ref.coef):
        v.setflags(write=False)
    return case


SHAPE_P = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
TOPK_N = {1: 7, TILE - 1: 5 * (TILE - 1) + 2, TILE: 5 * TILE + 2, TILE + 1: 5 * (TILE + 1) + 2}      # k -> n with int(0.2 n) = k


@functools.lru_cache(maxsize=None)
def shape_case(b, c, p):
    return make_case("shape/%d/%d/%d" % (b, c, p), b, c, p)


@functools.lru_cache(maxsize=None)
def topk_case(k):
    case = make_case("topk/%d" % k, 1, 3, TOPK_N[k])
    assert case.k == k
    return case


# name -> (B, C, P, logits, labels, ignore_index)
STEERED = {
    "all_ignored": (2, 3, 300, "normal", "all_ignored", 0),
    "one_valid": (2, 3, 300, "normal", "one_valid", 0),
    "one_valid_c2": (1, 2, TILE + 3, "normal", "one_valid", 0),
    "three_present": (2, 3, 700, "normal", "random", 255),
    "absent": (2, 3, 700, "normal", "absent", 255),
    "last_tile_fg": (1, 3, 2 * TILE + 100, "normal", "last_tile_fg", 255),
    "ignored_border": (1, 3, TILE + 42, "normal", "ignored_border", 0),
    "equal": (2, 3, TILE + 77, "equal", "random", 0),
    "equal_c2": (1, 2, 515, "equal", "random", 255),
    "pm200": (2, 3, 1500, "pm200", "random", 0),
    "pm200_c2": (1, 2, 900, "pm200", "random", 255),
    "ce_ties": (1, 3, TILE + 300, "ce_ties", "random", 0),
}


@functools.lru_cache(maxsize=None)
def steered_case(name):
    b, c, p, logits, labels, ignore = STEERED[name]
    return make_case("steered/" + name, b, c, p, logits, labels, ignore)


def all_cases():
    for c in (2, 3):
        for b in (1, 2):
            for p in SHAPE_P:
                yield shape_case(b, c, p)
    for k in TOPK_N:
        yield topk_case(k)
    for name in STEERED:
        yield steered_case(name)

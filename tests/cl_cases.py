"""The channels-last glue kernels of csrc/cl_kernels.hip (bias_act_cl, downsample_epilogue_cl2, colsum_partial, gate_mlp, gate_mlp_wide,
gate_apply_cl, upsample_concat_cl): cases, float64 references, float32 restatements and derived per-element bounds shared by
tests/test_host_cl_reference.py (no GPU) and tests/test_gpu_cl_kernels.py.  The conventions of tests/util.py: float64 arrays whose
entries are float32 numbers, seeded by case name, built once (lru_cache), read-only.  Maps are [B, H, W, C] here (channels-last).

Bounds.  u = 2^-24, gamma(k) = k u / (1 - k u): k roundings in a row multiply a term by at most 1 + gamma(k) (Higham, Lemma 3.1).
Every bound counts the roundings of the kernel's expression and multiplies by the sum of the magnitudes of the terms an output is
made of; none is fitted to an output.  Each function's docstring states its count.

Conditions on the inputs, asserted by the builders so that the reference alone stays inside them: every gate has
|pre-sigmoid| <= 6 on all channels (the weights of the second layer are scaled down to get there), every case that ends in a ReLU
has between 5 % and 60 % of the reference's outputs clipped, every "neg" pool input has p <= -1 everywhere.  A builder that misses
a condition with the seed of its name tries name#1, name#2, ... (still a function of the name alone) and fails after 32.

Exact twins (exact=True, names ending in "_x"): integer maps in [-8, 8], HW a power of two, gate tables of small dyadic numbers -- every sum of the gate
chain is then exact in float32 in ANY order (asserted: magnitude / quantum < 2^24 at every stage), so the column sums equal the
float64 ones bit for bit and the gate differs from the reference by expf, one add and one reciprocal only."""
import functools
import types

import numpy as np

from tests.util import _f32, _freeze, _seed, upconv_dyadic, upconv_lerp

U = 2.0 ** -24
F32 = np.float32
PER = 512                      # pixels per chunk of colsum_partial
SLOPE = 0.01                   # LeakyReLU of act code 2
EXP_ULPS = 2                   # expf of the device library is documented at 1 ulp; 2 are allowed (one ulp = 2 u relative)


def gamma(k):
    return k * U / (1.0 - k * U)


def _build(name, make, ok):
    """make(rng) for the first of the seeds name, name#1, ... whose case passes ok()."""
    for k in range(32):
        c = make(np.random.default_rng(_seed("cl/" + name + ("#%d" % k if k else ""))))
        if ok(c):
            c.name, c.attempt = name, k
            return _freeze(c)
    raise AssertionError("cl case %s: no seed met the conditions on the inputs" % name)


def clipped_share(want):
    return float((np.asarray(want) == 0.0).mean())


def _relu_ok(want):
    return 0.05 <= clipped_share(want) <= 0.60


def worst_ratio(got, want, bound):
    """tests/util.py::msda_worst_ratio: every element takes part, a zero bound asks for a zero error, a NaN is outside."""
    from tests.util import msda_worst_ratio
    return msda_worst_ratio(got, want, bound)


# ---------------------------------------------------------------------------------------------
# bias_act_cl: out = act(x + bias + res)
# ---------------------------------------------------------------------------------------------
# name -> B, H, W, C, act, bias, residual
BIAS_ACT_CASES = {
    "c4_none": (3, 3, 5, 4, 0, True, True),
    "c4_relu": (3, 3, 5, 4, 1, True, True),
    "c4_leaky": (3, 3, 5, 4, 2, True, True),
    "c36_relu_nobias": (3, 3, 5, 36, 1, False, True),
    "c36_leaky_nores": (3, 3, 5, 36, 2, True, False),
    "c36_none_plain": (2, 7, 3, 36, 0, False, False),
    "c36_relu_plain": (2, 7, 3, 36, 1, False, False),
    "c128_none": (3, 5, 7, 128, 0, True, True),
    "c128_relu": (3, 5, 7, 128, 1, True, True),
    "c128_leaky": (3, 5, 7, 128, 2, True, True),
    "p1_c4_leaky": (1, 1, 1, 4, 2, True, True),
    "p1_c36_relu": (1, 1, 1, 36, 1, True, True),
    "p1_c128_none": (1, 1, 1, 128, 0, True, True),
    # the second trip of the grid-stride loop: 256 * 16 * 256 + 300 float4 items, a ragged last block
    "sweep": (1, 877, 1196, 4, 2, True, True),
}


def bias_act_ref(x, bias, res, act, dtype=np.float64, order="kernel", slope=SLOPE):
    """act(x + bias + res) in `dtype`.  order "kernel": (x + bias) + res as bias_act_cl writes it; "other": x + (bias + res)."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    b = None if bias is None else np.asarray(bias).astype(dt)
    r = None if res is None else np.asarray(res).astype(dt)
    if order == "kernel" or b is None or r is None:
        v = x
        if b is not None:
            v = v + b
        if r is not None:
            v = v + r
    else:
        v = x + (b + r)
    assert v.dtype == np.dtype(dtype)
    if act == 1:
        return np.maximum(v, dt(0))
    if act == 2:
        return np.where(v > 0, v, v * dt(slope))
    return v


def bias_act_bound(c):
    """gamma(2 + [LeakyReLU]) (|x| + |bias| + |res|): two adds, and the product with the slope on the negative side; the
    activations are 1-Lipschitz and the maximum is exact."""
    mag = np.abs(c.x) + (0 if c.bias is None else np.abs(c.bias)) + (0 if c.res is None else np.abs(c.res))
    return gamma(2 + (c.act == 2)) * mag


@functools.lru_cache(maxsize=None)
def bias_act_case(name):
    b, h, w, ch, act, has_bias, has_res = BIAS_ACT_CASES[name]

    def make(rng):
        c = types.SimpleNamespace(b=b, h=h, w=w, c=ch, act=act)
        c.x = _f32(rng.standard_normal((b, h, w, ch)))
        c.bias = _f32(rng.standard_normal(ch) * 0.5) if has_bias else None
        c.res = _f32(rng.standard_normal((b, h, w, ch))) if has_res else None
        c.want = bias_act_ref(c.x, c.bias, c.res, act)
        return c
    return _build("bias_act/" + name, make, lambda c: act != 1 or _relu_ok(c.want))


# ---------------------------------------------------------------------------------------------
# downsample_epilogue_cl2: out = relu(a + bias + max_pool2d(p, 3, stride, 1)), the pool padded with -inf
# ---------------------------------------------------------------------------------------------
DS_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (6, 5), (31, 17))
DS_CASES = {"s%d_%dx%d_c%d_%s" % (s, h, w, ch, v): (2, h, w, ch, s, v)
            for s in (1, 2) for (h, w) in DS_SIZES for ch in (4, 36) for v in ("neg", "signed")}
DS_CASES["sweep"] = (1, 877, 1196, 4, 1, "neg")          # 256 * 16 * 256 + 300 float4 outputs


def ds_out_size(n, stride):
    return (n + 2 - 3) // stride + 1


def pool_ref(p, stride, pad=-np.inf):
    """max over the 3x3 window at (ho * stride - 1, wo * stride - 1); a tap outside the map counts as `pad`."""
    b, h, w, c = p.shape
    ho, wo = ds_out_size(h, stride), ds_out_size(w, stride)
    wide = np.full((b, h + 2, w + 2, c), pad, dtype=p.dtype)
    wide[:, 1:-1, 1:-1] = p
    m = np.full((b, ho, wo, c), -np.inf, dtype=p.dtype)
    for ky in range(3):
        for kx in range(3):
            m = np.maximum(m, wide[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride])
    return m


def ds_ref(a, p, bias, stride, dtype=np.float64, order="kernel", pad=-np.inf):
    """relu(a + bias + pool).  "kernel": (a + pool) + bias as downsample_epilogue_cl2 writes it; "other": a + (pool + bias)."""
    dt = np.dtype(dtype).type
    a, p, bias = (np.asarray(v).astype(dt) for v in (a, p, bias))
    m = pool_ref(p, stride, dt(pad))
    v = (a + m) + bias if order == "kernel" else a + (m + bias)
    assert v.dtype == np.dtype(dtype)
    return np.maximum(v, dt(0))


def ds_bound(c):
    """gamma(2) (|a| + |pool| + |bias|): two adds; the maximum of the window and the ReLU are exact."""
    return gamma(2) * (np.abs(c.a) + np.abs(pool_ref(c.p, c.stride)) + np.abs(c.bias))


@functools.lru_cache(maxsize=None)
def ds_case(name):
    b, h, w, ch, stride, variant = DS_CASES[name]
    ho, wo = ds_out_size(h, stride), ds_out_size(w, stride)

    def make(rng):
        c = types.SimpleNamespace(b=b, h=h, w=w, c=ch, stride=stride, variant=variant, ho=ho, wo=wo)
        p = rng.standard_normal((b, h, w, ch))
        c.p = _f32(-1.0 - np.abs(p)) if variant == "neg" else _f32(p)
        c.a = _f32(rng.standard_normal((b, ho, wo, ch)))
        pre = c.a + pool_ref(c.p, stride)
        c.bias = _f32(rng.standard_normal(ch) * 0.3 - np.quantile(pre, 0.3))      # about 30 % of the outputs clipped
        c.want = ds_ref(c.a, c.p, c.bias, stride)
        return c

    def ok(c):
        return _relu_ok(c.want) and (variant != "neg" or bool((c.p <= -1.0).all()))
    return _build("ds/" + name, make, ok)


# ---------------------------------------------------------------------------------------------
# the ChannelAtt gate: column sums -> sigmoid(W2 relu(W1 (sum / HW + bias) + b1) + b2) -> relu((y + bias) * g + xres)
# ---------------------------------------------------------------------------------------------
GATE_WIDE_C = (32, 64, 128, 256)


def gate_wide_chunks(c):
    parts = 1024 // c
    return (1, 3, parts - 1, parts, 7 * parts, 7 * parts + 1, 8 * parts - 1, 8 * parts, 8 * parts + 1, 21 * parts + 3)


def gate_wide_crs(c):
    return (1, c // 4, 64)


def gate_wide_twin_chunks(c):
    parts = 1024 // c
    return (7 * parts + 1, 8 * parts + 1, 21 * parts + 3)


GATE_RES_C = (4, 8, 16, 32, 64, 128, 256)
GATE_RES_HW = {1: (1, 1), 7: (1, 7), 255: (15, 17), 511: (7, 73), 512: (16, 32), 513: (19, 27), 1061: (1, 1061)}
GATE_RES_TWINS = ((4, (16, 32)), (32, (32, 64)), (256, (16, 32)), (256, (32, 64)))       # (C, (H, W)): HW = 512 and 2048
GATE_APPLY_C = (4, 8, 128)      # gate_apply_cl is reached through the gate entry points only: C divides 1024


def chunk_sums_ref(y, per=PER):
    """y [B, HW, C] -> [B, ceil(HW / per), C]: the table colsum_partial leaves in the workspace."""
    b, hw, c = y.shape
    chunks = (hw + per - 1) // per
    return np.stack([y[:, k * per:(k + 1) * per].sum(1) for k in range(chunks)], 1)


def chunk_sums_bound(y, per=PER):
    """gamma(n) sum |y| over the n pixels of the chunk: at most n - 1 adds touch a term, in any order."""
    b, hw, c = y.shape
    chunks = (hw + per - 1) // per
    return np.stack([gamma(min(per, hw - k * per)) * np.abs(y[:, k * per:(k + 1) * per]).sum(1) for k in range(chunks)], 1)


def gate_ref(total, hw, bias, w1, b1, w2, b2, divisor=None):
    """total [B, C] = the column sums -> (gate, pre-sigmoid, hidden, mean), float64."""
    mean = total / float(hw if divisor is None else divisor) + bias
    hidden = np.maximum(mean @ w1.T + b1, 0.0)
    pre = hidden @ w2.T + b2
    return 1.0 / (1.0 + np.exp(-pre)), pre, hidden, mean


def logit(g):
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(g / (1.0 - g))


def table_sum_f32(table, threads, chains):
    """The float32 total of a [B, chunks, C] table in the order of gate_mlp (threads = 256, chains = 1) or gate_mlp_wide
    (threads = 1024, chains = 8): the chunks of a channel are dealt to parts = threads / C threads, thread `part` takes
    part, part + parts, ...; gate_mlp_wide adds them into eight chains (a main loop of eight at a time while
    k + 7 parts < chunks, then a tail into chain u & 7) that it joins as a tree; the parts are added in order."""
    t = np.asarray(table).astype(F32)
    b, chunks, c = t.shape
    parts = threads // c
    total = np.zeros((b, c), dtype=F32)
    for part in range(parts):
        s = np.zeros((chains, b, c), dtype=F32)
        k = part
        if chains == 8:
            while k + 7 * parts < chunks:
                for u in range(8):
                    s[u] += t[:, k + u * parts]
                k += 8 * parts
        u = 0
        while k < chunks:
            s[u % chains] += t[:, k]
            k += parts
            u += 1
        ps = s[0] if chains == 1 else ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))
        total = total + ps
    assert total.dtype == F32
    return total


def gate_f32(total, hw, bias, w1, b1, w2, b2, order="kernel"):
    """The gate from a float32 total.  "kernel": mean = t / HW + bias, the two dot products term by term from the bias on
    (product rounded, then added), 1 / (1 + exp(-pre)); "other": numpy's float32 matrix products."""
    total, bias, w1, b1, w2, b2 = (np.asarray(v).astype(F32) for v in (total, bias, w1, b1, w2, b2))
    mean = total / F32(hw) + bias
    if order == "kernel":
        h = np.broadcast_to(b1, (mean.shape[0], b1.shape[0])).copy()
        for k in range(w1.shape[1]):
            h += w1[None, :, k] * mean[:, k:k + 1]
        h = np.maximum(h, F32(0))
        pre = np.broadcast_to(b2, (mean.shape[0], b2.shape[0])).copy()
        for j in range(w2.shape[1]):
            pre += w2[None, :, j] * h[:, j:j + 1]
    else:
        h = np.maximum(mean @ w1.T + b1, F32(0))
        pre = h @ w2.T + b2
    g = F32(1) / (F32(1) + np.exp(-pre))
    assert g.dtype == F32 and pre.dtype == F32
    return g, pre


def gate_bound(c, terms=None, exact=None):
    """-> (bound on the gate, bound on log(g / (1 - g)) against the reference's pre-sigmoid value), [B, C] each.  The chain, in
    the manner of tests/util.py::msda_qp_bound, with A = the sum of the magnitudes of the summed terms and n their number:

      sum     n terms in any order: at most n - 1 adds touch a term (the extra zero operands of the kernels' chains add
              exactly)                                                                    e_s = gamma(n) A
      mean    one divide by HW (exact as a float32 below 2^24), one add of the bias     e_m = (e_s + gamma(2) |S|) / HW + u |bias|
      hidden  a dot product of C terms from b1 on: C products and C adds, at most C + 1 touch a term; ReLU is 1-Lipschitz
                                          e_h = |W1| e_m (1 + gamma(C + 1)) + gamma(C + 1) (|b1| + |W1| |mean|)
      pre     the same with Cr terms      e_p = |W2| e_h (1 + gamma(Cr + 1)) + gamma(Cr + 1) (|b2| + |W2| |hidden|)
      expf    E = exp(-pre) moves by the relative exp(e_p) - 1, and expf itself by EXP_ULPS ulp    rho = expm1(e_p) + 2 EXP_ULPS u
      1 + E, 1 / (.)   one rounding each; d g / g = (1 - g) dE / E                        e_g = g ((1 - g) rho + 2 u)
      logit   d logit = d g / (g (1 - g))                                                 e_l = rho + 2 u / (1 - g)

    The last two carry a factor 1 + 2^-10 for the second-order terms.  On an exact twin (or exact=True) every sum is exact
    and only the expf, add and reciprocal terms remain.  `terms` overrides n (a table made of float32 partial sums)."""
    n = c.terms if terms is None else terms
    exact = c.exact if exact is None else exact
    g, pre, hidden, mean = gate_ref(c.total, c.hw, c.bias, c.w1, c.b1, c.w2, c.b2)
    if exact:
        e_p = np.zeros_like(pre)
    else:
        cc, cr = c.w1.shape[1], c.w1.shape[0]
        e_s = gamma(n) * c.mag
        e_m = (e_s + gamma(2) * np.abs(c.total)) / c.hw + U * np.abs(c.bias)
        aw1, aw2 = np.abs(c.w1), np.abs(c.w2)
        e_h = (e_m @ aw1.T) * (1 + gamma(cc + 1)) + gamma(cc + 1) * (np.abs(c.b1) + np.abs(mean) @ aw1.T)
        e_p = (e_h @ aw2.T) * (1 + gamma(cr + 1)) + gamma(cr + 1) * (np.abs(c.b2) + np.abs(hidden) @ aw2.T)
    rho = np.expm1(e_p) + 2 * EXP_ULPS * U
    slack = 1.0 + 2.0 ** -10
    return g * ((1.0 - g) * rho + 2 * U) * slack, (rho + 2 * U / (1.0 - g)) * slack


def gate_apply_ref(y, bias, g, xres, dtype=np.float64, form="plain", mutant=None):
    """relu((y + bias) * g + xres); y, xres [B, HW, C], g [B, C].  float32 forms: "plain" rounds the product and the sum,
    "fma" rounds (y + bias) * g + xres once (computed in float64 and rounded: the 48-bit product is exact there).
    Mutants of the reference: "gate_first" applies the gate before the bias, "no_residual" omits xres."""
    dt = np.dtype(dtype).type
    y, bias, g, xres = (np.asarray(v).astype(dt) for v in (y, bias, g, xres))
    g = g[:, None, :]
    s = y + bias
    if mutant == "gate_first":
        v = (y * g + bias) + xres
    elif mutant == "no_residual":
        v = s * g
    elif form == "fma" and dt is F32:
        v = (s.astype(np.float64) * g.astype(np.float64) + xres.astype(np.float64)).astype(F32)
    else:
        v = s * g
        v = v + xres
    assert v.dtype == np.dtype(dtype)
    return np.maximum(v, dt(0))


def gate_apply_bound(y, bias, g, xres):
    """gamma(3) ((|y| + |bias|) |g| + |xres|).  Written out: s = y + b, p = s * g, o = p + r -- three roundings on the y and
    bias terms, one on xres.  Contracted into an fma: two and one.  The bound holds for both forms; the gate is the
    kernel's own, so nothing of the gate chain enters."""
    return gamma(3) * ((np.abs(y) + np.abs(bias)) * np.abs(g)[:, None, :] + np.abs(xres))


def _gate_weights(rng, c, cr):
    w1 = _f32(rng.standard_normal((cr, c)) / np.sqrt(c))
    b1 = _f32(rng.standard_normal(cr) * 0.3)
    w2 = _f32(rng.standard_normal((c, cr)) / np.sqrt(cr))
    b2 = _f32(rng.standard_normal(c) * 0.5)
    return w1, b1, w2, b2


def _finish_gate(c):
    """Scales the second layer until |pre-sigmoid| <= 6 (a power of two: the entries stay float32 numbers), keeps every sample's
    gate a function of the sums (a live hidden unit), and stores the reference."""
    mean = c.total / c.hw + c.bias
    if c.w1.shape[0] == 1 and not c.exact:                  # Cr = 1: lift b1 so that the one hidden unit is alive in every sample
        c.b1 = _f32(np.abs(mean @ c.w1.T).max() + 0.5 + 0 * c.b1)
    for _ in range(40):
        c.gate, c.pre, c.hidden, c.mean = gate_ref(c.total, c.hw, c.bias, c.w1, c.b1, c.w2, c.b2)
        if np.abs(c.pre).max() <= 6.0:
            break
        c.w2, c.b2 = c.w2 * 0.5, c.b2 * 0.5
    c.w2, c.b2 = _f32(c.w2), _f32(c.b2)
    c.gate, c.pre, c.hidden, c.mean = gate_ref(c.total, c.hw, c.bias, c.w1, c.b1, c.w2, c.b2)
    return c


def _gate_ok(c):
    alive = (c.hidden > 0).any(1).all() and (c.hidden > 0).mean() >= (0.25 if c.w1.shape[0] > 1 else 1.0)
    ok = np.abs(c.pre).max() <= 6.0 and alive and _relu_ok(c.want)
    if c.exact:
        ok = ok and _gate_chain_exact(c)
    return bool(ok)


def _quantum(a):
    """The largest power of two that divides every entry of a (entries are dyadic)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[a > 0]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = (mant & -mant).astype(np.float64)                 # lowest set bit of the 53-bit mantissa
    return float((low * 2.0 ** (e - 53.0)).min())


def _gate_chain_exact(c):
    """Sufficient for every partial sum of the chain to be a float32 number whatever the order: at each stage the sum of the
    magnitudes of the terms, over the common quantum of the terms, is below 2^24."""
    lim = 2.0 ** 24
    q_s = _quantum(c.terms_array)
    ok = c.mag.max() / q_s < lim
    q_m = min(q_s / c.hw, _quantum(c.bias))
    ok = ok and (np.abs(c.total) / c.hw + np.abs(c.bias)).max() / q_m < lim
    q_h = min(q_m * _quantum(c.w1), _quantum(c.b1))
    ok = ok and (np.abs(c.b1) + np.abs(c.mean) @ np.abs(c.w1).T).max() / q_h < lim
    q_p = min(q_h * _quantum(c.w2), _quantum(c.b2))
    ok = ok and (np.abs(c.b2) + np.abs(c.hidden) @ np.abs(c.w2).T).max() / q_p < lim
    return bool(ok)


def _exact_gate_weights(rng, c, cr):
    w1 = rng.integers(-1, 2, (cr, c)).astype(np.float64) * (rng.random((cr, c)) < 0.5)
    b1 = rng.integers(-8, 9, cr) / 4.0
    w2 = rng.integers(-1, 2, (c, cr)).astype(np.float64)
    b2 = rng.integers(-4, 5, c) / 4.0
    return w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def gate_wide_case(ch, chunks, cr, exact=False):
    """A synthetic table [3, chunks, C] (gate_mlp_wide does not tie `chunks` to HW: the table is its input), a different one per
    sample, over a 3 x 5 map y (4 x 4 on the exact twins) with its residual input."""
    b, (h, w) = 3, ((4, 4) if exact else (3, 5))

    def make(rng):
        c = types.SimpleNamespace(b=b, h=h, w=w, hw=h * w, c=ch, cr=cr, chunks=chunks, exact=exact, terms=chunks)
        if exact:
            c.table = rng.integers(-8, 9, (b, chunks, ch)).astype(np.float64)
            c.y = rng.integers(-8, 9, (b, h * w, ch)).astype(np.float64)
            c.xres = rng.integers(-8, 9, (b, h * w, ch)).astype(np.float64)
            c.bias = rng.integers(-32, 33, ch) / 16.0
            c.w1, c.b1, c.w2, c.b2 = _exact_gate_weights(rng, ch, cr)
        else:
            c.table = _f32(rng.standard_normal((b, chunks, ch)))
            c.y = _f32(rng.standard_normal((b, h * w, ch)))
            c.xres = _f32(rng.standard_normal((b, h * w, ch)))
            c.bias = _f32(rng.standard_normal(ch) * 0.5)
            c.w1, c.b1, c.w2, c.b2 = _gate_weights(rng, ch, cr)
        c.terms_array = c.table
        c.total, c.mag = c.table.sum(1), np.abs(c.table).sum(1)
        _finish_gate(c)
        c.want = gate_apply_ref(c.y, c.bias, c.gate, c.xres)
        return c
    return _build("gate_wide/c%d_k%d_r%d%s" % (ch, chunks, cr, "_x" if exact else ""), make, _gate_ok)


@functools.lru_cache(maxsize=None)
def gate_res_case(ch, h, w, exact=False):
    """colsum_partial + gate_mlp + gate_apply_cl (ops.channel_gate_residual_cl) on y [3, H*W, C]; Cr = max(C / 4, 1)."""
    b, cr = 3, max(ch // 4, 1)

    def make(rng):
        c = types.SimpleNamespace(b=b, h=h, w=w, hw=h * w, c=ch, cr=cr, exact=exact, terms=h * w)
        if exact:
            c.y = rng.integers(-8, 9, (b, h * w, ch)).astype(np.float64)
            c.xres = rng.integers(-8, 9, (b, h * w, ch)).astype(np.float64)
            c.bias = rng.integers(-32, 33, ch) / 16.0
            c.w1, c.b1, c.w2, c.b2 = _exact_gate_weights(rng, ch, cr)
        else:
            # a mean of its own per (sample, channel): the gate then depends on the sums through more than their noise
            c.y = _f32(rng.standard_normal((b, h * w, ch)) + rng.standard_normal((b, 1, ch)))
            c.xres = _f32(rng.standard_normal((b, h * w, ch)))
            c.bias = _f32(rng.standard_normal(ch) * 0.5)
            c.w1, c.b1, c.w2, c.b2 = _gate_weights(rng, ch, cr)
        c.terms_array = c.y
        c.table = chunk_sums_ref(c.y)
        c.table_bound = chunk_sums_bound(c.y)
        c.chunks = c.table.shape[1]
        c.total, c.mag = c.y.sum(1), np.abs(c.y).sum(1)
        _finish_gate(c)
        c.want = gate_apply_ref(c.y, c.bias, c.gate, c.xres)
        return c
    return _build("gate_res/c%d_%dx%d%s" % (ch, h, w, "_x" if exact else ""), make, _gate_ok)


def gate_case_from_table(c, table):
    """The gate step alone: case c's weights on a GIVEN table [B, chunks, C] of float32 numbers (the one a kernel left behind,
    or a restatement's) -- the summed terms are the table's `chunks` entries per channel, so the bound starts from them and is
    as tight as the step; the table itself is judged by chunk_sums_bound."""
    table = np.asarray(table, dtype=np.float64)
    t = types.SimpleNamespace(name=c.name + "/table", hw=c.hw, bias=c.bias, w1=c.w1, b1=c.b1, w2=c.w2, b2=c.b2, exact=False,
                              terms=table.shape[1], table=table, chunks=table.shape[1])
    t.total, t.mag = table.sum(1), np.abs(table).sum(1)
    t.gate, t.pre, t.hidden, t.mean = gate_ref(t.total, t.hw, t.bias, t.w1, t.b1, t.w2, t.b2)
    return t


def gate_case_from_map(y, hw, bias, w1, b1, w2, b2, terms):
    """The reference gate and its bound for a map that a kernel produced (y [B, HW, C], float32 numbers): the real-table
    tests.  terms = the roundings that may touch a pixel's term: the pixels of one table entry plus the table's chunks."""
    c = types.SimpleNamespace(hw=hw, bias=bias, w1=w1, b1=b1, w2=w2, b2=b2, exact=False, terms=terms)
    c.total, c.mag = y.sum(1), np.abs(y).sum(1)
    c.gate, c.pre, c.hidden, c.mean = gate_ref(c.total, hw, bias, w1, b1, w2, b2)
    return c


@functools.lru_cache(maxsize=None)
def real_table_weights(ch):
    """(bias, w1, b1, w2, b2) for the real-table tests, Cr = C / 4, the second layer at a quarter of _gate_weights' scale; the
    test asserts |pre-sigmoid| <= 6 on the map the convolution produced."""
    rng = np.random.default_rng(_seed("cl/real_table/%d" % ch))
    w1, b1, w2, b2 = _gate_weights(rng, ch, ch // 4)
    return _f32(rng.standard_normal(ch) * 0.5), w1, b1, _f32(w2 * 0.25), _f32(b2 * 0.25)


@functools.lru_cache(maxsize=None)
def gate_apply_case(ch):
    """gate_apply_cl alone: B = 3 and HW = 15 (no power of two: the sample index is p / HW), through a three-chunk table.
    The kernel has no entry of its own and both gate entries take the divisors of 1024 only (C = 36 is refused), hence C 4, 8
    and 128: C / 4 = 1, 2 and 32 float4 columns."""
    return gate_wide_case(ch, 3, max(ch // 4, 1)) if ch >= 32 else _small_gate_case(ch)


def _small_gate_case(ch):
    b, h, w, cr, chunks = 3, 3, 5, max(ch // 4, 1), 3

    def make(rng):
        c = types.SimpleNamespace(b=b, h=h, w=w, hw=h * w, c=ch, cr=cr, chunks=chunks, exact=False, terms=chunks)
        c.table = _f32(rng.standard_normal((b, chunks, ch)) * 4.0)
        c.y = _f32(rng.standard_normal((b, h * w, ch)))
        c.xres = _f32(rng.standard_normal((b, h * w, ch)))
        c.bias = _f32(rng.standard_normal(ch) * 0.5)
        c.w1, c.b1, c.w2, c.b2 = _gate_weights(rng, ch, cr)
        c.terms_array = c.table
        c.total, c.mag = c.table.sum(1), np.abs(c.table).sum(1)
        _finish_gate(c)
        c.want = gate_apply_ref(c.y, c.bias, c.gate, c.xres)
        return c
    return _build("gate_apply/c%d" % ch, make, _gate_ok)


@functools.lru_cache(maxsize=None)
def gate_apply_sweep_case():
    """The second trip of gate_apply_cl's grid-stride loop: B * HW * C / 4 = 4 * 262219 = 256 * 16 * 256 + 300 float4 items."""
    b, h, w, ch, chunks = 4, 299, 877, 4, 3

    def make(rng):
        c = types.SimpleNamespace(b=b, h=h, w=w, hw=h * w, c=ch, cr=1, chunks=chunks, exact=False, terms=chunks)
        c.table = _f32(rng.standard_normal((b, chunks, ch)) * h * w)
        c.y = _f32(rng.standard_normal((b, h * w, ch)))
        c.xres = _f32(rng.standard_normal((b, h * w, ch)))
        c.bias = _f32(rng.standard_normal(ch) * 0.5)
        c.w1, c.b1, c.w2, c.b2 = _gate_weights(rng, ch, 1)
        c.terms_array = c.table
        c.total, c.mag = c.table.sum(1), np.abs(c.table).sum(1)
        _finish_gate(c)
        c.want = gate_apply_ref(c.y, c.bias, c.gate, c.xres)
        return c
    return _build("gate_apply/sweep", make, _gate_ok)


# ---------------------------------------------------------------------------------------------
# upsample_concat_cl: bilinear (align_corners=True) resize of up to three sources to (Ho, Wo), concatenated along C
# ---------------------------------------------------------------------------------------------
# name -> B, (Ho, Wo), ((C, (Hs, Ws)), ...)
UP_CASES = {
    "identity_4": (2, (6, 7), ((4, (6, 7)),)),
    "three_8_12_4": (2, (16, 24), ((8, (16, 24)), (12, (8, 12)), (4, (4, 6)))),
    "row_36_4": (2, (1, 9), ((36, (1, 4)), (4, (1, 9)))),                    # Ho = 1
    "col_36_4": (2, (9, 1), ((36, (4, 1)), (4, (9, 1)))),                    # Wo = 1
    "from_1x1_4": (2, (7, 5), ((4, (1, 1)),)),
    "from_1x1_8_12_4": (2, (7, 5), ((8, (1, 1)), (12, (7, 5)), (4, (1, 1)))),
    "nondyadic_32_64_32": (2, (16, 23), ((32, (7, 10)), (64, (16, 23)), (32, (7, 10)))),
    "nondyadic_36_4": (2, (16, 23), ((36, (7, 10)), (4, (3, 23)))),
    "dyadic_36_4": (2, (9, 9), ((36, (5, 5)), (4, (3, 3)))),                 # ratios 1/2 and 1/4: the float32 weights are exact
    "down_8_12_4": (2, (5, 5), ((8, (9, 9)), (12, (5, 5)), (4, (17, 3)))),   # ratios 2 and 4 (a source larger than the output)
    # 2 * 299 * 877 * 8 / 4 = 256 * 16 * 256 + 300 float4 outputs
    "sweep": (2, (299, 877), ((4, (20, 30)), (4, (299, 877)))),
}


def up_one_ref(v, ho, wo, dtype=np.float64, order="kernel"):
    """v [B, Hs, Ws, C] -> [B, Ho, Wo, C].  float64: the rational source position (tests/util.py::upconv_lerp).  float32: the
    positions and weights as upsample_concat_cl computes them, and its sum h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11)
    ("kernel") or the four weight products first ("other")."""
    dt = np.dtype(dtype).type
    v = np.asarray(v).astype(dt)
    hs, ws = v.shape[1:3]
    y0, y1, wy0, wy1 = upconv_lerp(hs, ho, dt)
    x0, x1, wx0, wx1 = upconv_lerp(ws, wo, dt)
    wy0, wy1 = (np.asarray(a, dtype=dt)[None, :, None, None] for a in (wy0, wy1))
    wx0, wx1 = (np.asarray(a, dtype=dt)[None, None, :, None] for a in (wx0, wx1))
    v00, v01, v10, v11 = v[:, y0][:, :, x0], v[:, y0][:, :, x1], v[:, y1][:, :, x0], v[:, y1][:, :, x1]
    if order == "kernel":
        out = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11)
    else:
        out = ((wy0 * wx0) * v00 + (wy0 * wx1) * v01) + ((wy1 * wx0) * v10 + (wy1 * wx1) * v11)
    assert out.dtype == np.dtype(dtype)
    return out


def up_ref(srcs, ho, wo, dtype=np.float64, order="kernel"):
    return np.concatenate([up_one_ref(v, ho, wo, dtype, order) for v in srcs], -1)


def up_bound(srcs, ho, wo):
    """Per element of a source's channels: gamma(6) Bil(|v|) + P.

      6  the roundings that touch a term w_y w_x v: of 1 - frac for each of the two weights, of the two products and of the two
         adds (fewer where the compiler contracts a product and an add).  Bil(|v|) is the reference on |v|.
      P  tests/util.py::upconv_perturbation: the kernel's position r * dst with r = float(n_src - 1) / float(n_dst - 1) carries
         two roundings, |ds| <= 2 u (n_src - 1), and the interpolant is piecewise linear in s with slope <= 2 max|v|, across a
         source sample too: 4 u (n_src - 1) max|v| per axis whose ratio is not dyadic; 0 for dyadic ratios, size-1 axes and
         the identity.
    A source of the output's own size has weights 1 and 0 and every product exact: bound 0, the map comes back bit for bit."""
    out = []
    for v in srcs:
        hs, ws = v.shape[1:3]
        if (hs, ws) == (ho, wo):
            out.append(np.zeros(v.shape[:1] + (ho, wo) + v.shape[3:]))
            continue
        n = (0 if upconv_dyadic(hs, ho) else hs - 1) + (0 if upconv_dyadic(ws, wo) else ws - 1)
        out.append(gamma(6) * up_one_ref(np.abs(v), ho, wo) + 4.0 * U * n * np.abs(v).max())
    return np.concatenate(out, -1)


@functools.lru_cache(maxsize=None)
def up_case(name):
    b, (ho, wo), specs = UP_CASES[name]
    rng = np.random.default_rng(_seed("cl/up/" + name))
    c = types.SimpleNamespace(name=name, b=b, ho=ho, wo=wo, specs=specs)
    c.srcs = [_f32(rng.standard_normal((b, hs, ws, ch))) for ch, (hs, ws) in specs]
    for v in c.srcs:
        v.setflags(write=False)
    c.want = up_ref(c.srcs, ho, wo)
    c.bound = up_bound(c.srcs, ho, wo)
    return _freeze(c)


# ---------------------------------------------------------------------------------------------
# the workspace of the three-pass gate
# ---------------------------------------------------------------------------------------------
def gate_ws_floats(b, c, hw):
    """What smos_channel_gate_residual_cl requires: the partial table and the gate."""
    return b * c * ((hw + PER - 1) // PER + 1)


def engine_ws_floats(b, c, hw):
    """What BasicBlock.run (streammos_amd/engine.py) asks for."""
    return (hw // PER + 2) * b * c

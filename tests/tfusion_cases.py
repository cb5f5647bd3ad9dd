"""The temporal fusion kernels (csrc/tfusion.hip: tfusion_layer, tfusion_project with a bias; csrc/epilogue.hip: add_layer_norm):
the float64 reference, two float32 restatements, mutants of the reference, the steered row groups, the case tables and the weight
stream / parameter block restated, shared by tests/test_host_tfusion_reference.py (no GPU) and tests/test_gpu_tfusion.py.
numpy only.

Arrays.  Every array is a float64 array whose entries are float32 numbers, seeded by the case name, built once and read-only.

Reference (layer_ref), the float64 chain of one layer; LayerNorm with the biased variance and eps inside the root:

    q1 = LN1(query + Wo sampled + bo);  out = LN2(q1 + W2 relu(W1 q1 + b1) + b2);  qp_next = Wq out + bq

Why no per-element bound.  A first-order worst-case bound through Linear -> LayerNorm -> Linear -> ReLU -> Linear -> LayerNorm is
four orders of magnitude above what a correct float32 chain uses, and a kernel that is a fifth of the range wrong stays inside it.
The instrument is the RMS comparison of the conv family, taken PER ROW GROUP: a kernel's RMS error against float64 over the rows
of a group may be at most RMS_FACTOR = 2 times that of the float32 restatement in the kernel's own order (layer_f32), and its
largest error at most MAX_FACTOR times that RMS.  Both factors are margins for another summation order over the same number of
roundings.  MAX_FACTOR is measured between the two restatements, never against a kernel: tests/test_host_tfusion_reference.py
prints max|second restatement - ref| / RMS(kernel-order restatement - ref) per case and group; MAX_FACTOR is the worst of those
figures doubled and rounded up to a power of two.

layer_f32, the kernel's order read from csrc/tfusion.hip.  A 128-term dot product (output_proj, linear1, the projections): k
walks the eight 16-channel tiles t; inside a tile the four MFMAs r = 0..3 (TF_ROW_PAIR) cover channels 16 t + 4 q + r, q = 0..3,
and alternate between two accumulators (r even / r odd) that are added at the end.  linear2: one accumulator per output tile,
hidden tiles j in order, inside a tile r = 0..3, channels 16 j + 4 q + r.  The order of the four products inside one
v_mfma_f32_16x16x4_f32 is not specified by the ISA document: here it is an fma chain over q = 0..3 onto the accumulator (one
rounding per product; formed as float32(float64 sum), whose double rounding differs from an fma in rare ties).  LayerNorm: per
lane q the sum over t of (x0 + x1) + (x2 + x3), the four lanes as (s0 + s1) + (s2 + s3), times 1/128; then the centred squares
in the same shape; 1 / sqrt(v / 128 + eps); (x rstd) g + b without contraction (the compiler may contract; RMS_FACTOR covers it).
layer_f32_plain is the second restatement: numpy float32 matmul (BLAS order) and numpy's own float32 mean.

Row groups, 16 rows each, judged separately (a one-pass variance is invisible on zero-mean rows, a wrong eps on rows of variance 2):

    randn          sampled, query standard normal                                                      baseline
    small_var      pre-norm row = 3.0 + 0.02 N(0,1) (sampled = 0, bo = 0: the row is query); variance 4e-4 < eps1    eps1
    big_mean       100 + 0.5 N(0,1)                                                                    one-pass variance cancels
    const          every channel -7.25: variance exactly 0, q1 = beta1, the 16 output rows identical   zero variance
    ffn_small_var  query = 1e-5 N(0,1): q1 = beta1 + O(3e-4); b2 is steered (below) so that the second pre-norm row has a
                   variance below eps2                                                                  eps2

The steered cases use eps1 = 1e-3, eps2 = 1e-6 and bo = 0.  b2 steering: b2 = float32(0.5 + 5e-4 z - beta1 - W2 relu(W1 beta1 +
b1)), z a fixed normal vector -- the second pre-norm row of a q1 = beta1 token is then 0.5 + 5e-4 z (variance 2.5e-7) up to the
rounding of b2, the same in every channel but for z: a scaling of W2 alone cannot do this, the residual q1 carries beta1's spread.

Exact twins of the project cases, in the conv family's sense: activations integers in [-4, 4], weights k / 16 with |k| <= 8,
bias multiples of 1 / 8 in [-4, 4].  Every partial sum is a multiple of 1 / 16; (|x| @ |W|^T + |bias|) * 16 < 2^24 (asserted), so
every order is exact and the kernel must return float32(reference) bit for bit.

Bound of the random project cases: tests/util.py::tap_products_bound (Cin u |x| @ |W|^T) + PROJECT_BIAS_C u |bias|.  TF_EMIT adds
the bias with ONE float32 addition: the bias passes one rounding, + 1 for the second order = 2; the product terms pass that
rounding too, 64 + 1 + 1 = 66 <= Cin = 128, inside the first term.
"""
import functools
import hashlib
import types

import numpy as np

U = 2.0 ** -24
C = 128                    # d_model of the fusion
RMS_FACTOR = 2.0
MAX_FACTOR = 32.0          # measured worst 15.88 (tests/test_host_tfusion_reference.py: layer case hot_f64_j3, small_var, out) -> doubled, next power of two
MUTANT_MARGIN = 4.0
PROJECT_BIAS_C = 2.0
GROUP_ROWS = 16
GROUPS = ("randn", "small_var", "big_mean", "const", "ffn_small_var")
EPS_STEERED = (1e-3, 1e-6)
EPS_MODEL = (1e-5, 1e-5)
Q_SLICE, O_SLICE = (160, 16), (192, 32)       # (pitch, channel offset) of a pitched query / output


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def ratio(num, den):
    """num / den with 0 / 0 = 0 (both exact) and x / 0 = inf; a NaN numerator is inf."""
    if not np.isfinite(num):
        return float("inf")
    if num == 0.0:
        return 0.0
    return float("inf") if den == 0.0 else num / den


def figures(got, ref, rest, rows=slice(None)):
    """-> (RMS(got - ref) / RMS(rest - ref), max|got - ref| / RMS(rest - ref)) over `rows`."""
    e = np.asarray(got, dtype=np.float64)[rows] - ref[rows]
    base = rms(np.asarray(rest, dtype=np.float64)[rows] - ref[rows])
    with np.errstate(invalid="ignore"):
        worst = float(np.abs(e).max()) if np.isfinite(e).all() else float("inf")
    return ratio(rms(e) if np.isfinite(e).all() else float("inf"), base), ratio(worst, base)


# ---------------------------------------------------------------------------------------------
# float64 reference and its mutants
# ---------------------------------------------------------------------------------------------
def layer_norm_ref(x, g, b, eps):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * g + b


def relu(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.maximum(x, 0.0))


LAYER_MUTANTS = {          # name -> the group it is built for
    "eps_swapped": "small_var", "eps_one": "ffn_small_var", "eps_1e5": "small_var", "one_pass": "big_mean", "b1_late": "randn",
    "w2_shift_up": "randn", "w2_shift_down": "randn"}
ALN_MUTANTS = {"eps_1e5": "small_var", "one_pass": "big_mean"}


def hidden_ref(c, q1):
    return relu(q1 @ c.w1.T + c.b1)


def layer_ref(c, sampled=None, query=None, mutant=None):
    """-> (out [tokens, 128], qp_next [tokens, nq] or None) in float64.  Mutants: eps_swapped (norm1 gets eps2, norm2 eps1),
    eps_one (eps1 for both), eps_1e5 (1e-5 whatever was passed), b1_late (hidden tile j takes b1 of tile j + 1, cyclic),
    w2_shift_up / _down (hidden tile j meets W2's k-tile j + 1 / j - 1, cyclic)."""
    sampled = c.sampled if sampled is None else sampled
    query = c.query if query is None else query
    e1, e2 = c.eps
    if mutant == "eps_swapped":
        e1, e2 = e2, e1
    elif mutant == "eps_one":
        e2 = e1
    elif mutant == "eps_1e5":
        e1 = e2 = 1e-5
    b1, w2 = c.b1, c.w2
    if mutant == "b1_late":
        b1 = np.roll(b1, -16)
    elif mutant == "w2_shift_up":
        w2 = np.roll(w2, -16, axis=1)
    elif mutant == "w2_shift_down":
        w2 = np.roll(w2, 16, axis=1)
    with np.errstate(invalid="ignore"):
        q1 = layer_norm_ref(query + sampled @ c.wo.T + c.bo, c.g1, c.be1, e1)
        out = layer_norm_ref(q1 + relu(q1 @ c.w1.T + b1) @ w2.T + c.b2, c.g2, c.be2, e2)
        nxt = out @ c.wq.T + c.bq if c.nq else None
    return out, nxt


# ---------------------------------------------------------------------------------------------
# float32 restatements
# ---------------------------------------------------------------------------------------------
F32 = np.float32


def _fma32(acc, a, b):
    """float32(acc + a * b) with the product unrounded: a float64 product of two float32 numbers is exact."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(F32)


def dot_rows_f32(x, w):
    """x [n, 128] float32, w [O, 128] float32 -> [n, O]: TF_SLOT_ROW's order (two accumulators by the parity of r)."""
    acc = [np.zeros((x.shape[0], w.shape[0]), dtype=F32), np.zeros((x.shape[0], w.shape[0]), dtype=F32)]
    for t in range(x.shape[1] // 16):
        for r in range(4):
            for q in range(4):
                k = 16 * t + 4 * q + r
                acc[r & 1] = _fma32(acc[r & 1], x[:, k:k + 1], w[None, :, k])
    with np.errstate(invalid="ignore"):
        return acc[0] + acc[1]


def dot_cols_f32(h, w):
    """h [n, F] float32, w [O, F] float32 -> [n, O]: TF_SLOT_COL's order (one accumulator, hidden tiles in turn, r-major)."""
    acc = np.zeros((h.shape[0], w.shape[0]), dtype=F32)
    for j in range(h.shape[1] // 16):
        for r in range(4):
            for q in range(4):
                k = 16 * j + 4 * q + r
                acc = _fma32(acc, h[:, k:k + 1], w[None, :, k])
    return acc


def layer_norm_tiles_f32(x, g, b, eps):
    """layer_norm_tiles of csrc/tfusion.hip on x [n, 128] float32."""
    n = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        xt = x.reshape(n, 8, 4, 4)                                    # [token, tile t, lane quarter q, r]
        s = np.zeros((n, 4), dtype=F32)
        for t in range(8):
            s = s + ((xt[:, t, :, 0] + xt[:, t, :, 1]) + (xt[:, t, :, 2] + xt[:, t, :, 3]))
        mean = ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) * F32(1.0 / C)
        xc = xt - mean[:, None, None, None]
        v = np.zeros((n, 4), dtype=F32)
        for t in range(8):
            v = v + ((xc[:, t, :, 0] * xc[:, t, :, 0] + xc[:, t, :, 1] * xc[:, t, :, 1]) +
                     (xc[:, t, :, 2] * xc[:, t, :, 2] + xc[:, t, :, 3] * xc[:, t, :, 3]))
        rstd = F32(1.0) / np.sqrt(((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) * F32(1.0 / C) + F32(eps))
        out = (xc.reshape(n, C) * rstd[:, None]) * g + b
    assert out.dtype == F32
    return out


def layer_norm_plain_f32(x, g, b, eps, one_pass=False):
    """numpy's float32 mean (pairwise); one_pass: the variance as E[x^2] - mean^2 in float32 (the mutant)."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.mean(-1, keepdims=True, dtype=F32)
        if one_pass:
            v = np.maximum((x * x).mean(-1, keepdims=True, dtype=F32) - m * m, F32(0))
        else:
            v = ((x - m) * (x - m)).mean(-1, keepdims=True, dtype=F32)
        out = (x - m) / np.sqrt(v + F32(eps)) * g + b
    assert out.dtype == F32
    return out


def _w32(c):
    return types.SimpleNamespace(**{k: v.astype(F32) for k, v in vars(c).items() if isinstance(v, np.ndarray)})


def layer_f32(c, sampled=None, query=None):
    """The kernel's order -> (out, qp_next or None) float32."""
    w = _w32(c)
    sampled = w.sampled if sampled is None else np.asarray(sampled, dtype=F32)
    query = w.query if query is None else np.asarray(query, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        q1 = layer_norm_tiles_f32((dot_rows_f32(sampled, w.wo) + w.bo) + query, w.g1, w.be1, c.eps[0])
        hsum = dot_rows_f32(q1, w.w1) + w.b1
        h = np.where(hsum > 0, hsum, F32(0))                          # fmaxf(v, 0): a NaN gives 0
        out = layer_norm_tiles_f32((dot_cols_f32(h, w.w2) + w.b2) + q1, w.g2, w.be2, c.eps[1])
        nxt = dot_rows_f32(out, w.wq) + w.bq if c.nq else None
    assert out.dtype == F32 and (nxt is None or nxt.dtype == F32)
    return out, nxt


def layer_f32_plain(c, one_pass=False):
    """The second restatement: numpy float32 matmul, numpy's float32 mean.  one_pass: the float32 mutant of both norms."""
    w = _w32(c)
    with np.errstate(invalid="ignore", over="ignore"):
        q1 = layer_norm_plain_f32(w.query + (w.sampled @ w.wo.T + w.bo), w.g1, w.be1, c.eps[0], one_pass)
        h = np.maximum(q1 @ w.w1.T + w.b1, F32(0))
        out = layer_norm_plain_f32(q1 + (h @ w.w2.T + w.b2), w.g2, w.be2, c.eps[1], one_pass)
        nxt = out @ w.wq.T + w.bq if c.nq else None
    assert out.dtype == F32
    return out, nxt


def project_f32(x, w, bias):
    with np.errstate(invalid="ignore"):
        y = dot_rows_f32(np.asarray(x, dtype=F32), np.asarray(w, dtype=F32))
        return y if bias is None else y + np.asarray(bias, dtype=F32)


def project_f32_plain(x, w, bias):
    y = np.asarray(x, dtype=F32) @ np.asarray(w, dtype=F32).T
    return y if bias is None else y + np.asarray(bias, dtype=F32)


# ---------------------------------------------------------------------------------------------
# the weight stream and the parameter block (header of csrc/tfusion.hip; ops.TfusionLayer, ops.tfusion_pack_linear)
# ---------------------------------------------------------------------------------------------
def pairs(w):
    """w [O, K] -> [O / 16, K / 16, 64, 4]: pair (o, t), lane 16 q + m holding w[16 o + m][16 t + 4 q + 0..3]."""
    o, k = w.shape
    return np.asarray(w).reshape(o // 16, 16, k // 16, 4, 4).transpose(0, 2, 3, 1, 4).reshape(o // 16, k // 16, 64, 4)


def _pad_rows(w, rows):
    out = np.zeros((rows, w.shape[1]))
    out[:w.shape[0]] = w
    return out


def project_stream(w):
    """w [cout, 128] -> float32 stream: cout zero-padded to a multiple of 64, slot o = pairs (o, t = 0..7)."""
    return pairs(_pad_rows(w, (w.shape[0] + 63) // 64 * 64)).reshape(-1).astype(F32)


def layer_stream(c, wq_tail=None):
    """Slots of 8 pairs: output_proj o = 0..7 (slot = the 8 k-tiles of output tile o); linear1(0); then linear1(j + 1) (the
    tile's 8 k-tiles) and linear2(j) (hidden tile j as the k-tile of the 8 output tiles) alternating; linear2(last); then
    4 slots of the next projection, its rows beyond nq zero.  wq_tail: the mutant that fills those rows with a number."""
    slots = list(pairs(c.wo))
    p1, p2 = pairs(c.w1), pairs(c.w2)
    n_t = c.ffn // 16
    slots.append(p1[0])
    for j in range(n_t - 1):
        slots.append(p1[j + 1])
        slots.append(p2[:, j])
    slots.append(p2[:, n_t - 1])
    if c.nq:
        wq = _pad_rows(c.wq, 64)
        if wq_tail is not None:
            wq[c.nq:] = wq_tail
        slots.extend(pairs(wq))
    return np.stack(slots).reshape(-1).astype(F32)


def layer_params(c, bq_tail=0.0):
    """bo g1 be1 b1[ffn] b2 g2 be2 bq[64] (zero beyond nq)."""
    bq = np.full(64, bq_tail)
    if c.nq:
        bq[:c.nq] = c.bq
    return np.concatenate([c.bo, c.g1, c.be1, c.b1, c.b2, c.g2, c.be2, bq]).astype(F32)


def stream_slot_count(ffn, nq):
    return 8 + 2 * (ffn // 16) + (4 if nq else 0)


# ---------------------------------------------------------------------------------------------
# tfusion_layer cases
# ---------------------------------------------------------------------------------------------
def _lspec(ffn, nq, tokens=None, groups=None, eps=EPS_STEERED, qpitch=False, opitch=False, hot=None):
    return dict(ffn=ffn, nq=nq, tokens=tokens, groups=groups, eps=eps, qpitch=qpitch, opitch=opitch, hot=hot)


def _layer_specs():
    s = {}
    # token counts: one lane, a wave edge, a block edge, three blocks (items 5, 6)
    for i, t in enumerate((1, 15, 16, 17, 63, 64, 65, 129)):
        s["t%d" % t] = _lspec(512, 48, tokens=t, qpitch=i % 2 == 1, opitch=i % 3 == 2)
    # ffn: the pipeline's ends (32: no loop pass, 96: two), the parameter rounds of 2048 floats (n_prm = 832 + ffn: 1216 -> 2048,
    # 1248 -> 2080, 3264 -> 4096, 3296 -> 4128), the ABI's largest; nq and the pitches follow the row
    for i, (f, nq) in enumerate(((32, 4), (64, 20), (96, 0), (512, 48), (1216, 64), (1248, 48), (3264, 20), (3296, 4), (4096, 64))):
        s["f%d" % f] = _lspec(f, nq, groups=GROUPS, qpitch=i % 2 == 0, opitch=i % 3 != 1)
    s["f512_model_eps"] = _lspec(512, 48, groups=GROUPS, eps=EPS_MODEL)
    # one live hidden tile
    for f in (32, 64, 96):
        n_t = f // 16
        for j in sorted({0, 1, n_t - 2, n_t - 1}):
            s["hot_f%d_j%d" % (f, j)] = _lspec(f, 48, groups=("randn", "small_var"), hot=j, opitch=j % 2 == 1)
    return s


LAYER_SPECS = _layer_specs()


@functools.lru_cache(maxsize=None)
def layer_case(name):
    sp = LAYER_SPECS[name]
    rng = np.random.default_rng(_seed("tfusion/layer/" + name))
    ffn, nq = sp["ffn"], sp["nq"]
    groups = sp["groups"] or ("randn",)
    steered = sp["groups"] is not None
    tokens = GROUP_ROWS * len(groups) if steered else sp["tokens"]
    c = types.SimpleNamespace(name=name, ffn=ffn, nq=nq, tokens=tokens, eps=sp["eps"], qpitch=sp["qpitch"], opitch=sp["opitch"],
                              hot=sp["hot"], steered=steered)
    c.rows = {g: slice(GROUP_ROWS * i, GROUP_ROWS * (i + 1)) for i, g in enumerate(groups)} if steered else {"randn": slice(0, tokens)}
    n = rng.standard_normal
    c.wo = _f32(n((C, C)) / C ** 0.5)
    c.bo = np.zeros(C) if steered else _f32(0.3 * n(C))
    c.g1, c.be1 = _f32(1.0 + 0.3 * n(C)), _f32(0.2 * n(C))
    c.w1, c.b1 = _f32(n((ffn, C)) / C ** 0.5), _f32(0.3 * n(ffn))
    if sp["hot"] is not None:
        b1 = np.full(ffn, -1e4)
        b1[16 * sp["hot"]:16 * sp["hot"] + 16] = c.b1[16 * sp["hot"]:16 * sp["hot"] + 16] + 0.5
        c.b1 = b1
    c.w2 = _f32(n((C, ffn)) / ffn ** 0.5)
    c.g2, c.be2 = _f32(1.0 + 0.3 * n(C)), _f32(0.2 * n(C))
    z = n(C)
    if "ffn_small_var" in groups or "const" in groups:
        c.b2 = _f32(0.5 + 5e-4 * z - c.be1 - relu(c.w1 @ c.be1 + c.b1) @ c.w2.T)
    else:
        c.b2 = _f32(0.3 * z)
    c.wq, c.bq = (_f32(n((nq, C)) / C ** 0.5), _f32(0.3 * n(nq))) if nq else (None, None)
    sampled, query = np.zeros((tokens, C)), np.zeros((tokens, C))
    for g, rows in c.rows.items():
        k = rows.stop - rows.start
        if g == "randn":
            sampled[rows], query[rows] = n((k, C)), n((k, C))
        elif g == "small_var":
            query[rows] = 3.0 + 0.02 * n((k, C))
        elif g == "big_mean":
            query[rows] = 100.0 + 0.5 * n((k, C))
        elif g == "const":
            query[rows] = -7.25
        elif g == "ffn_small_var":
            query[rows] = 1e-5 * n((k, C))
    c.sampled, c.query = _f32(sampled), _f32(query)
    c.ref, c.ref_next = layer_ref(c)
    if steered and "small_var" in groups:
        pre = c.query + c.sampled @ c.wo.T + c.bo
        assert pre[c.rows["small_var"]].var(-1).max() < c.eps[0] or c.eps != EPS_STEERED
    if "const" in groups:
        assert (c.query[c.rows["const"]].var(-1) == 0).all()
    if "ffn_small_var" in groups and c.eps == EPS_STEERED:
        q1 = layer_norm_ref(c.query + c.sampled @ c.wo.T + c.bo, c.g1, c.be1, c.eps[0])
        pre2 = q1 + hidden_ref(c, q1) @ c.w2.T + c.b2
        assert pre2[c.rows["ffn_small_var"]].var(-1).max() < c.eps[1], pre2[c.rows["ffn_small_var"]].var(-1).max()
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def layer_restatement(name):
    out, nxt = layer_f32(layer_case(name))
    out.setflags(write=False)
    if nxt is not None:
        nxt.setflags(write=False)
    return out, nxt


# ---------------------------------------------------------------------------------------------
# add_layer_norm cases
# ---------------------------------------------------------------------------------------------
ALN_GROUPS = ("randn", "small_var", "big_mean", "const")


def _aln_specs():
    s = {}
    for ch in (64, 128, 256, 512):
        for res in (False, True):
            s["c%d%s" % (ch, "_res" if res else "")] = dict(ch=ch, res=res, rows=None, eps=1e-3)
    # four waves per block: 4 and 5 rows straddle a block; 1000 rows: 250 blocks
    for i, (r, ch) in enumerate(((1, 128), (3, 64), (4, 256), (5, 512), (1000, 128))):
        s["r%d_c%d" % (r, ch)] = dict(ch=ch, res=i % 2 == 0, rows=r, eps=1e-5)
    return s


ALN_SPECS = _aln_specs()


def aln_ref(c, mutant=None):
    x = c.x if c.res is None else c.x + c.res
    return layer_norm_ref(x, c.g, c.b, 1e-5 if mutant == "eps_1e5" else c.eps)


def aln_f32(c):
    """add_layer_norm of csrc/epilogue.hip: lane l holds channels k 64 + l; sums over k in turn, then the xor butterfly 32 .. 1."""
    def wave_sum(v):                                   # [n, kper, 64] -> [n]
        s = np.zeros((v.shape[0], 64), dtype=F32)
        for k in range(v.shape[1]):
            s = s + v[:, k]
        w = 32
        while w:
            s = s[:, :w] + s[:, w:2 * w]
            w >>= 1
        return s[:, 0]
    x = c.x.astype(F32) + (F32(0) if c.res is None else c.res.astype(F32))
    n, ch = x.shape
    v = x.reshape(n, ch // 64, 64)
    mean = wave_sum(v) / F32(ch)
    d = v - mean[:, None, None]
    rstd = F32(1) / np.sqrt(wave_sum(d * d) / F32(ch) + F32(c.eps))
    out = (d.reshape(n, ch) * rstd[:, None]) * c.g.astype(F32) + c.b.astype(F32)
    assert out.dtype == F32
    return out


def aln_f32_plain(c, one_pass=False):
    x = c.x.astype(F32) + (F32(0) if c.res is None else c.res.astype(F32))
    return layer_norm_plain_f32(x, c.g.astype(F32), c.b.astype(F32), c.eps, one_pass)


@functools.lru_cache(maxsize=None)
def aln_case(name):
    sp = ALN_SPECS[name]
    rng = np.random.default_rng(_seed("tfusion/aln/" + name))
    ch, n = sp["ch"], rng.standard_normal
    groups = ALN_GROUPS if sp["rows"] is None else ("randn",)
    rows_n = GROUP_ROWS * len(groups) if sp["rows"] is None else sp["rows"]
    c = types.SimpleNamespace(name=name, ch=ch, eps=sp["eps"], n=rows_n)
    c.rows = {g: slice(GROUP_ROWS * i, GROUP_ROWS * (i + 1)) for i, g in enumerate(groups)} if sp["rows"] is None else {"randn": slice(0, rows_n)}
    want = np.zeros((rows_n, ch))
    for g, rows in c.rows.items():
        k = rows.stop - rows.start
        want[rows] = {"randn": lambda: n((k, ch)), "small_var": lambda: 3.0 + 0.02 * n((k, ch)),
                      "big_mean": lambda: 100.0 + 0.5 * n((k, ch)), "const": lambda: np.full((k, ch), -7.25)}[g]()
    if sp["res"]:
        c.x = rng.integers(-32, 33, (rows_n, ch)) / 8.0                 # x + res is the steered row up to one rounding; exact on const rows
        c.res = _f32(want - c.x)
    else:
        c.x, c.res = _f32(want), None
    c.g, c.b = _f32(1.0 + 0.3 * n(ch)), _f32(0.2 * n(ch))
    c.ref = aln_ref(c)
    if "const" in c.rows:
        assert ((c.x if c.res is None else c.x + c.res)[c.rows["const"]] == -7.25).all()
        assert np.array_equal(c.ref[c.rows["const"]], np.broadcast_to(c.b, (GROUP_ROWS, ch)))
    return _freeze(c)


# ---------------------------------------------------------------------------------------------
# tfusion_project with a bias: launches of jobs
# ---------------------------------------------------------------------------------------------
def _job(tokens, cout, bias=True, xpitch=False, wide=True):
    """wide: out is a column range of a wider NaN matrix"""
    return dict(tokens=tokens, cout=cout, bias=bias, xpitch=xpitch, wide=wide)


TOKEN_COUNTS = (1, 15, 16, 17, 63, 64, 65, 129)
PROJECT_SPECS = {
    # eight jobs: every token count (short jobs beside long ones: whole blocks leave early), with and without a bias
    "tok8": [_job(t, co, bias=i % 3 != 1, xpitch=i % 2 == 0, wide=i % 4 != 3)
             for i, (t, co) in enumerate(zip(TOKEN_COUNTS, (48, 4, 20, 100, 128, 48, 20, 4)))],
    # every cout: the store guard inside a tile (4, 20, 100), a partial last slot group (48, 100), the ABI's largest
    "cout6": [_job(70, co, xpitch=i % 2 == 1) for i, co in enumerate((4, 20, 48, 100, 128, 2048))],
    "mix3": [_job(1, 2048, xpitch=True), _job(65, 100, xpitch=True), _job(129, 20, xpitch=True)],
    "single_t1": [_job(1, 100)], "single_t17": [_job(17, 100, xpitch=True)], "single_t65": [_job(65, 100, wide=False)],
    "single_t129_nobias": [_job(129, 48, bias=False)],
}
PROJECT_NAMES = tuple(PROJECT_SPECS) + tuple(k + "/x" for k in PROJECT_SPECS)


@functools.lru_cache(maxsize=None)
def project_case(name):
    """-> list of jobs (x [tokens, 128], w [cout, 128], bias [cout] or None, ref [tokens, cout], mag, spec); name + "/x": the exact twin."""
    base, exact = (name[:-2], True) if name.endswith("/x") else (name, False)
    rng = np.random.default_rng(_seed("tfusion/project/" + name))
    jobs = []
    for sp in PROJECT_SPECS[base]:
        t, co = sp["tokens"], sp["cout"]
        j = types.SimpleNamespace(exact=exact, **sp)
        if exact:
            j.x = rng.integers(-4, 5, (t, C)).astype(np.float64)
            j.w = rng.integers(-8, 9, (co, C)) / 16.0
            j.b = rng.integers(-32, 33, co) / 8.0 if sp["bias"] else None
        else:
            j.x = _f32(rng.standard_normal((t, C)))
            j.w = _f32(rng.standard_normal((co, C)) / C ** 0.5)
            j.b = _f32(rng.standard_normal(co)) if sp["bias"] else None
        j.ref = j.x @ j.w.T + (0.0 if j.b is None else j.b)
        j.mag = np.abs(j.x) @ np.abs(j.w).T
        j.side = np.zeros(co) if j.b is None else np.abs(j.b)
        if exact:
            assert np.array_equal(j.x, np.round(j.x)) and np.array_equal(j.w * 16, np.round(j.w * 16))
            assert float((j.mag + j.side).max()) * 16 < 2.0 ** 24
        jobs.append(_freeze(j))
    return jobs


def project_bound(j):
    """Cin u |x| @ |W|^T (tests/util.py::tap_products_bound) + PROJECT_BIAS_C u |bias|"""
    return U * C * j.mag + PROJECT_BIAS_C * U * j.side


# ---------------------------------------------------------------------------------------------
# the engine's five launches on a small lattice
# ---------------------------------------------------------------------------------------------
CHAIN = dict(b=2, h=6, w=7, heads=4, points=4, ffn=512)


def _chain_layer(rng, nq_next):
    n = rng.standard_normal
    L = types.SimpleNamespace(name="chain", ffn=CHAIN["ffn"], nq=nq_next, eps=EPS_MODEL)
    L.wv, L.bv = _f32(n((C, C)) / C ** 0.5), _f32(0.3 * n(C))
    L.wo, L.bo = _f32(n((C, C)) / C ** 0.5), _f32(0.3 * n(C))
    L.g1, L.be1 = _f32(1.0 + 0.3 * n(C)), _f32(0.2 * n(C))
    L.w1, L.b1 = _f32(n((L.ffn, C)) / C ** 0.5), _f32(0.3 * n(L.ffn))
    L.w2, L.b2 = _f32(n((C, L.ffn)) / L.ffn ** 0.5), _f32(0.3 * n(C))
    L.g2, L.be2 = _f32(1.0 + 0.3 * n(C)), _f32(0.2 * n(C))
    return L


@functools.lru_cache(maxsize=None)
def chain_case():
    """src, query [B, H W, 128]; two layers; layer i's [offsets | logits] projection (wq, bq) lives with layer i - 1 as its `next`
    (layer 0's is the third job of the projection launch)."""
    rng = np.random.default_rng(_seed("tfusion/chain"))
    b, h, w, m, p = (CHAIN[k] for k in ("b", "h", "w", "heads", "points"))
    nq = m * p * 3
    c = types.SimpleNamespace(b=b, h=h, w=w, m=m, p=p, nq=nq, tokens=b * h * w)
    c.src, c.query = _f32(rng.standard_normal((b, h * w, C))), _f32(rng.standard_normal((b, h * w, C)))
    c.layers = [_chain_layer(rng, nq), _chain_layer(rng, 0)]
    c.wq0, c.bq0 = _f32(rng.standard_normal((nq, C)) / C ** 0.5), _f32(0.3 * rng.standard_normal(nq))
    c.layers[0].wq, c.layers[0].bq = _f32(rng.standard_normal((nq, C)) / C ** 0.5), _f32(0.3 * rng.standard_normal(nq))
    c.layers[1].wq = c.layers[1].bq = None
    for L in c.layers:
        _freeze(L)
    return _freeze(c)


def _sampler_problem(c, value, qp):
    from tests import util
    s = types.SimpleNamespace(n=c.b, h=c.h, w=c.w, m=c.m, p=c.p, s=c.h * c.w, d=32, l=1)
    s.shapes, s.lsi = util.msda_levels(((c.h, c.w),))
    s.value, s.qp = value.reshape(c.b, s.s, c.m, 32), qp.reshape(c.b, s.s, -1)
    return s


def chain_run(dtype):
    """The chain in float64 (the reference: util.msda_qp_formulation + oracle.ops_np.msda_forward + layer_ref) or in float32
    (util.msda_qp_float32_oracle + layer_f32, the projections in dot_rows_f32's order) -> out [tokens, 128] of the last layer."""
    from oracle import ops_np
    from tests import util
    c = chain_case()
    f64 = np.dtype(dtype) == np.float64
    src, query = c.src.reshape(-1, C), c.query.reshape(-1, C)

    def lin(x, w, b):
        return x @ w.T + b if f64 else project_f32(x, w, b).astype(np.float64)
    values = [lin(src, L.wv, L.bv) for L in c.layers]
    qp = lin(query, c.wq0, c.bq0)
    for L, value in zip(c.layers, values):
        s = _sampler_problem(c, value, qp)
        if f64:
            loc, attn = util.msda_qp_formulation(s, np.float64)
            sampled = ops_np.msda_forward(s.value, s.shapes, s.lsi, loc, attn, dtype=np.dtype(np.float64))
            query, qp = layer_ref(L, np.asarray(sampled).reshape(-1, C), query)
        else:
            sampled = util.msda_qp_float32_oracle(s)
            query, qp = layer_f32(L, np.asarray(sampled).reshape(-1, C), query)
            query, qp = query.astype(np.float64), None if qp is None else qp.astype(np.float64)
    return query

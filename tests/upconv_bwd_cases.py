"""The backward of the decoder's conv_1 path (csrc/upconv_bwd.hip, ops.upconv_adjoint, ops.upconv3x3_train): the float64
reference of the adjoint, the float32 restatement in the kernels' order, the cases and the derived bounds shared by
tests/test_host_upconv_bwd.py (no GPU) and tests/test_gpu_upconv_bwd.py.  Geometries, inputs and conventions are those of
tests/util.py (UPCONV_CASES): channels-last float64 arrays whose entries are float32 numbers, seeded by case name, read-only.

The operator.  With z the tap products [B, Hs, Ws, 3 (ky), 3 (kx), C] of one source, util.upconv_passes_ref(0, 0, [z], 0) is
    (L z)[b, Y, X, c] = sum_ky sum_kx  wy(Y + ky - 1 -> ys) wx(X + kx - 1 -> xs) z[b, ys, xs, ky, kx, c]
over the taps inside the Ho x Wo image; w(dst -> src) is what util.upconv_lerp gives destination dst for source index src
(w0 at i0, w1 at i1; both when i1 == i0).  upconv_adjoint_ref is L^T g, separably and in gather order:
    S[b, ky, ys, X, c]         = sum over D = Y + ky - 1 in [0, Ho), ascending, of wy(D -> ys) g[b, D - ky + 1, X, c]
    G[b, ys, xs, ky, kx, c]    = sum over D = X + kx - 1 in [0, Wo), ascending, of wx(D -> xs) S[b, ky, ys, D - kx + 1, c]
which is the order of upconv_bwd_ypass / upconv_bwd_xpass.  A term is w0 * a0 + w1 * a1 with a = g where the index matches
and 0 where not (a select on the value): an Inf in g reaches exactly the elements whose forward stencil holds that pixel.
Then dX = G nk ([P, 9C] x [9C, Cin]) and dNK = G^T X ([9C, P] x [P, Cin]), nk = util.tap_matrix(w).

The bounds, per element, u = 2^-24; nothing in them is fitted to a kernel's output.

  G:   u * ((n_y[ys] + n_x[xs] + 8) * A + Q)          A = upconv_adjoint_ref(|g|) in float64
       n_y[ys], n_x[xs]  the number of destinations summed into the element along each axis (every D whose i0 or i1 is the
           source index): a float32 sum of n terms in any fixed order rounds each term at most n times.
       8   what a path meets besides the adds: w0 = 1 - w1 rounded and the product, per pass (4); a term with two weights
           (i1 == i0) is one more add per pass (2); (1 + u)^n - 1 <= 1.0001 n u for the n here (the rest).
       Q   the transpose of util.upconv_perturbation.  On a non-dyadic axis lerp_of's float32 s differs from the rational s
           by |ds| <= 2 u (n_src - 1) (two roundings), which moves weight between neighbouring sources: every entry of the
           interpolation matrix moves by at most |ds| (also where int(s) changes, the interpolant being continuous), and an
           entry can be non-zero only for the destinations within one source step of it: at most n + 2 of them, n the
           largest n_y (n_x).  The other axis contributes its largest column sum of weights per tap, K_x (K_y) <= n_x (n_y).
           With M[c] = max over the pixels of |g[..., c]|:
               Q[c] = 2.02 * M[c] * sum over the non-dyadic axes of (n_src - 1) * (n_axis + 2) * K_other
           (2.02: the factor 2 of |ds| and 1 % for the second-order term).  Q = 0 for dyadic ratios.
  dX:  E_G |nk| + u * 9C * (A + E_G) |nk|            E_G the bound of G.  The product has 9C terms per element; in ANY
       summation order (the library's is unknown) at most 9C roundings touch a term.
  dW:  E_G^T |X| + u * P * (A + E_G)^T |X|           P = B * Hs * Ws terms per element, folded like dNK.

The float32 restatement (upconv_adjoint_ref(dtype=float32), numpy products) stays inside each bound on every case
(tests/test_host_upconv_bwd.py).  On dyadic geometries with integer g every weight is a multiple of a small power of two and
every partial sum exact: float32 equals float64 bit for bit in any order (the exact twins).
"""
import functools
import types

import numpy as np

from tests import util

U = util.UPCONV_U
PASS_CASES = util.UPCONV_PASS_CASES
TF_CASES = util.UPCONV_TF_CASES


def dyadic(name):
    """every axis of every source of the case has a dyadic ratio: lerp_of's float32 weights are exact"""
    _, (ho, wo), sizes, _, _, _ = util.UPCONV_CASES[name]
    return all(util.upconv_dyadic(hs, ho) and util.upconv_dyadic(ws, wo) for hs, ws in sizes)


# without the two large multi-block inputs (strip16, strip32: the 10 x 5 source geometry of strip8 on more pixels)
SMALL_CASES = tuple(k for k in PASS_CASES if k not in ("strip16", "strip32"))
DYADIC_CASES = tuple(k for k in PASS_CASES if dyadic(k))
EXACT_CASES = tuple(k for k in PASS_CASES if dyadic(k) and util.UPCONV_CASES[k][5] == "exact")


def _scatter_axis(v, axis_dst, n_src, n_dst, dt, descending=False):
    """One adjoint pass along one axis.  v [..., n_dst (axis_dst), ...] -> out with a new leading tap axis of 3 and the
    destination axis replaced by n_src: out[k, ..., src, ...] = sum over D of w(D -> src) v[..., D - k + 1, ...], D ascending
    (or descending), the taps D - k + 1 outside [0, n_dst) dropped."""
    i0, i1, w0, w1 = util.upconv_lerp(n_src, n_dst, dt)
    v = np.moveaxis(v, axis_dst, 0)                               # [n_dst, ...]
    out = np.zeros((3, n_src) + v.shape[1:], dtype=dt)
    order = range(n_dst - 1, -1, -1) if descending else range(n_dst)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in order:
            for k in range(3):
                p = d - k + 1
                if not 0 <= p < n_dst:
                    continue
                a = v[p]
                if i1[d] == i0[d]:
                    out[k, i0[d]] += dt(w0[d]) * a + dt(w1[d]) * a
                else:
                    out[k, i0[d]] += dt(w0[d]) * a
                    out[k, i1[d]] += dt(w1[d]) * a
    return out                                                    # [3, n_src, ...]


def upconv_adjoint_ref(g, sizes, dtype=np.float64, descending=False):
    """L^T g per source: g [B, Ho, Wo, C] -> list of G [B, Hs, Ws, 3, 3, C] (= the [B*Hs*Ws, 9*C] matrix of the kernels).
    float64: the reference, weights from the rational s.  float32: the kernels' arithmetic -- lerp_of's weights, the y
    adjoint then the x adjoint, each element summed over ascending destinations (descending: the other order of the exact
    twins)."""
    dt = np.dtype(dtype).type
    g = np.asarray(g).astype(dt)
    b, ho, wo, c = g.shape
    outs = []
    for hs, ws in sizes:
        s = _scatter_axis(g, 1, hs, ho, dt, descending)      # [ky, Hs, B, Wo, C]
        gz = _scatter_axis(s, 3, ws, wo, dt, descending)     # [kx, Ws, ky, Hs, B, C]
        assert gz.dtype == np.dtype(dtype)
        outs.append(np.ascontiguousarray(gz.transpose(4, 3, 1, 2, 0, 5)))      # [B, Hs, Ws, ky, kx, C]
    return outs


def fold_weight(dnk, c, cin):
    """dNK [9 C, Cin] (tap-major) -> grad w [C, Cin, 3, 3]: the inverse of util.tap_matrix."""
    return np.ascontiguousarray(np.asarray(dnk).reshape(3, 3, c, cin).transpose(2, 3, 0, 1))


def mix(gz, x, nk, dtype=np.float64):
    """(dX [B, Hs, Ws, Cin], dNK [9 C, Cin]) from G [B, Hs, Ws, 3, 3, C], x [B, Hs, Ws, Cin] and nk [9 C, Cin]."""
    c9, cin = nk.shape
    gm = np.asarray(gz).reshape(-1, c9).astype(dtype)
    dx = gm @ np.asarray(nk).astype(dtype)
    dnk = gm.T @ np.asarray(x).reshape(-1, cin).astype(dtype)
    return dx.reshape(x.shape), dnk


def axis_counts(n_src, n_dst):
    """(n[src]: destinations whose i0 or i1 is src, K: the largest column sum of the weights) of one axis."""
    i0, i1, w0, w1 = util.upconv_lerp(n_src, n_dst)
    n = np.zeros(n_src)
    k = np.zeros(n_src)
    np.add.at(n, i0, 1)
    np.add.at(n, i1[i1 != i0], 1)
    np.add.at(k, i0, w0)
    np.add.at(k, i1, w1)
    return n, float(k.max())


def adjoint_bound(g, sizes):
    """-> list of (A, E_G) per source, both [B, Hs, Ws, 3, 3, C]: the reference on |g| and the bound of G."""
    g = np.asarray(g, dtype=np.float64)
    b, ho, wo, c = g.shape
    mags = upconv_adjoint_ref(np.abs(g), sizes)
    m = np.abs(g).reshape(-1, c).max(0)
    out = []
    for a, (hs, ws) in zip(mags, sizes):
        ny, ky = axis_counts(hs, ho)
        nx, kx = axis_counts(ws, wo)
        terms = ny[None, :, None, None, None, None] + nx[None, None, :, None, None, None] + 8.0
        q = 0.0
        if not util.upconv_dyadic(hs, ho):
            q = q + (hs - 1) * (ny.max() + 2) * kx
        if not util.upconv_dyadic(ws, wo):
            q = q + (ws - 1) * (nx.max() + 2) * ky
        out.append((a, U * (terms * a + 2.02 * q * m)))
    return out


def mix_bounds(a, e_g, x, nk):
    """-> (bound of dX [B, Hs, Ws, Cin], bound of dNK [9 C, Cin]) from A and E_G of one source."""
    c9, cin = nk.shape
    am, em = a.reshape(-1, c9), e_g.reshape(-1, c9)
    xm = np.abs(np.asarray(x, dtype=np.float64)).reshape(-1, cin)
    nkm = np.abs(np.asarray(nk, dtype=np.float64))
    dx = em @ nkm + U * c9 * ((am + em) @ nkm)
    dnk = em.T @ xm + U * xm.shape[0] * ((am + em).T @ xm)
    return dx.reshape(x.shape), dnk


@functools.lru_cache(maxsize=None)
def case(name):
    """The forward case of tests/util.py plus g [B, Ho, Wo, C] (integers for the exact cases, normal otherwise), the
    float64 references G / dX / dNK per source and their bounds."""
    f = util.upconv_case(name)
    rng = np.random.default_rng(util._seed("upconv_bwd/" + name))
    c = types.SimpleNamespace(name=name, fwd=f, b=f.b, ho=f.ho, wo=f.wo, sizes=f.sizes, c=f.c, cin=f.cin, kind=f.kind)
    c.g = util.upconv_inputs(rng, (f.b, f.ho, f.wo, f.c), f.kind)
    c.gz = upconv_adjoint_ref(c.g, f.sizes)
    ab = adjoint_bound(c.g, f.sizes)
    c.mag = [a for a, _ in ab]
    c.gz_bound = [e for _, e in ab]
    c.dx, c.dnk, c.dx_bound, c.dnk_bound = [], [], [], []
    for i in range(len(f.sizes)):
        dx, dnk = mix(c.gz[i], f.x[i], f.nk[i])
        bx, bnk = mix_bounds(c.mag[i], c.gz_bound[i], f.x[i], f.nk[i])
        c.dx.append(dx), c.dnk.append(dnk), c.dx_bound.append(bx), c.dnk_bound.append(bnk)
    for group in (c.gz, c.mag, c.gz_bound, c.dx, c.dnk, c.dx_bound, c.dnk_bound):
        for arr in group:
            arr.setflags(write=False)
    return util._freeze(c)


def stencil_mask(sizes, shape, pixel):
    """Per source, the boolean [B, Hs, Ws, 3, 3, C] of the tap products the forward reads for output element pixel = (b, Y, X,
    c) of an output of `shape` = (B, Ho, Wo, C), straight from util.upconv_lerp: tap (ky, kx) of (Y, X) reads the fine pixel
    (Y + ky - 1, X + kx - 1) if it is inside the image, which reads the sources (i0 | i1) x (i0 | i1)."""
    bb, ho, wo, c = shape
    b0, y0, x0, c0 = pixel
    masks = []
    for hs, ws in sizes:
        iy0, iy1, _, _ = util.upconv_lerp(hs, ho)
        ix0, ix1, _, _ = util.upconv_lerp(ws, wo)
        m = np.zeros((bb, hs, ws, 3, 3, c), dtype=bool)
        for ky in range(3):
            fy = y0 + ky - 1
            if not 0 <= fy < ho:
                continue
            for kx in range(3):
                fx = x0 + kx - 1
                if not 0 <= fx < wo:
                    continue
                for ys in {int(iy0[fy]), int(iy1[fy])}:
                    for xs in {int(ix0[fx]), int(ix1[fx])}:
                        m[b0, ys, xs, ky, kx, c0] = True
        masks.append(m)
    return masks


def inf_pixels(name):
    """the output elements the Inf tests poison, one at a time: a corner, an edge and an inner pixel"""
    _, (ho, wo), _, ch, _, _ = util.UPCONV_CASES[name]
    b = util.UPCONV_CASES[name][0]
    return sorted({(0, 0, 0, 0), (b - 1, ho - 1, wo // 2, ch - 1), (0, ho // 2, wo - 1, 1 % ch), (b - 1, ho // 2, wo // 2, ch // 2)})

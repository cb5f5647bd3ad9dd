"""The five channels-last convolution kernels (csrc/conv_igemm.hip, conv_rows.hip, conv_wino.hip, conv_wino1d.hip, conv_bf16.hip):
the float64 reference, the per-element bounds, float32 restatements of each algorithm, the case tables and the item geometry
shared by tests/test_host_conv_reference.py (no GPU) and tests/test_gpu_conv_family.py.  numpy only.

Layout.  Every array is channels-last: x [B, H, W, Cin], w [Cout, Cin, KH, KW], bias [Cout], res / out [B, Ho, Wo, Cout].  Every
array is a float64 array whose entries are float32 numbers, seeded by the case name, built once and read-only.

Reference.  conv_direct: a plain direct convolution in float64 with explicit padding and stride, tap by tap.  epilogue: what
every kernel does behind its sum -- + bias, + residual, then max(v, 0) + slope * min(v, 0) with slope 1 (act 0, none), 0 (act 1,
ReLU) or float32(0.01) (act 2, LeakyReLU: the kernels hold the slope as a float32, so the reference takes that number).

Bounds, u = 2^-24.  Nothing here is fitted to a kernel; tests/test_host_conv_reference.py prints how much of each bound a
float32 restatement of the algorithm uses.

  Direct form (conv_igemm, conv_rows).  The matrix cores add one product at a time to a float32 accumulator: K = Cin KH KW
  steps, so a term passes at most K roundings (one more if the product is rounded on its own: still <= K + 1 for every term
  but the first).  Behind the sum: + bias, + residual, the slope product -- three roundings.  One more for the second-order
  terms ((1 + u)^n - 1 <= (n + 1) u as long as n^2 u <= 1, i.e. K <= 4096: asserted).  So

      |got - ref| <= u (K + 4) (|x| (*) |w|) + 4 u (|bias| + |res|)                                  DIRECT_C = 4

  ((*): the same convolution on magnitudes; bias and residual pass the three epilogue roundings, + 1 second order).

  Winograd F(2x2, 3x3) (conv_wino).  Y = A^T [ sum_cin (G g G^T) . (B^T d B) ] A.  The magnitude form of that algorithm is
  Mw = |A^T| [ sum_cin (|G| |g| |G^T|) . (|B^T| |d| |B|) ] |A|.  Roundings a term passes, from the code: U = G g G^T is computed
  in float64 and rounded once (ops.conv_wino_prepare): 1; B^T d B is two levels of float32 additions (WINO_T_ROWS,
  WINO_T_COLS): 2; the accumulation over the input channels: Cin; A^T M A is (a + b) + c twice (s0 / s1, then yv): 4; the
  epilogue: 3; second order: 1.  So

      |got - ref| <= u (Cin + 11) Mw + 4 u (|bias| + |res|)                                          WINO_C = 11

  Winograd F(2, 3) along the 3-tap axis (conv_wino1d).  (y0, y1) = A^T [ sum_{cin, kL} (G g_kL) . (B^T d_kL) ], magnitude form
  M1 accordingly.  U = G g rounded once: 1; B^T d is one level of additions: 1; the accumulation over Cin KL terms: Cin KL;
  A^T m is (a + b) + c: 2; the epilogue (no residual in this kernel): bias and slope, 2; second order: 1.  So

      |got - ref| <= u (Cin KL + 7) M1 + 3 u |bias|                                                   WINO1D_C = 7

  conv_bf16 keeps the bound of tests/test_gpu_conv_bf16.py::_reference: the reference runs on the bf16-rounded operands
  (round to nearest even), and |got - ref| <= 1e-5 (|x_bf| (*) |w_bf|) + 2^-23 (|bias| + |res|) + 1e-30.

  Channel sums.  A table entry is the float32 sum of n = 32 (conv_cl layout: one output row segment) or 64 (conv_wino layout:
  two row segments) stored outputs; the reference entry is the float64 sum of the reference outputs.  The errors of the
  outputs add up, and the float32 summation rounds r times per term: half_wave_sum is five DPP steps (r = 5); conv_wino adds
  the four outputs of a tile (the first to 0: exact) and runs four DPP steps (r = 8); + 1 second order:

      |got - ref| <= sum bound_o + u (r + 1) sum (|ref_o| + bound_o)

Exact inputs.  Activations are integers in [-4, 4], weights k / 16 with |k| <= 8, bias and residual multiples of 1 / 8 in
[-4, 4].  Every number any of the five algorithms forms on such data is a multiple of 1 / 64 (G halves twice, g is in 16ths;
B^T, A^T are +-1 / 0), and a multiple of 1 / 64 below 2^24 / 64 in magnitude is a float32 number: as long as the magnitude form
of the algorithm (plus |bias| + |res|) times 64 stays below 2^24 -- asserted per case, per algorithm, also for the sum
tables -- every partial sum in any order is exact and all five kernels must return float32(reference) bit for bit.  The values
are bf16 numbers too (4 significant bits), so conv_bf16 joins.  act 2 stays exact in this sense: its one rounding,
float32(slope * v), is the same correctly rounded product in every kernel and in float32(reference).
"""
import functools
import hashlib
import types

import numpy as np

U = 2.0 ** -24
SLOPE32 = float(np.float32(0.01))
ACT_SLOPE = {0: 1.0, 1: 0.0, 2: SLOPE32}
DIRECT_C, WINO_C, WINO1D_C = 4, 11, 7
EPI_C = 4                      # bias / residual: three epilogue roundings + 1
SUM_R = {1: 5, 2: 8}           # roundings per term of a table entry, by rows per entry (1: conv_cl layout, 2: conv_wino layout)
EXACT_DENOM = 64.0
FAMILIES = ("igemm", "rows", "wino", "wino1d", "bf16")
WINO1D_KERNELS = ((5, 3), (7, 3), (3, 5), (3, 7))

_G = np.array(((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0)))
_BT = np.array(((1.0, 0.0, -1.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, -1.0, 1.0, 0.0), (0.0, 1.0, 0.0, -1.0)))
_AT = np.array(((1.0, 1.0, 1.0, 0.0), (0.0, 1.0, -1.0, -1.0)))


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def bf16_round(a):
    """float32 numbers -> the nearest bf16 numbers (ties to even), as float64."""
    bits = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------
def out_size(h, w, k, stride, pad):
    return (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1


def conv_direct(x, w, stride, pad):
    """x [B, H, W, Cin], w [Cout, Cin, KH, KW] -> [B, Ho, Wo, Cout] in x's dtype arithmetic (float64 for the reference): one
    matrix product per tap over the zero-padded image."""
    b, h, wd, cin = x.shape
    cout, _, kh, kw = w.shape
    ho, wo = out_size(h, wd, (kh, kw), stride, pad)
    assert ho > 0 and wo > 0
    xp = np.zeros((b, h + 2 * pad[0], wd + 2 * pad[1], cin), dtype=x.dtype)
    xp[:, pad[0]:pad[0] + h, pad[1]:pad[1] + wd] = x
    out = np.zeros((b, ho, wo, cout), dtype=x.dtype)
    with np.errstate(invalid="ignore"):
        for ky in range(kh):
            for kx in range(kw):
                win = xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
                out += win @ w[:, :, ky, kx].T
    return out


def act_apply(v, act):
    with np.errstate(invalid="ignore"):
        return np.maximum(v, 0.0) + ACT_SLOPE[act] * np.minimum(v, 0.0)


def epilogue(acc, bias, res, act):
    v = acc
    if bias is not None:
        v = v + bias
    if res is not None:
        v = v + res
    return act_apply(v, act)


def conv_ref(x, w, bias, res, act, stride, pad):
    return epilogue(conv_direct(x, w, stride, pad), bias, res, act)


def sum_table(out, rows=1):
    """out [B, Ho, Wo, C] -> [B, chunks, C]: the channel sums per row segment in the table layout of conv_cl (rows = 1: chunk
    ((y / 4) xt + x0 / 32) 4 + y % 4 holds row y, columns x0 .. x0 + 31; ops.conv_sum_chunks) or of conv_wino_cl (rows = 2:
    chunk ((y0 / 8) xb + x0 / 32) 4 + v holds rows y0 + 2 v, y0 + 2 v + 1; ops.conv_wino_sum_chunks).  Outside the image: 0."""
    b, ho, wo, c = out.shape
    ny, nx = -(-ho // (4 * rows)), -(-wo // 32)
    full = np.zeros((b, ny * 4 * rows, nx * 32, c), dtype=out.dtype)
    full[:, :ho, :wo] = out
    return full.reshape(b, ny, 4, rows, nx, 32, c).sum(axis=(3, 5)).transpose(0, 1, 3, 2, 4).reshape(b, ny * nx * 4, c)


def sum_table_loop(out, rows=1):
    """sum_table as the plain loop its docstring describes."""
    b, ho, wo, c = out.shape
    ny, nx = -(-ho // (4 * rows)), -(-wo // 32)
    tab = np.zeros((b, ny * nx * 4, c), dtype=out.dtype)
    for s in range(b):
        for y in range(ho):
            for x in range(wo):
                y0, x0 = y // (4 * rows), x // 32
                chunk = (y0 * nx + x0) * 4 + (y - y0 * 4 * rows) // rows
                tab[s, chunk] += out[s, y, x]
    return tab


def sum_bound(ref_out, out_bound, rows=1):
    return sum_table(out_bound, rows) + U * (SUM_R[rows] + 1) * sum_table(np.abs(ref_out) + out_bound, rows)


# ---------------------------------------------------------------------------------------------
# the Winograd forms: magnitude form (float64) and float32 restatement share the tiling
# ---------------------------------------------------------------------------------------------
def _patches2d(x):
    """[B, H, W, C] -> d [B, ty, tx, 4, 4, C]: tile (i, j) = outputs (2 i .. 2 i + 1, 2 j .. 2 j + 1) reads input rows 2 i - 1 .. 2 i + 2
    and columns 2 j - 1 .. 2 j + 2, zeros outside the image."""
    b, h, w, c = x.shape
    ty, tx = (h + 1) // 2, (w + 1) // 2
    xp = np.zeros((b, 2 * ty + 2, 2 * tx + 2, c), dtype=x.dtype)
    xp[:, 1:h + 1, 1:w + 1] = x
    d = np.empty((b, ty, tx, 4, 4, c), dtype=x.dtype)
    for r in range(4):
        for s in range(4):
            d[:, :, :, r, s] = xp[:, r:r + 2 * ty:2, s:s + 2 * tx:2]
    return d


def _untile2d(y, h, w):
    """[B, ty, tx, 2, 2, O] -> [B, H, W, O]"""
    b, ty, tx, _, _, o = y.shape
    return y.transpose(0, 1, 3, 2, 4, 5).reshape(b, 2 * ty, 2 * tx, o)[:, :h, :w]


def wino_mag(x, w):
    """|A^T| [ sum_cin (|G| |g| |G^T|) . (|B^T| |d| |B|) ] |A| -> [B, H, W, Cout]"""
    b, h, wd, _ = x.shape
    um = np.einsum("xr,ocrs,ns->ocxn", np.abs(_G), np.abs(w), np.abs(_G))
    vm = np.einsum("xr,btjrsc,ns->btjxnc", np.abs(_BT), np.abs(_patches2d(x)), np.abs(_BT))
    mm = np.einsum("ocxn,btjxnc->btjxno", um, vm)
    return _untile2d(np.einsum("px,btjxno,qn->btjpqo", np.abs(_AT), mm, np.abs(_AT)), h, wd)


def _fma32(acc, a, b):
    """float32(acc + a * b) with the product unrounded: a float64 product of two float32 numbers is exact."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def _bt_f32(v, axis):
    """B^T d along `axis` (extent 4) in float32, the kernels' four expressions: d0 - d2, d1 + d2, d2 - d1, d1 - d3."""
    d0, d1, d2, d3 = (np.take(v, i, axis=axis) for i in range(4))
    return np.stack((d0 - d2, d1 + d2, d2 - d1, d1 - d3), axis=axis)


def _cin_order16(cin):
    """The order in which conv_wino / conv_wino1d add the input channels: chunks of 16, k-step i, lane quarter q -> 16 chunk + 4 q + i."""
    return [16 * ch + 4 * q + i for ch in range(cin // 16) for i in range(4) for q in range(4)]


def epilogue_f32(y, bias, res, act):
    f = np.float32
    v = y.astype(f)
    if bias is not None:
        v = v + bias.astype(f)                 # (without a bias the kernels add 0.0: exact)
    if res is not None:
        v = v + res.astype(f)
    with np.errstate(invalid="ignore"):
        neg = (np.minimum(v, f(0)).astype(np.float64) * SLOPE32).astype(f) if act == 2 else np.minimum(v, f(0)) * f(ACT_SLOPE[act])
        out = np.maximum(v, f(0)) + neg
    assert out.dtype == f
    return out


def wino_f32(x, w, bias, res, act):
    """conv_wino's arithmetic in float32 numpy: U rounded once from float64, B^T d B by rows then columns, a channel-ordered fma
    chain per transform position, A^T M A as (a + b) + c / (a - b) - c, the epilogue."""
    f = np.float32
    b, h, wd, cin = x.shape
    u = np.einsum("xr,ocrs,ns->ocxn", _G, w, _G).astype(f)                      # [O, C, 4, 4]
    v = _bt_f32(_bt_f32(_patches2d(x.astype(f)), 3), 4)                          # [B, ty, tx, 4, 4, C]
    acc = np.zeros(v.shape[:5] + (w.shape[0],), dtype=f)
    for c in _cin_order16(cin):
        acc = _fma32(acc, v[..., c][..., None], u[:, c].transpose(1, 2, 0))
    s0 = (acc[:, :, :, 0] + acc[:, :, :, 1]) + acc[:, :, :, 2]                   # [B, ty, tx, nu, O]
    s1 = (acc[:, :, :, 1] - acc[:, :, :, 2]) - acc[:, :, :, 3]
    rows = []
    for s in (s0, s1):
        rows.append(np.stack(((s[:, :, :, 0] + s[:, :, :, 1]) + s[:, :, :, 2], (s[:, :, :, 1] - s[:, :, :, 2]) - s[:, :, :, 3]), axis=3))
    y = _untile2d(np.stack(rows, axis=3), h, wd)
    assert y.dtype == f
    return epilogue_f32(y, bias, res, act)


def _patches1d(x, kl):
    """[B, nL, nS, C] -> d [B, nL + kl - 1, ts, 4, C]: input row l - kl // 2 (zeros outside), tile j = columns 2 j - 1 .. 2 j + 2."""
    b, nl, ns, c = x.shape
    ts, pad = (ns + 1) // 2, kl // 2
    xp = np.zeros((b, nl + 2 * pad, 2 * ts + 2, c), dtype=x.dtype)
    xp[:, pad:pad + nl, 1:ns + 1] = x
    return np.stack([xp[:, :, s:s + 2 * ts:2] for s in range(4)], axis=3)


def _long_axis_first(x, w, res=None):
    """A 3 x K layer is the K x 3 layer of the transposed image."""
    if w.shape[3] == 3:
        return x, w, res, False
    return x.transpose(0, 2, 1, 3), w.transpose(0, 1, 3, 2), None if res is None else res.transpose(0, 2, 1, 3), True


def wino1d_mag(x, w):
    x, w, _, flip = _long_axis_first(x, w)
    b, nl, ns, _ = x.shape
    kl = w.shape[2]
    um = np.einsum("pr,ockr->ockp", np.abs(_G), np.abs(w))                      # [O, C, KL, 4]
    vm = np.einsum("pr,bljrc->bljpc", np.abs(_BT), np.abs(_patches1d(x, kl)))    # [B, nL + KL - 1, ts, 4, C]
    mm = sum(np.einsum("ocp,bljpc->bljpo", um[:, :, k], vm[:, k:k + nl]) for k in range(kl))
    y = np.einsum("ep,bljpo->bljeo", np.abs(_AT), mm).reshape(b, nl, -1, w.shape[0])[:, :, :ns]
    return y.transpose(0, 2, 1, 3) if flip else y


def wino1d_f32(x, w, bias, act):
    f = np.float32
    x, w, _, flip = _long_axis_first(x, w)
    b, nl, ns, cin = x.shape
    kl = w.shape[2]
    u = np.einsum("pr,ockr->ockp", _G, w).astype(f)
    v = _bt_f32(_patches1d(x.astype(f), kl), 3)
    acc = np.zeros((b, nl, v.shape[2], 4, w.shape[0]), dtype=f)
    order = _cin_order16(cin)
    for g in range(0, cin, 4):                  # one k-step (four channels) at a time: its long-axis taps in turn, then the next
        for k in range(kl):
            for c in order[g:g + 4]:
                acc = _fma32(acc, v[:, k:k + nl, :, :, c][..., None], u[:, c, k].T)
    y = np.stack(((acc[:, :, :, 0] + acc[:, :, :, 1]) + acc[:, :, :, 2], (acc[:, :, :, 1] - acc[:, :, :, 2]) - acc[:, :, :, 3]), axis=3)
    y = y.reshape(b, nl, -1, w.shape[0])[:, :, :ns]
    y = np.ascontiguousarray(y.transpose(0, 2, 1, 3)) if flip else y
    return epilogue_f32(y, bias, None, act)


def direct_f32(x, w, bias, res, act, stride, pad):
    """The direct form as a k-ordered float32 fma chain: tap by tap, the input channels of a tap in turn."""
    f = np.float32
    b, h, wd, cin = x.shape
    cout, _, kh, kw = w.shape
    ho, wo = out_size(h, wd, (kh, kw), stride, pad)
    xp = np.zeros((b, h + 2 * pad[0], wd + 2 * pad[1], cin), dtype=f)
    xp[:, pad[0]:pad[0] + h, pad[1]:pad[1] + wd] = x
    w32 = w.astype(f)
    acc = np.zeros((b, ho, wo, cout), dtype=f)
    for ky in range(kh):
        for kx in range(kw):
            win = xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
            for c in range(cin):
                acc = _fma32(acc, win[..., c][..., None], w32[:, c, ky, kx])
    return epilogue_f32(acc, bias, res, act)


# ---------------------------------------------------------------------------------------------
# which family takes a case, and in which tiles
# ---------------------------------------------------------------------------------------------
def same_padding(c):
    return c.k[0] % 2 == 1 and c.k[1] % 2 == 1 and c.pad == (c.k[0] // 2, c.k[1] // 2)


def family_takes(family, c):
    """The shape rules of the five entry points (ops.conv_cl_supported, conv_rows_ok, conv_wino_ok, conv_wino1d_ok, conv_bf16_ok)."""
    if family in ("igemm", "bf16"):
        ok = c.cin % 32 == 0 and c.cout % 32 == 0
        return ok and (family == "igemm" or bf16_cfg(c.b, c.ho, c.wo, c.cout, c.k, c.stride, c.res is not None) is not None)
    if family == "rows":
        return c.cin % 32 == 0 and c.cout % 32 == 0 and c.stride == 1 and same_padding(c) and c.k[1] in (3, 5, 7)
    if family == "wino":
        return c.k == (3, 3) and c.stride == 1 and same_padding(c) and c.cin % 16 == 0 and c.cout % 16 == 0
    if family == "wino1d":
        return c.k in WINO1D_KERNELS and c.stride == 1 and same_padding(c) and c.cin % 16 == 0 and c.cout % 16 == 0 and c.res is None
    raise KeyError(family)


def tiles(family, c):
    """mt (32-channel output blocks per wave: igemm 1 / 2 / 4, with a residual <= 2; rows 1 / 2), mb (16-channel blocks: 1 / 2);
    conv_bf16 picks its block shape itself."""
    if family == "igemm":
        return [mt for mt in (1, 2, 4) if c.cout % (32 * mt) == 0 and (c.res is None or mt <= 2)]
    if family == "rows":
        return [mt for mt in (1, 2) if c.cout % (32 * mt) == 0]
    if family in ("wino", "wino1d"):
        return [mb for mb in (1, 2) if c.cout % (16 * mb) == 0]
    return [0]


def sum_rows(family):
    return 2 if family == "wino" else 1


# ---------------------------------------------------------------------------------------------
# item geometry: what a persistent block walks
# ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def items_direct(b, ho, wo, cout, mt):
    """conv_igemm / conv_rows: 4 output rows x 32 columns x 32 mt channels."""
    return b * _cdiv(ho, 4) * _cdiv(wo, 32) * (cout // (32 * mt))


def items_wino(b, h, w, cout, mb):
    """conv_wino: 8 rows x 32 columns x 16 mb channels."""
    return b * _cdiv(h, 8) * _cdiv(w, 32) * (cout // (16 * mb))


def items_wino1d(b, h, w, cout, mb, k):
    """conv_wino1d: 16 rows along the long axis x 32 columns along the 3-tap axis x 16 mb channels."""
    nl, ns = (h, w) if k[1] == 3 else (w, h)
    return b * _cdiv(nl, 16) * _cdiv(ns, 32) * (cout // (16 * mb))


def bf16_cfg(b, ho, wo, cout, k, stride, res):
    """pick_cfg of csrc/conv_bf16.hip restated: the block shape (mt, wc, rw, rb) the kernel runs a layer in, None if it refuses it."""
    nq, best, best_key = cout // 32, None, -1
    for mt in (4, 2, 1):
        for wc in (1, 2, 4):
            for rw in (2, 1):
                g = mt * wc
                if g > 4 or nq % g or mt * rw > 4 or (res and mt * rw > 2):
                    continue
                rb = (4 // wc) * rw
                rr, cc = (rb - 1) * stride + k[0], 31 * stride + k[1]
                if rr * cc * 4 > 256 * 8 or (4 * g * 128 + rr * cc * 5) * 16 + cout * 4 > 80 * 1024:
                    continue
                items = b * _cdiv(ho, rb) * _cdiv(wo, 32) * (nq // g)
                key = (min(items, 512) * 8 + g) * 64 + mt * 8 + rw
                if key > best_key:
                    best_key, best = key, types.SimpleNamespace(mt=mt, wc=wc, rw=rw, rb=rb)
    return best


def items_bf16(b, ho, wo, cout, k, stride, res, sums):
    cfg = bf16_cfg(b, ho, wo, cout, k, stride, res)
    rows = _cdiv(ho, 4) * 4 if sums else ho       # with channel sums the row groups span the whole table
    return b * _cdiv(rows, cfg.rb) * _cdiv(wo, 32) * (cout // 32 // (cfg.mt * cfg.wc))


def items(family, c, tile, sums=False):
    if family in ("igemm", "rows"):
        return items_direct(c.b, c.ho, c.wo, c.cout, tile)
    if family == "wino":
        return items_wino(c.b, c.h, c.w, c.cout, tile)
    if family == "wino1d":
        return items_wino1d(c.b, c.h, c.w, c.cout, tile, c.k)
    return items_bf16(c.b, c.ho, c.wo, c.cout, c.k, c.stride, c.res is not None, sums)


def block_shares(n_items, grid):
    """Items per block of a launch of min(n_items, grid) persistent blocks: ceil(n / g) each until the items run out."""
    g = min(n_items, grid)
    per = _cdiv(n_items, g)
    return [max(0, min(per, n_items - i * per)) for i in range(g)]


def xcd_remap(grid):
    """lblock of every blockIdx.x as the kernels compute it."""
    xq, xr = grid >> 3, grid & 7
    return [((x & 7) * (xq + 1) if (x & 7) < xr else xr * (xq + 1) + ((x & 7) - xr) * xq) + (x >> 3) for x in range(grid)]


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
SIZES = [(h, w) for h in (3, 4, 5, 8, 9) for w in (31, 32, 33)]     # one below, on and one above the tile edges (4 / 8 rows, 32 columns)


def _spec(b, cin, cout, k, hw, stride=1, pad=None, act=0, bias=True, res=False, sums=False, exact=False):
    return dict(b=b, cin=cin, cout=cout, k=k, hw=hw, stride=stride, pad=pad, act=act, bias=bias, res=res, sums=sums, exact=exact)


def _bound_specs():
    s = {}
    # 3 x 3, stride 1, every size around the tile edges; Cin follows the column, the epilogue the row; every tile width
    for i, (h, w) in enumerate(SIZES):
        mode = ("plain", "res", "sums")[(i // 3) % 3]
        s["k3x3_%dx%d" % (h, w)] = _spec(2, (32, 64, 128)[i % 3], (32, 64, 128, 64, 32)[i // 3], (3, 3), (h, w), act=(i + i // 3) % 3,
                                          bias=i % 2 == 0, res=mode == "res", sums=mode == "sums")
    s["k3x3_b3"] = _spec(3, 32, 128, (3, 3), (9, 33), act=1, res=True)
    for j, k in enumerate(((1, 1), (1, 3), (7, 3), (3, 7), (5, 3), (3, 5))):
        tag = "k%dx%d" % k
        s[tag + "_5x33"] = _spec(2, (32, 64)[j % 2], 64, k, (5, 33), act=j % 3, bias=True, sums=j % 2 == 1)
        s[tag + "_9x31"] = _spec(2, (64, 32)[j % 2], 32, k, (9, 31), act=(j + 1) % 3, bias=j % 2 == 1, res=j % 2 == 0 and k not in WINO1D_KERNELS)
        s[tag + "_17x33"] = _spec(1, 32, 32, k, (17, 33), act=1)                      # more than one 16-row block of conv_wino1d
    s["k7x3_c128"] = _spec(1, 128, 32, (7, 3), (4, 33), act=2)
    s["k3x5_c128"] = _spec(1, 128, 64, (3, 5), (5, 32), act=1)
    # stride 2 (conv_igemm, conv_bf16)
    s["s2_k3x3_9x33"] = _spec(2, 64, 64, (3, 3), (9, 33), stride=2, act=1)
    s["s2_k3x3_8x64"] = _spec(2, 32, 128, (3, 3), (8, 64), stride=2, act=2, bias=False, sums=True)
    s["s2_k3x3_17x65"] = _spec(1, 128, 64, (3, 3), (17, 65), stride=2, act=0, res=True)
    s["s2_k1x1_5x33"] = _spec(2, 32, 64, (1, 1), (5, 33), stride=2, pad=(0, 0), act=0)
    # a single pixel
    for k in ((3, 3), (1, 1), (7, 3), (3, 7)):
        s["pixel_k%dx%d" % k] = _spec(2, 32, 32, k, (1, 1), act=2 if k == (3, 3) else 0, res=k == (3, 3))
    # Cin / Cout in sixteenths of a wave tile: the two Winograd kernels alone
    s["c16_k3x3"] = _spec(2, 16, 16, (3, 3), (5, 33), act=1, res=True)
    s["c48_k3x3"] = _spec(2, 48, 48, (3, 3), (9, 31), act=2, sums=True)
    s["c16_k5x3"] = _spec(2, 16, 48, (5, 3), (5, 33), act=1)
    s["c48_k3x7"] = _spec(2, 48, 16, (3, 7), (9, 31), act=0, bias=False)
    return s


def _exact_specs():
    s = {}
    s["x_k3x3_c128"] = _spec(2, 128, 64, (3, 3), (9, 33), act=1, exact=True)
    s["x_k3x3_res"] = _spec(3, 64, 64, (3, 3), (5, 34), act=2, res=True, exact=True)
    s["x_k3x3_sums"] = _spec(2, 32, 128, (3, 3), (9, 33), act=1, sums=True, exact=True)
    s["x_k3x3_none"] = _spec(2, 32, 32, (3, 3), (8, 31), act=0, bias=False, sums=True, exact=True)
    s["x_k7x3"] = _spec(2, 32, 32, (7, 3), (17, 33), act=1, exact=True)
    s["x_k3x7"] = _spec(2, 32, 64, (3, 7), (9, 33), act=0, exact=True)
    s["x_k5x3"] = _spec(2, 64, 64, (5, 3), (9, 31), act=2, exact=True)
    s["x_k3x5"] = _spec(2, 64, 32, (3, 5), (5, 33), act=1, exact=True)
    s["x_k1x1"] = _spec(2, 128, 128, (1, 1), (5, 33), act=0, res=False, exact=True)
    s["x_s2_k3x3"] = _spec(2, 64, 64, (3, 3), (9, 33), stride=2, act=1, exact=True)
    return s


# Walks under the grid cap (tests/util.py::conv_grid_cap).  name -> (family, tile, with sums, caps, spec).  Every cap is below the
# item count (asserted on the host); igemm at 1 x 1 / Cin 32 has ONE stage per item, so the three-stage operand prefetch spans
# three items: 2, 3 and 4 items under a cap of one block, 2 + 2 + 1 under a cap of three, 3 per block under a cap of 11 (which
# gives xq = 1, xr = 3 in the XCD remap).  conv_bf16 (block shapes by bf16_cfg, checked in tests/test_host_conv_reference.py):
# Cout 32 -> <MT 1, RW 1> as 4-row blocks (wc 1); Cout 64 at Ho % 4 == 0 (with a residual) and at stride 2 -> wc 2, 2-row
# blocks; Cout 128 at Ho % 4 == 0 -> wc 4, 1-row blocks; with sums at Ho = 9 the row groups run to 12 rows.  Below 512 items
# pick_cfg takes the shape with the most items, which is always an <MT 1, RW 1> one: <4, 1>, <2, 2>, <2, 1> and <1, 2> stay
# with the full-size layers of tests/test_gpu_conv_bf16.py.
def _walk_specs():
    s = {}
    for n in (2, 3, 4):
        s["igemm_1x1_%ditems" % n] = ("igemm", 1, False, (1,), dict(b=1, cin=32, cout=32, k=(1, 1), hw=(4 * n, 32)))
    s["igemm_1x1_5items"] = ("igemm", 1, False, (3,), dict(b=1, cin=32, cout=32, k=(1, 1), hw=(20, 32)))
    s["igemm_1x1_24items"] = ("igemm", 1, False, (1, 3, 11), dict(b=3, cin=32, cout=32, k=(1, 1), hw=(13, 33), act=1))
    s["igemm_3x3_nct3"] = ("igemm", 1, False, (1, 3, 11), dict(b=2, cin=32, cout=96, k=(3, 3), hw=(5, 33), act=2))
    s["igemm_3x3_res"] = ("igemm", 2, False, (1, 3, 11), dict(b=2, cin=64, cout=64, k=(3, 3), hw=(9, 33), act=1, res=True))
    s["igemm_3x3_sums"] = ("igemm", 4, True, (1, 3, 11), dict(b=2, cin=32, cout=128, k=(3, 3), hw=(9, 33), act=1))
    s["igemm_s2"] = ("igemm", 1, False, (1, 3, 11), dict(b=2, cin=32, cout=64, k=(3, 3), hw=(17, 65), stride=2, act=0))
    s["rows_1x3"] = ("rows", 1, False, (1, 3, 11), dict(b=2, cin=32, cout=32, k=(1, 3), hw=(9, 33), act=0))
    s["rows_3x3"] = ("rows", 1, False, (1, 3, 11), dict(b=2, cin=32, cout=32, k=(3, 3), hw=(9, 33), act=1))
    s["rows_3x3_nct3"] = ("rows", 1, False, (1, 3, 11), dict(b=2, cin=32, cout=96, k=(3, 3), hw=(5, 33), act=2))
    s["rows_3x5_res"] = ("rows", 2, False, (1, 3, 11), dict(b=2, cin=64, cout=64, k=(3, 5), hw=(9, 33), act=1, res=True))
    s["rows_3x3_sums"] = ("rows", 1, True, (1, 3, 11), dict(b=2, cin=32, cout=32, k=(3, 3), hw=(9, 33), act=1, bias=False))
    s["rows_7x7_sums2"] = ("rows", 2, True, (1, 3, 11), dict(b=3, cin=32, cout=64, k=(7, 7), hw=(5, 33), act=0))
    s["bf16_3x3_c32"] = ("bf16", 0, False, (1, 3, 11), dict(b=2, cin=32, cout=32, k=(3, 3), hw=(9, 33), act=1))
    s["bf16_1x1_c32"] = ("bf16", 0, False, (1, 3, 11), dict(b=3, cin=32, cout=32, k=(1, 1), hw=(13, 33), act=0))
    s["bf16_3x3_res"] = ("bf16", 0, False, (1, 3, 11), dict(b=2, cin=64, cout=64, k=(3, 3), hw=(8, 33), act=1, res=True))
    s["bf16_3x3_c128"] = ("bf16", 0, False, (1, 3, 11), dict(b=2, cin=32, cout=128, k=(3, 3), hw=(8, 33), act=2))
    s["bf16_3x3_sums"] = ("bf16", 0, True, (1, 3, 11), dict(b=2, cin=32, cout=96, k=(3, 3), hw=(9, 33), act=1))
    s["bf16_s2"] = ("bf16", 0, False, (1, 3, 11), dict(b=2, cin=32, cout=64, k=(3, 3), hw=(17, 65), stride=2, act=0))
    return s


def _pad_specs():
    """padding= of conv_cl / conv_bf16_cl: none, more than k // 2 (columns, and with (3, 1) rows, whose whole window is
    padding), one-sided, stride 2 without padding, even kernels."""
    s = {}
    base = dict(b=2, cin=32, cout=128, hw=(6, 35))
    s["p_3x3_none"] = dict(base, k=(3, 3), pad=(0, 0), act=1)
    s["p_3x3_over"] = dict(base, k=(3, 3), pad=(2, 3), act=2)
    s["p_3x3_rows_out"] = dict(base, k=(3, 3), pad=(3, 1), act=2)
    s["p_5x3_over"] = dict(base, k=(5, 3), pad=(3, 3), act=1)
    s["p_3x3_h"] = dict(base, k=(3, 3), pad=(2, 0), act=0)
    s["p_3x3_w"] = dict(base, k=(3, 3), pad=(0, 2), act=1, bias=False)
    s["p_3x3_s2_none"] = dict(base, k=(3, 3), pad=(0, 0), stride=2, act=1, res=True, cout=64)
    s["p_2x2_s2"] = dict(base, k=(2, 2), pad=(0, 0), stride=2, act=2)
    s["p_4x2"] = dict(base, k=(4, 2), pad=(2, 1), act=1, res=True, cout=64)
    s["p_3x3_s2_over"] = dict(base, k=(3, 3), pad=(2, 3), stride=2, act=0)
    return s


BOUND_SPECS = _bound_specs()
EXACT_SPECS = _exact_specs()
WALK_SPECS = _walk_specs()
PAD_SPECS = {k: _spec(**v) for k, v in _pad_specs().items()}
# non-finite surroundings and the Inf pixel: one layer per family (3 x 3 for four of them, the two orientations of conv_wino1d)
POISON_SPECS = {"n_3x3": _spec(2, 32, 32, (3, 3), (6, 35), act=0, res=True), "n_7x3": _spec(2, 32, 32, (7, 3), (6, 35), act=0),
                "n_3x5": _spec(2, 32, 32, (3, 5), (6, 35), act=0)}
LIMIT_SPECS = {"cout2048": _spec(1, 32, 2048, (1, 1), (1, 3), act=0), "cout2048_x": _spec(1, 32, 2048, (1, 1), (1, 3), act=0, exact=True)}
SPECS = dict(BOUND_SPECS)
SPECS.update(EXACT_SPECS)
SPECS.update({k: _spec(**v[4]) for k, v in WALK_SPECS.items()})
SPECS.update({k + "/x": _spec(exact=True, **v[4]) for k, v in WALK_SPECS.items()})
SPECS.update(PAD_SPECS)
SPECS.update({k + "/x": dict(v, exact=True) for k, v in PAD_SPECS.items()})
SPECS.update(POISON_SPECS)
SPECS.update(LIMIT_SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    sp = SPECS[name]
    rng = np.random.default_rng(_seed("conv/" + name))
    b, cin, cout, k, stride = sp["b"], sp["cin"], sp["cout"], tuple(sp["k"]), sp["stride"]
    h, w = sp["hw"]
    pad = (k[0] // 2, k[1] // 2) if sp["pad"] is None else tuple(sp["pad"])
    ho, wo = out_size(h, w, k, stride, pad)
    c = types.SimpleNamespace(name=name, b=b, cin=cin, cout=cout, k=k, stride=stride, pad=pad, h=h, w=w, ho=ho, wo=wo, act=sp["act"],
                              sums=sp["sums"], exact=sp["exact"], K=cin * k[0] * k[1])
    if sp["exact"]:
        c.x = rng.integers(-4, 5, (b, h, w, cin)).astype(np.float64)
        c.wt = rng.integers(-8, 9, (cout, cin) + k) / 16.0
        c.bias = rng.integers(-32, 33, cout) / 8.0 if sp["bias"] else None
        c.res = rng.integers(-32, 33, (b, ho, wo, cout)) / 8.0 if sp["res"] else None
    else:
        c.x = _f32(rng.standard_normal((b, h, w, cin)))
        c.wt = _f32(rng.standard_normal((cout, cin) + k) * (2.0 / c.K) ** 0.5)
        c.bias = _f32(rng.standard_normal(cout)) if sp["bias"] else None
        c.res = _f32(rng.standard_normal((b, ho, wo, cout))) if sp["res"] else None
    if name.startswith("cout2048"):
        c.bias = np.arange(cout) / 8.0 - 100.0               # every entry its own number, the last ones included
    c.ref = conv_ref(c.x, c.wt, c.bias, c.res, c.act, stride, pad)
    c.mag = conv_direct(np.abs(c.x), np.abs(c.wt), stride, pad)
    c.side = (0.0 if c.bias is None else np.abs(c.bias)) + (0.0 if c.res is None else np.abs(c.res))
    # outputs whose whole window is padding
    c.all_pad = conv_direct(np.ones((1, h, w, 1)), np.ones((1, 1) + k), stride, pad)[0, :, :, 0] == 0
    assert c.K <= 4096
    if sp["exact"]:
        assert exact_condition(c, "igemm"), name
    return _freeze(c)


def mag_of(c, family):
    """The magnitude form of the family's own algorithm, [B, Ho, Wo, Cout]."""
    if family == "wino":
        return wino_mag(c.x, c.wt)
    if family == "wino1d":
        return wino1d_mag(c.x, c.wt)
    if family == "bf16":
        return conv_direct(np.abs(bf16_round(c.x)), np.abs(bf16_round(c.wt)), c.stride, c.pad)
    return c.mag


def exact_condition(c, family, sums=False):
    """Sufficient for every partial sum of the family's algorithm to be a float32 number on the case's data: everything is a
    multiple of 1 / 64, and the magnitude form (with bias and residual; with the sum table, summed per entry) stays below 2^24 / 64."""
    for a in (c.x, c.wt * 16, np.zeros(1) if c.bias is None else c.bias * 8, np.zeros(1) if c.res is None else c.res * 8):
        if not np.array_equal(a, np.round(a)):
            return False
    if np.abs(c.x).max() > 4 or np.abs(c.wt).max() > 0.5:
        return False
    m = mag_of(c, family) + c.side
    if sums:
        if c.act == 2:
            return False                         # a LeakyReLU output is no multiple of 1 / 64
        m = sum_table(m, sum_rows(family))
    return bool(m.max() * EXACT_DENOM < 2.0 ** 24)


@functools.lru_cache(maxsize=None)
def reference(name, family):
    """(ref, bound) [B, Ho, Wo, Cout] of a case for a family: conv_bf16 is held to the float64 result on bf16-rounded operands."""
    c = case(name)
    if family == "bf16":
        ref = conv_ref(bf16_round(c.x), bf16_round(c.wt), c.bias, c.res, c.act, c.stride, c.pad)
        bound = 1e-5 * mag_of(c, family) + 2.0 ** -23 * c.side + 1e-30
    elif family == "wino":
        ref, bound = c.ref, U * (c.cin + WINO_C) * mag_of(c, family) + U * EPI_C * c.side
    elif family == "wino1d":
        ref, bound = c.ref, U * (c.cin * max(c.k) + WINO1D_C) * mag_of(c, family) + U * (EPI_C - 1) * c.side
    else:
        ref, bound = c.ref, U * (c.K + DIRECT_C) * c.mag + U * EPI_C * c.side
    ref, bound = np.asarray(ref), np.asarray(bound) + np.zeros_like(c.ref)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


@functools.lru_cache(maxsize=None)
def restatement(name, family):
    """The family's algorithm in float32 numpy, [B, Ho, Wo, Cout] float32."""
    c = case(name)
    if family == "wino":
        out = wino_f32(c.x, c.wt, c.bias, c.res, c.act)
    elif family == "wino1d":
        out = wino1d_f32(c.x, c.wt, c.bias, c.act)
    elif family == "bf16":
        out = direct_f32(bf16_round(c.x), bf16_round(c.wt), c.bias, c.res, c.act, c.stride, c.pad)
    else:
        out = direct_f32(c.x, c.wt, c.bias, c.res, c.act, c.stride, c.pad)
    out.setflags(write=False)
    return out


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a)))


def worst_ratio(got, want, lim):
    """-> (every element inside its bound, worst error / bound).  Where the bound is 0 the error has to be 0; a NaN is outside
    every bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    ok = bool((err <= lim).all())
    pos = lim > 0
    return ok, (float((err[pos] / lim[pos]).max()) if pos.any() else 0.0)


# ---------------------------------------------------------------------------------------------
# where one non-finite input pixel may show
# ---------------------------------------------------------------------------------------------
def reach(c, y, x):
    """[Ho, Wo] bool: outputs whose window holds input pixel (y, x) -- the reference's, and a direct kernel's, reach."""
    probe = np.zeros((1, c.h, c.w, 1))
    probe[0, y, x, 0] = 1.0
    return conv_direct(probe, np.ones((1, 1) + c.k), c.stride, c.pad)[0, :, :, 0] > 0


def tile_reach(c, family, y, x):
    """[Ho, Wo] bool: the outputs of every Winograd tile whose input window holds pixel (y, x) -- a tile's input transform
    spreads a non-finite pixel over the tile (Inf - Inf).  conv_wino: 2 x 2 tiles; conv_wino1d: 1 x 2 tiles along the 3-tap axis."""
    r = reach(c, y, x)
    if family == "wino":
        ty, tx = (c.h + 1) // 2, (c.w + 1) // 2
        full = np.zeros((2 * ty, 2 * tx), dtype=bool)
        full[:c.h, :c.w] = r
        t = full.reshape(ty, 2, tx, 2).any(axis=(1, 3))
        return np.repeat(np.repeat(t, 2, axis=0), 2, axis=1)[:c.h, :c.w]
    assert family == "wino1d"
    if c.k[1] != 3:
        r = r.T
    ns = r.shape[1]
    ts = (ns + 1) // 2
    full = np.zeros((r.shape[0], 2 * ts), dtype=bool)
    full[:, :ns] = r
    t = np.repeat(full.reshape(-1, ts, 2).any(axis=2), 2, axis=1)[:, :ns]
    return t if c.k[1] == 3 else t.T

"""The temporal fusion kernels (csrc/tfusion.hip: tfusion_layer, tfusion_project with a bias; csrc/epilogue.hip: add_layer_norm)
against the float64 reference of tests/tfusion_cases.py on steered rows, at every size at which the kernels take another path:
(a) tfusion_layer per row group, (b) position independence, (c) non-finite inputs, (d) tfusion_project with a bias, (e)
add_layer_norm, (f) the engine's five launches as a chain, (g) the refusals, (h) InferenceEngine._add_norm.  Operands are slices
of wider NaN-filled buffers; the outputs start as sentinel-filled, wider and longer buffers (qp_next is dense by the ABI: longer
only).

The bars, per row group of 16 rows (tests/tfusion_cases.py says why no per-element bound): RMS error against float64 <=
RMS_FACTOR (2) x that of the float32 restatement in the kernel's order, largest error <= MAX_FACTOR x that RMS.  Both factors
are measured between two float32 restatements on the host (tests/test_host_tfusion_reference.py), never against a kernel.
Everything else is bitwise equality or the derived bound of the projection.

What the suite could not see before, and the case that covers it here:
  1. eps1 / eps2 swapped, one for both, or the model's 1e-5 whatever was passed: groups small_var and ffn_small_var of every
     steered case (f32 .. f4096: eps1 = 1e-3, eps2 = 1e-6); f512_model_eps keeps the model's pair.  test_layer_row_groups.
  2. one-pass moments: group big_mean (test_layer_row_groups, test_add_layer_norm_row_groups).
  3. the parameter block beyond one round of 2048 floats: f1216 / f1248 (2048 / 2080 floats), f3264 / f3296 (4096 / 4128), f4096.
  4. the pipeline's ends: f32 (two hidden tiles: prologue and epilogue slots only), f96 (six: two loop passes), hot_f*_j*: one live
     hidden tile j* in {0, 1, last - 1, last} at ffn 32, 64, 96 (b1 one tile late, a hidden tile on a neighbour's W2 k-tile).
  5. o_pitch > 128 and what the kernel leaves beside and behind its output: every case with opitch; the sentinel checks of _run_layer.
  6. nq in {0, 4, 20, 48, 64} and tokens in {1, 15, 16, 17, 63, 64, 65, 129}: f* and t*; test_layer_position_independence.
  7. tfusion_project with a bias at cout 4, 20, 48, 100, 128, 2048, eight jobs, jobs with and without a bias and of
     1 .. 129 tokens in one launch: test_project_with_bias.
  8. InferenceEngine._add_norm at a width the kernel is not built for: test_engine_add_norm_widths.

With SMOS_TFUSION_RATIOS_FILE set, the per-case figures are appended to that file (profiles/tfusion_error_ratios.txt is made from it)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import tfusion_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = -1.25e30                 # what the outputs hold before a launch
TAIL = 3                        # rows behind `tokens` in every output buffer
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("SMOS_TFUSION_RATIOS_FILE")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("\n".join(_LINES) + "\n")


def _note(line):
    print(line)
    _LINES.append(line)


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _rows_in_nan(a, pitch=None, off=0):
    """a [n, c] -> a view of a NaN-filled buffer that holds it: a channel slice at `off` of rows of `pitch` floats, or (pitch
    None) a row range of a longer dense buffer."""
    n, c = a.shape
    if pitch is None:
        buf = torch.full((n + 2, c), NAN, device=DEV)
        buf[1:n + 1] = _t(a)
        return buf[1:n + 1]
    buf = torch.full((n, pitch), NAN, device=DEV)
    buf[:, off:off + c] = _t(a)
    return buf[:, off:off + c]


def _sentinel(rows, pitch):
    return torch.full((rows, pitch), SENT, device=DEV)


def _is_sentinel(t):
    return bool((t == SENT).all())


@functools.lru_cache(maxsize=None)
def _prep(name):
    c = cases.layer_case(name)
    return _prep_of(c)


def _prep_of(c):
    return ops.TfusionLayer((_t(c.wo), _t(c.bo)), (_t(c.g1), _t(c.be1), c.eps[0]), (_t(c.w1), _t(c.b1)), (_t(c.w2), _t(c.b2)),
                            (_t(c.g2), _t(c.be2), c.eps[1]), next_qproj=(_t(c.wq), _t(c.bq)) if c.nq else None)


def _layer_raw(sampled_ptr, query_ptr, q_pitch, prep, out_ptr, o_pitch, nxt_ptr, nq, tokens, ffn, eps, dev_tensor):
    """smos_tfusion_layer itself (include/smos.h): the wrapper allocates qp_next and so cannot show what lies behind it."""
    lib = _lib.load()
    rc = lib.smos_tfusion_layer(sampled_ptr, query_ptr, q_pitch, prep.stream.data_ptr(), prep.params.data_ptr(), out_ptr, o_pitch,
                                nxt_ptr, nq, tokens, ffn, eps[0], eps[1], ops._stream(dev_tensor))
    _lib.check(rc, "smos_tfusion_layer")


def _run_layer(c, prep, sampled=None, query=None):
    """One launch on NaN-surrounded operands into sentinel-filled outputs -> (out [tokens, 128], qp_next [tokens, nq] or None) as
    float32 numpy.  Asserts that the neighbour channels of `out` and the rows behind `tokens` of both outputs keep the sentinel."""
    s = _rows_in_nan(c.sampled if sampled is None else sampled)
    q = _rows_in_nan(c.query if query is None else query, *(cases.Q_SLICE if c.qpitch else (None, 0)))
    pitch, off = cases.O_SLICE if c.opitch else (128, 0)
    obuf = _sentinel(c.tokens + TAIL, pitch)
    nbuf = _sentinel(c.tokens + TAIL, c.nq) if c.nq else None
    out = obuf[:c.tokens, off:off + 128]
    _layer_raw(s.data_ptr(), q.data_ptr(), q.stride(0), prep, out.data_ptr(), pitch, nbuf.data_ptr() if c.nq else None, c.nq,
               c.tokens, c.ffn, c.eps, s)
    assert _is_sentinel(obuf[c.tokens:]) and _is_sentinel(obuf[:, :off]) and _is_sentinel(obuf[:, off + 128:]), "out: wrote outside its slice"
    assert nbuf is None or _is_sentinel(nbuf[c.tokens:]), "qp_next: wrote behind its rows"
    return out.cpu().numpy(), None if nbuf is None else nbuf[:c.tokens].cpu().numpy()


def _check_groups(tag, c, got, ref, rest):
    for g, rows in c.rows.items():
        r, m = cases.figures(got, ref, rest, rows)
        _note("tfusion-ratio %-36s %-14s rms %.3f  max %.2f" % (tag, g, r, m))
        assert r <= cases.RMS_FACTOR, (tag, g, "RMS error against float64 over twice the float32 restatement's", r)
        assert m <= cases.MAX_FACTOR, (tag, g, "largest error over MAX_FACTOR times the float32 restatement's RMS error", m)


# ---------------------------------------------------------------------------------------------
# a. tfusion_layer, every case
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.LAYER_SPECS))
def test_layer_row_groups(name):
    """Every case of tests/tfusion_cases.py::LAYER_SPECS: both bars per row group for the output and for qp_next, the sentinels
    around both, and the 16 constant rows (q1 = beta1) as 16 identical output rows.
    Item 1 (eps1 / eps2): groups small_var and ffn_small_var of f32 .. f4096 at eps (1e-3, 1e-6); f512_model_eps at the model's pair.
    Item 2 (two-pass moments): group big_mean of the same cases.
    Item 3 (parameter rounds of 2048 floats): f1216 / f1248, f3264 / f3296, f4096 -- the last b1 tiles, b2, g2, be2 and bq come
    from the second and third round.
    Item 4 (the pipeline's ends): f32 (no loop pass), f96 (two), hot_f32_j0 .. hot_f96_j5 (one live hidden tile).
    Item 5 (o_pitch 192 at channel offset 32, sentinels beside and behind): t16, t64, f32, f96, f512, f1248, f3264, f4096, hot_*_j1 / j3 / j5.
    Item 6 (nq 0, 4, 20, 48, 64; tokens 1, 15, 16, 17, 63, 64, 65, 129): f96 (no next projection), f32 / f3296 (4), f64 / f3264 (20),
    f1216 / f4096 (64), t1 .. t129."""
    c = cases.layer_case(name)
    got, nxt = _run_layer(c, _prep(name))
    rest, rest_next = cases.layer_restatement(name)
    _check_groups("layer/" + name + " out", c, got, c.ref, rest)
    if c.nq:
        _check_groups("layer/" + name + " qp_next", c, nxt, c.ref_next, rest_next)
    if "const" in c.rows:
        rows = got[c.rows["const"]]
        assert np.array_equal(rows.view(np.uint32), np.broadcast_to(rows[0], rows.shape).view(np.uint32))
        if c.nq:
            rows = nxt[c.rows["const"]]
            assert np.array_equal(rows.view(np.uint32), np.broadcast_to(rows[0], rows.shape).view(np.uint32))


# ---------------------------------------------------------------------------------------------
# b. position independence
# ---------------------------------------------------------------------------------------------
def test_layer_position_independence():
    """Item 6: a token's result depends on its row alone -- row r of the 129-token launch equals, bit for bit, the same row run
    alone (tokens = 1) and placed at index 0, 15, 16 and 64 of another launch; a second call gives the same bits.  Through
    ops.tfusion_layer, the engine's call."""
    c = cases.layer_case("t129")
    prep = _prep("t129")
    sampled, query = _t(c.sampled), _t(c.query)
    out, nxt = ops.tfusion_layer(sampled, query, prep)
    out2, nxt2 = ops.tfusion_layer(sampled, query, prep)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(nxt.view(torch.int32), nxt2.view(torch.int32))
    rng = np.random.default_rng(7)
    fill_s, fill_q = _t(rng.standard_normal((65, 128))), _t(rng.standard_normal((65, 128)))
    for r in (0, 5, 63, 64, 77, 128):
        o1, n1 = ops.tfusion_layer(sampled[r:r + 1].contiguous(), query[r:r + 1].contiguous(), prep)
        assert torch.equal(o1[0].view(torch.int32), out[r].view(torch.int32)) and torch.equal(n1[0].view(torch.int32), nxt[r].view(torch.int32)), r
        s, q = fill_s.clone(), fill_q.clone()
        for at in (0, 15, 16, 64):
            s[at], q[at] = sampled[r], query[r]
        o2, n2 = ops.tfusion_layer(s, q, prep)
        for at in (0, 15, 16, 64):
            assert torch.equal(o2[at].view(torch.int32), out[r].view(torch.int32)), (r, at)
            assert torch.equal(n2[at].view(torch.int32), nxt[r].view(torch.int32)), (r, at)


# ---------------------------------------------------------------------------------------------
# c. non-finite inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,row,ch,value", [("sampled", 70, 5, NAN), ("query", 3, 100, float("inf")), ("query", 128, 0, -float("inf"))])
def test_layer_non_finite_input_stays_in_its_row(which, row, ch, value):
    """One NaN in `sampled` or one Inf in `query` at row r: row r of out and qp_next is all NaN, as in the reference; every other
    row has the bits of the clean launch."""
    c = cases.layer_case("t129")
    prep = _prep("t129")
    clean, clean_next = _run_layer(c, prep)
    sampled, query = c.sampled.copy(), c.query.copy()
    (sampled if which == "sampled" else query)[row, ch] = value
    want, want_next = cases.layer_ref(c, sampled, query)
    assert np.isnan(want[row]).all() and np.isnan(want_next[row]).all() and np.isfinite(np.delete(want, row, 0)).all()
    got, got_next = _run_layer(c, prep, sampled, query)
    assert np.isnan(got[row]).all() and np.isnan(got_next[row]).all()
    keep = np.arange(c.tokens) != row
    assert np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))
    assert np.array_equal(got_next[keep].view(np.uint32), clean_next[keep].view(np.uint32))


# ---------------------------------------------------------------------------------------------
# d. tfusion_project with a bias
# ---------------------------------------------------------------------------------------------
P_PAD, P_OFF = 24, 8            # extra columns / column offset of a wide output matrix


def _project_jobs(jobs):
    dev, bufs = [], []
    for j in jobs:
        x = _rows_in_nan(j.x, *(cases.Q_SLICE if j.xpitch else (None, 0)))
        buf = torch.full((j.tokens + TAIL, j.cout + P_PAD), NAN, device=DEV) if j.wide else None
        out = None if buf is None else buf[:j.tokens, P_OFF:P_OFF + j.cout]
        dev.append((x, ops.tfusion_pack_linear(_t(j.w)), _t(j.b) if j.b is not None else j.cout, out))
        bufs.append(buf)
    return dev, bufs


@pytest.mark.parametrize("name", cases.PROJECT_NAMES)
def test_project_with_bias(name):
    """Item 7: the launches of tests/tfusion_cases.py::PROJECT_SPECS.  The exact twins ("/x") bit for bit; the random ones inside
    Cin u |x| @ |W|^T + 2 u |bias| (tests/util.py::tap_products_bound and the one addition of TF_EMIT); pitched x; out as a column
    range of a wider NaN matrix whose other columns and rows stay NaN."""
    jobs = cases.project_case(name)
    dev, bufs = _project_jobs(jobs)
    outs = ops.tfusion_project(dev)
    worst = 0.0
    for j, o, buf in zip(jobs, outs, bufs):
        got = o.cpu().numpy()
        assert got.shape == (j.tokens, j.cout)
        if buf is not None:
            assert o.data_ptr() == buf[:, P_OFF:].data_ptr()
            assert bool(torch.isnan(buf[j.tokens:]).all()) and bool(torch.isnan(buf[:, :P_OFF]).all()) and bool(torch.isnan(buf[:, P_OFF + j.cout:]).all())
        if j.exact:
            assert np.array_equal(got.view(np.uint32), j.ref.astype(np.float32).view(np.uint32)), (name, j.tokens, j.cout)
        else:
            err, lim = np.abs(got.astype(np.float64) - j.ref), cases.project_bound(j)
            assert (err <= lim).all(), (name, j.tokens, j.cout, float((err / lim).max()))
            worst = max(worst, float((err / lim).max()))
    if not jobs[0].exact:
        _note("tfusion-ratio project/%-28s worst error / bound %.4f" % (name, worst))


def test_project_eight_jobs_run_nine_raise():
    """Eight jobs are one launch (tok8 above); nine raise and write nothing."""
    jobs = cases.project_case("tok8")
    dev, bufs = _project_jobs(jobs + jobs[:1])
    with pytest.raises(RuntimeError, match="1..8 jobs"):
        ops.tfusion_project(dev)
    assert all(b is None or bool(torch.isnan(b).all()) for b in bufs)
    assert len(ops.tfusion_project(dev[:8])) == 8


# ---------------------------------------------------------------------------------------------
# e. add_layer_norm
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.ALN_SPECS))
def test_add_layer_norm_row_groups(name):
    """Items 1 and 2 for the SMOS_TFUSION=0 route: the same row groups and bars at C = 64, 128, 256, 512 with and without `res`, and
    1, 3, 4, 5 and 1000 rows (four waves per block)."""
    c = cases.aln_case(name)
    x = _rows_in_nan(c.x)
    res = None if c.res is None else _rows_in_nan(c.res)
    got = ops.add_layer_norm(x, res, _t(c.g), _t(c.b), c.eps).cpu().numpy()
    _check_groups("aln/" + name, c, got, c.ref, cases.aln_f32(c))


# ---------------------------------------------------------------------------------------------
# f. the engine's five launches
# ---------------------------------------------------------------------------------------------
def test_chain_of_five_launches():
    """tfusion_project (two value projections + the first offset / logit projection), msda_fwd_qp, tfusion_layer with the next
    projection, msda_fwd_qp, tfusion_layer on a 6 x 7 lattice, B = 2, as InferenceEngine._temporal_fusion issues them, against
    the float64 chain (util.msda_qp_formulation + the layer reference) with both bars against the float32 chain
    (util.msda_qp_float32_oracle + the layer restatement): the [offsets | logits] layout of qp_next and the [B, Lq, heads, 32]
    view of the value projection are what the sampler reads."""
    c = cases.chain_case()
    b, lq = c.b, c.h * c.w
    src, query = _t(c.src), _t(c.query)
    preps = [_prep_of(L) for L in c.layers]
    jobs = [(src, ops.tfusion_pack_linear(_t(L.wv)), _t(L.bv)) for L in c.layers]
    jobs.append((query, ops.tfusion_pack_linear(_t(c.wq0)), _t(c.bq0)))
    outs = ops.tfusion_project(jobs)
    qp = outs[-1]
    for i, prep in enumerate(preps):
        sampled = ops.msda_fwd_qp(outs[i].view(b, lq, c.m, 32), qp.view(b, lq, -1), c.h, c.w, c.p)
        query, qp = ops.tfusion_layer(sampled, query, prep)
    assert qp is None
    want, rest = cases.chain_run(np.float64), cases.chain_run(np.float32)
    r, m = cases.figures(query.reshape(-1, 128).cpu().numpy(), want, rest)
    _note("tfusion-ratio %-36s %-14s rms %.3f  max %.2f" % ("chain", "all", r, m))
    assert r <= cases.RMS_FACTOR and m <= cases.MAX_FACTOR, (r, m)


# ---------------------------------------------------------------------------------------------
# g. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    """tokens = 2^22, ffn 48 and 4128, nq 6 and 68, a pointer 8 bytes off alignment, pitch 124 and C = 192 for
    smos_add_layer_norm raise RuntimeError and write nothing."""
    c = cases.layer_case("t17")
    prep = _prep("t17")
    s, q = _t(c.sampled), _t(c.query)
    obuf, nbuf = _sentinel(c.tokens + TAIL, 128), _sentinel(c.tokens + TAIL, c.nq)
    ok = dict(sampled_ptr=s.data_ptr(), query_ptr=q.data_ptr(), q_pitch=128, prep=prep, out_ptr=obuf.data_ptr(), o_pitch=128,
              nxt_ptr=nbuf.data_ptr(), nq=c.nq, tokens=c.tokens, ffn=c.ffn, eps=c.eps, dev_tensor=s)
    for change in (dict(tokens=1 << 22), dict(ffn=48), dict(ffn=4128), dict(ffn=16), dict(nq=6), dict(nq=68), dict(sampled_ptr=s.data_ptr() + 8),
                   dict(out_ptr=obuf.data_ptr() + 8), dict(q_pitch=124), dict(o_pitch=124), dict(tokens=0)):
        with pytest.raises(RuntimeError, match="tfusion_layer"):
            _layer_raw(**dict(ok, **change))
        assert _is_sentinel(obuf) and _is_sentinel(nbuf), change
    w = lambda o, i: (torch.zeros((o, i), device=DEV), torch.zeros(o, device=DEV))
    norm = (torch.ones(128, device=DEV), torch.zeros(128, device=DEV), 1e-5)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.TfusionLayer(w(128, 128), norm, w(48, 128), w(128, 48), norm)
    for nq in (6, 68):
        with pytest.raises(RuntimeError, match="4..64 output channels"):
            ops.TfusionLayer(w(128, 128), norm, w(64, 128), w(128, 64), norm, next_qproj=w(nq, 128))
    big = ops.TfusionLayer(w(128, 128), norm, w(4128, 128), w(128, 4128), norm)              # the packer takes it, the kernel does not
    with pytest.raises(RuntimeError, match="tfusion_layer"):
        ops.tfusion_layer(s, q, big, out=obuf[:c.tokens])
    assert _is_sentinel(obuf)
    # smos_add_layer_norm is built for 64, 128, 256 and 512 channels
    x, out = torch.zeros((5, 192), device=DEV), _sentinel(5, 192)
    lib = _lib.load()
    rc = lib.smos_add_layer_norm(x.data_ptr(), None, x.data_ptr(), x.data_ptr(), out.data_ptr(), 5, 192, 1e-5, ops._stream(x))
    assert rc != 0 and _is_sentinel(out)
    with pytest.raises(RuntimeError, match="add_layer_norm"):
        ops.add_layer_norm(x, None, x[0], x[0], 1e-5)
    # the launch after a refusal is a good one
    _layer_raw(**ok)
    assert not _is_sentinel(obuf[:c.tokens]) and _is_sentinel(obuf[c.tokens:]) and _is_sentinel(nbuf[c.tokens:])


# ---------------------------------------------------------------------------------------------
# h. InferenceEngine._add_norm
# ---------------------------------------------------------------------------------------------
def _stable_layer_norm_bound(c):
    """Per element, for ANY float32 LayerNorm(x + res) that takes its moments stably (two-pass or Welford, in any order), u = 2^-24:

        u ((C + 2) max|x| rstd |g|  +  (C / 2 + 8) |ref - beta|  +  2 |ref|)

    The mean is a sum of C terms: at most C roundings of at most u C max|x| each, over C -- the centred value is off by at most
    (C + 2) u max|x| with the roundings of x + res and of the subtraction, which rstd |g| carries to the output.  That common
    shift moves the variance in the second order only; its own sum has a relative error of at most (C + 4) u, half of it arrives
    in rstd, + 4 for the root, the division and the two products: (C / 2 + 8) u of |ref - beta|.  The last product and the
    addition of beta: 2 u |ref|.  The two float32 restatements of tests/tfusion_cases.py use 0.012 of it on these rows; it does not
    tell moment algorithms apart (a one-pass variance reaches 0.96 of it here) -- it holds the route, the operands and eps."""
    x = c.x + c.res
    rstd = 1.0 / np.sqrt(x.var(-1, keepdims=True) + c.eps)
    return cases.U * ((c.ch + 2) * np.abs(x).max(-1, keepdims=True) * rstd * np.abs(c.g) + (c.ch / 2 + 8) * np.abs(c.ref - c.b) + 2 * np.abs(c.ref))


@pytest.mark.parametrize("ch", (128, 192))
def test_engine_add_norm_widths(ch):
    """Item 8: _add_norm takes the kernel for the widths it is built for (128: the two bars of the kernel) and torch's layer_norm
    for the others (192, which smos_add_layer_norm refuses and the engine used to send there).  torch's kernel is not this
    project's: it is held to the derived bound of any stable float32 LayerNorm (_stable_layer_norm_bound), which the `eps = 1e-5
    whatever was passed` mutant of the reference exceeds on the small-variance rows (asserted)."""
    from streammos_amd.engine import InferenceEngine
    rng = np.random.default_rng(cases._seed("tfusion/add_norm/%d" % ch))
    c = types.SimpleNamespace(ch=ch, eps=1e-3, n=37, rows={"randn": slice(0, 16), "small_var": slice(16, 32), "tail": slice(32, 37)})
    want = rng.standard_normal((37, ch))
    want[16:32] = 3.0 + 0.02 * rng.standard_normal((16, ch))
    c.x = cases._f32(rng.standard_normal((37, ch)))
    c.res = cases._f32(want - c.x)
    c.g, c.b = cases._f32(1.0 + 0.3 * rng.standard_normal(ch)), cases._f32(0.2 * rng.standard_normal(ch))
    c.ref = cases.aln_ref(c)
    got = InferenceEngine._add_norm(_t(c.x), _t(c.res), (_t(c.g), _t(c.b), c.eps), ch)
    assert got.shape == (37, ch)
    got = got.cpu().numpy()
    if ch == 128:
        _check_groups("engine_add_norm/c%d" % ch, c, got, c.ref, cases.aln_f32(c))
        return
    lim = _stable_layer_norm_bound(c)
    err = np.abs(got.astype(np.float64) - c.ref)
    _note("tfusion-ratio %-36s worst error / bound %.4f" % ("engine_add_norm/c%d (torch)" % ch, float((err / lim).max())))
    assert (err <= lim).all(), float((err / lim).max())
    wrong = np.abs(cases.aln_ref(c, "eps_1e5") - c.ref)[c.rows["small_var"]]
    assert (wrong > 4 * lim[c.rows["small_var"]]).mean() > 0.9

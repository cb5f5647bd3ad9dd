"""The decoder's tap products as three exact bf16 limbs per fp32 operand on the bf16 matrix pipe (csrc/tap_bf16x3.hip,
ops.tap_products_bf16x3; the default of ops.upconv3x3) against float64, inside the bound the fp32 form is held to:
Cin u |x| |W|^T per element, u = 2^-24 (tests/util.py::tap_products_bound; the host side of the derivation:
tests/test_host_tap_bf16x3.py).  Modelled on tests/test_gpu_upconv.py::test_tap_products_column_range_jobs_of_tfusion_project.

  column-range jobs   token pairs at every tile edge of a 32 / 64 / 128-token geometry, a 1-token job beside a long one,
                      cout 12 .. 1152 per job, dense and sliced x, out inside a sentinel frame, 1 / 2 / 3 ranges: same bits
  values              exact inputs bit for bit; random ones, rows scaled by 2^40 and 2^-40, 1e6 beside 1e-6 in a row inside
                      the bound; the fp32 kernel's worst ratio printed beside this one's (profiles/tap_bf16x3.txt)
  limb products       operands built limb by limb whose product is exact in fp32: each of the six products bit for bit
  cout edges          4 .. 2048 as eight jobs of one launch on 70 tokens; nine jobs raise
  ops.upconv3x3       the default form on the 128-channel cases, against float64 and against the fp32 form
  engine              two streamed frames, default against SMOS_TAP_GEMM=tf
"""
import contextlib
from unittest import mock

import numpy as np
import pytest
import torch

from streammos_amd import ops
from tests import cases, util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0
_PAD_L, _PAD_R, _PAD_ROWS = 8, 8, 3
_TOKEN_PAIRS = ((1, 15), (31, 33), (63, 64), (65, 200), (200, 1), (127, 129))      # (source 1, source 2) of one launch


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _check(label, got, want, bound):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert tuple(got.shape) == tuple(want.shape), (label, got.shape, want.shape)
    ok, ratio = util.msda_worst_ratio(got, want, bound)
    print("tap-bf16x3-ratio %-72s %.4f" % (label, ratio))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)
    return ratio


def _ratio(got, want, bound):
    return util.msda_worst_ratio(got.detach().cpu().numpy(), want, bound)[1]


def _framed(tokens, width):
    buf = torch.full((tokens + _PAD_ROWS, _PAD_L + width + _PAD_R), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[:tokens, _PAD_L:_PAD_L + width]


def _frame_intact(buf, tokens, width):
    return (bool((buf[:, :_PAD_L] == SENTINEL).all()) and bool((buf[:, _PAD_L + width:] == SENTINEL).all()) and
            bool((buf[tokens:] == SENTINEL).all()))


# ------------------------------------------------------------------------------------------
# 1. column-range jobs
# ------------------------------------------------------------------------------------------
def _tap_problem(ch, kind):
    rng = np.random.default_rng(util._seed("tap_bf16x3/taps/%d/%s" % (ch, kind)))
    nks = [util.tap_matrix(util.upconv_inputs(rng, (ch, 128, 3, 3), kind, (2.0 / (9 * 128)) ** 0.5)) for _ in range(2)]
    xs = {t: util.upconv_inputs(rng, (t, 128), kind) for t in sorted(set(sum(_TOKEN_PAIRS, ())))}
    return nks, xs


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("ch", [4, 32, 128])
def test_column_range_jobs(ch, kind):
    """[tokens, 9*C] matrices of two sources, each written by 1, 2 and 3 column-range jobs of one launch into a view of a wider
    and taller sentinel buffer: exact inputs bit for bit equal to x @ nk.T in float64, random ones inside Cin u |x| |nk|^T; the
    same bits for every number of ranges; the sentinel survives left of, right of and below the matrix.  9*4 / 2 = 18 is no
    multiple of 4: the kernel refuses that job list and writes nothing."""
    nks, xs = _tap_problem(ch, kind)
    wts = []
    for nk in nks:
        w = _t(nk).reshape(3, 3, ch, 128).permute(2, 3, 0, 1).contiguous()
        wts.append(ops.upconv_tap_weights(w, 0, 128))
        assert torch.equal(wts[-1].nk, _t(nk))
    width = 9 * ch
    for pair in _TOKEN_PAIRS:
        for layout in ("dense", "slice"):
            dev_x = []
            for t in pair:
                if layout == "dense":
                    dev_x.append(_t(xs[t]))
                else:
                    wide = torch.full((t, 192), SENTINEL, dtype=torch.float32, device=DEV)
                    wide[:, 32:160] = _t(xs[t])
                    dev_x.append(wide[:, 32:160])
            results = {}
            for parts in (1, 2, 3):
                n = width // parts
                framed = [_framed(t, width) for t in pair]
                jobs = [(x, ws_k, n, view[:, k * n:(k + 1) * n])
                        for x, wt, (_, view) in zip(dev_x, wts, framed) for k, ws_k in enumerate(wt.limb_stream(parts))]
                assert len(jobs) == 2 * parts
                if n % 4:
                    with pytest.raises(RuntimeError, match="tap_products_bf16x3: bad job"):
                        ops.tap_products_bf16x3(jobs)
                    torch.cuda.synchronize()
                    assert all(bool((buf == SENTINEL).all()) for buf, _ in framed)
                    continue
                outs = ops.tap_products_bf16x3(jobs)
                assert all(o is job[3] for o, job in zip(outs, jobs))
                for (buf, _), t in zip(framed, pair):
                    assert _frame_intact(buf, t, width), "tokens %s, %s x, %d ranges: the sentinel frame was written" % (pair, layout, parts)
                results[parts] = [view.cpu().numpy() for _, view in framed]
            for parts in results:
                for a, b in zip(results[parts], results[1]):
                    assert np.array_equal(a, b), "tokens %s, %s x: %d column ranges differ from 1" % (pair, layout, parts)
            for t, nk, got in zip(pair, nks, results[1]):
                want = util.tap_products_ref(xs[t], nk)
                label = "taps C=%d %s %s x tokens=%d (next to %d)" % (ch, kind, layout, t, pair[0] + pair[1] - t)
                if kind == "exact":
                    assert np.array_equal(got.astype(np.float64), want), label
                _check(label, got, want, util.tap_products_bound(xs[t], nk))


# ------------------------------------------------------------------------------------------
# 2. values
# ------------------------------------------------------------------------------------------
def _value_cases():
    """name -> (x [200, 128], nk [1152, 128]) as float64 arrays of float32 numbers."""
    rng = np.random.default_rng(util._seed("tap_bf16x3/values"))
    nk_exact = util.tap_matrix(util.upconv_inputs(rng, (128, 128, 3, 3), "exact", 0.5))
    nk = util.tap_matrix(util.upconv_inputs(rng, (128, 128, 3, 3), "random", (2.0 / (9 * 128)) ** 0.5))
    x = util.upconv_inputs(rng, (200, 128), "random")
    scale = np.where(np.arange(200) % 2 == 0, 2.0 ** 40, 2.0 ** -40)[:, None]                   # exact scalings
    mixed = util._f32(np.where(rng.random((200, 128)) < 0.5, 1e6, 1e-6) * rng.standard_normal((200, 128)))
    return {
        "exact": (util.upconv_inputs(rng, (200, 128), "exact"), nk_exact),
        "random": (x, nk),
        "relu activations": (util._f32(3.0 * np.maximum(x, 0.0)), nk),
        "rows scaled by 2^40 and 2^-40": (x * scale, nk),
        "1e6 and 1e-6 within a row": (mixed, nk),
    }


def test_values_against_float64_beside_the_fp32_kernel():
    """The assertion is the project's bound for the fp32 form itself.  The worst error / bound of this kernel and of
    ops.tfusion_project on the same inputs are printed side by side (MI355X figures: profiles/tap_bf16x3.txt)."""
    for name, (x, nk) in _value_cases().items():
        assert np.array_equal(util._f32(x), x) and np.isfinite(x).all()
        want, bound = util.tap_products_ref(x, nk), util.tap_products_bound(x, nk)
        dx, dw = _t(x), _t(nk)
        got = ops.tap_products_bf16x3([(dx, ops.tap_limbs_pack(dw), 1152)])[0]
        fp32 = ops.tfusion_project([(dx, ops.tfusion_pack_linear(dw), 1152)])[0]
        print("tap-bf16x3-ratio values %-34s fp32 kernel (tfusion_project) %.4f" % (name, _ratio(fp32, want, bound)))
        if name == "exact":
            assert np.array_equal(got.cpu().numpy().astype(np.float64), want)
        _check("values %s" % name, got, want, bound)
        again = ops.tap_products_bf16x3([(dx, ops.tap_limbs_pack(dw), 1152)])[0]
        assert torch.equal(got, again), "a second call gives other bits"


def _sparse_rows(rng, shape, values, nonzero=8):
    """`nonzero` entries per row at random channels drawn from `values`, the rest 0."""
    out = np.zeros(shape)
    for row in out:
        row[rng.choice(shape[1], nonzero, replace=False)] = rng.choice(values, nonzero)
    return out


def test_each_of_the_six_limb_products_bit_for_bit():
    """Operands built limb by limb, 8 non-zero terms per output, so that every partial sum is a multiple of 2^-18 below 2^5
    and the whole product is exact in float32: the kernel must equal float64 bit for bit, and it cannot if one of its six limb
    products is missing or reads the wrong limb.  +-1.5 (or +-1) is the high limb, +-2^-9 the middle one, +-2^-18 the low one
    (in the binade of 1.5 half a bf16 step is 2^-8, and 2^-9 (1 +- 2^-9) rounds to 2^-9: the limbs are exactly these).
      two limbs x two limbs      hh, hm, mh and mm (a multiple of 2^-18: nothing else reaches those bits)
      three limbs x high only    xl wh and xm wh
      high only x three limbs    xh wl and xh wm"""
    rng = np.random.default_rng(util._seed("tap_bf16x3/limbs"))
    one = np.array([-1.0, 1.0])
    two = np.array([s * (1.5 + m * 2.0 ** -9) for s in (-1.0, 1.0) for m in (-1.0, 1.0)])
    three = np.array([s * (1.5 + m * 2.0 ** -9 + l * 2.0 ** -18) for s in (-1.0, 1.0) for m in (-1.0, 1.0) for l in (-1.0, 1.0)])
    for name, xv, wv in (("two limbs x two limbs", two, two), ("three limbs x high only", three, one),
                         ("high only x three limbs", one, three)):
        x = _sparse_rows(rng, (70, 128), xv)
        w = rng.choice(wv, (96, 128))
        for v, vals in ((x, xv), (w, wv)):                          # the limbs are what the construction says
            lo, mid, hi = (t.double().numpy() for t in ops.tap_limbs_split(torch.tensor(v, dtype=torch.float32)))
            assert np.array_equal(hi + mid + lo, v) and set(np.unique(np.abs(hi))) <= {0.0, 1.0, 1.5}
            assert (np.abs(mid[v != 0]) == (2.0 ** -9 if len(vals) > 2 else 0.0)).all()
            assert (np.abs(lo[v != 0]) == (2.0 ** -18 if len(vals) > 4 else 0.0)).all()
        want = util.tap_products_ref(x, w)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        got = ops.tap_products_bf16x3([(_t(x), ops.tap_limbs_pack(_t(w)), 96)])[0].cpu().numpy().astype(np.float64)
        # what a missing product would leave: the sum without it differs from the full one somewhere
        assert np.array_equal(got, want), "%s: not the exact product" % name
        print("tap-bf16x3-ratio limbs %-30s exact" % name)


def test_non_finite_inputs_give_non_finite_outputs():
    rng = np.random.default_rng(util._seed("tap_bf16x3/nonfinite"))
    x = util.upconv_inputs(rng, (40, 128), "random")
    nk = util.upconv_inputs(rng, (36, 128), "random", 0.1)
    x[3, 17], x[9, 100], x[33, 0] = np.inf, np.nan, -np.inf
    got = ops.tap_products_bf16x3([(_t(x), ops.tap_limbs_pack(_t(nk)), 36)])[0].cpu().numpy()
    bad = np.zeros(40, dtype=bool)
    bad[[3, 9, 33]] = True
    assert not np.isfinite(got[bad]).any() and np.isfinite(got[~bad]).all()
    clean = np.where(np.isfinite(x), x, 0.0)
    _check("finite rows beside non-finite ones", got[~bad], util.tap_products_ref(clean, nk)[~bad], util.tap_products_bound(clean, nk)[~bad])


# ------------------------------------------------------------------------------------------
# 3. cout edges, job count
# ------------------------------------------------------------------------------------------
def test_cout_edges_as_eight_jobs_and_nine_raise():
    """cout = 4, 28, 32, 36, 60, 64, 68 and 2048 (one to 64 output tiles of 32, the last one partly or wholly used; an odd and
    an even tile count) as eight jobs of one launch on 70 tokens, each into its own sentinel frame.  A ninth job: refused,
    nothing written."""
    rng = np.random.default_rng(util._seed("tap_bf16x3/edges"))
    tokens, couts = 70, (4, 28, 32, 36, 60, 64, 68, 2048, 8)
    x = util.upconv_inputs(rng, (tokens, 128), "random")
    ws = [util.upconv_inputs(rng, (o, 128), "random", 128 ** -0.5) for o in couts]
    framed = [_framed(tokens, o) for o in couts]
    dev_x = _t(x)
    jobs = [(dev_x, ops.tap_limbs_pack(_t(w)), o, view) for w, o, (_, view) in zip(ws, couts, framed)]
    with pytest.raises(RuntimeError, match="1..8 jobs"):
        ops.tap_products_bf16x3(jobs)
    torch.cuda.synchronize()
    assert all(bool((buf == SENTINEL).all()) for buf, _ in framed)
    ops.tap_products_bf16x3(jobs[:8])
    for w, o, (buf, view) in list(zip(ws, couts, framed))[:8]:
        assert _frame_intact(buf, tokens, o), o
        _check("plain job cout=%d" % o, view, util.tap_products_ref(x, w), util.tap_products_bound(x, w))
    assert bool((framed[8][0] == SENTINEL).all())
    with pytest.raises(RuntimeError, match="limb stream"):
        ops.tap_products_bf16x3([(dev_x, ops.tfusion_pack_linear(_t(ws[0])), 4)])        # the fp32 kernel's weight stream
    with pytest.raises(RuntimeError, match="GPU"):
        ops.tap_products_bf16x3([(dev_x.cpu(), jobs[0][1], 4)])


# ------------------------------------------------------------------------------------------
# 4. the whole op
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _tap_form(gemm, parts=3):
    with mock.patch.object(ops, "_TAP_GEMM", gemm), mock.patch.object(ops, "_TAP_GEMM_OWN", gemm == "conv"), \
            mock.patch.object(ops, "_TAP_PARTS", parts):
        yield


@contextlib.contextmanager
def _counted():
    seen = {"x3": 0, "x3_jobs": 0, "tf": 0}
    x3, tf = ops.tap_products_bf16x3, ops.tfusion_project

    def counted_x3(jobs):
        seen["x3"] += 1
        seen["x3_jobs"] += len(jobs)
        return x3(jobs)

    def counted_tf(jobs):
        seen["tf"] += 1
        return tf(jobs)

    with mock.patch.object(ops, "tap_products_bf16x3", counted_x3), mock.patch.object(ops, "tfusion_project", counted_tf):
        yield seen


def _sources(c):
    return [(_t(c.x[i]).permute(0, 3, 1, 2), ops.upconv_tap_weights(_t(c.w[i]), 0, c.cin)) for i in range(len(c.sizes))]


def _upconv(c, srcs, layout):
    if layout == "pitched":
        abuf = torch.full((c.b, c.ho, c.wo, c.c + 12), SENTINEL, dtype=torch.float32, device=DEV)
        abuf[..., 4:4 + c.c] = _t(c.conv_a)
        obuf = torch.full((c.b, c.ho, c.wo, c.c + 20), SENTINEL, dtype=torch.float32, device=DEV)
        a, o = abuf[..., 4:4 + c.c].permute(0, 3, 1, 2), obuf[..., 8:8 + c.c].permute(0, 3, 1, 2)
        got = ops.upconv3x3(a, _t(c.bias), srcs, 2, out=o)
        assert got is o
        assert bool((obuf[..., :8] == SENTINEL).all()) and bool((obuf[..., 8 + c.c:] == SENTINEL).all())
        assert torch.equal(abuf[..., 4:4 + c.c], _t(c.conv_a))
    else:
        a = _t(c.conv_a).permute(0, 3, 1, 2)
        got = ops.upconv3x3(a, _t(c.bias), srcs, 2)
        assert got is a
    return got.permute(0, 2, 3, 1).cpu().numpy()


@pytest.mark.parametrize("name", ["tf_fused_dyadic", "tf_pair_dyadic", "tf_random"])
def test_upconv3x3_on_the_limb_form(name):
    """conv_a in place (the engine's form) and pitched: inside util.upconv_bound; one launch of 2 x 3 column-range jobs; on exact
    inputs the bits of the fp32 form."""
    c = util.upconv_case(name)
    want, bound = util.upconv_want(name, 2), util.upconv_bound(name)
    srcs = _sources(c)
    with _tap_form("x3"), _counted() as seen:
        got = _upconv(c, srcs, "inplace")
        assert (seen["x3"], seen["x3_jobs"], seen["tf"]) == (1, 6, 0), seen
        pitched = _upconv(c, srcs, "pitched")
    _check("upconv3x3 %s taps by x3, in place" % name, got, want, bound)
    _check("upconv3x3 %s taps by x3, pitched" % name, pitched, want, bound)
    assert np.array_equal(got, pitched)
    with _tap_form("x3", 1), _counted() as seen:
        assert np.array_equal(_upconv(c, srcs, "inplace"), got), "1 column range gives other bits than 3"
        assert (seen["x3"], seen["x3_jobs"]) == (1, 2), seen
    with _tap_form("tf"), _counted() as seen:
        fp32 = _upconv(c, srcs, "inplace")
        assert (seen["x3"], seen["tf"]) == (0, 1), seen
    _check("upconv3x3 %s taps by tf" % name, fp32, want, bound)
    if c.kind == "exact":
        assert np.array_equal(got, fp32), "exact inputs: x3 gives other bits than tf"


def test_upconv3x3_row_range_split_gives_the_bits_of_the_unsplit_call():
    name = "tf_300_tokens"
    c = util.upconv_case(name)
    srcs = _sources(c)
    with _tap_form("x3"):
        with _counted() as seen:
            whole = _upconv(c, srcs, "inplace")
        assert (seen["x3"], seen["x3_jobs"]) == (1, 6), seen
        with mock.patch.object(ops, "_TAP_JOB_ROWS", 128), _counted() as seen:
            split = _upconv(c, srcs, "inplace")
        assert (seen["x3"], seen["x3_jobs"]) == (2, 12), seen
    assert np.array_equal(split, whole)
    _check("upconv3x3 %s by x3, row ranges of 128" % name, split, util.upconv_want(name, 2), util.upconv_bound(name))


def test_upconv3x3_sources_the_limb_kernel_does_not_take_fall_back():
    """A source without 128 channels goes to the library GEMM as under `tf`; the limb kernel is not called."""
    c = util.upconv_case("fused_5to10")
    srcs = [(_t(c.x[i]).permute(0, 3, 1, 2), ops.upconv_tap_weights(_t(c.w[i]), 0, c.cin)) for i in range(len(c.sizes))]
    with _tap_form("x3"), _counted() as seen:
        got = _upconv(c, srcs, "inplace")
        assert (seen["x3"], seen["tf"]) == (0, 0), seen
    _check("upconv3x3 fused_5to10 (8-channel source) under x3", got, util.upconv_want("fused_5to10", 2), util.upconv_bound("fused_5to10"))


# ------------------------------------------------------------------------------------------
# 5. the engine
# ------------------------------------------------------------------------------------------
def test_engine_default_against_the_fp32_tap_products():
    """Two streamed frames with the default tap products and with SMOS_TAP_GEMM=tf: the bars tests/test_gpu_e2e.py holds engine
    variants to (1e-5 of the logit range, 5e-5 of the memory's)."""
    from streammos_amd import synth
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    model = StreamMOS.AttNet(cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(DEV).eval()
    model.fast_inference, model.engine_layout = True, "cl"
    frames = list(cases.e2e_frames(2))
    outs, calls = {}, {}
    for form in ("x3", "tf"):
        with _tap_form(form), _counted() as seen:
            memory, res = None, []
            with torch.no_grad():
                for i, batch in enumerate(frames):
                    tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
                    pred, _, _, _, memory = model.infer(tb, i, memory)
                    res.append((pred.clone(), memory.clone()))
        outs[form], calls[form] = res, dict(seen)
    assert calls["x3"]["x3"] >= len(frames) and calls["tf"]["x3"] == 0, calls
    for f, ((p0, m0), (p1, m1)) in enumerate(zip(outs["tf"], outs["x3"])):
        pe, me = (p0 - p1).abs().max().item() / p0.abs().max().item(), (m0 - m1).abs().max().item() / m0.abs().max().item()
        print("tap-bf16x3-ratio engine frame %d: logits %.2e of range, memory %.2e" % (f, pe, me))
        assert pe <= 1e-5 and me <= 5e-5, (f, pe, me)

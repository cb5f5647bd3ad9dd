"""The decoder's conv_1 path -- tap products at source resolution (the column-range jobs of csrc/tfusion.hip::tfusion_project),
then the separable align_corners=True interpolation of csrc/upconv.hip (upconv_xy, or upconv_xpass + upconv_ypass) -- against
float64 references, stage by stage, element by element, inside derived bounds.

What reaches what (cases, references and bounds: tests/util.py, checked on the host by tests/test_host_upconv_reference.py):
  tfusion_project   column-range jobs with pitched `out` slices, TapWeights.stream(1 / 2 / 3), cout = 36 .. 1152 per job,
                    1 .. 200 tokens, a 1-token job next to a 200-token one (its later blocks leave), dense and sliced x,
                    cout edges 4 .. 2048 with and without bias, eight jobs and nine         test_tap_products_*
  upconv_xy         one launch: strips of 8, 16 and 32 rows with a partial last strip and a window that slides, one and two
                    sources, C/4 = 1, 9, 32, Hs = 1, Wo = 1, Ho = Wo = 1                      test_passes_*, test_border_*
  upconv_xpass +    the pair, on every geometry (it is the only form for 2 (Hs - 1) >= Ho - 1: 5 -> 9, 15 -> 20, the
  upconv_ypass      identity, Ho = 1 from Hs = 3); bit-identical to the one launch wherever both apply
  ops.upconv3x3     128-channel sources through the tf / conv / mm tap products, 1 / 2 / 3 column ranges, the row-range
                    split with more than 8 jobs, the refusals                                test_upconv3x3_*

Bounds, per element, u = 2^-24 (derivation in tests/util.py): u ((Cin + 24) A + P) for the whole op, u (24 A_z + P) for the
passes fed a known z, u Cin |x| |W|^T for a tap product; A the float64 reference on the inputs' magnitudes, P the weight
perturbation of a non-dyadic size ratio (0 for dyadic ones).  Exact inputs (small integers, weights k / 64) make every tap
product exact in float32 in any summation order: there the kernels must reproduce the float64 products bit for bit.
Everything that is the same arithmetic twice -- one launch against the pair, 1 / 2 / 3 column ranges, tf / conv / mm on exact
inputs, split against unsplit, a sample alone against the same sample in a batch, a second call -- is compared bit for bit.
Every check prints its worst error / bound (pytest -s); the figures of the MI355X run are kept in
profiles/upconv_error_ratios.txt.

Not reached: the multi-unit-per-block loop of upconv_xy (more than 8192 units of work: no shape of a few seconds).
On a strip's FIRST row the window never slides (base is lerp_of(Y0 - 1).i0, which is what row Y0 asks for); the strip cases
slide on the second row of their last strip, from a base above 0.
"""
import contextlib
from unittest import mock

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _check(label, got, want, bound):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert tuple(got.shape) == tuple(want.shape), (label, got.shape, want.shape)
    ok, ratio = util.msda_worst_ratio(got, want, bound)
    print("upconv-ratio %-66s %.4f" % (label, ratio))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


@contextlib.contextmanager
def _launches():
    """Counts the launches behind ops.upconv3x3: {"xy", "xpass", "ypass"} calls of the library, "project" calls of
    ops.tfusion_project and "jobs", the jobs they carried."""
    lib = _lib.load()
    seen = {"xy": 0, "xpass": 0, "ypass": 0, "project": 0, "jobs": 0}

    def counted(key, fn):
        def call(*args):
            seen[key] += 1
            return fn(*args)
        return call

    project = ops.tfusion_project

    def counted_project(jobs):
        seen["project"] += 1
        seen["jobs"] += len(jobs)
        return project(jobs)

    with mock.patch.object(lib, "smos_upconv_xy", counted("xy", lib.smos_upconv_xy)), \
            mock.patch.object(lib, "smos_upconv_xpass", counted("xpass", lib.smos_upconv_xpass)), \
            mock.patch.object(lib, "smos_upconv_ypass", counted("ypass", lib.smos_upconv_ypass)), \
            mock.patch.object(ops, "tfusion_project", counted_project):
        yield seen


def _embed(arr, pitch, at):
    """arr [B, H, W, C] as channels [at, at + C) of a sentinel-filled [B, H, W, pitch] buffer -> (buffer, [B, C, H, W] view)."""
    b, h, w, c = arr.shape
    buf = torch.full((b, h, w, pitch), SENTINEL, dtype=torch.float32, device=DEV)
    buf[..., at:at + c] = _t(arr)
    return buf, buf[..., at:at + c].permute(0, 3, 1, 2)


def _untouched(buf, at, c):
    return bool((buf[..., :at] == SENTINEL).all()) and bool((buf[..., at + c:] == SENTINEL).all())


def _sources(c, zs="known", samples=slice(None)):
    """The source tuples of ops.upconv3x3: (x channels-last, TapWeights[, z [B*Hs*Ws, 9*C]])."""
    srcs = []
    for i, (hs, ws) in enumerate(c.sizes):
        x = _t(c.x[i][samples]).permute(0, 3, 1, 2)
        wt = ops.upconv_tap_weights(_t(c.w[i]), 0, c.cin)
        if zs is None:
            srcs.append((x, wt))
        else:
            z = c.z[i] if isinstance(zs, str) else zs[i]
            srcs.append((x, wt, _t(z[samples]).reshape(-1, 9 * c.c)))
    return srcs


def _fusable(c):
    lib = _lib.load()
    ok = all(bool(lib.smos_upconv_xy_ok(hs, c.ho)) for hs, _ in c.sizes)
    assert ok == all(util.upconv_xy_ok(hs, c.ho) for hs, _ in c.sizes)
    return ok


def _upconv(c, srcs, act, layout, fused, samples=slice(None)):
    """One ops.upconv3x3 call.  layout "pitched": conv_a = channels [4, 4 + C) of a buffer of pitch C + 12, out = channels
    [8, 8 + C) of another of pitch C + 20 -- both sentinel-filled, the neighbours checked; "inplace": dense, out = conv_a.
    -> [B, Ho, Wo, C] on the host.  Asserts which launches ran."""
    conv_a = c.conv_a[samples]
    with mock.patch.object(ops, "_UPCONV_XY", fused), _launches() as seen:
        if layout == "pitched":
            abuf, a = _embed(conv_a, c.c + 12, 4)
            obuf, o = _embed(np.full(conv_a.shape, SENTINEL), c.c + 20, 8)
            got = ops.upconv3x3(a, _t(c.bias), srcs, act, out=o)
            assert got is o
            assert _untouched(abuf, 4, c.c) and torch.equal(a, _embed(conv_a, c.c + 12, 4)[1]), "conv_a was written"
            assert _untouched(obuf, 8, c.c), "channels next to out were written"
        else:
            a = _t(conv_a).permute(0, 3, 1, 2)
            got = ops.upconv3x3(a, _t(c.bias), srcs, act)
            assert got is a
    if fused and _fusable(c):
        assert (seen["xy"], seen["xpass"], seen["ypass"]) == (1, 0, 0), seen
    else:
        assert (seen["xy"], seen["xpass"], seen["ypass"]) == (0, len(c.sizes), 1), seen
    return got.permute(0, 2, 3, 1).cpu().numpy()


# ------------------------------------------------------------------------------------------
# a. the tap products, as upconv3x3 issues them to tfusion_project
# ------------------------------------------------------------------------------------------
_TOKEN_PAIRS = ((1, 15), (16, 17), (63, 64), (65, 200), (200, 1))      # (source 1, source 2) of one launch
_PAD_L, _PAD_R, _PAD_ROWS = 8, 8, 3


def _tap_problem(ch, kind):
    rng = np.random.default_rng(util._seed("upconv/taps/%d/%s" % (ch, kind)))
    nks = [util.tap_matrix(util.upconv_inputs(rng, (ch, 128, 3, 3), kind, (2.0 / (9 * 128)) ** 0.5)) for _ in range(2)]
    xs = {t: util.upconv_inputs(rng, (t, 128), kind) for t in sorted(set(sum(_TOKEN_PAIRS, ())))}
    return nks, xs


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("ch", [4, 32, 128])
def test_tap_products_column_range_jobs_of_tfusion_project(ch, kind):
    """[tokens, 9*C] matrices of two sources, each written by 1, 2 and 3 column-range jobs of one launch into a view of a
    wider and taller sentinel buffer: exact inputs bit for bit equal to x @ nk.T in float64, random ones inside Cin u |x| |nk|^T;
    the same bits for every number of ranges; the sentinel survives left of, right of and below the matrix.  9*4 / 2 = 18 is no
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
                bufs = [torch.full((t + _PAD_ROWS, _PAD_L + width + _PAD_R), SENTINEL, dtype=torch.float32, device=DEV) for t in pair]
                views = [buf[:t, _PAD_L:_PAD_L + width] for buf, t in zip(bufs, pair)]
                jobs = [(x, ws_k, n, view[:, k * n:(k + 1) * n])
                        for x, wt, view in zip(dev_x, wts, views) for k, ws_k in enumerate(wt.stream(parts))]
                assert len(jobs) == 2 * parts
                if n % 4:
                    with pytest.raises(RuntimeError, match="tfusion_project: bad job"):
                        ops.tfusion_project(jobs)
                    torch.cuda.synchronize()
                    assert all(bool((buf == SENTINEL).all()) for buf in bufs)
                    continue
                outs = ops.tfusion_project(jobs)
                assert all(o is job[3] for o, job in zip(outs, jobs))
                for buf, t in zip(bufs, pair):
                    assert bool((buf[:, :_PAD_L] == SENTINEL).all()), "columns left of the first range were written"
                    assert bool((buf[:, _PAD_L + width:] == SENTINEL).all()), "columns right of the last range were written"
                    assert bool((buf[t:] == SENTINEL).all()), "rows past `tokens` were written"
                results[parts] = [v.cpu().numpy() for v in views]
            for parts in results:
                for a, b in zip(results[parts], results[1]):
                    assert np.array_equal(a, b), "tokens %s, %s x: %d column ranges differ from 1" % (pair, layout, parts)
            for t, nk, got in zip(pair, nks, results[1]):
                want = util.tap_products_ref(xs[t], nk)
                label = "taps C=%d %s %s x tokens=%d (next to %d)" % (ch, kind, layout, t, pair[0] + pair[1] - t)
                if kind == "exact":
                    assert np.array_equal(got.astype(np.float64), want), label
                _check(label, got, want, util.tap_products_bound(xs[t], nk))


@pytest.mark.parametrize("with_bias", [False, True])
def test_tap_products_plain_jobs_at_cout_edges(with_bias):
    """cout = 4, 48, 60, 64, 68 and 2048 (one to 128 output tiles of 16, the last one partly or wholly past cout) as six
    jobs of one launch on 70 tokens (two blocks, the second with 6 live rows), each into its own sentinel frame."""
    rng = np.random.default_rng(util._seed("upconv/plain/%d" % with_bias))
    tokens, couts = 70, (4, 48, 60, 64, 68, 2048)
    x = util.upconv_inputs(rng, (tokens, 128), "random")
    ws = [util.upconv_inputs(rng, (o, 128), "random", 128 ** -0.5) for o in couts]
    bs = [util.upconv_inputs(rng, (o,), "random") for o in couts]
    bufs = [torch.full((tokens + _PAD_ROWS, _PAD_L + o + _PAD_R), SENTINEL, dtype=torch.float32, device=DEV) for o in couts]
    dev_x = _t(x)
    jobs = [(dev_x, ops.tfusion_pack_linear(_t(w)), _t(b) if with_bias else o, buf[:tokens, _PAD_L:_PAD_L + o])
            for w, b, o, buf in zip(ws, bs, couts, bufs)]
    ops.tfusion_project(jobs)
    for w, b, o, buf in zip(ws, bs, couts, bufs):
        assert bool((buf[:, :_PAD_L] == SENTINEL).all()) and bool((buf[:, _PAD_L + o:] == SENTINEL).all()) and bool((buf[tokens:] == SENTINEL).all())
        want = util.tap_products_ref(x, w) + (b if with_bias else 0.0)
        bound = util.tap_products_bound(x, w) + util.UPCONV_U * (np.abs(want) + (np.abs(b) if with_bias else 0.0))   # + the bias add
        _check("plain job cout=%d %s" % (o, "bias" if with_bias else "no bias"), buf[:tokens, _PAD_L:_PAD_L + o], want, bound)


def test_tap_products_eight_jobs_run_and_nine_raise():
    rng = np.random.default_rng(util._seed("upconv/eight"))
    xs = [util.upconv_inputs(rng, (3 + j, 128), "exact") for j in range(9)]
    ws = [util.upconv_inputs(rng, (4, 128), "exact", 0.5) for _ in range(9)]
    outs = [torch.full((3 + j, 4), SENTINEL, dtype=torch.float32, device=DEV) for j in range(9)]
    jobs = [(_t(x), ops.tfusion_pack_linear(_t(w)), 4, o) for x, w, o in zip(xs, ws, outs)]
    with pytest.raises(RuntimeError, match="1..8 jobs"):
        ops.tfusion_project(jobs)
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    ops.tfusion_project(jobs[:8])
    for x, w, o in zip(xs[:8], ws, outs):
        assert np.array_equal(o.cpu().numpy().astype(np.float64), util.tap_products_ref(x, w))
    assert bool((outs[8] == SENTINEL).all())


# ------------------------------------------------------------------------------------------
# b. the passes alone, fed a known z
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", util.UPCONV_PASS_CASES)
def test_passes_fused_launch_and_pair_against_float64(name):
    """LeakyReLU, conv_a and out different channel slices of wider buffers with different pitches.  The pair runs on every
    geometry, the one launch where smos_upconv_xy_ok allows it -- same bits."""
    c = util.upconv_case(name)
    want, bound = util.upconv_passes_want(name, 2), util.upconv_passes_bound(name)
    if name.startswith("strip"):
        assert util.upconv_strip(c.b, c.ho, c.wo, c.c) == int(name[5:]) and c.ho % int(name[5:]) and _fusable(c)
    srcs = _sources(c)
    pair = _upconv(c, srcs, 2, "pitched", fused=False)
    _check("passes %s x pass + y pass" % name, pair, want, bound)
    if _fusable(c):
        fused = _upconv(c, srcs, 2, "pitched", fused=True)
        _check("passes %s one launch (window of three x-pass rows)" % name, fused, want, bound)
        assert np.array_equal(fused, pair), "the one launch and the pair differ"
    if name == "identity":          # weights 1 and 0: a plain sum of nine taps of multiples of 2^-6, exact in float32 without the LeakyReLU
        assert c.kind == "exact"
        assert np.array_equal(_upconv(c, srcs, 0, "pitched", fused=False).astype(np.float64), util.upconv_passes_want(name, 0))


@pytest.mark.parametrize("act", util.UPCONV_ACTS)
@pytest.mark.parametrize("name", ["fused_5to10", "pair_15to20", "two_ratios", "all_one"])
def test_passes_in_place_every_activation_and_twice(name, act):
    c = util.upconv_case(name)
    want, bound = util.upconv_passes_want(name, act), util.upconv_passes_bound(name)
    srcs = _sources(c)
    for fused in ((False, True) if _fusable(c) else (False,)):
        form = "one launch" if fused else "pair"
        got = _upconv(c, srcs, act, "inplace", fused)
        _check("passes %s act %d in place, %s" % (name, act, form), got, want, bound)
        assert np.array_equal(got, _upconv(c, srcs, act, "inplace", fused)), "a second call gives other bits"
        assert np.array_equal(got, _upconv(c, srcs, act, "pitched", fused)), "in place and pitched differ"
    if act == 1:
        assert (want == 0).any() and (want > 0).any()


@pytest.mark.parametrize("name", ["fused_5to10", "pair_15to20", "two_ratios"])
def test_passes_a_sample_alone_equals_the_sample_in_its_batch(name):
    c = util.upconv_case(name)
    assert c.b > 1
    for fused in ((False, True) if _fusable(c) else (False,)):
        batch = _upconv(c, _sources(c), 2, "pitched", fused)
        for b in range(c.b):
            alone = _upconv(c, _sources(c, samples=slice(b, b + 1)), 2, "pitched", fused, samples=slice(b, b + 1))
            assert np.array_equal(alone[0], batch[b]), (name, fused, b)


@pytest.mark.parametrize("name", ["fused_3to9_dyadic", "pair_5to9_dyadic"])
def test_border_taps_are_dropped_by_a_select_not_a_zero_weight(name):
    """Inf in the z elements that only DROPPED taps address at an image border (upconv_poison_borders): source column 0 of
    the kx = 0 blocks, the last column of the kx = 2 blocks, row 0 of the ky = 0 blocks, the last row of the ky = 2 blocks.
    The outputs on that border must be finite and inside the bound of the reference, which never reads them; further
    inside, the Inf is legitimately read (with weight 0 as well: NaN) -- those outputs must be non-finite in both.  The
    ratios are dyadic, so kernel and reference pick the same source samples and agree on which outputs are which."""
    c = util.upconv_case(name)
    clean, bound = util.upconv_passes_want(name, 0), util.upconv_passes_bound(name)
    for sides in [(s,) for s in util.UPCONV_SIDES] + [util.UPCONV_SIDES]:
        zs = [util.upconv_poison_borders(z, sides) for z in c.z]
        ref = util.upconv_passes_ref(c.conv_a, c.bias, zs, 0)
        finite = np.isfinite(ref)
        lines = [util.upconv_border_line(s, c.ho, c.wo) for s in sides] if len(sides) == 1 else [np.s_[:, 0, 0], np.s_[:, -1, -1]]
        assert all(finite[line].all() for line in lines) and not finite.all()
        srcs = _sources(c, zs)
        for fused in ((False, True) if _fusable(c) else (False,)):
            got = _upconv(c, srcs, 0, "pitched", fused)
            label = "border %s Inf at %s, %s" % (name, "+".join(sides), "one launch" if fused else "pair")
            for line in lines:
                assert np.isfinite(got[line]).all(), label + ": a dropped tap leaked into the border outputs"
            assert np.array_equal(np.isfinite(got), finite), label
            _check(label, np.where(finite, got, 0.0), np.where(finite, clean, 0.0), np.where(finite, bound, 0.0))


# ------------------------------------------------------------------------------------------
# c. the whole op with 128-channel sources
# ------------------------------------------------------------------------------------------
_FORMS = (("tf", 1), ("tf", 2), ("tf", 3), ("conv", 3), ("mm", 3))


@contextlib.contextmanager
def _tap_form(gemm, parts):
    with mock.patch.object(ops, "_TAP_GEMM", gemm), mock.patch.object(ops, "_TAP_GEMM_OWN", gemm == "conv"), \
            mock.patch.object(ops, "_TAP_PARTS", parts):
        yield


@pytest.mark.parametrize("name", ["tf_fused_dyadic", "tf_pair_dyadic", "tf_random"])
def test_upconv3x3_with_128_channel_sources_in_every_tap_product_form(name):
    """conv_a in place (the engine's form) and pitched.  tf issues 2 x parts column-range jobs in one launch; conv and mm
    none.  Exact inputs: the tap products are exact in every form, so every form gives the same bits."""
    c = util.upconv_case(name)
    want, bound = util.upconv_want(name, 2), util.upconv_bound(name)
    srcs = _sources(c, zs=None)
    first = None
    for gemm, parts in _FORMS:
        with _tap_form(gemm, parts), _launches() as seen:
            got = _upconv(c, srcs, 2, "inplace", fused=True)
            assert (seen["project"], seen["jobs"]) == ((1, 2 * parts) if gemm == "tf" else (0, 0)), (gemm, parts, seen)
            assert np.array_equal(got, _upconv(c, srcs, 2, "pitched", fused=True))
            if _fusable(c):
                assert np.array_equal(got, _upconv(c, srcs, 2, "inplace", fused=False))
        _check("upconv3x3 %s taps by %s, %d column ranges" % (name, gemm, parts), got, want, bound)
        if gemm == "tf" or c.kind == "exact":
            first = got if first is None else first
            assert np.array_equal(got, first), "%s / %d ranges gives other bits than tf / 1 range" % (gemm, parts)


def test_upconv3x3_row_range_split_takes_several_launches_and_gives_the_same_bits():
    """The row limit of a tap-product job (ops._TAP_JOB_ROWS; a job's z slice has to stay below 2 GiB) brought down to 128
    rows on a 300-token source: 3 row ranges x 3 column ranges + 3 jobs of the 24-token source = 12 jobs, two launches."""
    name = "tf_300_tokens"
    c = util.upconv_case(name)
    assert c.b * c.sizes[0][0] * c.sizes[0][1] == 300
    srcs = _sources(c, zs=None)
    with _tap_form("tf", 3):
        with _launches() as seen:
            whole = _upconv(c, srcs, 2, "inplace", fused=True)
        assert (seen["project"], seen["jobs"]) == (1, 6)
        with mock.patch.object(ops, "_TAP_JOB_ROWS", 128), _launches() as seen:
            split = _upconv(c, srcs, 2, "inplace", fused=True)
        assert seen["jobs"] == 12 and seen["project"] == 2, seen
    assert np.array_equal(split, whole)
    _check("upconv3x3 %s split into row ranges of 128" % name, split, util.upconv_want(name, 2), util.upconv_bound(name))


# ------------------------------------------------------------------------------------------
# d. refusals
# ------------------------------------------------------------------------------------------
def test_upconv3x3_refusals_leave_the_output_alone():
    c = util.upconv_case("pair_5to9_dyadic")
    src = _sources(c)[0]
    abuf, a = _embed(c.conv_a, c.c + 12, 4)
    obuf, o = _embed(np.full(c.conv_a.shape, SENTINEL), c.c + 20, 8)
    bias = _t(c.bias)

    def untouched():
        torch.cuda.synchronize()
        return bool((obuf == SENTINEL).all()) and torch.equal(a, _embed(c.conv_a, c.c + 12, 4)[1])

    with pytest.raises(RuntimeError, match="upconv3x3: one or two upsampled sources, got 3"):
        ops.upconv3x3(a, bias, [src, src, src], 2, out=o)
    assert untouched()
    with pytest.raises(RuntimeError, match="upconv3x3: one or two upsampled sources, got 0"):
        ops.upconv3x3(a, bias, [], 2, out=o)
    assert untouched()
    wrong_cin = ops.upconv_tap_weights(_t(np.concatenate((c.w[0], c.w[0]), 1)), 0, 2 * c.cin)
    with pytest.raises(RuntimeError, match="upconv3x3: tap weights are for 16 -> 4 channels, got 8 -> 4"):
        ops.upconv3x3(a, bias, [(src[0], wrong_cin, src[2])], 2, out=o)
    assert untouched()
    wrong_cout = ops.upconv_tap_weights(_t(np.concatenate((c.w[0], c.w[0]), 0)), 0, c.cin)
    with pytest.raises(RuntimeError, match="upconv3x3: tap weights are for 8 -> 8 channels, got 8 -> 4"):
        ops.upconv3x3(a, bias, [src, (src[0], wrong_cout, src[2])], 2, out=o)         # behind a good source
    assert untouched()
    for bad in (src[2][:-1], src[2][:, :-4], src[2].reshape(-1, 3, 3 * c.c), src[2].t().contiguous().t()):
        with pytest.raises(RuntimeError, match="upconv3x3: tap products must be a contiguous"):
            ops.upconv3x3(a, bias, [(src[0], src[1], bad)], 2, out=o)
        assert untouched()
    # the one launch on a source taller than half the output, called directly: an error that names the op, nothing written
    lib = _lib.load()
    hs, ws = c.sizes[0]
    assert not lib.smos_upconv_xy_ok(hs, c.ho) and lib.smos_upconv_xy_ok(hs, c.ho + 1)
    rc = lib.smos_upconv_xy(a.data_ptr(), c.c + 12, bias.data_ptr(), src[2].data_ptr(), hs, ws, None, 0, 0, o.data_ptr(), c.c + 20,
                            c.b, c.ho, c.wo, c.c, 2, ops._stream(a))
    assert rc != 0
    with pytest.raises(RuntimeError, match="upconv_xy: a source is taller than half the output"):
        _lib.check(rc, "smos_upconv_xy")
    assert untouched()
    # and the same call is accepted as the pair
    got = _upconv(c, [src], 2, "pitched", fused=True)
    _check("refusals: pair_5to9_dyadic still runs as the pair", got, util.upconv_passes_want(c.name, 2), util.upconv_passes_bound(c.name))

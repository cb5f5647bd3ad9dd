"""The channels-last glue kernels of csrc/cl_kernels.hip (bias_act_cl, downsample_epilogue_cl2, colsum_partial, gate_mlp,
gate_mlp_wide, gate_apply_cl, upsample_concat_cl, zero_views) through streammos_amd.ops against the float64 references of
tests/cl_cases.py, every element judged against its derived bound (tests/util.py::msda_worst_ratio: a zero bound asks for a zero
error, a NaN is outside every bound).

What no unit test reached before, and where it is reached here:
  1. the eight-way main loop of gate_mlp_wide (chunks >= 7 parts + 1), its tail in one thread only, two main trips, and C = 256:
     test_gate_wide_synthetic_tables (the table is the kernel's input: a tiny y suffices), test_gate_on_real_tables.
  2. gate_mlp / colsum_partial at C < 32, HW below the pixel lanes of a block, HW around the 512-pixel chunk border, a workspace
     of exactly the required size full of NaN inside a NaN buffer: test_three_pass_gate.
  3. pool windows whose real taps are all <= -1 (a pad of 0 would win), 1 x N and N x 1 maps: test_downsample_epilogue.
  4. Ho = 1, Wo = 1, 1 x 1 sources, non-dyadic ratios, sliced sources, channel splits off the multiples of 32: test_upsample_concat.
  5. the in-place calls of the engine (out = y2, out = a, out = x): the "in_place" runs of every elementwise test.
  6. the second trip of every grid-stride loop: the "sweep" cases (256 * 16 * 256 + 300 float4 items).

With SMOS_CL_RATIOS_FILE set, the worst error / bound per test is appended to that file (profiles/cl_error_ratios.txt is made from it)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import cl_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = -1.25e30                 # what neighbours of an output hold before a launch
_LINES = []


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("SMOS_CL_RATIOS_FILE")
    if path and _LINES:
        with open(path, "a") as f:
            f.write("\n".join(_LINES) + "\n")


def _note(tag, worst):
    line = "cl-ratio %-52s worst error / bound %.4f" % (tag, worst)
    print(line)
    _LINES.append(line)


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _dense(a):
    """[B, H, W, C] numpy -> the logical [B, C, H, W] channels-last view the ops take."""
    return _t(a).permute(0, 3, 1, 2)


def _sliced(a, fill=NAN, off=4, extra=8):
    """The same map as a channel slice at `off` of a map `extra` channels wider whose other channels hold `fill` -> (view, wide)."""
    b, h, w, c = a.shape
    wide = torch.full((b, h, w, c + extra), fill, device=DEV)
    wide[..., off:off + c] = _t(a)
    return wide[..., off:off + c].permute(0, 3, 1, 2), wide


def _neighbours_keep(wide, c, fill, off=4):
    rest = torch.cat((wide[..., :off], wide[..., off + c:]), -1)
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


def _np(t):
    """logical [B, C, H, W] device view -> [B, H, W, C] float64 numpy"""
    return t.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64)


def _judge(tag, got, want, bound, worst):
    ok, r = cases.worst_ratio(got, want, bound)
    assert ok, (tag, "worst error / bound", r)
    return max(worst, r)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------
# bias_act_cl
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.BIAS_ACT_CASES))
def test_bias_act(name):
    """Every act code, bias / residual absent, C 4 / 36 / 128, P = 1, the sweep case.  Three runs: dense operands out of place; x,
    residual and out as channel slices of NaN / sentinel maps; the same slices with out = x (in place, as the engine calls it)."""
    c = cases.bias_act_case(name)
    bound, bias = cases.bias_act_bound(c), None if c.bias is None else _t(c.bias)
    worst = 0.0
    got = ops.bias_act_cl(_dense(c.x), bias, c.act, residual=None if c.res is None else _dense(c.res))
    worst = _judge(name + " dense", _np(got), c.want, bound, worst)
    if name != "sweep":
        x, xw = _sliced(c.x)
        res = None if c.res is None else _sliced(c.res, off=8, extra=12)[0]
        out, ow = _sliced(np.zeros_like(c.x), fill=SENT, off=12, extra=16)
        assert ops.bias_act_cl(x, bias, c.act, out=out, residual=res) is out
        worst = _judge(name + " sliced", _np(out), c.want, bound, worst)
        assert _neighbours_keep(ow, c.c, SENT, 12) and _neighbours_keep(xw, c.c, NAN)
        ops.bias_act_cl(x, bias, c.act, out=x, residual=res)
        assert _same_bits(x, out) and _neighbours_keep(xw, c.c, NAN)
    _note("bias_act/" + name, worst)


# ---------------------------------------------------------------------------------------------
# downsample_epilogue_cl2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.DS_CASES))
def test_downsample_epilogue(name):
    """Stride 1 and 2, maps from 1 x 1 to 31 x 17 with 1 x N and N x 1, C 4 and 36, pool inputs that are <= -1 everywhere (a
    border tap counted as 0 instead of -inf moves an output by >= 1) and signed ones.  Dense out of place, then a, p and out
    as slices with out = a (in place)."""
    c = cases.ds_case(name)
    bound, bias = cases.ds_bound(c), _t(c.bias)
    got = ops.downsample_epilogue_cl(_dense(c.a), _dense(c.p), bias, c.stride)
    assert tuple(got.shape) == (c.b, c.c, c.ho, c.wo)
    worst = _judge(name + " dense", _np(got), c.want, bound, 0.0)
    if name != "sweep":
        a, aw = _sliced(c.a, fill=SENT)
        p, pw = _sliced(c.p, off=8, extra=12)
        assert ops.downsample_epilogue_cl(a, p, bias, c.stride, out=a) is a
        assert _same_bits(a, got) and _neighbours_keep(aw, c.c, SENT) and _neighbours_keep(pw, c.c, NAN, 8)
    _note("downsample/" + name, worst)


# ---------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------
def _gate_operands(c):
    return _t(c.bias), _t(c.w1), _t(c.b1), _t(c.w2), _t(c.b2)


def _map(a, c):
    return np.asarray(a).reshape(c.b, c.h, c.w, c.c)


def _check_gate(tag, c, gate, worst, ref=None):
    """gate [B, C] read back from the kernel against the reference gate, and its logit against the pre-sigmoid value."""
    ref = c if ref is None else ref
    bg, bl = cases.gate_bound(ref)
    g = gate.cpu().numpy().astype(np.float64).reshape(ref.gate.shape)
    worst = _judge(tag + " gate", g, ref.gate, bg, worst)
    return _judge(tag + " logit", cases.logit(g), ref.pre, bl, worst)


def _check_apply(tag, c, gate, out, worst):
    """relu((y + bias) * g + xres) with g the kernel's own gate: the bound is on this step alone."""
    g = gate.cpu().numpy().astype(np.float64).reshape(c.b, c.c)
    want = cases.gate_apply_ref(c.y, c.bias, g, c.xres)
    return _judge(tag + " apply", _np(out).reshape(want.shape), want, cases.gate_apply_bound(c.y, c.bias, g, c.xres), worst)


def _run_wide(c):
    """One ops.channel_gate_apply_cl on case c -> (gate [B * C], out); gate_ws sits inside a NaN buffer that must stay NaN."""
    ws = torch.full((c.b * c.c + 16,), NAN, device=DEV)
    y = _dense(_map(c.y, c))
    out = ops.channel_gate_apply_cl(y, *_gate_operands(c), _dense(_map(c.xres, c)), _t(c.table), ws[8:8 + c.b * c.c])
    assert bool(torch.isnan(ws[:8]).all()) and bool(torch.isnan(ws[8 + c.b * c.c:]).all())
    return ws[8:8 + c.b * c.c].clone(), out


@pytest.mark.parametrize("cr_kind", ("one", "quarter", "max"))
@pytest.mark.parametrize("ch", cases.GATE_WIDE_C)
def test_gate_wide_synthetic_tables(ch, cr_kind):
    """gate_mlp_wide on tables of 1, 3, parts - 1, parts, 7 parts, 7 parts + 1 (only part 0 enters the eight-way loop),
    8 parts - 1, 8 parts (no tail), 8 parts + 1 (a tail in one thread) and 21 parts + 3 (two main trips and a tail of five or
    six steps) chunks, parts = 1024 / C, at C 32 .. 256 and Cr 1, C / 4, 64; B = 3 with a table per sample over a 3 x 5 map.
    Each case twice with bitwise equal results.  With Cr = C / 4 also the exact twins: only expf, one add and one reciprocal
    separate the gate from the reference there."""
    cr = {"one": 1, "quarter": ch // 4, "max": 64}[cr_kind]
    todo = [cases.gate_wide_case(ch, k, cr) for k in cases.gate_wide_chunks(ch)]
    if cr_kind == "quarter":
        todo += [cases.gate_wide_case(ch, k, cr, True) for k in cases.gate_wide_twin_chunks(ch)]
    worst = worst_x = worst_a = 0.0
    for c in todo:
        gate, out = _run_wide(c)
        gate2, out2 = _run_wide(c)
        assert _same_bits(gate, gate2) and _same_bits(out, out2), c.name
        if c.exact:
            worst_x = _check_gate(c.name, c, gate, worst_x)
        else:
            worst = _check_gate(c.name, c, gate, worst)
        worst_a = _check_apply(c.name, c, gate, out, worst_a)
    _note("gate_mlp_wide/c%d_%s_cr%d" % (ch, cr_kind, cr), worst)
    if cr_kind == "quarter":
        _note("gate_mlp_wide/c%d_%s_cr%d exact twins" % (ch, cr_kind, cr), worst_x)
    _note("gate_apply (wide)/c%d_%s_cr%d" % (ch, cr_kind, cr), worst_a)


REAL_TABLES = ((32, (61, 130)), (64, (30, 130)), (128, (61, 33)), (256, (30, 33)))


@pytest.mark.parametrize("family", ("conv_cl", "conv_wino_cl"))
@pytest.mark.parametrize("ch,hw", REAL_TABLES)
def test_gate_on_real_tables(ch, hw, family):
    """conv_cl / conv_wino_cl(chan_sums=...) into channel_gate_apply_cl with out = y (the engine's call) at shapes whose tables,
    zero rows for the segments outside the image included, are long enough for the eight-way loop (every conv_cl table here; the
    Winograd tables at C 128 and 256), against the float64 gate of the float64 sums of the kernel's own y.  A pixel's term meets
    the adds of its table entry (32 pixels for conv_cl, 64 for conv_wino_cl) and those of the table's chunks."""
    b, (h, w) = 2, hw
    rng = np.random.default_rng(cases._seed("cl/real/%d" % ch))
    x = _dense(cases._f32(rng.standard_normal((b, h, w, ch))))
    wt = _t(cases._f32(rng.standard_normal((ch, ch, 3, 3)) * (2.0 / (9 * ch)) ** 0.5))
    if family == "conv_cl":
        assert ops.conv_cl_supported(x, ch, (3, 3))
        chunks, seg = ops.conv_sum_chunks(h, w), 32
        sums = torch.full((b, chunks, ch), NAN, device=DEV)
        mt = 1 if ch == 32 else 2
        y = ops.conv_cl(x, ops.conv_prepare(wt, mt), None, 0, ch, (3, 3), mt=mt, chan_sums=sums)
    else:
        assert ops.conv_wino_ok((3, 3), 1, ch, ch)
        chunks, seg = ops.conv_wino_sum_chunks(h, w), 64
        sums = torch.full((b, chunks, ch), NAN, device=DEV)
        y = ops.conv_wino_cl(x, ops.conv_wino_prepare(wt, 2), None, 0, ch, mb=2, chan_sums=sums)
    parts = 1024 // ch
    assert (chunks > 7 * parts) == (family == "conv_cl" or ch >= 128)         # where the main loop runs
    bias, w1, b1, w2, b2 = cases.real_table_weights(ch)
    c = cases.gate_case_from_map(_np(y).reshape(b, h * w, ch), h * w, bias, w1, b1, w2, b2, terms=seg + chunks)
    c.name, c.b, c.c, c.y = "real/%s_c%d" % (family, ch), b, ch, _np(y).reshape(b, h * w, ch)
    assert np.abs(c.pre).max() <= 6.0 and (c.hidden > 0).any(1).all()
    # the table adds up to the map: every entry is a float32 sum of at most `seg` pixels
    table = sums.cpu().numpy().astype(np.float64)
    worst_t = _judge(c.name + " table total", table.sum(1), c.total, cases.gamma(seg) * c.mag, 0.0)
    c.xres = cases._f32(rng.standard_normal((b, h * w, ch)))
    xres = _dense(c.xres.reshape(b, h, w, ch))
    ws = torch.full((b * ch,), NAN, device=DEV)
    out = ops.channel_gate_apply_cl(y, _t(bias), _t(w1), _t(b1), _t(w2), _t(b2), xres, sums, ws, out=y)
    assert out is y
    worst = _check_gate(c.name, c, ws, 0.0)
    worst_a = _check_apply(c.name, c, ws, out, 0.0)
    assert 0.05 <= cases.clipped_share(_np(out)) <= 0.60
    _note("gate_real_table/%s_c%d_k%d gate" % (family, ch, chunks), worst)
    _note("gate_real_table/%s_c%d_k%d table total" % (family, ch, chunks), worst_t)
    _note("gate_real_table/%s_c%d_k%d apply" % (family, ch, chunks), worst_a)


def _run_three_pass(c, short=0, in_place=False):
    """ops.channel_gate_residual_cl with y as a channel slice (pitch C + 8) and a workspace of exactly the required size (less
    `short`) inside a NaN buffer -> (table, gate, out, the buffer's floats outside the workspace)."""
    need = cases.gate_ws_floats(c.b, c.c, c.hw) - short
    big = torch.full((need + 24,), NAN, device=DEV)
    y, _ = _sliced(_map(c.y, c))
    xres = _dense(_map(c.xres, c))
    out = ops.channel_gate_residual_cl(y, *_gate_operands(c), xres, big[8:8 + need], out=y if in_place else None)
    n_tab = c.b * c.c * c.chunks
    outside = torch.cat((big[:8], big[8 + need:]))
    return big[8:8 + n_tab].view(c.b, c.chunks, c.c), big[8 + n_tab:8 + need].view(c.b, c.c), out, outside


@pytest.mark.parametrize("ch", cases.GATE_RES_C)
def test_three_pass_gate(ch):
    """colsum_partial + gate_mlp + gate_apply_cl at C 4 .. 256 and HW 1, 7, 255, 511, 512, 513, 1061 (B = 3, y sliced): the
    partial table against the float64 chunk sums inside n u sum|y|; the gate against the float64 gate of that very table (a sum
    of `chunks` terms: the step alone) and against the case's reference (a sum of HW terms); the output against the kernel's
    own gate.  The workspace has exactly B C (chunks + 1) floats, holds NaN and lies in a NaN buffer that stays NaN; one
    float less is refused; out = y gives the same bits.  The exact twins (HW 512, 2048): the table bit for bit."""
    worst_t = worst_g = worst = 0.0
    todo = [cases.gate_res_case(ch, h, w) for h, w in cases.GATE_RES_HW.values()]
    todo += [cases.gate_res_case(c2, h, w, True) for c2, (h, w) in cases.GATE_RES_TWINS if c2 == ch]
    for c in todo:
        table, gate, out, outside = _run_three_pass(c)
        assert bool(torch.isnan(outside).all()), c.name
        tab = table.cpu().numpy().astype(np.float64)
        if c.exact:
            assert np.array_equal(tab, c.table), c.name
            _check_gate(c.name, c, gate, 0.0)
        else:
            worst_t = _judge(c.name + " table", tab, c.table, c.table_bound, worst_t)
            worst_g = _check_gate(c.name + " step", c, gate, worst_g, ref=cases.gate_case_from_table(c, tab))
            _check_gate(c.name + " whole", c, gate, 0.0)
        worst = _check_apply(c.name, c, gate, out, worst)
        with pytest.raises(RuntimeError, match="channel_gate_residual_cl"):
            _run_three_pass(c, short=1)
        table2, gate2, out2, _ = _run_three_pass(c, in_place=True)
        assert _same_bits(table, table2) and _same_bits(gate, gate2) and _same_bits(out, out2), c.name
    _note("colsum_partial/c%d" % ch, worst_t)
    _note("gate_mlp/c%d" % ch, worst_g)
    _note("gate_apply (three-pass)/c%d" % ch, worst)


@pytest.mark.parametrize("ch", cases.GATE_APPLY_C + ("sweep",))
def test_gate_apply(ch):
    """gate_apply_cl behind ops.channel_gate_apply_cl at C 4, 8 and 128 (the entry points take the divisors of 1024 only), B = 3,
    HW = 15: the sample index is p / HW.  Out of place with y, xres and out as slices of wider maps whose other channels keep
    their sentinel, and with out = y.  "sweep": 4 x 299 x 877 x 4, the second trip of the grid-stride loop."""
    c = cases.gate_apply_sweep_case() if ch == "sweep" else cases.gate_apply_case(ch)
    ws = torch.full((c.b * c.c,), NAN, device=DEV)
    if ch == "sweep":
        out = ops.channel_gate_apply_cl(_dense(_map(c.y, c)), *_gate_operands(c), _dense(_map(c.xres, c)), _t(c.table), ws)
        _check_gate(c.name, c, ws, 0.0)
        _note("gate_apply/sweep", _check_apply(c.name, c, ws, out, 0.0))
        return
    y, yw = _sliced(_map(c.y, c), fill=SENT)
    xres, xw = _sliced(_map(c.xres, c), fill=SENT, off=8, extra=12)
    out, ow = _sliced(np.zeros((c.b, c.h, c.w, c.c)), fill=SENT, off=12, extra=16)
    assert ops.channel_gate_apply_cl(y, *_gate_operands(c), xres, _t(c.table), ws, out=out) is out
    _check_gate(c.name, c, ws, 0.0)
    worst = _check_apply(c.name, c, ws, out, 0.0)
    assert _neighbours_keep(ow, c.c, SENT, 12) and _neighbours_keep(yw, c.c, SENT) and _neighbours_keep(xw, c.c, SENT, 8)
    ops.channel_gate_apply_cl(y, *_gate_operands(c), xres, _t(c.table), ws, out=y)
    assert _same_bits(y, out) and _neighbours_keep(yw, c.c, SENT) and _neighbours_keep(xw, c.c, SENT, 8)
    _note("gate_apply/c%d" % ch, worst)


# ---------------------------------------------------------------------------------------------
# upsample_concat_cl
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.UP_CASES))
def test_upsample_concat(name):
    """One to three sources, channel splits (4), (8, 12, 4), (36, 4), (32, 64, 32); the identity (bit for bit: bound 0), 16 x 24
    from 8 x 12 and 4 x 6, Ho = 1, Wo = 1, 1 x 1 sources, the non-dyadic 16 x 23 from 7 x 10, dyadic ratios both ways, the sweep
    case.  Dense sources, then every source as a channel slice of a wider NaN map: the same bits."""
    c = cases.up_case(name)
    got = ops.upsample_concat_cl([_dense(v) for v in c.srcs], (c.ho, c.wo))
    assert tuple(got.shape) == (c.b, c.want.shape[-1], c.ho, c.wo)
    worst = _judge(name, _np(got), c.want, c.bound, 0.0)
    if name != "sweep":
        again = ops.upsample_concat_cl([_sliced(v, off=4 * (i + 1), extra=4 * (i + 2))[0] for i, v in enumerate(c.srcs)], (c.ho, c.wo))
        assert _same_bits(got, again)
    _note("upsample_concat/" + name, worst)


# ---------------------------------------------------------------------------------------------
# zero_views
# ---------------------------------------------------------------------------------------------
def _zero_view(shape, off, extra):
    b, h, w, c = shape
    wide = torch.full((b, h, w, c + extra), NAN, device=DEV)
    return wide[..., off:off + c].permute(0, 3, 1, 2), wide, off, c


ZERO_SHAPES = ((1, 1, 1, 4), (2, 5, 7, 36), (3, 31, 17, 128), (1, 2, 3, 8))


@pytest.mark.parametrize("n", (1, 2, 3, 4, "sweep"))
def test_zero_views(n):
    """One to four views of unequal size (the grid is sized by the largest; the first is one row of 4 floats), each a channel
    slice whose NaN neighbours survive; a view with zero rows beside a live one; "sweep": a 877 x 1196 x 4 view (the second trip
    of the grid-stride loop) with the one-row view behind it."""
    if n == "sweep":
        views = [_zero_view((1, 877, 1196, 4), 0, 0), _zero_view(ZERO_SHAPES[0], 4, 8)]
    else:
        order = ZERO_SHAPES[:n] if n != 3 else (ZERO_SHAPES[2], ZERO_SHAPES[0], ZERO_SHAPES[1])       # the largest first, too
        views = [_zero_view(s, 4 * (i + 1), 4 * (i + 3)) for i, s in enumerate(order)]
    ops.zero_views_cl([v[0] for v in views])
    for view, wide, off, c in views:
        assert bool((view == 0).all())
        assert wide.shape[-1] == c or _neighbours_keep(wide, c, NAN, off)
    if n == 2:
        # zero rows: nothing of that view is written (the wrapper cannot pass an empty tensor's pointer: the C entry itself)
        live, dead = _zero_view(ZERO_SHAPES[1], 4, 8), _zero_view(ZERO_SHAPES[3], 4, 8)
        ptrs = (ctypes.c_void_p * 2)(dead[0].data_ptr(), live[0].data_ptr())
        rc = _lib.load().smos_zero_views_cl(2, ptrs, _lib.i64_array([0, 2 * 5 * 7]), _lib.i64_array([8, 36]), _lib.i64_array([16, 44]),
                                            ops._stream(live[0]))
        assert rc == 0 and bool((live[0] == 0).all()) and bool(torch.isnan(dead[1]).all()) and _neighbours_keep(live[1], 36, NAN)
        rc = _lib.load().smos_zero_views_cl(1, ptrs, _lib.i64_array([0]), _lib.i64_array([8]), _lib.i64_array([16]), ops._stream(live[0]))
        assert rc == 0 and bool(torch.isnan(dead[1]).all())


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _gate_args(c, cr):
    z = lambda *s: torch.zeros(s, device=DEV)
    return z(c), z(cr, c), z(cr), z(c, cr), z(c)


def test_refusals_name_the_op_and_write_nothing():
    """C = 96 (and 36) for channel_gate_residual_cl; C = 96, 512 (and 36) for channel_gate_apply_cl; Cr = 65; C % 4 != 0; a slice at channel
    offset 2 (8 bytes off the alignment): each raises a RuntimeError that names the op, and the output keeps its sentinel.  The
    C entry of upsample_concat_cl also refuses a source pitch below its channel count, a non-positive source size and an output
    that is not 16-byte aligned (the wrapper cannot produce these)."""
    def cl(c, fill=SENT, h=2, w=3):
        return torch.full((2, h, w, c), fill, device=DEV).permute(0, 3, 1, 2)

    def refused(op, fn, *outs):
        with pytest.raises(RuntimeError, match=op):
            fn()
        assert all(bool((o == SENT).all()) for o in outs), op

    ws = torch.zeros(4096, device=DEV)
    # channel counts
    out = cl(96)
    refused("channel_gate_residual_cl", lambda: ops.channel_gate_residual_cl(cl(96, 1.0), *_gate_args(96, 24), cl(96, 1.0), ws, out=out), out)
    for c in (96, 512):
        out = cl(c)
        refused("channel_gate_apply_cl", lambda: ops.channel_gate_apply_cl(cl(c, 1.0), *_gate_args(c, 8), cl(c, 1.0),
                                                                            torch.zeros((2, 3, c), device=DEV), ws, out=out), out)
    out = cl(36)                                                     # a multiple of 4 that divides neither 256 nor 1024
    refused("channel_gate_residual_cl", lambda: ops.channel_gate_residual_cl(cl(36, 1.0), *_gate_args(36, 9), cl(36, 1.0), ws, out=out), out)
    refused("channel_gate_apply_cl", lambda: ops.channel_gate_apply_cl(cl(36, 1.0), *_gate_args(36, 9), cl(36, 1.0),
                                                                        torch.zeros((2, 3, 36), device=DEV), ws, out=out), out)
    # Cr = 65
    out = cl(32)
    refused("channel_gate_residual_cl", lambda: ops.channel_gate_residual_cl(cl(32, 1.0), *_gate_args(32, 65), cl(32, 1.0), ws, out=out), out)
    refused("channel_gate_apply_cl", lambda: ops.channel_gate_apply_cl(cl(32, 1.0), *_gate_args(32, 65), cl(32, 1.0),
                                                                        torch.zeros((2, 3, 32), device=DEV), ws, out=out), out)
    # C % 4 != 0
    out = cl(6)
    refused("bias_act_cl", lambda: ops.bias_act_cl(cl(6, 1.0), torch.zeros(6, device=DEV), 1, out=out), out)
    refused("downsample_epilogue_cl", lambda: ops.downsample_epilogue_cl(cl(6, 1.0), cl(6, 1.0), torch.zeros(6, device=DEV), 1, out=out), out)
    refused("channel_gate_residual_cl", lambda: ops.channel_gate_residual_cl(cl(6, 1.0), *_gate_args(6, 2), cl(6, 1.0), ws, out=out), out)
    refused("channel_gate_apply_cl", lambda: ops.channel_gate_apply_cl(cl(6, 1.0), *_gate_args(6, 2), cl(6, 1.0),
                                                                        torch.zeros((2, 3, 6), device=DEV), ws, out=out), out)
    refused("upsample_concat_cl", lambda: ops.upsample_concat_cl([cl(6, 1.0)], (4, 6)))
    refused("zero_views_cl", lambda: ops.zero_views_cl([out]), out)
    # a slice at channel offset 2
    wide_in, wide_out = cl(16, 1.0), cl(16)
    x, out = wide_in[:, 2:10], wide_out[:, 2:10]
    good, good_out = wide_in[:, 4:12], wide_out[:, 4:12]
    bias = torch.zeros(8, device=DEV)
    refused("bias_act_cl", lambda: ops.bias_act_cl(x, bias, 1, out=good_out), wide_out)
    refused("bias_act_cl", lambda: ops.bias_act_cl(good, bias, 1, out=out), wide_out)
    refused("bias_act_cl", lambda: ops.bias_act_cl(good, bias, 1, out=good_out, residual=x), wide_out)
    refused("downsample_epilogue_cl", lambda: ops.downsample_epilogue_cl(good, x, bias, 1, out=good_out), wide_out)
    refused("downsample_epilogue_cl", lambda: ops.downsample_epilogue_cl(good, good, bias, 1, out=out), wide_out)
    refused("channel_gate_residual_cl", lambda: ops.channel_gate_residual_cl(x, *_gate_args(8, 2), good, ws, out=good_out), wide_out)
    refused("channel_gate_residual_cl", lambda: ops.channel_gate_residual_cl(good, *_gate_args(8, 2), good, ws[1:], out=good_out), wide_out)
    refused("channel_gate_apply_cl", lambda: ops.channel_gate_apply_cl(good, *_gate_args(8, 2), x, torch.zeros((2, 3, 8), device=DEV), ws,
                                                                        out=good_out), wide_out)
    refused("upsample_concat_cl", lambda: ops.upsample_concat_cl([good, x], (4, 6)))
    refused("zero_views_cl", lambda: ops.zero_views_cl([good_out, out]), wide_out)
    # the C entry of upsample_concat_cl
    lib = _lib.load()
    src = torch.ones((2, 2, 3, 8), device=DEV)
    dst = torch.full((2 * 4 * 6 * 8 + 4,), SENT, device=DEV)

    def raw(c=8, h=2, w=3, pitch=8, out_off=0):
        ptrs = (ctypes.c_void_p * 1)(src.data_ptr())
        rc = lib.smos_upsample_concat_cl(ptrs, _lib.i64_array([c]), _lib.i64_array([h]), _lib.i64_array([w]), _lib.i64_array([pitch]), 1,
                                         dst.data_ptr() + 4 * out_off, 2, 4, 6, ops._stream(src))
        _lib.check(rc, "smos_upsample_concat_cl")
    for change in (dict(pitch=4), dict(h=0), dict(w=-1), dict(out_off=1), dict(out_off=2)):
        refused("upsample_concat_cl", lambda: raw(**change), dst)
    raw()                                                            # and the launch after the refusals is a good one
    assert bool(((dst[:2 * 4 * 6 * 8] - 1.0).abs() <= 1e-6).all()) and bool((dst[2 * 4 * 6 * 8:] == SENT).all())

"""upconv_xy (csrc/upconv.hip) through smos_upconv_xy_units, the entry that takes the unit geometry: strip height and a cap
on the blocks.  The kernel keeps, per unit of work (sample, strip of rows, block of 256 threads of a row), a table of the y
taps of its rows and a three-slot window of x-pass rows in LDS (source row i in slot i % 3); the units are handed to blocks
in XCD order.  What can go wrong there and no existing case reaches:

  A  strips of 8, 8 and 5 rows x two column blocks, the second ragged (13 * 32 = 416 threads per row)     seams both ways
  B  strips of 32, 32 and 6 rows: source 1 slides about every second row, source 2 about every eighth,
     the strips start at rows that are no multiple of either period                                      table, i % 3
  C  1 and 3 blocks for A's 12 units: a block walks several, table and window rebuilt each time            barriers
  D  one source only, as z1 and as z2; the other pointer is null                                          never read
  E  Inf / NaN behind every dropped border tap; interior strip seams and the block seam keep their taps   drop by address
  F  out = conv_a, channels [16, 144) of a pitch of 160                                                   in place
  G  a 1 x 1 source, one-row and one-column sources, Wo = 1, C = 4                                        degenerate
  H  a sample alone against the sample in its batch                                                       unit decode

Every case: the one launch equals smos_upconv_xpass + smos_upconv_ypass bit for bit.  A, B, G also against
util.upconv_passes_ref in float64 inside UPCONV_U (24 A_z + P) of the case's own magnitudes (the bound of the pass tests of
tests/test_gpu_upconv.py; derivation in tests/util.py).  The kernels are handed known float32 tap products z.
"""
import functools
import types

import numpy as np
import pytest
import torch

from streammos_amd import _lib, ops
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0

# name -> B, (Ho, Wo), ((Hs, Ws), ...), C, strip
CASES = {
    "A": (2, (21, 13), ((10, 6), (5, 4)), 128, 8),
    "B": (1, (70, 5), ((33, 3), (9, 2)), 32, 32),
    "G_1x1": (2, (3, 2), ((1, 1),), 4, 8),                      # ratio 0 both ways
    "G_one_row_one_column": (2, (7, 9), ((1, 4), (3, 1)), 4, 8),
    "G_wo1": (2, (9, 1), ((4, 3),), 8, 16),
    "G_c4": (1, (10, 12), ((5, 4), (3, 3)), 4, 8),              # one lane per pixel
}


@functools.lru_cache(maxsize=None)
def _case(name):
    b, (ho, wo), sizes, ch, strip = CASES[name]
    rng = np.random.default_rng(util._seed("upconv_xy_units/" + name))
    c = types.SimpleNamespace(name=name, b=b, ho=ho, wo=wo, sizes=sizes, c=ch, strip=strip)
    c.conv_a = util.upconv_inputs(rng, (b, ho, wo, ch), "random")
    c.bias = util.upconv_inputs(rng, (ch,), "random")
    c.z = [util.upconv_inputs(rng, (b, hs, ws, 3, 3, ch), "random", 0.25) for hs, ws in sizes]
    assert all(util.upconv_xy_ok(hs, ho) for hs, _ in sizes)
    for a in [c.conv_a, c.bias] + c.z:
        assert a.dtype == np.float32 or np.array_equal(a, a.astype(np.float32))
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want(name, act):
    c = _case(name)
    want = util.upconv_passes_ref(c.conv_a, c.bias, c.z, act)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _bound(name):
    """u (24 A_z + P), [B, Ho, Wo, C], from the case's own magnitudes."""
    c = _case(name)
    mag = util.upconv_passes_ref(np.abs(c.conv_a), np.abs(c.bias), [np.abs(z) for z in c.z], 0)
    bound = util.UPCONV_U * (24.0 * mag + util.upconv_perturbation([(np.abs(z), s) for z, s in zip(c.z, c.sizes)], c.ho, c.wo))
    bound.setflags(write=False)
    return bound


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def _embed(arr, pitch, at):
    """arr [B, H, W, C] as channels [at, at + C) of a sentinel-filled [B, H, W, pitch] buffer -> (buffer, [B, C, H, W] view)."""
    b, h, w, c = arr.shape
    buf = torch.full((b, h, w, pitch), SENTINEL, dtype=torch.float32, device=DEV)
    buf[..., at:at + c] = _t(arr)
    return buf, buf[..., at:at + c].permute(0, 3, 1, 2)


def _zs(c, zs=None, samples=slice(None)):
    """(z [B*Hs*Ws, 9*C] on the device, Hs, Ws) per source."""
    zs = c.z if zs is None else zs
    return [(_t(np.asarray(z)[samples]).reshape(-1, 9 * c.c), hs, ws) for z, (hs, ws) in zip(zs, c.sizes)]


def _views(c, samples):
    """conv_a = channels [4, 4 + C) of a buffer of pitch C + 12, out = channels [8, 8 + C) of another of pitch C + 20."""
    conv_a = c.conv_a[samples]
    abuf, a = _embed(conv_a, c.c + 12, 4)
    obuf, o = _embed(np.full(conv_a.shape, SENTINEL), c.c + 20, 8)
    return abuf, a, obuf, o


def _host(c, abuf, a, obuf, o, samples):
    torch.cuda.synchronize()
    assert bool((abuf[..., :4] == SENTINEL).all()) and bool((abuf[..., 4 + c.c:] == SENTINEL).all()), "channels next to conv_a were written"
    assert torch.equal(a, _embed(c.conv_a[samples], c.c + 12, 4)[1]), "conv_a was written"
    assert bool((obuf[..., :8] == SENTINEL).all()) and bool((obuf[..., 8 + c.c:] == SENTINEL).all()), "channels next to out were written"
    return o.permute(0, 2, 3, 1).cpu().numpy()


def _fused(c, dev_zs, act, strip=None, max_blocks=0, samples=slice(None)):
    """One smos_upconv_xy_units launch, pitched out of place -> [B, Ho, Wo, C] on the host.  dev_zs: (z1, z2), either may be None."""
    abuf, a, obuf, o = _views(c, samples)
    z1, z2 = (tuple(dev_zs) + (None,))[:2]
    got = ops.upconv_xy_units(a, _t(c.bias), z1, z2, act, c.strip if strip is None else strip, max_blocks, out=o)
    assert got is o
    return _host(c, abuf, a, obuf, o, samples)


def _pair(c, dev_zs, act, samples=slice(None)):
    """smos_upconv_xpass per source + smos_upconv_ypass, the same layout."""
    lib = _lib.load()
    abuf, a, obuf, o = _views(c, samples)
    bias = _t(c.bias)
    st = ops._stream(a)
    b = a.shape[0]
    ts = []
    for z, hs, ws in dev_zs:
        t = torch.empty((b, 3, hs, c.wo, c.c), dtype=torch.float32, device=DEV)
        _lib.check(lib.smos_upconv_xpass(z.data_ptr(), t.data_ptr(), b, hs, ws, c.c, c.wo, st), "smos_upconv_xpass")
        ts.append((t, hs))
    (t1, h1), (t2, h2) = ts[0], (ts[1] if len(ts) > 1 else (None, 0))
    _lib.check(lib.smos_upconv_ypass(a.data_ptr(), c.c + 12, bias.data_ptr(), t1.data_ptr(), h1, t2.data_ptr() if t2 is not None else None, h2,
                                     o.data_ptr(), c.c + 20, b, c.ho, c.wo, c.c, int(act), st), "smos_upconv_ypass")
    return _host(c, abuf, a, obuf, o, samples)


def _check(label, got, want, bound):
    ok, ratio = util.msda_worst_ratio(got, want, bound)
    print("upconv-xy-units-ratio %-58s %.4f" % (label, ratio))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_geometry_of_the_cases():
    """What the docstring claims about A and B, from the numbers."""
    a = _case("A")
    assert [min(8, a.ho - y) for y in range(0, a.ho, 8)] == [8, 8, 5] and a.wo * a.c // 4 == 416 and 416 - 256 == 160
    assert all(2 * (hs - 1) < a.ho - 1 for hs, _ in a.sizes)
    b = _case("B")
    assert [min(32, b.ho - y) for y in range(0, b.ho, 32)] == [32, 32, 6]
    for (hs, _), period in zip(b.sizes, (2, 8)):
        i0 = util.upconv_lerp(hs, b.ho, np.float32)[0]
        slides = int((np.diff(i0) > 0).sum())
        assert period <= b.ho / slides < period + 1, (hs, slides)
        assert i0[31] % 3 != 0 or i0[63] % 3 != 0       # a strip starts with its first row away from slot 0


@pytest.mark.parametrize("act", util.UPCONV_ACTS)
def test_a_seams_in_both_directions(act):
    c = _case("A")
    zs = _zs(c)
    fused, pair = _fused(c, zs, act), _pair(c, zs, act)
    _check("A act %d, one launch (strip 8)" % act, fused, _want("A", act), _bound("A"))
    _check("A act %d, x pass + y pass" % act, pair, _want("A", act), _bound("A"))
    assert _same_bits(fused, pair), "the one launch and the pair differ"
    if act == 1:
        assert (fused == 0).any() and (fused > 0).any()
    if act == 0:        # every other strip height: the same bits
        for strip in (16, 32):
            assert _same_bits(_fused(c, zs, act, strip=strip), fused), "strip %d gives other bits than strip 8" % strip


def test_b_long_strips_slide_many_times():
    c = _case("B")
    zs = _zs(c)
    fused, pair = _fused(c, zs, 2), _pair(c, zs, 2)
    _check("B one launch (strip 32)", fused, _want("B", 2), _bound("B"))
    _check("B x pass + y pass", pair, _want("B", 2), _bound("B"))
    assert _same_bits(fused, pair), "the one launch and the pair differ"
    for strip in (8, 16):
        assert _same_bits(_fused(c, zs, 2, strip=strip), fused), "strip %d gives other bits than strip 32" % strip


@pytest.mark.parametrize("max_blocks", [1, 3])
def test_c_a_block_walks_several_units(max_blocks):
    c = _case("A")
    zs = _zs(c)
    assert c.b * 3 * 2 == 12 and 12 % max_blocks == 0
    free = _fused(c, zs, 2)
    capped = _fused(c, zs, 2, max_blocks=max_blocks)
    assert _same_bits(capped, free), "%d block(s) for 12 units give other bits than one block per unit" % max_blocks
    assert _same_bits(capped, _pair(c, zs, 2))


@pytest.mark.parametrize("which", [0, 1])
def test_d_one_source_and_the_absent_one_is_never_read(which):
    """The present source sits at offset 0 of an allocation of its own, larger than the sizes the caching allocator pools
    (a segment straight from the driver); the absent one is a null pointer.  As z1 and as z2: the same bits as the pair."""
    c = _case("A")
    hs, ws = c.sizes[which]
    one = types.SimpleNamespace(**{**vars(c), "sizes": (c.sizes[which],), "z": [c.z[which]]})
    n = c.b * hs * ws * 9 * c.c
    own = torch.empty(6 << 20, dtype=torch.float32, device=DEV)           # 24 MiB
    z = own[:n].view(-1, 9 * c.c)
    z.copy_(_t(c.z[which]).reshape(-1, 9 * c.c))
    assert z.data_ptr() == own.data_ptr()
    pair = _pair(one, [(z, hs, ws)], 2)
    as_z1 = _fused(one, ((z, hs, ws), None), 2)
    as_z2 = _fused(one, (None, (z, hs, ws)), 2)
    assert _same_bits(as_z1, pair) and _same_bits(as_z2, pair)
    want = util.upconv_passes_ref(c.conv_a, c.bias, one.z, 2)
    mag = util.upconv_passes_ref(np.abs(c.conv_a), np.abs(c.bias), [np.abs(one.z[0])], 0)
    bound = util.UPCONV_U * (24.0 * mag + util.upconv_perturbation([(np.abs(one.z[0]), (hs, ws))], c.ho, c.wo))
    _check("D source %d alone" % (which + 1), as_z1, want, bound)


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
def test_e_border_taps_are_dropped_and_interior_seams_keep_theirs(value):
    """The poison sits where, at an image border, only dropped taps read (upconv_poison_borders, all four sides); further
    inside the same elements are real taps.  An output is finite exactly where the float32 emulation of the passes, which
    reads no dropped tap, is finite -- every corner among them -- and there it has the bits of the clean run.  The rows at
    the strip seams 7|8 and 15|16 and the columns at the block seam 7|8 are no image borders: they equal the pair, taps and
    all, on the clean and on the poisoned input.
    The expected mask rests on util.upconv_lerp(dtype=float32) picking the same source rows and the same zero weights as
    lerp_of of csrc/upconv.hip at the non-dyadic ratios of case A (21 <- 10, 5 and 13 <- 6, 4): if only the mask assertion
    fails, and the pair fails it in the same places, compare the two lerp forms first."""
    c = _case("A")
    clean = _fused(c, _zs(c), 0)
    poisoned = [util.upconv_poison_borders(z, util.UPCONV_SIDES, value) for z in c.z]
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(util.upconv_passes_ref(c.conv_a, c.bias, poisoned, 0, dtype=np.float32))
    corners = [np.s_[:, 0, 0], np.s_[:, 0, -1], np.s_[:, -1, 0], np.s_[:, -1, -1]]
    assert all(finite[k].all() for k in corners) and not finite.all()
    zs = _zs(c, poisoned)
    got, pair = _fused(c, zs, 0), _pair(c, zs, 0)
    for k in corners:
        assert np.isfinite(got[k]).all(), "a dropped tap leaked into a corner"
    assert np.array_equal(np.isfinite(got), finite), "an output is finite where a real tap reads the poison, or the reverse"
    assert _same_bits(np.where(finite, got, 0.0).astype(np.float32), np.where(finite, clean, 0.0).astype(np.float32))
    assert np.array_equal(np.isfinite(pair), finite) and _same_bits(np.where(finite, pair, 0.0).astype(np.float32), np.where(finite, got, 0.0).astype(np.float32))
    clean_pair = _pair(c, _zs(c), 0)
    seams = [np.s_[:, 7], np.s_[:, 8], np.s_[:, 15], np.s_[:, 16], np.s_[:, :, 7], np.s_[:, :, 8]]
    for k in seams:
        assert _same_bits(np.ascontiguousarray(clean[k]), np.ascontiguousarray(clean_pair[k])), "an interior seam differs from the pair"
        assert not finite[k].all()                          # real taps of the seam lines do read the poison


def test_f_in_place_through_a_channel_slice():
    c = _case("A")
    zs = _zs(c)
    want = _fused(c, zs, 2)
    buf, view = _embed(c.conv_a, 160, 16)
    assert c.c == 128 and view.stride(3) == 160
    got = ops.upconv_xy_units(view, _t(c.bias), zs[0], zs[1], 2, c.strip)
    torch.cuda.synchronize()
    assert got is view
    assert _same_bits(view.permute(0, 2, 3, 1).cpu().numpy(), want), "in place differs from out of place"
    assert bool((buf[..., :16] == SENTINEL).all()) and bool((buf[..., 144:] == SENTINEL).all()), "the 32 foreign channels were written"


@pytest.mark.parametrize("name", [k for k in CASES if k.startswith("G_")])
def test_g_degenerate_geometry(name):
    c = _case(name)
    zs = _zs(c)
    for act in (0, 2):
        fused, pair = _fused(c, zs, act), _pair(c, zs, act)
        _check("%s act %d one launch" % (name, act), fused, _want(name, act), _bound(name))
        assert _same_bits(fused, pair), "the one launch and the pair differ"
    assert _same_bits(_fused(c, zs, 2, strip=32, max_blocks=1), fused)


def test_h_a_sample_alone_equals_the_sample_in_its_batch():
    c = _case("A")
    batch = _fused(c, _zs(c), 2)
    for b in range(c.b):
        alone = _fused(c, _zs(c, samples=slice(b, b + 1)), 2, samples=slice(b, b + 1))
        assert _same_bits(alone[0], batch[b]), b


def test_refusals_of_the_unit_geometry():
    c = _case("G_c4")
    zs = _zs(c)
    abuf, a, obuf, o = _views(c, slice(None))
    for strip, blocks in ((0, 0), (12, 0), (64, 0), (8, -1)):
        with pytest.raises(RuntimeError, match="upconv_xy: strip must be 8, 16 or 32"):
            ops.upconv_xy_units(a, _t(c.bias), zs[0], zs[1], 2, strip, blocks, out=o)
    with pytest.raises(RuntimeError, match="upconv_xy: null / unaligned pointer or no source"):
        ops.upconv_xy_units(a, _t(c.bias), None, None, 2, 8, out=o)
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all())

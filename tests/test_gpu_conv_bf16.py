"""The opt-in bf16 convolutions (csrc/conv_bf16.hip, InferenceEngine(conv_precision="bf16")): the kernel against float64 on the
bf16-rounded operands, the engine against a torch emulation of the mode, routing, the runners in bf16, and an accuracy
report of bf16 against fp32 on the seeded network."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from streammos_amd import engine as engine_mod
from streammos_amd import ops, preprocess, streaming, synth
from streammos_amd.refapi.config import StreamMOS as cfg
from streammos_amd.refapi.models import StreamMOS
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the layer classes of tools/ubench_conv.py LAYERS: name, cin, cout, (kh, kw), stride, (h, w) at network size
LAYERS = [
    ("hdr_bev 3x3 32", 32, 32, (3, 3), 1, (256, 256)), ("hdr_bev 7x3", 32, 32, (7, 3), 1, (256, 256)),
    ("hdr_bev 3x7", 32, 32, (3, 7), 1, (256, 256)), ("hdr_bev 64->32", 64, 32, (3, 3), 1, (256, 256)),
    ("hdr_rv 3x3 32", 32, 32, (3, 3), 1, (32, 1024)), ("hdr_rv 1x1", 32, 32, (1, 1), 1, (32, 1024)),
    ("res1 down 3x3s2", 64, 64, (3, 3), 2, (256, 256)), ("res1 down 1x1", 64, 64, (1, 1), 1, (256, 256)),
    ("res1 5x3", 64, 64, (5, 3), 1, (128, 128)), ("res1 3x5", 64, 64, (3, 5), 1, (128, 128)),
    ("res1 128->64", 128, 64, (3, 3), 1, (128, 128)), ("res1 3x3 64", 64, 64, (3, 3), 1, (128, 128)),
    ("res1_rv 3x3 64", 64, 64, (3, 3), 1, (16, 512)), ("res1_rv 1x1", 64, 64, (1, 1), 1, (16, 512)),
    ("res2 down 3x3s2", 128, 128, (3, 3), 2, (128, 128)), ("res2 down 1x1", 128, 128, (1, 1), 1, (128, 128)),
    ("res2 3x3 128", 128, 128, (3, 3), 1, (64, 64)),
    ("conv_1a 64->128", 64, 128, (3, 3), 1, (256, 256)), ("conv_2 128->64", 128, 64, (3, 3), 1, (256, 256)),
]
# one layer per class at full size (B = 4): every kernel shape, both strides, all three cout widths
FULL = ("hdr_bev 3x3 32", "hdr_bev 7x3", "hdr_bev 3x7", "hdr_bev 64->32", "hdr_rv 3x3 32", "res1 5x3", "res1 3x5",
        "res1 down 3x3s2", "res1 128->64", "res1_rv 3x3 64", "res2 down 1x1", "res2 3x3 128", "conv_1a 64->128",
        "conv_2 128->64")
SENTINEL = 1234.5


def _bf(t):
    return t.to(torch.bfloat16).double()


def _cl_buffer(b, c, h, w, extra=0, off=0, fill=None, gen=None):
    """channels-last [B, C, H, W] view at channel offset `off` of a [B, H, W, C + extra] buffer (the rest = fill)"""
    buf = torch.randn(b, h, w, c + extra, generator=gen).to(DEV) if fill is None else torch.full((b, h, w, c + extra), fill, device=DEV)
    return buf, buf[..., off:off + c].permute(0, 3, 1, 2)


def _reference(x, w, bias, act, stride, pad, res=None):
    """float64 on the bf16-rounded operands, the kernel's epilogue; plus the error bound of the test"""
    xb, wb = _bf(x), _bf(w)
    acc = F.conv2d(xb, wb, None, stride, pad)
    mag = F.conv2d(xb.abs(), wb.abs(), None, stride, pad)
    v = acc
    slack = torch.zeros_like(v)
    if bias is not None:
        v = v + bias.double().view(1, -1, 1, 1)
        slack = slack + bias.double().abs().view(1, -1, 1, 1) * 2.0 ** -23
    if res is not None:
        v = v + res.double()
        slack = slack + res.double().abs() * 2.0 ** -23          # the fp32 add of the residual rounds once more
    if act == 1:
        v = v.clamp_min(0)
    elif act == 2:
        v = torch.where(v >= 0, v, 0.01 * v)
    return v, 1e-5 * mag + slack + 1e-30


def _run_case(b, cin, cout, k, stride, hw, act=1, bias=True, res=False, sums=False, sliced=False, seed=0, x=None):
    gen = torch.Generator().manual_seed(seed)
    kh, kw = k
    h, wd = hw
    pad = (kh // 2, kw // 2)
    ho, wo = (h + 2 * pad[0] - kh) // stride + 1, (wd + 2 * pad[1] - kw) // stride + 1
    if x is None:
        if sliced:
            _, x = _cl_buffer(b, cin, h, wd, extra=64, off=32, gen=gen)
        else:
            _, x = _cl_buffer(b, cin, h, wd, gen=gen)
    w = torch.randn(cout, cin, kh, kw, generator=gen).to(DEV) / (cin * kh * kw) ** 0.5
    bv = torch.randn(cout, generator=gen).to(DEV) if bias else None
    r = None
    if res:
        if sliced:
            _, r = _cl_buffer(b, cout, ho, wo, extra=32, off=32, gen=gen)
        else:
            _, r = _cl_buffer(b, cout, ho, wo, gen=gen)
    if sliced:
        obuf, out = _cl_buffer(b, cout, ho, wo, extra=64, off=32, fill=SENTINEL)
    else:
        obuf, out = None, ops.empty_cl(b, cout, ho, wo, DEV)
    # NaN-filled: a chunk of the table the kernel leaves unwritten fails the check below
    cs = torch.full((b, ops.conv_sum_chunks(ho, wo), cout), float("nan"), device=DEV) if sums else None
    wp = ops.conv_bf16_prepare(w)
    y = ops.conv_bf16_cl(x, wp, bv, act, cout, k, stride=stride, residual=r, out=out, chan_sums=cs)
    ref, bound = _reference(x, w, bv, act, stride, pad, r)
    err = (y.double() - ref).abs()
    ratio = (err / bound).max().item()
    assert ratio <= 1.0, ("error over the bound", b, cin, cout, k, stride, hw, act, bias, res, ratio)
    if obuf is not None:
        assert torch.all(obuf[..., :32] == SENTINEL) and torch.all(obuf[..., 32 + cout:] == SENTINEL), "neighbour channels written"
    if sums:
        yd = y.double().permute(0, 2, 3, 1)                     # [B, Ho, Wo, C]
        xt, hq = (wo + 31) // 32, (ho + 3) // 4
        pad_y = torch.zeros(b, hq * 4, xt * 32, cout, dtype=torch.float64, device=DEV)
        pad_y[:, :ho, :wo] = yd
        want = pad_y.view(b, hq, 4, xt, 32, cout).sum(4).permute(0, 1, 3, 2, 4).reshape(b, hq * xt * 4, cout)
        scale = pad_y.abs().view(b, hq, 4, xt, 32, cout).sum(4).permute(0, 1, 3, 2, 4).reshape(b, hq * xt * 4, cout)
        assert ((cs.double() - want).abs() <= 1e-6 * scale + 1e-30).all(), "channel sums"
    # deterministic: a second launch is bit-identical
    y2 = ops.conv_bf16_cl(x, wp, bv, act, cout, k, stride=stride, residual=r, out=out.clone() if obuf is None else None,
                          chan_sums=cs.clone() if sums else None)
    assert torch.equal(y2, y)
    return ratio


@pytest.mark.parametrize("name,cin,cout,k,stride,hw", [l for l in LAYERS])
def test_kernel_reduced_sizes(name, cin, cout, k, stride, hw):
    """every layer class at small, ragged sizes (H, W not multiples of 4 or 32), B in {1, 3}, all activations, bias on and off"""
    for i, (b, h, w) in enumerate(((1, 13, 37), (3, 9, 70))):
        act = (0, 1, 2)[i % 3]
        _run_case(b, cin, cout, k, stride, (h, w), act=act, bias=i == 0, seed=i)
    _run_case(1, cin, cout, k, stride, (6, 45), act=2, bias=True, seed=7)


@pytest.mark.parametrize("name", FULL)
def test_kernel_full_size(name):
    _, cin, cout, k, stride, hw = next(l for l in LAYERS if l[0] == name)
    _run_case(4, cin, cout, k, stride, hw, act=1, bias=True, seed=11)


@pytest.mark.parametrize("cin,cout,k", [(32, 32, (3, 3)), (64, 64, (3, 3)), (128, 128, (3, 3)), (64, 32, (3, 3)), (32, 32, (1, 1))])
def test_kernel_residual_sums_and_slices(cin, cout, k):
    """residual (BasicBlock / Unbalance fuse convs), channel sums in the conv_cl table layout, and input / residual / output as
    channel slices of wider buffers whose other channels hold a sentinel that must stay untouched"""
    _run_case(2, cin, cout, k, 1, (19, 41), act=1, res=True, seed=3)
    _run_case(2, cin, cout, k, 1, (19, 41), act=0, bias=False, sums=True, seed=4)
    _run_case(2, cin, cout, k, 1, (11, 70), act=1, res=True, sliced=True, seed=5)
    _run_case(2, cin, cout, k, 1, (11, 70), act=2, sums=True, sliced=True, seed=6)


@pytest.mark.parametrize("b,cin,cout,hw", [(4, 128, 128, (66, 64)), (2, 64, 64, (130, 128)), (1, 32, 32, (67, 33))])
def test_kernel_sums_table_rows_past_the_image(b, cin, cout, hw):
    """Ho % 4 != 0 at block shapes of 1 and 2 output rows: every row segment of the table up to 4 * ceil(Ho / 4) rows is
    written (zeros past Ho), as smos_conv_cl writes it -- the table starts NaN-filled"""
    _run_case(b, cin, cout, (3, 3), 1, hw, act=0, bias=False, sums=True, seed=8)


def test_kernel_rounding_ties():
    """activations on or one ulp beside a bf16 rounding tie (low 16 bits 0x8000, 0x7FFF, 0x8001): truncation or round-half-up
    instead of round-to-nearest-even changes every product"""
    gen = torch.Generator().manual_seed(21)
    b, cin, h, w = 2, 64, 12, 40
    hi = torch.randint(0, 1 << 16, (b, h, w, cin), generator=gen, dtype=torch.int64)
    hi = (hi & 0x807F) | (0x3F00 + (torch.randint(0, 4, hi.shape, generator=gen) << 7))     # |x| in [0.5, 8)
    lo = torch.tensor([0x8000, 0x7FFF, 0x8001])[torch.randint(0, 3, hi.shape, generator=gen)]
    bits = ((hi << 16) | lo).to(torch.int64)
    bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32)
    x = bits.view(torch.float32).to(DEV).permute(0, 3, 1, 2)
    assert (bits.view(torch.float32).view(torch.int32) & 0xFFFF).eq(0x8000).any()
    _run_case(b, cin, 64, (3, 3), 1, (h, w), act=0, bias=False, x=x, seed=22)
    # and the rounding mode itself, without the matrix: a 1x1 conv with one-hot weights returns bf16(x) exactly
    w1 = torch.eye(64, device=DEV).view(64, 64, 1, 1)
    y = ops.conv_bf16_cl(x, ops.conv_bf16_prepare(w1), None, 0, 64, (1, 1))
    assert torch.equal(y, x.to(torch.bfloat16).float())


# ---- engine level ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    m = StreamMOS.AttNet(cfg.get_config()[2])
    m.load_state_dict(synth.seeded_state_dict(m.state_dict()), strict=True)
    return m.to(DEV).eval()


def _unpack(wprep, cout, cin, kh, kw):
    v = wprep.float().view(cin // 32, kh, kw, cout // 32, 2, 2, 32, 8)      # [chunk, ky, kx, q, s, h, m, j]
    return v.permute(3, 6, 0, 4, 5, 7, 1, 2).reshape(cout, cin, kh, kw)


def _emulated_conv_bf16_cl(x, wprep, bias, act, cout, kernel, stride=1, padding=None, residual=None, out=None, chan_sums=None):
    """torch emulation of the mode: float64 conv on bf16-rounded weights and inputs, the kernel's fp32 epilogue"""
    b, cin, h, w = x.shape
    kh, kw = kernel
    pad = padding if padding is not None else (kh // 2, kw // 2)
    wb = _unpack(wprep, cout, cin, kh, kw).double()
    v = F.conv2d(_bf(x), wb, None, stride, pad).float()
    if bias is not None:
        v = v + bias.view(1, -1, 1, 1)
    if residual is not None:
        v = v + residual
    if act == 1:
        v = v.clamp_min(0)
    elif act == 2:
        v = torch.where(v >= 0, v, 0.01 * v)
    ho, wo = v.shape[2:]
    if out is None:
        out = ops.empty_cl(b, cout, ho, wo, x.device)
    out.copy_(v)
    if chan_sums is not None:
        xt, hq = (wo + 31) // 32, (ho + 3) // 4
        pad_y = torch.zeros(b, hq * 4, xt * 32, cout, device=x.device)
        pad_y[:, :ho, :wo] = v.permute(0, 2, 3, 1)
        chan_sums.copy_(pad_y.view(b, hq, 4, xt, 32, cout).sum(4).permute(0, 1, 3, 2, 4).reshape(b, hq * xt * 4, cout))
    return out


_REAL_CONV_BF16 = ops.conv_bf16_cl


def _checked_emulation(worst):
    """the emulation, which also runs the real kernel on the SAME engine operands and records the worst error of the kernel
    against float64 (as a fraction of the kernel test's bound) -- a per-launch check that chaos downstream cannot blur"""
    def conv(x, wprep, bias, act, cout, kernel, stride=1, padding=None, residual=None, out=None, chan_sums=None):
        kh, kw = kernel
        pad = padding if padding is not None else (kh // 2, kw // 2)
        sums = None if chan_sums is None else torch.full_like(chan_sums, float("nan"))
        real = _REAL_CONV_BF16(x, wprep, bias, act, cout, kernel, stride=stride, padding=padding, residual=residual,
                               chan_sums=sums)
        w = _unpack(wprep, cout, x.shape[1], kh, kw)
        ref, bound = _reference(x, w, bias, act, stride, pad, residual)
        worst[0] = max(worst[0], ((real.double() - ref).abs() / bound).max().item())
        worst[1] += 1
        if sums is not None:          # the kernel's sums against float64 sums of its own output, in the conv_cl layout
            b, c, ho, wo = real.shape
            xt, hq = (wo + 31) // 32, (ho + 3) // 4
            pad_y = torch.zeros(b, hq * 4, xt * 32, c, dtype=torch.float64, device=DEV)
            pad_y[:, :ho, :wo] = real.double().permute(0, 2, 3, 1)
            cut = lambda t: t.view(b, hq, 4, xt, 32, c).sum(4).permute(0, 1, 3, 2, 4).reshape(b, hq * xt * 4, c)
            ok = ((sums.double() - cut(pad_y)).abs() <= 1e-6 * cut(pad_y.abs()) + 1e-30).all().item()
            worst[2] += 0 if ok else 1
            worst[3] += 1
        return _emulated_conv_bf16_cl(x, wprep, bias, act, cout, kernel, stride, padding, residual, out, chan_sums)
    return conv


def _infer_frames(m, frames):
    outs, memory = [], None
    with torch.no_grad():
        for i, batch in enumerate(frames):
            tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
            pred, _, _, _, memory = m.infer(tb, i, memory)
            outs.append(pred.clone())
    return outs


def test_engine_matches_emulated_mode(model, monkeypatch):
    """the bf16 engine with the real kernel against the same engine with ops.conv_bf16_cl replaced by a torch emulation
    (float64 conv on bf16-rounded operands, the same epilogue): pins the engine-level semantics of the mode (which layers,
    which epilogue, which operands) independently of how close bf16 is to fp32.

    Bars, measured: the two runs differ only in the fp32 summation order, but an activation one fp32 ulp apart rounds to
    another bf16 value now and then, and each layer turns a relative perturbation d into about sqrt(d * 2^-8) / 2: after a
    few layers the difference sits at the bf16 noise level itself (max 2.8e-3 of the logit range on frame 0, the same order
    as bf16 against fp32).  So the end-to-end bars are a max of 1e-2 and a mean of 5e-4 of the range with >= 99.9 % equal
    labels, and every launch of the emulated run also runs the real kernel on the same engine operands, checked against
    float64 at the kernel tests' bound."""
    frames = list(cases.e2e_frames(3))
    model.engine_conv_precision = "bf16"
    worst = [0.0, 0, 0, 0]          # worst error / bound, launches, launches with wrong sums, launches with sums
    seen = {"real": [], "emu": []}

    def recording(tag, fn):
        def conv(*a, **k):
            y = fn(*a, **k)
            if len(seen[tag]) < 64:
                seen[tag].append(y.clone())
            return y
        return conv
    try:
        monkeypatch.setattr(ops, "conv_bf16_cl", recording("real", _REAL_CONV_BF16))
        real = _infer_frames(model, frames)
        stats = model._engine.conv_precision_stats()
        monkeypatch.setattr(ops, "conv_bf16_cl", recording("emu", _checked_emulation(worst)))
        emu = _infer_frames(model, frames)
    finally:
        model.engine_conv_precision = "fp32"
    assert stats["bf16"] >= 25 and stats["fallback"] == 0, stats
    print("%d emulated launches, worst kernel error %.3f of the bound; %d launches with channel sums, %d wrong" % (
        worst[1], worst[0], worst[3], worst[2]))
    assert worst[1] >= 3 * stats["bf16"] and worst[0] <= 1.0 and worst[3] > 0 and worst[2] == 0, worst
    # measured error growth along frame 0: the layer outputs of the two runs, launch by launch
    growth = []
    for k, (a, e) in enumerate(zip(seen["real"][:stats["bf16"]], seen["emu"][:stats["bf16"]])):
        growth.append((a - e).abs().max().item() / max(e.abs().max().item(), 1e-30))
    print("frame 0, layer by layer, max |kernel run - emulated run| / max |emulated|: " + " ".join("%.1e" % g for g in growth))
    for i, (a, e) in enumerate(zip(real, emu)):
        rng = (e.max() - e.min()).item()
        d = (a - e).abs() / rng
        agree = (a.argmax(1) == e.argmax(1)).float().mean().item()
        print("frame %d: bf16 kernel vs emulation max %.2e mean %.2e of the logit range, labels %.5f" % (
            i, d.max().item(), d.mean().item(), agree))
        assert d.max().item() <= 1e-2 and d.mean().item() <= 5e-4 and agree >= 0.999, (i, d.max().item(), agree)


_FP32_KERNELS = ("conv_cl", "conv_rows_cl", "conv_wino_cl", "conv_wino1d_cl", "basic_block_cl", "unbalance_block_cl")


def test_routing(model, monkeypatch):
    frames = list(cases.e2e_frames(1))
    model.engine_conv_precision = "bf16"
    try:
        with monkeypatch.context() as mp:
            for name in _FP32_KERNELS:
                def boom(*a, _n=name, **k):
                    raise AssertionError("fp32 conv %s called in bf16 mode" % _n)
                mp.setattr(ops, name, boom)
            _infer_frames(model, frames)
        eng = model._engine
        assert eng.conv_precision == "bf16" and eng.conv_precision_stats()["fallback"] == 0
        assert eng.conv_precision_stats()["bf16"] > 0
    finally:
        model.engine_conv_precision = "fp32"
    with monkeypatch.context() as mp:
        def boom16(*a, **k):
            raise AssertionError("conv_bf16_cl called in the default mode")
        mp.setattr(ops, "conv_bf16_cl", boom16)
        _infer_frames(model, frames)
    assert model._engine is not eng and model._engine.conv_precision == "fp32"       # rebuilt on the change
    assert model._engine.conv_precision_stats() == {"bf16": 0, "fallback": 0}
    with pytest.raises(ValueError):
        engine_mod.InferenceEngine(model, conv_precision="fp16")


# ---- runners in bf16 -------------------------------------------------------------------------------------------------

def _small_sequence(n, seed=0):
    spec = preprocess.VoxelSpec()
    scans = [synth.synthetic_scan(seed + k, 16, 120) for k in range(n + 2)]
    poses = [synth.synthetic_pose(k) for k in range(n + 2)]
    samples = []
    for i in range(n):
        idx = preprocess.window_indices(i, n + 2, 3)
        samples.append(preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True))
    return scans, poses, samples


def _run(runner, scans, poses, samples, lookahead=False):
    devs = [runner.upload(s, scans[i]) for i, s in enumerate(samples)]
    outs = []
    for i in range(len(samples)):
        kw = {"next_dev": devs[i + 1] if i + 1 < len(samples) else None} if lookahead else {}
        o = runner.step(devs[i], poses[i], **kw)
        outs.append((o["pred_cls"].clone(), o["raw_labels"].clone(), [(f, l.clone()) for f, l in o.get("voted") or []]))
    torch.cuda.synchronize()
    return outs


def test_runners_in_bf16(model):
    scans, poses, samples = _small_sequence(5)
    try:
        plain = _run(streaming.StreamRunner(model, DEV, vote=True, conv_precision="bf16"), scans, poses, samples)
        assert model.engine_conv_precision == "bf16"
        piped = _run(streaming.StreamRunner(model, DEV, vote=True, pipeline=True, conv_precision="bf16"), scans, poses, samples,
                     lookahead=True)
        for (p0, r0, v0), (p1, r1, v1) in zip(plain, piped):
            assert torch.equal(p0, p1) and torch.equal(r0, r1)
            assert [f for f, _ in v0] == [f for f, _ in v1] and all(torch.equal(a[1], b[1]) for a, b in zip(v0, v1))
        full = _run(streaming.StreamRunner(model, DEV, vote=False, skip_padding=False, conv_precision="bf16"), scans, poses, samples)
        for (p0, r0, _), (p1, r1, _) in zip(plain, full):
            assert torch.equal(r0, r1)                     # the labels of every real point
            live = (p0 != 0).any(1)                        # skip_padding leaves the padding tail's logits at zero
            assert torch.equal(p0.movedim(1, -1)[live], p1.movedim(1, -1)[live])
        graph = _run(streaming.StreamRunner(model, DEV, vote=False, graph=True, conv_precision="bf16"), scans, poses, samples)
        for (p0, r0, _), (p1, r1, _) in zip(plain, graph):
            assert torch.equal(r0, r1)
            live = (p0 != 0).any(1)                        # the graphs compute the padding tail's logits too
            assert torch.equal(p0.movedim(1, -1)[live], p1.movedim(1, -1)[live])
    finally:
        model.engine_conv_precision = "fp32"


def test_seg_model_instance_vote_in_bf16():
    from streammos_amd.refapi.config import StreamMOS_seg as seg_cfg
    from streammos_amd.refapi.models import StreamMOS_seg
    m = StreamMOS_seg.AttNet(seg_cfg.get_config()[2])
    m.load_state_dict(synth.seeded_state_dict(m.state_dict()), strict=True)
    m = m.to(DEV).eval()
    assert m.engine_conv_precision == "fp32"
    scans, poses, samples = _small_sequence(4, seed=30)
    outs = _run(streaming.StreamRunner(m, DEV, vote="instance", conv_precision="bf16"), scans, poses, samples)
    assert m._engine.conv_precision == "bf16" and m._engine.conv_precision_stats()["fallback"] == 0
    assert all(torch.isfinite(p).all() for p, _, _ in outs)


def test_multi_stream_runner_in_bf16(model):
    """as test_gpu_e2e's concurrent-streams test, in bf16: two sequences in one batch give each stream its solo labels"""
    seqs = [_small_sequence(3, seed=50 * q) for q in range(2)]
    try:
        solo = []
        for scans, poses, samples in seqs:
            r = streaming.StreamRunner(model, DEV, vote=False, skip_padding=False, conv_precision="bf16")
            solo.append(_run(r, scans, poses, samples))
        ms = streaming.MultiStreamRunner(model, DEV, n_streams=2, vote=False, conv_precision="bf16")
        up = streaming.StreamRunner(model, DEV, vote=False)
        for i in range(3):
            batched = ms.batch_inputs([up.upload(seqs[q][2][i], seqs[q][0][i]) for q in range(2)])
            pred, outs = ms.step(batched, [seqs[q][1][i] for q in range(2)])
            for q in range(2):
                want_pred, want_raw, _ = solo[q][i]
                err = (pred[4 * q:4 * q + 4] - want_pred).abs().max().item() / want_pred.abs().max().item()
                flips = int((outs[q]["raw_labels"] != want_raw).sum().item())
                assert err <= 1e-5 and flips == 0, (i, q, err, flips)
    finally:
        model.engine_conv_precision = "fp32"


def _write_sequence(root, n):
    from streammos_amd import kitti
    seq = os.path.join(root, "sequences", "08")
    os.makedirs(os.path.join(seq, "velodyne"))
    for k in range(n):
        synth.synthetic_scan(k, 16, 120).tofile(os.path.join(seq, "velodyne", "%06d.bin" % k))
    kitti.write_poses(os.path.join(seq, "poses.txt"), [synth.synthetic_pose(k) for k in range(n)])
    kitti.write_calibration(os.path.join(seq, "calib.txt"))
    return seq


def test_run_sequence_conv_precision_cli(tmp_path):
    """run_sequence --conv-precision bf16 writes the same files (names, sizes, formats) as the fp32 run"""
    seq = _write_sequence(str(tmp_path), 3)
    files = {}
    for prec in ("fp32", "bf16"):
        out = str(tmp_path / ("out_" + prec))
        cmd = [sys.executable, "-m", "streammos_amd.run_sequence", "--seq-dir", seq, "--out-dir", out, "--frame-point-num", "4096",
               "--conv-precision", prec]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        json.loads(r.stdout.strip().splitlines()[-1])
        files[prec] = {os.path.relpath(os.path.join(d, f), out): os.path.getsize(os.path.join(d, f))
                       for d, _, fs in os.walk(out) for f in fs}
    assert files["fp32"] and files["fp32"] == files["bf16"]


# ---- accuracy report: bf16 against fp32 ------------------------------------------------------------------------------

def _report(tag, i, a, b):
    """a, b: logits [B, C, N, 1]; points whose logits are all zero in fp32 (the skipped padding tail) are left out"""
    live = (b != 0).any(1)
    a, b = a.movedim(1, -1)[live], b.movedim(1, -1)[live]          # [points, C]
    rng = (b.max() - b.min()).item()
    d = (a - b).abs() / rng
    agree = (a.argmax(1) == b.argmax(1)).float().mean().item()
    print("%s frame %d: logit error mean %.2e max %.2e of the range, label agreement %.5f" % (tag, i, d.mean().item(), d.max().item(), agree))
    return d.mean().item(), agree


def test_accuracy_report_bf16_vs_fp32(model):
    """a sanity bar, not a claim about real data: the golden e2e frames and 8 chained full-size synthetic frames
    (N = 160 000, B = 4 TTA, voting on) in bf16 against fp32, the recurrent memory chained in each mode"""
    import bench
    frames = list(cases.e2e_frames(3))
    try:
        ref = _infer_frames(model, frames)
        model.engine_conv_precision = "bf16"
        got = _infer_frames(model, frames)
    finally:
        model.engine_conv_precision = "fp32"
    for i, (a, b) in enumerate(zip(got, ref)):
        mean, agree = _report("golden e2e", i, a, b)
        assert agree >= 0.98 and mean <= 1e-2, (i, mean, agree)
    seq = bench.make_frames(8, seq_seed=7)
    res = {}
    try:
        for prec in ("fp32", "bf16"):
            r = streaming.StreamRunner(model, DEV, vote=True, conv_precision=prec)
            outs = []
            for sample, raw, pose in seq:
                o = r.step(r.upload(sample, raw), pose)
                outs.append((o["pred_cls"].clone(), o["raw_labels"].clone(), len(raw)))
            torch.cuda.synchronize()
            res[prec] = outs
            del r
    finally:
        model.engine_conv_precision = "fp32"
    for i, ((p16, r16, n), (p32, r32, _)) in enumerate(zip(res["bf16"], res["fp32"])):
        mean, agree = _report("full-size", i, p16, p32)
        raw_agree = (r16 == r32).float().mean().item()
        print("full-size frame %d: raw-scan label agreement %.5f (%d points)" % (i, raw_agree, n))
        # the flipped points: their fp32 margin (best minus second-best logit) as a fraction of the logit range
        live = (p32 != 0).any(1)
        a32, a16 = p32.movedim(1, -1)[live], p16.movedim(1, -1)[live]
        flip = a32.argmax(1) != a16.argmax(1)
        if flip.any():
            top = a32[flip].topk(2, dim=1).values
            margin = (top[:, 0] - top[:, 1]) / (a32.max() - a32.min())
            print("full-size frame %d: %d flipped TTA labels, fp32 margins %.1e .. %.1e of the range" % (
                i, int(flip.sum()), margin.min().item(), margin.max().item()))
        assert agree >= 0.98 and raw_agree >= 0.98 and mean <= 1e-2, (i, mean, agree, raw_agree)

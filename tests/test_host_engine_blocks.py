"""The engine's block records on the host: the three block classes built from tiny CPU modules (folded weights against an
independent float64 fold, memory format, declared fields) and the table of A/B switches.  No GPU, no HIP library."""
import numpy as np
import pytest
import torch

from streammos_amd import engine
from streammos_amd.refapi.networks import backbone
from streammos_amd.refapi.networks import multi_view_encoder as mve


def _randomise(module, seed):
    """Random eval statistics and affine parameters for every BatchNorm, random conv weights (seeded)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen))
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) + 0.25)
                m.weight.copy_(torch.randn(m.num_features, generator=gen))
                m.bias.copy_(torch.randn(m.num_features, generator=gen))
            elif isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=gen))
    return module.eval()


def _fold64(conv, bn):
    """conv (no bias) followed by eval BatchNorm as (w', b'), in numpy float64, each rounded once to float32."""
    w = conv.weight.detach().numpy().astype(np.float64)
    s = bn.weight.detach().numpy().astype(np.float64) / np.sqrt(bn.running_var.numpy().astype(np.float64) + bn.eps)
    b = bn.bias.detach().numpy().astype(np.float64) - bn.running_mean.numpy().astype(np.float64) * s
    return (w * s[:, None, None, None]).astype(np.float32), b.astype(np.float32)


def _same(t, a):
    return t.dtype == torch.float32 and tuple(t.shape) == a.shape and np.array_equal(t.numpy(), a)


def _public(p):
    return {k for k in type(p).__slots__ if hasattr(p, k)}


def _build(module, seed):
    eng = engine.InferenceEngine.__new__(engine.InferenceEngine)            # _block alone: no network, no GPU
    m = _randomise(module, seed)
    return m, eng._block(m)


def _check_weights(p, names):
    for k in names:
        w = getattr(p, k)
        assert w.dim() == 4 and (w.shape[1] == 1 or w.stride(1) == 1), (k, w.stride())     # channels-last
        assert w.is_contiguous(memory_format=torch.channels_last), k


def test_down_block():
    m, p = _build(backbone.DownSample2D(8, 16, stride=2), 1)
    assert type(p) is engine.DownBlock and p.kind == "down" and p.stride == 2
    assert {"wa", "wp", "bias", "stride"} <= _public(p)
    _check_weights(p, ("wa", "wp"))
    wa, ba = _fold64(m.conv_branch[0], m.conv_branch[1])
    wp, bp = _fold64(m.pool_branch[0], m.pool_branch[1])
    assert _same(p.wa, wa) and _same(p.wp, wp)
    assert _same(p.bias, ba + bp)                       # both branches' biases, summed in float32 behind the max pool
    assert p.pool_pack is None                          # made by the first fused launch
    with pytest.raises(AttributeError):
        p.plan = None                                   # not a field of this class


def test_unbalance_block():
    m, p = _build(mve.Unbalance_BasicBlock(16, kernel_size=(7, 3), padding=(3, 1)), 2)
    assert type(p) is engine.UnbalanceBlock and p.kind == "unbalance"
    assert {"wa", "ba", "pa", "wb", "bb", "pb", "wc", "bc"} <= _public(p)
    assert tuple(p.pa) == (3, 1) and tuple(p.pb) == (1, 3)
    assert tuple(p.wa.shape) == (16, 16, 7, 3) and tuple(p.wb.shape) == (16, 16, 3, 7) and tuple(p.wc.shape) == (16, 32, 3, 3)
    _check_weights(p, ("wa", "wb", "wc"))
    for (wk, bk), seq in ((("wa", "ba"), m.layer7x3), (("wb", "bb"), m.layer3x7), (("wc", "bc"), m.layer3x3)):
        w, b = _fold64(seq[0], seq[1])
        assert _same(getattr(p, wk), w) and _same(getattr(p, bk), b), wk
    assert p.plan is None                               # made by the first block call
    with pytest.raises(AttributeError):
        p.ws = {}


@pytest.mark.parametrize("use_att", [False, True])
def test_basic_block(use_att):
    m, p = _build(backbone.BasicBlock(16, use_att=use_att), 3)
    assert type(p) is engine.BasicBlock and p.kind == "basic" and p.att is use_att
    assert {"w1", "b1", "w2", "b2", "att", "cw1", "cb1", "cw2", "cb2"} <= _public(p)
    _check_weights(p, ("w1", "w2"))
    for (wk, bk), (conv, bn) in ((("w1", "b1"), (m.layer[0], m.layer[1])), (("w2", "b2"), (m.layer[3], m.layer[4]))):
        w, b = _fold64(conv, bn)
        assert _same(getattr(p, wk), w) and _same(getattr(p, bk), b), wk
    if use_att:
        c1, c2 = m.channel_att.cnet[1], m.channel_att.cnet[3]
        assert _same(p.cw1, c1.weight.detach().numpy().reshape(4, 16)) and _same(p.cb1, c1.bias.detach().numpy())
        assert _same(p.cw2, c2.weight.detach().numpy().reshape(16, 4)) and _same(p.cb2, c2.bias.detach().numpy())
        assert p.cw1.is_contiguous() and p.cw2.is_contiguous()
    else:
        assert p.cw1 is None and p.cb1 is None and p.cw2 is None and p.cb2 is None
    assert p.plan is None                               # made by the first block call
    assert type(p.tag) is int if use_att else p.tag is None     # a gated block's slot in the engine's scratch table
    with pytest.raises(AttributeError):
        p.wq = None


def test_an_unexpected_module_is_an_error():
    eng = engine.InferenceEngine.__new__(engine.InferenceEngine)
    with pytest.raises(RuntimeError, match="unexpected module"):
        eng._block(torch.nn.ReLU())


# every switch attribute the engine read from the environment before there was a table: (attribute, variable, default)
_SWITCHES = [
    ("sparse_stem", "SMOS_SPARSE_STEM", True), ("tfusion", "SMOS_TFUSION", True), ("upconv", "SMOS_UPCONV", True),
    ("fused_head", "SMOS_FUSED_HEAD", True), ("head_gather", "SMOS_HEAD_GATHER", True), ("own_conv", "SMOS_OWN_CONV", True),
    ("conv_rows_mt", "SMOS_CONV_ROWS_MT", 1), ("conv_rows", "SMOS_CONV_ROWS", 3), ("fused_gate_sums", "SMOS_GATE_SUMS", True),
    ("wino", "SMOS_WINO", True), ("wino1d", "SMOS_WINO1D", True), ("pool_fused", "SMOS_POOL_FUSED", True),
    ("block_call", "SMOS_BLOCK_CALL", True),
]


def test_switch_table_lists_every_switch():
    assert sorted((a, v, d) for a, v, d, _ in engine.SWITCHES) == sorted(_SWITCHES)
    for attr, _, default, kind in engine.SWITCHES:
        assert kind == ("int" if attr in ("conv_rows", "conv_rows_mt") else "bool"), attr
        assert type(default) is (int if kind == "int" else bool), attr

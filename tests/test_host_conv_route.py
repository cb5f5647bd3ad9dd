"""Which kernel and which tile width a conv layer of the channels-last engine gets (ops.conv_route), pinned as literals
that were worked out by hand from the engine's routing rules, and the per-weight operand cache (ops.ConvLayer)."""
import pytest
import torch

from streammos_amd import ops

B = 4
LAYERS = [  # name, cin, cout, (kh, kw), stride, (h, w) of the input: the 19 conv shapes of the network (tools/ubench_conv.py)
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
# the layers that take a residual in the network: the second conv of a BasicBlock, the 2c -> c conv of an Unbalance block
WITH_RESIDUAL = ("hdr_bev 3x3 32", "hdr_bev 64->32", "hdr_rv 3x3 32", "res1 128->64", "res1 3x3 64", "res1_rv 3x3 64", "res2 3x3 128")

W2, D2 = ("wino", 2), ("wino1d", 2)
R1, R2 = ("rows", 1), ("rows", 2)
G1, G2, G4 = ("igemm", 1), ("igemm", 2), ("igemm", 4)

# Expected routes in LAYERS order.  By hand: wave tiles = ceil(B * Ho * Wo / 32) * Cout / (32 * mt) must reach 2048 for the widest
# mt in (4, 2, 1) -- (2, 1) with a residual -- that divides Cout / 32, else mt = 1; Winograd where the kernel is 3x3 / stride 1,
# 1-D Winograd for 5x3 / 7x3 / 3x5 / 3x7, row staging for stride 1 with KW >= conv_rows at mt <= conv_rows_mt, else igemm.
# In this network no layer's mt changes with its residual, so one row serves both.
#                                      bev3x3 7x3 3x7 64>32 rv3x3 rv1x1 d3x3s2 d1x1 5x3 3x5 128>64 3x3_64 rv3x3 rv1x1 d3x3s2 d1x1 3x3_128 c1a c2
DEFAULT = [W2, D2, D2, W2, W2, G1, G2, G2, D2, D2, W2, W2, W2, G1, G1, G4, W2, W2, W2]
ROUTES = {
    "default": (ops.ConvSwitches(), DEFAULT),
    "rows 0": (ops.ConvSwitches(conv_rows=0), DEFAULT),            # with both Winograd kernels on, only 1x1 and stride-2 layers are left
    "rows 5": (ops.ConvSwitches(conv_rows=5), DEFAULT),
    "rows_mt 2": (ops.ConvSwitches(conv_rows_mt=2), DEFAULT),
    "wino off": (ops.ConvSwitches(wino=False),
                 [R1, D2, D2, R1, R1, G1, G2, G2, D2, D2, G2, G2, R1, G1, G1, G4, R1, G4, G2]),
    "wino off, rows_mt 2": (ops.ConvSwitches(wino=False, conv_rows_mt=2),
                            [R1, D2, D2, R1, R1, G1, G2, G2, D2, D2, R2, R2, R1, G1, G1, G4, R1, G4, R2]),
    "wino off, rows 5": (ops.ConvSwitches(wino=False, conv_rows=5),
                         [G1, D2, D2, G1, G1, G1, G2, G2, D2, D2, G2, G2, G1, G1, G1, G4, G1, G4, G2]),
    "wino1d off": (ops.ConvSwitches(wino1d=False),
                   [W2, R1, R1, W2, W2, G1, G2, G2, G2, G2, W2, W2, W2, G1, G1, G4, W2, W2, W2]),
    "wino1d off, rows 5": (ops.ConvSwitches(wino1d=False, conv_rows=5),
                           [W2, G1, R1, W2, W2, G1, G2, G2, G2, G2, W2, W2, W2, G1, G1, G4, W2, W2, W2]),
    "wino1d off, rows_mt 2": (ops.ConvSwitches(wino1d=False, conv_rows_mt=2),
                              [W2, R1, R1, W2, W2, G1, G2, G2, R2, R2, W2, W2, W2, G1, G1, G4, W2, W2, W2]),
    "all off": (ops.ConvSwitches(wino=False, wino1d=False, conv_rows=0),
                [G1, G1, G1, G1, G1, G1, G2, G2, G2, G2, G2, G2, G1, G1, G1, G4, G1, G4, G2]),
}


def _route(layer, switches, residual=False, sums=False):
    name, cin, cout, (kh, kw), stride, (h, w) = layer
    ho, wo = (h + 2 * (kh // 2) - kh) // stride + 1, (w + 2 * (kw // 2) - kw) // stride + 1
    return ops.conv_route(cin, cout, (kh, kw), stride, B * ho * wo, residual, sums, switches)


@pytest.fixture(autouse=True)
def _default_tuning(monkeypatch):
    monkeypatch.setattr(ops, "_CONV_MIN_WAVE_TILES", 2048)       # the table is for the shipped value of the tuning knob


@pytest.mark.parametrize("setting", sorted(ROUTES))
def test_routing_table(setting):
    switches, want = ROUTES[setting]
    assert len(want) == len(LAYERS) == 19
    for layer, route in zip(LAYERS, want):
        assert _route(layer, switches) == route, (setting, layer[0])
        if layer[0] in WITH_RESIDUAL:
            assert _route(layer, switches, residual=True) == route, (setting, layer[0], "+res")


def test_residual_and_channel_sums_change_the_route_where_the_kernels_differ():
    by_name = {layer[0]: layer for layer in LAYERS}
    off = ops.ConvSwitches(wino=False)
    # a residual tile is held in registers: mt <= 2 (the network has no such layer; 8192 pixel tiles x 2 channel tiles)
    assert _route(by_name["conv_1a 64->128"], off) == G4
    assert _route(by_name["conv_1a 64->128"], off, residual=True) == G2
    assert _route(by_name["conv_1a 64->128"], ops.ConvSwitches(wino=False, conv_rows_mt=2), residual=True) == R2
    assert _route(by_name["res2 down 1x1"], ops.ConvSwitches(), residual=True) == G2
    # the 1-D Winograd kernel has neither a residual input nor channel sums; the others have both
    for kw in ({"residual": True}, {"sums": True}):
        assert _route(by_name["hdr_bev 7x3"], ops.ConvSwitches(), **kw) == R1
        assert _route(by_name["res1 3x5"], ops.ConvSwitches(), **kw) == G2
    assert _route(by_name["hdr_bev 3x3 32"], ops.ConvSwitches(), sums=True) == W2
    assert _route(by_name["hdr_bev 3x3 32"], off, sums=True) == R1
    assert _route(by_name["res1 3x3 64"], off, sums=True) == G2


def test_route_reads_the_switches_of_whatever_carries_them():
    class Engine:                                                # InferenceEngine passes itself
        wino, wino1d, conv_rows, conv_rows_mt = True, True, 3, 1
    eng = Engine()
    assert _route(LAYERS[0], eng) == W2
    eng.wino = False
    assert _route(LAYERS[0], eng) == R1


def test_conv_layer_packs_each_operand_once():
    g = torch.Generator().manual_seed(3)
    w3 = torch.randn(64, 64, 3, 3, generator=g)        # two 32-channel chunks: the "rows" stage order differs from "igemm"
    w7 = torch.randn(32, 32, 7, 3, generator=g)
    layer = ops.ConvLayer(w3)
    assert layer.w is w3 and layer.ran_bf16 is None
    want = {("wino", 2): ops.conv_wino_prepare(w3, 2), ("wino", 1): ops.conv_wino_prepare(w3, 1),
            ("igemm", 1): ops.conv_prepare(w3, 1), ("igemm", 2): ops.conv_prepare(w3, 2),
            ("rows", 1): ops.conv_prepare(w3, 1, order="rows"), ("rows", 2): ops.conv_prepare(w3, 2, order="rows"),
            "bf16": ops.conv_bf16_prepare(w3)}
    got = {key: layer.operand(key) for key in want}
    for key in want:
        assert layer.operand(key) is got[key], key                 # asked twice: the same tensor object
        assert got[key].dtype == want[key].dtype and torch.equal(got[key], want[key]), key
    assert len({t.data_ptr() for t in got.values()}) == len(want)  # every key its own block
    assert not torch.equal(got[("igemm", 1)], got[("rows", 1)]) and not torch.equal(got[("igemm", 1)], got[("igemm", 2)])
    assert set(layer.packed) == set(want)
    long = ops.ConvLayer(w7)
    assert torch.equal(long.operand(("wino1d", 2)), ops.conv_wino1d_prepare(w7, 2))
    assert long.operand(("wino1d", 2)) is long.operand(("wino1d", 2))


def test_engine_keeps_one_layer_per_weight_tensor():
    """Keyed by id(w) and holding w: two live weights never share a layer, also where they are equal or views of one storage
    (an address-keyed cache cannot tell those apart)."""
    from streammos_amd import engine
    eng = engine.InferenceEngine.__new__(engine.InferenceEngine)           # the layer table alone: no network, no GPU
    eng._conv_layers = {}
    base = torch.randn(32, 64, 3, 3, generator=torch.Generator().manual_seed(4))
    a, b, view = base[:, :32], base[:, :32].clone(), base[:, :32]
    assert a.data_ptr() == view.data_ptr()
    la, lb, lv = eng._conv_layer(a), eng._conv_layer(b), eng._conv_layer(view)
    assert la is not lb and la is not lv and lb is not lv
    assert eng._conv_layer(a) is la and eng._conv_layer(b) is lb and eng._conv_layer(view) is lv
    assert la.w is a and lb.w is b and lv.w is view and len(eng._conv_layers) == 3
    assert la.operand(("wino", 2)) is not lv.operand(("wino", 2))
    assert eng.conv_precision_stats() == {"bf16": 0, "fallback": 0}       # nothing launched in bf16 mode
    la.ran_bf16, lb.ran_bf16 = True, False
    assert eng.conv_precision_stats() == {"bf16": 1, "fallback": 1}

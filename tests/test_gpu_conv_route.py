"""InferenceEngine._conv against the direct call of the kernel ops.conv_route names, bit for bit, with the launch's profiling
label and family; and the replay closure of each of the five conv wrappers.  B = 1, 32 -> 32 channels, 9 x 33 pixels: every
kernel has a partial row block and a partial 32-column tile."""
import pytest
import torch

from streammos_amd import engine as engine_mod, ops, profiling
from tests.test_gpu_e2e import model  # noqa: F401 -- the module-scoped AttNet fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, C, H, W = 1, 32, 9, 33


def _inputs(kernel, stride, seed):
    g = torch.Generator().manual_seed(seed)
    kh, kw = kernel
    x = torch.randn((B, H, W, C), generator=g).to(DEV).permute(0, 3, 1, 2)
    w = (torch.randn((C, C, kh, kw), generator=g) * 0.1).to(DEV).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(C, generator=g).to(DEV)
    ho, wo = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
    res = torch.randn((B, ho, wo, C), generator=g).to(DEV).permute(0, 3, 1, 2)
    return x, w, bias, res, ho, wo


def _direct(x, w, route, bias, act, kernel, stride, residual, sums):
    if route == "bf16":
        return ops.conv_bf16_cl(x, ops.conv_bf16_prepare(w), bias, act, C, kernel, stride=stride, residual=residual, chan_sums=sums)
    family, tile = route
    if family == "wino":
        return ops.conv_wino_cl(x, ops.conv_wino_prepare(w, tile), bias, act, C, mb=tile, residual=residual, chan_sums=sums)
    if family == "wino1d":
        return ops.conv_wino1d_cl(x, ops.conv_wino1d_prepare(w, tile), bias, act, C, kernel, mb=tile)
    if family == "rows":
        return ops.conv_rows_cl(x, ops.conv_prepare(w, tile, order="rows"), bias, act, C, kernel, mt=tile, residual=residual,
                                chan_sums=sums)
    return ops.conv_cl(x, ops.conv_prepare(w, tile), bias, act, C, kernel, stride=stride, mt=tile, residual=residual, chan_sums=sums)


def _sum_table(route, ho, wo):
    chunks = ops.conv_wino_sum_chunks(ho, wo) if route != "bf16" and route[0] == "wino" else ops.conv_sum_chunks(ho, wo)
    return torch.zeros((B, chunks, C), device=DEV)


def _check(eng, kernel, stride, route, extra, seed):
    """eng._conv on the hot path and under a kernel timer against the direct call; returns the weight"""
    x, w, bias, res, ho, wo = _inputs(kernel, stride, seed)
    residual = res if extra == "res" else None
    act = ops.ACT_NONE if extra == "sums" else ops.ACT_RELU
    if route != "bf16":
        assert ops.conv_route(C, C, kernel, stride, B * ho * wo, residual is not None, extra == "sums", eng) == route
    sums = [_sum_table(route, ho, wo) if extra == "sums" else None for _ in range(3)]
    want = _direct(x, w, route, bias, act, kernel, stride, residual, sums[0])
    assert tuple(want.shape) == (B, C, ho, wo) and bool(torch.isfinite(want).all()) and want.abs().max().item() > 0
    hot = eng._conv(x, w, bias, act, stride=stride, residual=residual, chan_sums=sums[1])
    with profiling.kernel_timer() as kt:
        timed = eng._conv(x, w, bias, act, stride=stride, residual=residual, chan_sums=sums[2])
    assert torch.equal(hot, want) and torch.equal(timed, want)
    if extra == "sums":
        assert sums[0].abs().max().item() > 0 and torch.equal(sums[1], sums[0]) and torch.equal(sums[2], sums[0])
    family = "conv_bf16" if route == "bf16" else "conv_" + route[0]
    label = "%s[%dx%dx%dx%d->%dx%dx%dk%dx%d%s]" % (("conv_bf16" if route == "bf16" else "conv_cl", B, C, H, W, C, ho, wo) + kernel +
                                                   ("+res" if residual is not None else "",))
    assert kt.sequence == [label] and kt.family == {label: family}
    return w


CASES = [  # kernel, stride, the route, "res" / "sums" / None
    ((1, 1), 1, ("igemm", 1), None), ((3, 3), 2, ("igemm", 1), None), ((3, 3), 1, ("wino", 2), None),
    ((7, 3), 1, ("wino1d", 2), None), ((3, 5), 1, ("wino1d", 2), None),
    ((3, 3), 1, ("wino", 2), "res"), ((3, 3), 1, ("wino", 2), "sums"),
    ((3, 3), 2, ("igemm", 1), "res"), ((1, 1), 1, ("igemm", 1), "sums"),
]


@pytest.fixture(scope="module")
def eng(model):  # noqa: F811
    model.fast_inference, model.engine_layout = True, "cl"
    with torch.no_grad():
        e = model._engine_for(torch.zeros(1, device=DEV))
    assert e is not None and e.layout == "cl" and e.conv_precision == "fp32" and e.own_conv and e.wino and e.wino1d
    return e


@pytest.mark.parametrize("kernel,stride,route,extra", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_engine_conv_equals_direct_call(eng, kernel, stride, route, extra):
    before = len(eng._conv_layers)
    w = _check(eng, kernel, stride, route, extra, seed=11)
    layer = eng._conv_layers[id(w)]
    assert len(eng._conv_layers) == before + 1 and layer.w is w and list(layer.packed) == [route] and layer.ran_bf16 is None
    assert eng.conv_precision_stats() == {"bf16": 0, "fallback": 0}


@pytest.mark.parametrize("extra", [None, "res", "sums"])
def test_switch_flipped_on_a_live_engine_reroutes_the_same_weight(eng, extra):
    """wino off: the stride-1 3x3 layer goes to the row-staging kernel, and back -- the route is not cached per weight."""
    try:
        eng.wino = False
        w = _check(eng, (3, 3), 1, ("rows", 1), extra, seed=12)
    finally:
        eng.wino = True
    x, _, bias, res, ho, wo = _inputs((3, 3), 1, 12)
    with profiling.kernel_timer() as kt:
        y = eng._conv(x, w, bias, ops.ACT_RELU)
    assert list(kt.family.values()) == ["conv_wino"]
    assert torch.equal(y, ops.conv_wino_cl(x, ops.conv_wino_prepare(w, 2), bias, ops.ACT_RELU, C))
    assert set(eng._conv_layers[id(w)].packed) == {("rows", 1), ("wino", 2)}


@pytest.fixture(scope="module")
def eng16(model):  # noqa: F811
    return engine_mod.InferenceEngine(model, conv_precision="bf16")


@pytest.mark.parametrize("extra", [None, "res", "sums"])
def test_bf16_engine_routes_to_the_bf16_kernel(eng16, extra):
    w = _check(eng16, (3, 3), 1, "bf16", extra, seed=13)
    assert list(eng16._conv_layers[id(w)].packed) == ["bf16"] and eng16._conv_layers[id(w)].ran_bf16 is True
    assert eng16.conv_precision_stats() == {"bf16": len(eng16._conv_layers), "fallback": 0}


def _replay_cases():
    k3, k7 = (3, 3), (7, 3)
    return {
        "conv_igemm": (k3, lambda x, w, b, out: ops.conv_cl(x, ops.conv_prepare(w, 1), b, 1, C, k3, out=out)),
        "conv_rows": (k3, lambda x, w, b, out: ops.conv_rows_cl(x, ops.conv_prepare(w, 1, order="rows"), b, 1, C, k3, out=out)),
        "conv_wino": (k3, lambda x, w, b, out: ops.conv_wino_cl(x, ops.conv_wino_prepare(w, 2), b, 1, C, out=out)),
        "conv_wino1d": (k7, lambda x, w, b, out: ops.conv_wino1d_cl(x, ops.conv_wino1d_prepare(w, 2), b, 1, C, k7, out=out)),
        "conv_bf16": (k3, lambda x, w, b, out: ops.conv_bf16_cl(x, ops.conv_bf16_prepare(w), b, 1, C, k3, out=out)),
    }


@pytest.mark.parametrize("family", sorted(_replay_cases()))
def test_requested_replay_reproduces_the_launch(family):
    kernel, launch = _replay_cases()[family]
    x, w, bias, _, ho, wo = _inputs(kernel, 1, 14)
    label = "%s[%dx%dx%dx%d->%dx%dx%dk%dx%d]" % (("conv_bf16" if family == "conv_bf16" else "conv_cl", B, C, H, W, C, ho, wo) + kernel)
    out = ops.empty_cl(B, C, ho, wo, DEV)
    profiling.request_replay(label)
    try:
        assert profiling.enabled()
        assert launch(x, w, bias, out) is out
        assert not profiling.enabled()                  # the offer was taken: the request is spent
        again = profiling.replay_of(label)
        assert again is not None
        want = out.clone()
        assert bool(torch.isfinite(want).all()) and want.abs().max().item() > 0
        out.fill_(float("nan"))
        with profiling.kernel_timer() as kt:
            again()
        assert torch.equal(out, want)
        assert kt.sequence == [label] and kt.family == {label: family}
        # a launch nobody asked for offers nothing
        profiling._replay.pop(label, None)
        launch(x, w, bias, out)
        assert profiling.replay_of(label) is None
    finally:
        profiling._replay_label = None
        profiling._replay.pop(label, None)

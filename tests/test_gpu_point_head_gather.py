"""The point head that gathers the decoder's BEV rows itself (smos_point_head_gather, csrc/point_head.hip) against the
two launches it replaces, against float64, and inside the engine; and the layer-1 operand order both forms share."""
import pytest
import torch

from streammos_amd import ops

DEV = "cuda:0"
B, N, HG, WG = 2, 70, 5, 7                  # three 32-point tiles per sample, the last one ragged
SCALE = (0.5, 0.5)
N_LIVE = (0, 1, 45, 64, 70, None)


def _weights(gen, m3=3, dev=DEV):
    l1 = ((torch.randn((96, 192, 1, 1), generator=gen) * 0.1).to(dev), (torch.randn(96, generator=gen) * 0.2).to(dev))
    l2 = ((torch.randn((64, 96, 1, 1), generator=gen) * 0.15).to(dev), (torch.randn(64, generator=gen) * 0.2).to(dev))
    l3 = ((torch.randn((m3, 64, 1, 1), generator=gen) * 0.2).to(dev), torch.randn(m3, generator=gen).to(dev))
    return l1, l2, l3


def _coords(gen):
    """[B, N, 2] (row, column) coordinates; position = coordinate * 0.5.  Interior points, exactly integer positions, the last
    row and column, just outside (-0.5 and size - 0.5: one row / column of taps absent), further outside (all taps absent) and
    the padding value of a scan's tail."""
    c = torch.rand((B, N, 2), generator=gen) * torch.tensor([2.0 * (HG - 1), 2.0 * (WG - 1)])
    special = torch.tensor([[0.0, 0.0], [2.0, 4.0], [4.0, 6.0],                                  # integer positions
                            [2.0 * (HG - 1), 3.3], [1.7, 2.0 * (WG - 1)], [2.0 * (HG - 1), 2.0 * (WG - 1)],
                            [-1.0, 3.0], [3.0, -1.0], [2.0 * HG - 1.0, 5.0], [5.0, 2.0 * WG - 1.0], [-1.0, 2.0 * WG - 1.0],
                            [-2.5, 3.0], [3.0, 2.0 * WG + 0.5], [-1000.0, -1000.0]])
    c[0, 3:3 + len(special)] = special
    c[1, 40:40 + len(special)] = special
    c[:, 66:] = -1000.0                                                                            # a padding tail
    assert torch.isfinite(c).all()
    return c


@pytest.fixture(scope="module")
def case():
    gen = torch.Generator(device="cpu").manual_seed(77)
    rows = torch.randn((B, N, 192), generator=gen).to(DEV)
    grid_wide = torch.randn((B, HG, WG, 96), generator=gen).to(DEV)
    coords = _coords(gen)
    l1, l2, l3 = _weights(gen)
    wprep, m3 = ops.point_head_prepare(l1, l2, l3)
    pcds = torch.zeros((B, 3, N, 3, 1))
    pcds[:, 0, :, :2, 0] = coords
    pcds[:, 1:] = 7.0
    return {"rows": rows, "grid_wide": grid_wide, "coords": coords.to(DEV), "pcds": pcds.to(DEV), "layers": (l1, l2, l3),
            "wprep": wprep, "m3": m3}


def _grid(case, layout):
    if layout == "slice":                      # 64 channels of a 96-channel buffer: pixel pitch 96, 64-byte channel offset
        return case["grid_wide"].permute(0, 3, 1, 2)[:, 16:80]
    return case["grid_wide"][..., 16:80].contiguous().permute(0, 3, 1, 2)


def _coord_view(case, layout):
    return case["pcds"][:, 0, :, :2, 0] if layout == "strided" else case["coords"]


@pytest.mark.gpu
@pytest.mark.parametrize("grid_layout,coord_layout", [("dense", "dense"), ("slice", "dense"), ("dense", "strided"), ("slice", "strided")])
def test_fold_equals_gather_then_head_bit_for_bit(case, grid_layout, coord_layout):
    """Same position arithmetic, same tap sum, same K walk: the one launch equals gather_scatter_cl(pts_out=...) followed by
    point_head on every point below n_live, and writes exact zeros above it.  The fold's rows carry NaN in the BEV third:
    nobody reads it."""
    grid, coord = _grid(case, grid_layout), _coord_view(case, coord_layout)
    pair_rows = case["rows"].clone()
    ops.gather_scatter_cl(grid, coord, SCALE, pts_out=pair_rows[:, :, 64:128])
    fold_rows = case["rows"].clone()
    fold_rows[:, :, 64:128] = float("nan")
    for n_live in N_LIVE:
        live = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=DEV)
        nl = N if n_live is None else n_live
        want = ops.point_head(pair_rows, case["wprep"], case["m3"], n_live=live)
        got = ops.point_head(fold_rows, case["wprep"], case["m3"], n_live=live, gather=(grid, coord, SCALE))
        assert got.shape == want.shape == (B, case["m3"], N)
        assert torch.equal(got[:, :, :nl], want[:, :, :nl]), n_live
        assert (got[:, :, nl:] == 0).all() and (want[:, :, nl:] == 0).all(), n_live
    assert torch.isnan(fold_rows[:, :, 64:128]).all()                 # and nobody wrote it


def _bilinear_f64(grid, coord, scale):
    """BilinearSample with zeros padding: the float32 positions of grid_sample's normalise / un-normalise round trip
    (networks/backbone.py:453-475), the four taps and their sum in float64.  grid [B, C, H, W] -> [B, N, C]."""
    b, c, h, w = grid.shape
    g = grid.permute(0, 2, 3, 1).double()
    out = torch.zeros((b, coord.shape[1], c), dtype=torch.float64, device=grid.device)
    pos = []
    for d, size in ((0, h), (1, w)):
        x = coord[..., d].float()
        gn = (2.0 * x) * scale[d] / float(size - 1) - 1.0
        pos.append((((gn + 1.0) / 2.0) * float(size - 1)).double())
    y0, x0 = torch.floor(pos[0]), torch.floor(pos[1])
    bi = torch.arange(b, device=grid.device)[:, None].expand(b, coord.shape[1])
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = y0 + dy, x0 + dx
            wgt = (1.0 - (pos[0] - yy).abs()) * (1.0 - (pos[1] - xx).abs())
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            v = g[bi, yy.clamp(0, h - 1).long(), xx.clamp(0, w - 1).long()]
            out += torch.where(ok, wgt, torch.zeros_like(wgt))[..., None] * v
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("grid_layout,coord_layout", [("dense", "dense"), ("slice", "strided")])
def test_fold_against_float64_reference(case, grid_layout, coord_layout):
    """The fold against a float64 restatement (bilinear taps in float64 from the float32 positions, then the three layers);
    the bar of test_point_head_against_float64_reference: 2e-5 of the output range."""
    grid, coord = _grid(case, grid_layout), _coord_view(case, coord_layout)
    l1, l2, l3 = case["layers"]
    m3 = case["m3"]
    rows = case["rows"]
    got = ops.point_head(rows, case["wprep"], m3, gather=(grid, coord, SCALE))
    x = torch.cat((rows[:, :, :64].double(), _bilinear_f64(grid, coord, SCALE), rows[:, :, 128:].double()), 2).reshape(B * N, 192)
    z = torch.relu(x @ l1[0].double().view(96, 192).t() + l1[1].double())
    z = torch.relu(z @ l2[0].double().view(64, 96).t() + l2[1].double())
    want = (z @ l3[0].double().view(m3, 64).t() + l3[1].double()).view(B, N, m3).permute(0, 2, 1)
    err = (got.double() - want).abs().max().item()
    print("fold vs float64: %.3e of the range" % (err / want.abs().max().item()))
    assert err <= 2e-5 * want.abs().max().item()


def test_layer1_operand_order_reproduces_w1_times_row():
    """Host only.  Lane half h of the MFMA chain streams channels point_head_k_order()[:, h] of a row; the prepared A1 block
    holds W1's columns in that order, so walking both reproduces W1 @ row.  Pins the layout the kernel and the prepare share:
    k-steps [32 t, 32 t + 32) = segment t of the row, channels [32 h, 32 h + 32) of it."""
    gen = torch.Generator(device="cpu").manual_seed(5)
    order = ops.point_head_k_order()
    assert tuple(order.shape) == (96, 2) and sorted(order.reshape(-1).tolist()) == list(range(192))
    for t in range(3):
        for h in range(2):
            assert order[32 * t:32 * t + 32, h].tolist() == list(range(64 * t + 32 * h, 64 * t + 32 * h + 32))
    w1 = (torch.arange(96 * 192, dtype=torch.float32).view(96, 192) % 251.0) - 125.0        # known, exact in float32
    l1, l2, l3 = _weights(gen, dev="cpu")
    flat, _ = ops.point_head_prepare((w1.view(96, 192, 1, 1), l1[1]), l2, l3)
    a1 = flat[:3 * 96 * 64].view(3, 96, 2, 32).double()                                       # (mt, s, h, m)
    row = torch.randn(192, generator=gen, dtype=torch.float64)
    lanes = row[order]                                                                         # [s, h]: what lane half h feeds at step s
    got = torch.einsum("tshm,sh->tm", a1, lanes).reshape(96)
    want = w1.double() @ row
    assert (got - want).abs().max().item() <= 1e-9 * want.abs().max().item()


@pytest.mark.gpu
def test_engine_with_and_without_the_fold():
    """InferenceEngine over two streamed frames with the head gathering its BEV rows (the default) and with the gather launch
    in front of it: both run the same kernels' arithmetic, logits and labels equal bit for bit.  Against the library-GEMM head
    (SMOS_FUSED_HEAD=0's path, another summation order): the engine variants' bar, 1e-5 of the range."""
    from streammos_amd import synth
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    from tests import cases
    model = StreamMOS.AttNet(cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(DEV).eval()
    model.fast_inference, model.engine_layout = True, "cl"
    frames = list(cases.e2e_frames(2))
    with torch.no_grad():
        eng = model._engine_for(torch.zeros(1, device=DEV))
    assert eng.head_gather and eng.fused_head and eng.head_w is not None        # the defaults
    calls = []
    real = ops.gather_scatter_cl

    def counting(*args, **kwargs):
        calls.append(kwargs.get("out") is None)                # True: a gather-only launch (the decoder's)
        return real(*args, **kwargs)

    outs = {}
    ops.gather_scatter_cl = counting
    try:
        for name, gather, fused in (("fold", True, True), ("pair", False, True), ("gemm", False, False)):
            eng.head_gather, eng.fused_head = gather, fused
            del calls[:]
            memory, res = None, []
            with torch.no_grad():
                for i, batch in enumerate(frames):
                    tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
                    pred, a0, a1, a2, memory = model.infer(tb, i, memory)
                    res.append(pred.clone())
            outs[name] = res
            assert sum(calls) == (0 if gather else len(frames)), (name, calls)   # the gather launch is gone / is there
    finally:
        ops.gather_scatter_cl = real
        eng.head_gather, eng.fused_head = True, True
    for fold, pair, gemm in zip(outs["fold"], outs["pair"], outs["gemm"]):
        assert torch.equal(fold, pair)
        assert torch.equal(fold.argmax(1), pair.argmax(1))
        assert (fold - gemm).abs().max().item() <= 1e-5 * gemm.abs().max().item()

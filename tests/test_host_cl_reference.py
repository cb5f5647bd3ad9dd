"""tests/cl_cases.py without a GPU: the float64 references against independent formulations (torch.nn.functional in float64), the
float32 restatements of every kernel -- in the kernel's written order and in another one -- inside the derived bounds, the exact
twins bit for bit, every mutant of a reference outside its bound four times over on its target case, and the engine's workspace
request against what the three-pass gate requires.  Run with -s for the margins and the mutant table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import cl_cases as cases

MUTANT_FACTOR = 4.0            # a mutant has to exceed the bound this many times on its target case (the tfusion tests' convention)


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _close(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(1.0, np.abs(b).max())


def _ratio(got, want, bound):
    ok, r = cases.worst_ratio(got, want, bound)
    return ok, r


def _margin(tag, worst):
    print("cl-margin %-44s worst error / bound %.4f" % (tag, worst))


def _mutant(tag, worst):
    print("cl-mutant %-44s worst error / bound %10.3g" % (tag, worst))


WIDE = [(c, k, r) for c in cases.GATE_WIDE_C for k in cases.gate_wide_chunks(c) for r in cases.gate_wide_crs(c)]
WIDE_TWINS = [(c, k) for c in cases.GATE_WIDE_C for k in cases.gate_wide_twin_chunks(c)]
RES = [(c, hw) for c in cases.GATE_RES_C for hw in cases.GATE_RES_HW]


# ---------------------------------------------------------------------------------------------
# 1. independent references
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.BIAS_ACT_CASES))
def test_bias_act_reference_equals_torch_float64(name):
    c = cases.bias_act_case(name)
    v = _t(c.x)
    if c.bias is not None:
        v = v + _t(c.bias)
    if c.res is not None:
        v = v + _t(c.res)
    want = (v, F.relu(v), F.leaky_relu(v, 0.01))[c.act].numpy()
    assert _close(c.want, want)
    if c.act == 1:
        assert 0.05 <= cases.clipped_share(c.want) <= 0.60


@pytest.mark.parametrize("name", sorted(cases.DS_CASES))
def test_downsample_reference_equals_torch_float64(name):
    c = cases.ds_case(name)
    want = _nhwc(F.relu(_nchw(c.a) + _t(c.bias).view(1, -1, 1, 1) + F.max_pool2d(_nchw(c.p), 3, c.stride, 1)))
    assert c.want.shape == want.shape == (c.b, c.ho, c.wo, c.c) and _close(c.want, want)
    assert 0.05 <= cases.clipped_share(c.want) <= 0.60
    if c.variant == "neg":
        assert (c.p <= -1.0).all()


def _torch_gate(c):
    mean = _t(c.total) / c.hw + _t(c.bias)
    pre = F.linear(F.relu(F.linear(mean, _t(c.w1), _t(c.b1))), _t(c.w2), _t(c.b2))
    return torch.sigmoid(pre).numpy(), pre.numpy()


def _check_gate_reference(c):
    g, pre = _torch_gate(c)
    assert _close(c.gate, g) and _close(c.pre, pre)
    assert np.abs(c.pre).max() <= 6.0 and (c.hidden > 0).any(1).all()
    assert _close(cases.logit(c.gate), c.pre)
    want = F.relu((_t(c.y) + _t(c.bias)) * _t(c.gate)[:, None, :] + _t(c.xres)).numpy()
    assert _close(c.want, want) and 0.05 <= cases.clipped_share(c.want) <= 0.60


@pytest.mark.parametrize("ch", cases.GATE_WIDE_C)
def test_gate_wide_references_equal_torch_float64(ch):
    for k in cases.gate_wide_chunks(ch):
        for r in cases.gate_wide_crs(ch):
            _check_gate_reference(cases.gate_wide_case(ch, k, r))
    for k in cases.gate_wide_twin_chunks(ch):
        _check_gate_reference(cases.gate_wide_case(ch, k, ch // 4, True))


@pytest.mark.parametrize("ch", cases.GATE_RES_C)
def test_gate_residual_references_equal_torch_float64(ch):
    for hw, (h, w) in cases.GATE_RES_HW.items():
        c = cases.gate_res_case(ch, h, w)
        _check_gate_reference(c)
        # the chunk table: torch sums of the 512-pixel pieces, and the mean it leads to = adaptive_avg_pool2d
        pieces = torch.stack([p.sum(1) for p in torch.split(_t(c.y), cases.PER, 1)], 1).numpy()
        assert c.table.shape == (c.b, (hw + 511) // 512, ch) and _close(c.table, pieces)
        pooled = F.adaptive_avg_pool2d(_t(c.y).view(c.b, h, w, ch).permute(0, 3, 1, 2), 1).view(c.b, ch).numpy()
        assert _close(c.table.sum(1) / hw, pooled) and _close(c.mean, pooled + c.bias)


@pytest.mark.parametrize("name", sorted(cases.UP_CASES))
def test_upsample_reference_equals_torch_float64(name):
    c = cases.up_case(name)
    want = torch.cat([F.interpolate(_nchw(v), size=(c.ho, c.wo), mode="bilinear", align_corners=True) for v in c.srcs], 1)
    assert _close(c.want, _nhwc(want))
    at = 0
    for v, (ch, size) in zip(c.srcs, c.specs):
        if size == (c.ho, c.wo):                                             # the identity: bit for bit, bound 0
            assert np.array_equal(c.want[..., at:at + ch], v) and not c.bound[..., at:at + ch].any()
        else:
            assert (c.bound[..., at:at + ch] > 0).all()
        at += ch


# ---------------------------------------------------------------------------------------------
# 2. the float32 restatements inside the bounds
# ---------------------------------------------------------------------------------------------
def test_bias_act_restatements_inside_the_bound():
    worst = 0.0
    for name in sorted(cases.BIAS_ACT_CASES):
        c = cases.bias_act_case(name)
        for order in ("kernel", "other"):
            ok, r = _ratio(cases.bias_act_ref(c.x, c.bias, c.res, c.act, np.float32, order), c.want, cases.bias_act_bound(c))
            assert ok, (name, order, r)
            worst = max(worst, r)
    _margin("bias_act", worst)


def test_downsample_restatements_inside_the_bound():
    worst = 0.0
    for name in sorted(cases.DS_CASES):
        c = cases.ds_case(name)
        for order in ("kernel", "other"):
            ok, r = _ratio(cases.ds_ref(c.a, c.p, c.bias, c.stride, np.float32, order), c.want, cases.ds_bound(c))
            assert ok, (name, order, r)
            worst = max(worst, r)
    _margin("downsample_epilogue", worst)


def _gate_restatements(c, threads, chains):
    """The gate of the table in the kernel's order and in numpy's: both inside the bound, gate and logit."""
    bg, bl = cases.gate_bound(c)
    worst = 0.0
    for total, order in ((cases.table_sum_f32(c.table, threads, chains), "kernel"),
                         (np.asarray(c.table).astype(np.float32).sum(1, dtype=np.float32), "other")):
        g, _ = cases.gate_f32(total, c.hw, c.bias, c.w1, c.b1, c.w2, c.b2, order)
        ok, r = _ratio(g, c.gate, bg)
        ok2, r2 = _ratio(cases.logit(g), c.pre, bl)
        assert ok and ok2, (c.name, order, r, r2)
        worst = max(worst, r, r2)
    return worst


@pytest.mark.parametrize("ch", cases.GATE_WIDE_C)
def test_gate_wide_restatements_inside_the_bound(ch):
    worst = 0.0
    for k in cases.gate_wide_chunks(ch):
        for r in cases.gate_wide_crs(ch):
            worst = max(worst, _gate_restatements(cases.gate_wide_case(ch, k, r), 1024, 8))
    _margin("gate_mlp_wide c%d" % ch, worst)


@pytest.mark.parametrize("ch", cases.GATE_WIDE_C)
def test_gate_wide_exact_twins(ch):
    """On the twins the table's total and the mean are float32 numbers in any order: both summation orders give the float64
    total bit for bit, the pre-sigmoid value of the restatement equals the reference's, and the gate is inside the bound that
    is left (expf, one add, one reciprocal)."""
    for k in cases.gate_wide_twin_chunks(ch):
        c = cases.gate_wide_case(ch, k, ch // 4, True)
        a, b = cases.table_sum_f32(c.table, 1024, 8), c.table.astype(np.float32).sum(1, dtype=np.float32)
        assert np.array_equal(a.astype(np.float64), c.total) and np.array_equal(b.astype(np.float64), c.total)
        mean32 = a / np.float32(c.hw) + c.bias.astype(np.float32)
        assert np.array_equal(mean32.astype(np.float64), c.mean)
        for order in ("kernel", "other"):
            g, pre = cases.gate_f32(a, c.hw, c.bias, c.w1, c.b1, c.w2, c.b2, order)
            assert np.array_equal(pre.astype(np.float64), c.pre)
            bg, bl = cases.gate_bound(c)
            assert _ratio(g, c.gate, bg)[0] and _ratio(cases.logit(g), c.pre, bl)[0]
        assert (cases.gate_bound(c)[0] < cases.gate_bound(c, exact=False)[0]).all()


@pytest.mark.parametrize("ch", cases.GATE_RES_C)
def test_gate_residual_restatements_inside_the_bound(ch):
    """colsum_partial in its order (256 / (C/4) pixel lanes, lane l takes pixels l, l + lanes, ..., the lanes added in order) and
    as numpy's float32 sum: the table inside n u sum|y|; gate_mlp on it inside the gate's bound."""
    worst_t, worst_g = 0.0, 0.0
    for hw, (h, w) in cases.GATE_RES_HW.items():
        c = cases.gate_res_case(ch, h, w)
        y32 = c.y.astype(np.float32)
        lanes = 256 // (ch // 4)
        tabs = []
        for k in range(c.chunks):
            piece = y32[:, k * 512:(k + 1) * 512]
            acc = np.zeros((lanes,) + piece[:, 0].shape, dtype=np.float32)
            for p in range(piece.shape[1]):
                acc[p % lanes] += piece[:, p]
            s = np.zeros_like(acc[0])
            for lane in range(lanes):
                s = s + acc[lane]
            tabs.append(s)
        kernel_table = np.stack(tabs, 1)
        other_table = np.stack([y32[:, k * 512:(k + 1) * 512].sum(1, dtype=np.float32) for k in range(c.chunks)], 1)
        for t in (kernel_table, other_table):
            ok, r = _ratio(t, c.table, c.table_bound)
            assert ok, (c.name, r)
            worst_t = max(worst_t, r)
            g, _ = cases.gate_f32(cases.table_sum_f32(t, 256, 1), c.hw, c.bias, c.w1, c.b1, c.w2, c.b2)
            # against the case's reference (a sum of HW terms) and, tighter, against the float64 gate of this very table
            for ref in (c, cases.gate_case_from_table(c, t)):
                bg, bl = cases.gate_bound(ref)
                ok, r = _ratio(g, ref.gate, bg)
                ok2, r2 = _ratio(cases.logit(g), ref.pre, bl)
                assert ok and ok2, (ref.name, r, r2)
            worst_g = max(worst_g, r, r2)
    _margin("colsum_partial c%d" % ch, worst_t)
    _margin("gate_mlp c%d" % ch, worst_g)


def test_gate_residual_exact_twins():
    for ch, (h, w) in cases.GATE_RES_TWINS:
        c = cases.gate_res_case(ch, h, w, True)
        y32 = c.y.astype(np.float32)
        table = np.stack([y32[:, k * 512:(k + 1) * 512].sum(1, dtype=np.float32) for k in range(c.chunks)], 1)
        assert np.array_equal(table.astype(np.float64), c.table) and not c.table_bound.min() < 0
        total = cases.table_sum_f32(table, 256, 1)
        assert np.array_equal(total.astype(np.float64), c.total)
        assert np.array_equal((total / np.float32(c.hw) + c.bias.astype(np.float32)).astype(np.float64), c.mean)
        g, pre = cases.gate_f32(total, c.hw, c.bias, c.w1, c.b1, c.w2, c.b2)
        assert np.array_equal(pre.astype(np.float64), c.pre)
        bg, bl = cases.gate_bound(c)
        assert _ratio(g, c.gate, bg)[0] and _ratio(cases.logit(g), c.pre, bl)[0]


def _apply_cases():
    return [cases.gate_apply_case(ch) for ch in cases.GATE_APPLY_C] + [cases.gate_wide_case(256, 3, 64), cases.gate_res_case(4, 15, 17)]


def test_gate_apply_restatements_inside_the_bound():
    """Written out and contracted into an fma, with a float32 gate (the float64 gate rounded: what a kernel's gate looks like)."""
    worst = 0.0
    for c in _apply_cases():
        g32 = c.gate.astype(np.float32).astype(np.float64)
        want = cases.gate_apply_ref(c.y, c.bias, g32, c.xres)
        bound = cases.gate_apply_bound(c.y, c.bias, g32, c.xres)
        for form in ("plain", "fma"):
            ok, r = _ratio(cases.gate_apply_ref(c.y, c.bias, g32, c.xres, np.float32, form), want, bound)
            assert ok, (c.name, form, r)
            worst = max(worst, r)
    _margin("gate_apply", worst)


def test_upsample_restatements_inside_the_bound():
    worst = {}
    for name in sorted(cases.UP_CASES):
        c = cases.up_case(name)
        kind = "non-dyadic" if any(not (cases.upconv_dyadic(hs, c.ho) and cases.upconv_dyadic(ws, c.wo)) for _, (hs, ws) in c.specs) else "dyadic"
        for order in ("kernel", "other"):
            ok, r = _ratio(cases.up_ref(c.srcs, c.ho, c.wo, np.float32, order), c.want, c.bound)
            assert ok, (name, order, r)
            worst[kind] = max(worst.get(kind, 0.0), r)
    for kind, r in sorted(worst.items()):
        _margin("upsample_concat " + kind, r)


# ---------------------------------------------------------------------------------------------
# 3. the mutants
# ---------------------------------------------------------------------------------------------
def _caught(tag, got, want, bound):
    ok, r = _ratio(got, want, bound)
    _mutant(tag, r)
    assert not ok and r >= MUTANT_FACTOR, (tag, r)


def test_mutant_pool_padded_with_zero():
    """Target: every all-negative pool input (p <= -1), where a border output that the ReLU does not clip moves by at least 1."""
    for name in sorted(cases.DS_CASES):
        c = cases.ds_case(name)
        if c.variant == "neg":
            _caught("pool pad 0 / " + name, cases.ds_ref(c.a, c.p, c.bias, c.stride, pad=0.0), c.want, cases.ds_bound(c))


def test_mutant_align_corners_false():
    for name in ("three_8_12_4", "row_36_4", "col_36_4", "nondyadic_32_64_32", "dyadic_36_4"):
        c = cases.up_case(name)
        got = torch.cat([F.interpolate(_nchw(v), size=(c.ho, c.wo), mode="bilinear", align_corners=False) for v in c.srcs], 1)
        _caught("align_corners=False / " + name, _nhwc(got), c.want, c.bound)


def test_mutant_second_source_four_channels_late():
    """Everything behind the first source sits four channels further on, its last four channels standing in the gap.  Targets:
    the cases whose second source is resized (where it is the identity the bound is 0 and any change is caught)."""
    for name in ("three_8_12_4", "nondyadic_36_4", "dyadic_36_4"):
        c = cases.up_case(name)
        c0 = c.specs[0][0]
        got = c.want.copy()
        got[..., c0 + 4:] = c.want[..., c0:-4]
        got[..., c0:c0 + 4] = c.want[..., c0 - 4:c0]
        _caught("second source 4 channels late / " + name, got, c.want, c.bound)


def _gate_mutants(c):
    """-> {mutant: gate} for a case with a table."""
    out = {}
    args = (c.hw, c.bias, c.w1, c.b1, c.w2, c.b2)
    if c.chunks > 1:
        out["last chunk dropped"] = cases.gate_ref(c.table[:, :-1].sum(1), *args)[0]
    out["one chunk twice"] = cases.gate_ref(c.table.sum(1) + c.table[:, c.chunks // 2], *args)[0]
    return out


def test_mutants_of_the_sums_on_the_wide_gate():
    """Target: the cases with chunks >= 7 parts + 1 (the eight-way loop) at every C, Cr = C / 4 -- gate and logit."""
    for ch in cases.GATE_WIDE_C:
        parts = 1024 // ch
        for k in (7 * parts + 1, 8 * parts, 21 * parts + 3):
            c = cases.gate_wide_case(ch, k, ch // 4)
            bg, bl = cases.gate_bound(c)
            for tag, g in _gate_mutants(c).items():
                _caught("%s / wide c%d k%d" % (tag, ch, k), g, c.gate, bg)
                assert cases.worst_ratio(cases.logit(g), c.pre, bl)[1] >= MUTANT_FACTOR


def test_mutants_of_the_sums_on_the_three_pass_gate():
    """Judged as the GPU test judges gate_mlp: against the float64 gate of the table, a sum of `chunks` terms.  Targets: HW 513
    and 1061 (a short last chunk) for the dropped and the doubled chunk, in the gate and in the table itself; every HW that is
    no multiple of 512 for the divisor chunks * 512."""
    for ch in cases.GATE_RES_C:
        for hw in (513, 1061):
            c = cases.gate_res_case(ch, *cases.GATE_RES_HW[hw])
            t = cases.gate_case_from_table(c, c.table)
            bg, bl = cases.gate_bound(t)
            for tag, g in _gate_mutants(t).items():
                _caught("%s / c%d hw%d" % (tag, ch, hw), g, t.gate, bg)
                assert cases.worst_ratio(cases.logit(g), t.pre, bl)[1] >= MUTANT_FACTOR
            _caught("last chunk dropped (table) / c%d hw%d" % (ch, hw), np.concatenate((c.table[:, :-1], 0 * c.table[:, -1:]), 1),
                    c.table, c.table_bound)
        for hw in (1, 7, 255, 511, 513, 1061):
            c = cases.gate_res_case(ch, *cases.GATE_RES_HW[hw])
            t = cases.gate_case_from_table(c, c.table)
            g = cases.gate_ref(t.total, t.hw, t.bias, t.w1, t.b1, t.w2, t.b2, divisor=t.chunks * 512)[0]
            _caught("mean over chunks * 512 / c%d hw%d" % (ch, hw), g, t.gate, cases.gate_bound(t)[0])


def test_mutants_of_the_elementwise_kernels():
    for c in _apply_cases():
        g32 = c.gate.astype(np.float32).astype(np.float64)
        want, bound = cases.gate_apply_ref(c.y, c.bias, g32, c.xres), cases.gate_apply_bound(c.y, c.bias, g32, c.xres)
        _caught("gate before the bias / " + c.name, cases.gate_apply_ref(c.y, c.bias, g32, c.xres, mutant="gate_first"), want, bound)
        _caught("residual omitted / " + c.name, cases.gate_apply_ref(c.y, c.bias, g32, c.xres, mutant="no_residual"), want, bound)
    for name in sorted(cases.BIAS_ACT_CASES):
        c = cases.bias_act_case(name)
        if c.res is not None:
            _caught("residual omitted / bias_act " + name, cases.bias_act_ref(c.x, c.bias, None, c.act), c.want, cases.bias_act_bound(c))
        if c.act == 2:
            _caught("LeakyReLU slope 0.1 / bias_act " + name, cases.bias_act_ref(c.x, c.bias, c.res, 2, slope=0.1), c.want,
                    cases.bias_act_bound(c))


# ---------------------------------------------------------------------------------------------
# 4. workspace sizing
# ---------------------------------------------------------------------------------------------
def test_engine_workspace_request_covers_the_three_pass_gate():
    """BasicBlock.run asks for (HW // 512 + 2) * B * C floats; smos_channel_gate_residual_cl requires B * C * (ceil(HW / 512) + 1)."""
    import inspect
    from streammos_amd import engine
    assert "// 512 + 2)" in inspect.getsource(engine.BasicBlock.run)        # the formula restated in tests/cl_cases.py
    for hw in range(1, 4097):
        for b, c in ((1, 4), (3, 32), (2, 256)):
            assert cases.engine_ws_floats(b, c, hw) >= cases.gate_ws_floats(b, c, hw), hw
    assert any(cases.engine_ws_floats(1, 4, hw) == cases.gate_ws_floats(1, 4, hw) for hw in range(1, 4097))   # and not padded everywhere

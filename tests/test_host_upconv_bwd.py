"""The backward of the decoder's conv_1 path without a GPU (tests/upconv_bwd_cases.py): (a) the float64 adjoint reference is the
adjoint of util.upconv_passes_ref and, with the two matrix products behind it, equals torch's float64 autograd of the
reference's formulation (interpolate -> cat -> conv2d); (b) the float32 restatement in the kernels' order stays inside the
derived bounds of G, dX and dW on every geometry; (c) on dyadic geometries with integer g float32 equals float64 bit for bit
in two summation orders; (d) one Inf in g makes exactly the elements non-finite whose forward stencil holds that pixel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import upconv_bwd_cases as cases
from tests import util


def _rel(got, want):
    return float(np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("name", cases.PASS_CASES)
def test_the_reference_is_the_adjoint_of_the_forward_passes(name):
    """<L z, g> = <z, L^T g> to 1e-12 of the product's magnitude, L = upconv_passes_ref with zero conv_a and zero bias."""
    c = cases.case(name)
    f = c.fwd
    zero = np.zeros((f.b, f.ho, f.wo, f.c))
    lz = util.upconv_passes_ref(zero, np.zeros(f.c), f.z, 0)
    left = float((lz * c.g).sum())
    right = float(sum((z * gz).sum() for z, gz in zip(f.z, c.gz)))
    mag = float(sum((np.abs(z) * m).sum() for z, m in zip(f.z, c.mag)))
    print("upconv-bwd %-20s <Lz, g> %.15g  <z, L^T g> %.15g  magnitude %.3g" % (name, left, right, mag))
    assert abs(left - right) <= 1e-12 * mag


def _autograd(c):
    """float64 autograd of the direct form: grads of sum(out * g) with respect to every x_src and w_src, channels-last x."""
    f = c.fwd
    xs = [torch.tensor(x).permute(0, 3, 1, 2).requires_grad_() for x in f.x]
    ws = [torch.tensor(w).requires_grad_() for w in f.w]
    ups = [F.interpolate(x, size=(f.ho, f.wo), mode="bilinear", align_corners=True) for x in xs]
    out = F.conv2d(torch.cat(ups, 1), torch.cat(ws, 1), None, 1, 1)
    out.backward(torch.tensor(c.g).permute(0, 3, 1, 2))
    return [x.grad.permute(0, 2, 3, 1).numpy() for x in xs], [w.grad.numpy() for w in ws]


def _autograd_gz(c, i):
    """float64 autograd of the direct form applied to the tap products themselves: z as a map of C groups of nine channels
    (channel 9 c + t = tap t of output channel c), resized, then the grouped 3x3 convolution whose group c sums tap (ky, kx)
    of its channel 3 ky + kx -- interpolate -> conv2d, at a cost that does not grow with C^2."""
    f = c.fwd
    hs, ws = f.sizes[i]
    z = torch.tensor(f.z[i].reshape(f.b, hs, ws, 9, f.c)).permute(0, 4, 3, 1, 2).reshape(f.b, 9 * f.c, hs, ws).requires_grad_()
    pick = torch.zeros((f.c, 9, 3, 3), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            pick[:, 3 * ky + kx, ky, kx] = 1.0
    out = F.conv2d(F.interpolate(z, size=(f.ho, f.wo), mode="bilinear", align_corners=True), pick, None, 1, 1, 1, f.c)
    out.backward(torch.tensor(c.g).permute(0, 3, 1, 2))
    return z.grad.reshape(f.b, f.c, 3, 3, hs, ws).permute(0, 4, 5, 2, 3, 1).numpy()


@pytest.mark.parametrize("name", cases.PASS_CASES)
def test_adjoint_dx_and_dw_equal_float64_autograd_of_the_direct_form(name):
    c = cases.case(name)
    f = c.fwd
    dxs, dws = _autograd(c)
    for i in range(len(f.sizes)):
        assert _rel(c.gz[i], _autograd_gz(c, i)) <= 1e-12, (name, i)
        assert _rel(c.dx[i], dxs[i]) <= 1e-12, (name, i)
        assert _rel(cases.fold_weight(c.dnk[i], f.c, f.cin), dws[i]) <= 1e-12, (name, i)


@pytest.mark.parametrize("name", cases.PASS_CASES + cases.TF_CASES)
def test_the_float32_restatement_stays_inside_the_bounds(name):
    c = cases.case(name)
    f = c.fwd
    gz32 = cases.upconv_adjoint_ref(c.g, f.sizes, np.float32)
    for i in range(len(f.sizes)):
        ok, r_g = util.msda_worst_ratio(gz32[i], c.gz[i], c.gz_bound[i])
        assert ok, (name, i, "G", r_g)
        dx32, dnk32 = cases.mix(gz32[i], f.x[i], f.nk[i], np.float32)
        ok, r_x = util.msda_worst_ratio(dx32, c.dx[i], c.dx_bound[i])
        assert ok, (name, i, "dX", r_x)
        ok, r_w = util.msda_worst_ratio(dnk32, c.dnk[i], c.dnk_bound[i])
        assert ok, (name, i, "dW", r_w)
        print("upconv-bwd-ratio %-20s source %d  G %.4f  dX %.4f  dW %.4f" % (name, i, r_g, r_x, r_w))


def test_the_bound_has_no_perturbation_term_on_dyadic_axes():
    for name in cases.PASS_CASES:
        c = cases.case(name)
        for i, (hs, ws) in enumerate(c.sizes):
            ny, _ = cases.axis_counts(hs, c.ho)
            nx, _ = cases.axis_counts(ws, c.wo)
            rounding = cases.U * (ny[None, :, None, None, None, None] + nx[None, None, :, None, None, None] + 8.0) * c.mag[i]
            if util.upconv_dyadic(hs, c.ho) and util.upconv_dyadic(ws, c.wo):
                assert np.array_equal(c.gz_bound[i], rounding), name
            else:
                assert (c.gz_bound[i] > rounding).all(), name


def test_there_are_exact_twins_and_degenerate_dyadic_cases():
    assert set(cases.EXACT_CASES) == {"fused_3to9_dyadic", "pair_5to9_dyadic", "identity"}
    assert set(cases.DYADIC_CASES) == set(cases.EXACT_CASES) | {"ws1", "all_one"}


def test_the_block_cap_cases_reach_the_second_trip():
    """tests/test_gpu_upconv_bwd.py caps both grids at 1 and 3 blocks of 256 threads: these cases have more than 3 x 256
    float4 elements in the y adjoint (B 3 Hs Wo C/4) and in the x adjoint (B Hs Ws 9 C/4) of every source."""
    many = []
    for n in cases.PASS_CASES:
        b, (_, wo), sizes, ch, _, _ = util.UPCONV_CASES[n]
        if all(b * 3 * hs * wo * (ch // 4) > 3 * 256 and b * hs * ws * 9 * (ch // 4) > 3 * 256 for hs, ws in sizes):
            many.append(n)
    assert {"two_ratios", "c128_two", "strip8", "strip16", "strip32"} <= set(many)


@pytest.mark.parametrize("name", cases.EXACT_CASES)
def test_exact_twins_float32_equals_float64_in_two_orders(name):
    c = cases.case(name)
    assert np.array_equal(c.g, np.round(c.g))
    for descending in (False, True):
        gz32 = cases.upconv_adjoint_ref(c.g, c.sizes, np.float32, descending)
        gz64 = cases.upconv_adjoint_ref(c.g, c.sizes, np.float64, descending)
        for a, b, ref in zip(gz32, gz64, c.gz):
            assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b) and np.array_equal(b, ref), (name, descending)


@pytest.mark.parametrize("name", cases.SMALL_CASES)
def test_one_inf_in_g_reaches_exactly_its_forward_stencil(name):
    c = cases.case(name)
    shape = (c.b, c.ho, c.wo, c.c)
    for pixel in cases.inf_pixels(name):
        g = np.array(c.g)
        g[pixel] = np.inf
        for dtype in (np.float64, np.float32):
            if dtype == np.float32 and not cases.dyadic(name):
                continue                   # float32 indices may differ from the rational ones by design on non-dyadic axes
            got = cases.upconv_adjoint_ref(g, c.sizes, dtype)
            for gz, mask, ref in zip(got, cases.stencil_mask(c.sizes, shape, pixel), c.gz):
                assert np.array_equal(~np.isfinite(gz), mask), (name, pixel, dtype)
                if dtype == np.float64:
                    assert np.array_equal(gz[~mask], ref[~mask]), (name, pixel)
                assert mask.any()

"""The fused training transfer without a GPU: the numpy chain of tests/cross_view_cases.py (ops_np.bilinear_sample ->
voxel_maxpool_fwd -> voxel_maxpool_bwd -> bilinear_bwd_cases.backward_ref) against torch's CPU autograd of BilinearSample ->
VoxelMaxPool, the coverage the steered cases promise, the switch, and the three C entries."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from oracle import ops_np
from streammos_amd import _lib, ops
from streammos_amd.refapi import deep_point
from streammos_amd.refapi.networks import backbone
from tests import bilinear_bwd_cases as bcases
from tests import cross_view_cases as cases
from tests import util
from tests.test_host_abi import mismatches

ENTRIES = ("smos_gather_scatter_train_fwd", "smos_gather_scatter_train_bwd", "smos_gather_scatter_train_point_grad")


def _without_nan(case):
    """The case with its NaN rows turned into padding rows (-1000): torch is not asked about NaN positions."""
    gcoord, scoord = case.gcoord.copy(), case.scoord.copy()
    gcoord[np.isnan(gcoord[..., :2]).any(-1), :2] = -1000.0
    scoord[np.isnan(scoord).any(-1)] = -1000.0
    return gcoord, scoord


def _chain(case, gcoord, scoord, with_pts):
    """x by the numpy chain (float32), then S, A, m."""
    size = (case.ho, case.wo)
    pts = ops_np.bilinear_sample(case.grid, gcoord[..., :2].astype(np.float32), cases.GSCALE)
    out = ops_np.voxel_maxpool_fwd(pts, scoord, size, cases.SSCALE)[0]
    x = ops_np.voxel_maxpool_bwd(pts, scoord, out, case.grad_out.astype(np.float32), size, cases.SSCALE).astype(np.float64)
    if with_pts:
        x = x + case.grad_pts
    s, a, m = bcases.backward_ref(x, gcoord, cases.GSCALE, case.hg, case.wg)
    return pts, out, x, types.SimpleNamespace(S=s, A=a, m=m, extra=1 if with_pts else 0)


@pytest.mark.parametrize("with_pts", [False, True])
@pytest.mark.parametrize("shape,kind", [sk for sk in cases.ALL if sk[0] != "empty"])
def test_numpy_chain_matches_torch_cpu_autograd(shape, kind, with_pts):
    case = cases.case_of(shape, kind)
    gcoord, scoord = _without_nan(case)
    pts_np, out_np, x_np, ref = _chain(case, gcoord, scoord, with_pts)
    grid = torch.tensor(case.grid, dtype=torch.float32, requires_grad=True)
    sampler = backbone.BilinearSample(case.c, cases.GSCALE)
    pts = sampler(grid, torch.tensor(gcoord[..., :2], dtype=torch.float32).unsqueeze(-1))
    out = deep_point.VoxelMaxPool(pts, torch.tensor(scoord, dtype=torch.float32).unsqueeze(-1), (case.ho, case.wo), cases.SSCALE)
    loss = (out.double() * torch.tensor(case.grad_out)).sum()
    if with_pts:
        loss = loss + (pts[..., 0].double() * torch.tensor(case.grad_pts)).sum()
    loss.backward()
    # the same winners on both sides (exact ties and zeros are the same numbers in any rounding), so the same selection
    cell = ops_np.voxel_cell_index(scoord, (case.ho, case.wo), cases.SSCALE)
    assert np.array_equal(cases.winners(pts[..., 0].detach().numpy(), cell, out.detach().numpy()), cases.winners(pts_np, cell, out_np))
    ok, ratio = cases.worst_ratio(grid.grad.numpy(), ref)
    print("cross-view host ratio %-28s grad_pts=%d %.4f" % (case.name, with_pts, ratio))
    assert ok, ratio
    # the rows that were rewritten add nothing: the chain on the case as it is gives the same sums
    s0 = _chain(case, case.gcoord, case.scoord, with_pts)[3]
    assert np.array_equal(s0.S, ref.S) and np.array_equal(s0.A, ref.A) and np.array_equal(s0.m, ref.m)
    # and the case's own mask is the chain's
    want = cases.reference(case, case.win_np, with_pts)
    assert np.array_equal(want.S, ref.S) and np.array_equal(want.m, ref.m)


@pytest.mark.parametrize("shape,kind", cases.ALL)
def test_steered_cases_keep_their_coverage(shape, kind):
    case = cases.case_of(shape, kind)
    have = cases.self_check(case)
    print("cross-view case %-22s %s" % (case.name, have))
    if shape == "empty":
        assert case.n == 0 and not any(have.values())
        return
    for prop in ("multi", "zero", "dropped", "loser"):
        if prop in cases.EXPECT[kind]:
            assert have[prop] > 0, (case.name, prop, have)
    if kind == "dropped":
        assert have["kept"] == 0 and not case.out_np.any()
    if kind == "onecell":
        assert have["dropped"] == 0
    dup = np.arange(9, case.n, 10)
    assert np.array_equal(case.gcoord[:, dup, :2], case.gcoord[:, dup - 1, :2], equal_nan=True)
    assert np.array_equal(case.scoord[:, dup], case.scoord[:, dup - 1], equal_nan=True)
    if kind == "mix":
        assert np.isnan(case.gcoord).any() and (case.gcoord[..., 0] == -1000.0).any() and np.isnan(case.scoord).any()


def test_signed_case_has_cells_with_a_negative_maximum():
    case = cases.signed_case()
    have = cases.self_check(case)
    assert (case.out_np < 0).any() and (case.out_np > 0).any() and (case.grid < 0).any()
    assert all(have[p] > 0 for p in ("multi", "zero", "dropped", "loser")), have


def test_switch_spelling(monkeypatch):
    assert ops.cross_view_fused.var == "SMOS_CROSS_VIEW_TRAIN" and ops.cross_view_fused.default is False
    assert ops.set_cross_view_fused == ops.cross_view_fused.set
    monkeypatch.delenv("SMOS_CROSS_VIEW_TRAIN", raising=False)
    prev = ops.set_cross_view_fused(None)
    try:
        assert ops.cross_view_fused() is False                       # off unless asked for
        for text, want in (("", False), ("0", False), (" False ", False), ("OFF", False), ("no", False), ("1", True),
                           ("true", True), ("on", True), ("2", True)):
            monkeypatch.setenv("SMOS_CROSS_VIEW_TRAIN", text)
            assert ops.cross_view_fused() is want, text
        monkeypatch.setenv("SMOS_CROSS_VIEW_TRAIN", "1")
        assert ops.set_cross_view_fused(False) is None and ops.cross_view_fused() is False      # set() goes first
        assert ops.set_cross_view_fused(None) is False and ops.cross_view_fused() is True
    finally:
        ops.set_cross_view_fused(prev)


def test_the_three_entries_are_declared_bound_and_exported():
    declared = util.header_declarations()
    lib = ctypes.CDLL(_lib.LIB_PATH)          # loads without a GPU; no compute call is made
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name) and name not in _lib.INT64_RESULTS
    assert mismatches({n: _lib.SIGNATURES[n] for n in ENTRIES}, (), declared) == []
    fwd, bwd, pg = (_lib.SIGNATURES[n] for n in ENTRIES)
    assert bwd == pg and fwd[:10] == bwd[:10] and len(fwd) == 21 and len(bwd) == 24
    # host arrays are typed, device addresses are not
    assert fwd[1] is _lib.c_i64p and fwd[4] is _lib.c_f32p and fwd[7] is _lib.c_f32p and fwd[0] is _lib.vp and fwd[-1] is _lib.vp
    assert util.header_abi_version() == _lib.ABI_VERSION >= 4
    head = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smos.h")).read().split("int smos_debug_set_conv_grid_cap(int32_t")[0]
    assert "smos_gather_scatter_train_*" in head            # the grid cap's comment lists them


def test_cpu_tensors_are_refused():
    grid = torch.zeros((1, 8, 4, 4))
    coord = torch.zeros((1, 5, 2))
    with pytest.raises(RuntimeError, match="GPU memory"):
        ops.gather_scatter_train(grid, coord, (0.5, 0.5), coord, (4, 4), (0.5, 0.5))

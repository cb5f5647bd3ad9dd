"""Backward of the bilinear gather without a GPU: the float64 reference of tests/bilinear_bwd_cases.py against torch's CPU
autograd of F.grid_sample, the C ABI of smos_bilinear_gather_bwd, and the refusal of a coordinate gradient."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ops_np
from streammos_amd import _lib, ops
from tests import bilinear_bwd_cases as cases
from tests import util

NAME = "smos_bilinear_gather_bwd"


def _torch_grad(case, keep):
    """d/d grid of sum(grid_sample(grid, positions) * grad_out) in float64 on the CPU, on the float32 positions the kernels
    use, for the points `keep` [B, N] of every sample (the same number per sample)."""
    b, c, h, w = case.b, case.c, case.h, case.w
    iy, ix = ops_np.bilinear_pixel_coords(case.coord[..., :2], case.scale, h, w)
    n = int(keep[0].sum())
    iy = np.stack([iy[s][keep[s]] for s in range(b)]).astype(np.float64)
    ix = np.stack([ix[s][keep[s]] for s in range(b)]).astype(np.float64)
    go = np.stack([case.grad_out[s][:, keep[s]] for s in range(b)])
    norm = torch.tensor(np.stack((2.0 * ix / (w - 1) - 1.0, 2.0 * iy / (h - 1) - 1.0), -1)).view(b, n, 1, 2)
    grid = torch.zeros((b, c, h, w), dtype=torch.float64, requires_grad=True)
    out = F.grid_sample(grid, norm, mode="bilinear", padding_mode="zeros", align_corners=True)
    out.backward(torch.tensor(go).view(b, c, n, 1))
    return grid.grad.numpy()


@pytest.mark.parametrize("kind", cases.COORD_SETS)
@pytest.mark.parametrize("shape", [s for s in cases.SHAPES if s != "empty"])
def test_reference_matches_torch_cpu_autograd(shape, kind):
    case = cases.case_of(shape, kind)
    finite = np.isfinite(case.coord[..., :2]).all(-1)
    # torch is not asked about NaN positions: the NaN rows of every sample and as many others as it takes to keep the
    # samples equally long are left out, and the reference on the remaining points has to agree with torch ...
    n_keep = int(finite.sum(1).min())
    keep = np.zeros_like(finite)
    for s in range(case.b):
        keep[s, np.flatnonzero(finite[s])[:n_keep]] = True
    sub_coord = np.stack([case.coord[s][keep[s]] for s in range(case.b)])
    sub_go = np.stack([case.grad_out[s][:, keep[s]] for s in range(case.b)])
    s_ref, a_ref, m_ref = cases.backward_ref(sub_go, sub_coord, case.scale, case.h, case.w)
    want = _torch_grad(case, keep)
    assert np.abs(s_ref - want).max() <= 1e-12 * max(np.abs(s_ref).max(), 1e-300)
    assert (a_ref >= np.abs(s_ref) - 1e-12).all() and not (a_ref * (m_ref == 0)).any()      # nothing arrives where m = 0
    # ... and the rows that were left out for being NaN add nothing: with them dropped alone the reference does not move
    if kind == "mix":
        assert (~finite).any() and (case.coord[..., 0] == -1000.0).any()
        go0 = np.where(finite[:, None, :], case.grad_out, 0.0)
        coord0 = np.where(finite[..., None], case.coord, -1000.0)
        s0, a0, m0 = cases.backward_ref(go0, coord0, case.scale, case.h, case.w)
        assert np.array_equal(s0, case.S) and np.array_equal(a0, case.A) and np.array_equal(m0, case.m)


def test_cases_reach_all_four_borders_and_the_padding_rows():
    case = cases.case_of("c64", "uniform")
    iy, ix = ops_np.bilinear_pixel_coords(case.coord[..., :2], case.scale, case.h, case.w)
    assert (iy < 0).any() and (iy > case.h - 1).any() and (ix < 0).any() and (ix > case.w - 1).any()
    assert (iy < -1).any() and (iy > case.h).any() and (ix < -1).any() and (ix > case.w).any()      # wholly outside too
    runs = cases.case_of("c64", "runs")
    iy, ix = (np.floor(v) for v in ops_np.bilinear_pixel_coords(runs.coord[..., :2], runs.scale, runs.h, runs.w))
    for edge in range(cases.TILE, runs.n, cases.TILE):          # a run across every tile (and block) border of the kernel
        assert (iy[:, edge - 1] == iy[:, edge]).all() and (ix[:, edge - 1] == ix[:, edge]).all()
    assert cases.case_of("c32", "onecell").m.max() == 257 and (cases.sparse_case().m == 0).any()
    assert cases.case_of("empty", "uniform").S.shape == (1, 32, 8, 8) and not cases.case_of("empty", "mix").m.any()


def test_grid_stride_case_has_more_tiles_than_waves_and_whole_tiles_of_padding():
    case = cases.grid_stride_case()
    per_sample = -(-case.n // cases.TILE)
    assert case.b * per_sample > cases.GRID_WAVES and case.n % cases.TILE
    iy, ix = ops_np.bilinear_pixel_coords(case.coord[..., :2], case.scale, case.h, case.w)
    live = np.isfinite(iy) & np.isfinite(ix) & (iy > -1) & (iy < case.h) & (ix > -1) & (ix < case.w)
    pad = np.zeros((case.b, per_sample * cases.TILE), dtype=bool)
    pad[:, :case.n] = live
    tile_live = pad.reshape(case.b * per_sample, cases.TILE).any(1)            # in the kernel's tile order
    first, second = tile_live[:cases.GRID_WAVES], tile_live[cases.GRID_WAVES:]
    wave_first = first[:len(second)]
    # every combination of (first tile skipped / worked, second tile skipped / worked) occurs on some wave
    assert {(bool(a), bool(b_)) for a, b_ in zip(wave_first, second)} == {(True, True), (True, False), (False, True), (False, False)}
    assert (~first).sum() > 100 and (~second).sum() > 100 and case.m.max() > 1000


def test_header_declares_and_library_exports_the_backward():
    declared = util.header_declarations()
    assert NAME in declared
    lib = ctypes.CDLL(_lib.LIB_PATH)          # loads without a GPU; no compute call is made
    assert hasattr(lib, NAME)
    args = declared[NAME][1]
    assert len(_lib.SIGNATURES[NAME]) == len(args) == len(_lib.SIGNATURES["smos_bilinear_gather_fwd"])
    assert util.header_abi_version() == _lib.ABI_VERSION


def test_coordinate_gradient_is_refused():
    grid = torch.zeros((1, 8, 4, 4))
    coord = torch.zeros((1, 5, 2), requires_grad=True)
    with pytest.raises(RuntimeError, match="coord"):
        ops.bilinear_gather(grid, coord, (0.5, 0.5))
    with pytest.raises(RuntimeError):                          # without a gradient it is the device check that refuses a CPU tensor
        ops.bilinear_gather(grid, coord.detach(), (0.5, 0.5))

"""tests/voxel_maxpool_cases.py without a GPU: its reference against oracle.ops_np (np.maximum.at) and against the CPU twin
(libsmos_cpu.so through deep_point.VoxelMaxPool and point_deep.cpu_kernel, float32 and float64, voxel_max_idx included) on every
case, the union of the cases against the list of kernel paths they have to reach (through launch_path, the restatement of the
host dispatch), and the four properties every case has to hold.  All comparisons are exact: a maximum returns one of its inputs.
"""
import numpy as np
import pytest
import torch

from oracle import ops_np
from streammos_amd.refapi import deep_point
from streammos_amd.refapi.point_deep import cpu_kernel
from tests import voxel_maxpool_cases as cases

SMALL = cases.small_cases()
NAMES = sorted(SMALL) + sorted(cases.SWEEP_CASES)


def _case(name):
    return SMALL[name]() if name in SMALL else cases.sweep_case(name)


def _grad_out(case):
    return cases._rng(case.name + "/grad").normal(0.0, 1.0, case.out.shape).astype(case.feat.dtype)


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_ops_np(name):
    case = _case(name)
    scale = np.asarray(case.scale, dtype=np.float32)
    assert np.array_equal(ops_np.voxel_cell_index(case.ind, case.size, scale), case.cell)
    with np.errstate(invalid="ignore"):                                      # (np.maximum.at warns about the NaN member)
        want, want_idx = ops_np.voxel_maxpool_fwd(case.feat, case.ind, case.size, scale)
    assert cases.same(want, case.out)
    assert np.array_equal(want_idx, cases.cell_offsets(case.cell, case.size, torch.empty(case.out.shape, device="meta")))
    go = _grad_out(case)
    assert cases.same(ops_np.voxel_maxpool_bwd(case.feat, case.ind, want, go, case.size, scale), cases.grad_ref(case.feat, case.cell, case.out, go))


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_cpu_twin(name):
    """Forward and backward through the autograd function on contiguous CPU tensors in float32 and float64, and the forward
    with voxel_max_idx through point_deep.cpu_kernel in every layout (the twin takes strides)."""
    case = _case(name)
    own = torch.float64 if case.feat.dtype == np.float64 else torch.float32
    for dtype in ((own,) if name.startswith("special_values") else (torch.float32, torch.float64)):
        feat, ind, out, cell = cases.rounded(case, dtype)
        f = torch.from_numpy(feat).unsqueeze(-1).requires_grad_(True)
        i = torch.from_numpy(ind).to(dtype).unsqueeze(-1)
        y = deep_point.VoxelMaxPool(f, i, case.size, case.scale)
        assert y.dtype == dtype and cases.same(y.detach().numpy(), out)
        go = _grad_out(case).astype(feat.dtype)
        y.backward(torch.from_numpy(go))
        assert cases.same(f.grad[..., 0].numpy(), cases.grad_ref(feat, cell, out, go))
        for layout in (cases.LAYOUTS if name in SMALL else (case.layout,)):
            fv, ov = cases.place(feat, case.size, layout, dtype, "cpu")
            idx = torch.full(cell.shape, -1, dtype=torch.int64)
            cpu_kernel.voxel_maxpooling_cpu_forward(fv, i[..., 0], ov, idx, None, None, None, torch.tensor(case.scale, dtype=torch.float32))
            assert cases.same(ov.numpy(), out), layout
            assert np.array_equal(idx.numpy(), cases.cell_offsets(cell, case.size, ov)), layout


def test_layout_strides_are_the_strides_place_builds():
    case = cases.matrix_case("mixed", 9)
    for layout in cases.LAYOUTS:
        f, out = cases.place(case.feat, case.size, layout, torch.float32, "cpu")
        assert (f.stride(1), out.stride(1)) == cases.layout_strides(layout, case.n, case.size)
        assert tuple(f.shape) == case.feat.shape and np.array_equal(f.numpy(), case.feat) and not out.any()
    f, out = cases.place(case.feat, case.size, "sliced", torch.float32, "cpu")
    assert f.stride(0) > case.c * f.stride(1) and f.stride(1) > case.n * f.stride(2) and f.stride(2) == 2


def test_the_cases_reach_every_kernel_path():
    """Through launch_path: rows G = 8 / 16 / 32 / 64, rows with C % G != 0 and with C > 64, points with one chunk and with
    several whose last has a tail (c1 - c0) % 8 of 0, 1, 4 and 7, a negative in a chunk above the first only, the exact path in
    both mappings, D = 1 .. 4, BS = 1 and 3, N = 1 / 63 / 64 / 65, and a second sweep of every kernel."""
    rows, points, signed, dims, batches, ns = set(), set(), set(), set(), set(), set()
    for name in sorted(SMALL):
        case = SMALL[name]()
        dims.add(case.d), batches.add(case.bs), ns.add(case.n)
        for layout in cases.LAYOUTS:
            kernel, k, c_chunk = cases.path_of(case, layout)
            if case.signed:
                signed.add(kernel)
            if kernel == "rows":
                rows.add((k, case.c % k != 0, case.c > 64))
            else:
                tail = (case.c - (k - 1) * c_chunk) % 8
                assert c_chunk % 8 == 0 and 0 < case.c - (k - 1) * c_chunk <= c_chunk
                late_neg = case.sign == "neg_in_last_chunk" and k > 1 and c_chunk <= 16
                points.add((k > 1, tail, late_neg))
    assert {g for g, _, _ in rows} == {8, 16, 32, 64}
    assert any(ragged for _, ragged, _ in rows) and any(big for _, _, big in rows)
    assert (64, True, True) in rows                                            # C = 71, 130: a second / third trip with a ragged end
    assert {tail for many, tail, _ in points if many} >= {0, 1, 4, 7} and any(not many for many, _, _ in points)
    assert any(late for _, _, late in points)
    assert signed == {"rows", "points"}
    assert dims == {1, 2, 3, 4} and batches >= {1, 3} and ns >= {1, 63, 64, 65}
    # the chunk arithmetic of the issue's list: 16 -> 2 x 8; 17, 20 -> 16 + 1 / 4; 71 -> 4 x 16 + 7
    for c, want in ((16, (2, 8)), (17, (2, 16)), (20, (2, 16)), (71, (5, 16)), (9, (1, 16)), (1, (1, 8))):
        assert cases.launch_path(torch.float32, c, 514, 257, 30)[1:] == want
    assert cases.launch_path(torch.float32, 64, 1 << 20, 5, 30) == ("points", 1, 64)          # 2^20 points and more: no chunks
    assert cases.launch_path(torch.float16, 20, 514, 1, 1) == ("generic", 1, 20)
    # sweeps
    sp, sr = cases.sweep_case("sweep_points"), cases.sweep_case("sweep_rows")
    assert cases.path_of(sp, sp.layout) == ("points", 1, 8) and sp.bs * sp.n > cases.points_per_sweep("points") and sp.signed
    assert sp.bs * sp.n > 2 * cases.points_per_sweep("signed")
    assert cases.path_of(sr, sr.layout) == ("rows", 64, None) and sr.bs * sr.n > 2 * cases.points_per_sweep("rows", 64) and sr.signed
    for case in (sp, sr):                                                      # kept points beyond the first sweep
        assert (case.cell.reshape(-1)[cases.points_per_sweep(cases.path_of(case, case.layout)[0], 64):] >= 0).any()


@pytest.mark.parametrize("name", NAMES)
def test_every_case_holds_its_four_properties(name):
    case = _case(name)
    held = dict(zip(cases.PROPERTY_NAMES, cases.properties(case)))
    assert held["empty_cell"]
    assert set(n for n, h in held.items() if not h) <= set(case.lacks)
    assert not case.lacks or name == "n1"
    # features are multiples of 1/8 (the special values aside): exact in float16, so ties survive the rounding
    if not name.startswith("special_values"):
        assert np.array_equal(case.feat * 8, np.round(case.feat * 8)) and np.abs(case.feat).max() < 64
    want_signed = {"relu": False, "mixed": True, "neg": True, "neg_in_last_chunk": True}[case.sign] or name.startswith("special_values")
    assert case.signed == want_signed


def test_sign_modes_are_what_they_are_named_for():
    relu, neg, late = cases.matrix_case("relu", 20), cases.matrix_case("neg", 20), cases.matrix_case("neg_in_last_chunk", 20)
    assert (relu.feat >= 0).all() and not np.signbit(relu.feat).any() and (relu.feat == 0).any() and (relu.feat > 0).any()
    assert (neg.feat <= 0).all() and (neg.out <= 0).all() and (neg.out < 0).any()
    assert (np.signbit(neg.feat) & (neg.feat == 0)).any()                      # -0.0 is among them
    assert (late.feat[:, :16] >= 0).all() and (late.feat[:, 16:] < 0).all()
    mixed = cases.matrix_case("mixed", 20)
    occupied = np.zeros(mixed.out[:, 0].shape, dtype=bool).reshape(mixed.bs, -1)
    for b in range(mixed.bs):
        occupied[b, mixed.cell[b][mixed.cell[b] >= 0]] = True
    out = mixed.out.reshape(mixed.bs, mixed.c, -1)
    assert (out[:, 0][occupied] < 0).any() and (out[:, 0][occupied] > 0).any() and not out[:, 0][~occupied].any()
    sparse = cases.shape_case("sparse")
    assert (np.bincount(sparse.cell[0][sparse.cell[0] >= 0], minlength=576) == 0).sum() > 288


def test_special_cases_hold_what_their_docstrings_say():
    for dtype in (torch.float32, torch.float64):
        fi = np.finfo(cases.NP_DTYPE[dtype])
        relu, mixed = cases.special_values("relu", dtype), cases.special_values("mixed", dtype)
        with np.errstate(invalid="ignore"):
            assert not (relu.feat < 0).any() and not np.signbit(relu.feat[~np.isnan(relu.feat)]).any() and (mixed.feat < 0).any()
        for case in (relu, mixed):
            cells = case.out[0, 0].reshape(-1)
            assert cells[0] == np.inf and cells[1] == fi.max and cells[2] == fi.smallest_subnormal and np.isnan(cells[3])
            assert cells[4] == np.inf and cells[5] == fi.max and cells[6] == fi.smallest_subnormal and cells[6] > 0
            assert np.array_equal(case.out[0], case.out[1], equal_nan=True)    # sample 1: the same members, reversed
        cells = mixed.out[0, 0].reshape(-1)
        assert list(cells[9:15]) == [-np.inf, fi.min, -fi.smallest_subnormal, -np.inf, fi.min, -fi.smallest_subnormal]
        assert cells[15] == 0 and cells[16] == fi.smallest_subnormal and cells[17] == 3.0
    case = cases.scale_rounding("mixed")
    # kept, and in another cell than a float64 product says: on either axis of either sample (sizes 7 and 9 leave room for one
    # such k per axis: 5 / 0.7 and one below 9 / 0.3; the other seeds lie beyond the far edge, or on it)
    moved = [(b, i, d) for b, i, d, p32, p64 in case.planted if np.trunc(p32) != np.trunc(p64) and p32 < case.size[d]]
    assert {(b, d) for b, i, d in moved} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for b, i, d in moved:
        assert case.cell[b, i] >= 0 and cases.winners(case.feat, case.cell, case.out)[b, :, i].all()
    case = cases.edge_coords("mixed")
    assert np.isnan(case.ind).any() and np.isinf(case.ind).any() and (case.ind == cases.PAD).any() and (np.abs(case.ind) > 1e29).any()

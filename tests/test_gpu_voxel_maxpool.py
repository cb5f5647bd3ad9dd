"""csrc/voxel_maxpool.hip on the GPU against the float64 reference of tests/voxel_maxpool_cases.py, through ops.voxel_maxpool_fwd /
_bwd, deep_point.VoxelMaxPool and the two spellings of point_deep.cuda_kernel.

ALL COMPARISONS ARE EXACT.  A maximum returns one of its inputs and the backward copies a gradient, so the kernels have nothing
to round: outputs are compared with np.array_equal on the values (NaN equal to NaN; +0 equal to -0, because which zero an
all-zero cell ends with depends on the order of racing stores on the exact path), cells and voxel_max_idx as integers, and the
surroundings of a destination bit for bit through an integer view.  float16 / float64 runs round the inputs to the dtype first
and the reference runs on the rounded values.

Case -> kernel path reached (float32; layouts (a) nchw, (b) cl, (c) pm_nchw, (d) sliced of tests/voxel_maxpool_cases.py):

    case (sign modes: relu / mixed / neg / neg_in_last_chunk)       layout     kernel path
    m_<sign>_c1 | c7 | c8 | c9 | c12                                a, c, d    vmp_fwd_points, one chunk: tail loop of 1 | 7 | 0 | 1 | 4
    m_<sign>_c16 | c17 | c20 | c32 | c33                            a, c, d    vmp_fwd_points, chunks 2x8 | 16+1 | 16+4 | 4x8 | 16+16+1;
    m_<sign>_c64 | c71 | c130                                                  8x8 | 4x16+7 | 8x16+2; voxel_max_idx by blockIdx.y == 0
    m_<sign>_c1, c7                                                 b          vmp_fwd_points (C < 8), out_c == 1
    m_<sign>_c8 | c9, c12, c16 | c17, c20, c32 | c33, c64           b          vmp_fwd_rows<8> | <16> | <32> | <64>, one trip
    m_<sign>_c71, c130                                              b          vmp_fwd_rows<64>, two / three trips, ragged last
    m_mixed_*, m_neg_*                                              all        + vmp_fwd_signed<0/1> after either fast kernel
    m_neg_in_last_chunk_c17 ... c130                                a, c, d    the flag raised by blockIdx.y > 0 only
    d1, d3, d4, d4_relu, n1, n63, n64, n65, sparse                  all        D = 1 .. 4, BS = 1 / 3, N = 1 / 63 / 64 / 65, a sparse grid
    scale_rounding_*, edge_coords_*                                 a, b       cell_offset: the float32 product, every edge of the keep rule
    special_values_relu                                             a, b       fast kernels; the NaN raises the flag -> vmp_fwd_signed
    special_values_mixed                                            a, b       vmp_fwd_signed with +-inf, +-max, +-denormal, -0.0
    sweep_points (1 100 000 points)                                 a          second sweep of vmp_fwd_points, vmp_fwd_signed,
                                                                               vmp_fwd_generic<half / double>, vmp_bwd_points
    sweep_rows (40 000 points, C = 33)                              b          third sweep of vmp_fwd_rows<64>
    any case in float16 / float64                                   a, b, d    vmp_fwd_generic / vmp_bwd_generic (half: CAS on the word)
    backward, float32                                               a, b       vmp_bwd_points
"""
import numpy as np
import pytest
import torch

from streammos_amd import ops
from streammos_amd.refapi import deep_point
from tests import voxel_maxpool_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.5                                   # exact in float16
INT_VIEW = {2: torch.int16, 4: torch.int32, 8: torch.int64}
SMALL = cases.small_cases()
DTYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16}


def _ind(ind, dtype):
    return torch.from_numpy(np.ascontiguousarray(ind)).to(device=DEV, dtype=dtype)


def _idx(cell):
    return torch.full(cell.shape, -1, dtype=torch.int64, device=DEV)


def _forward(case, layout, dtype=torch.float32, with_idx=True):
    """One launch of a case in a layout: the output and voxel_max_idx against the reference."""
    feat, ind, want, cell = cases.rounded(case, dtype)
    f, out = cases.place(feat, case.size, layout, dtype, DEV)
    assert case.c == 1 or (f.stride(1), out.stride(1)) == cases.layout_strides(layout, case.n, case.size)
    idx = _idx(cell) if with_idx else None
    ops.voxel_maxpool_fwd(f, _ind(ind, dtype), out, case.size, case.scale, voxel_max_idx=idx)
    got = out.cpu().numpy()
    assert cases.same(got, want), "%s %s: %d cells differ" % (case.name, layout, int((~_eq(got, want)).sum()))
    if with_idx:                                   # dropped points keep the caller's -1
        assert np.array_equal(idx.cpu().numpy(), cases.cell_offsets(cell, case.size, out))
    return got


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _like_feat(f, layout, fill):
    """A tensor with the strides of ``f`` filled with ``fill`` (for "sliced": the same slice of a wider buffer), and its parent."""
    if layout == "sliced":
        bs, c, n = f.shape
        wide = torch.full((bs, c + 3, 2 * n + 5), fill, dtype=f.dtype, device=f.device)
        return wide[:, 2:2 + c, 3:3 + 2 * n:2], wide
    g = torch.empty_like(f).fill_(fill)
    assert _strides(g) == _strides(f)
    return g, g


def _strides(t):
    """strides of the dims that have more than one element (the others are arbitrary)"""
    return [s for s, n in zip(t.stride(), t.shape) if n > 1]


def _backward(case, layout, dtype=torch.float32):
    """vmp_bwd_* on the REFERENCE's pooled grid: winners receive the cell's gradient, every other element of grad_feat -- losers,
    dropped points, and for "sliced" the buffer around the slice -- keeps the sentinel it was filled with."""
    feat, ind, want, cell = cases.rounded(case, dtype)
    f, out = cases.place(feat, case.size, layout, dtype, DEV)
    out.copy_(torch.from_numpy(want).to(dtype))
    go_np = cases._rng(case.name + "/grad").normal(0.0, 1.0, want.shape).astype(cases.NP_DTYPE[dtype])
    go = torch.empty_like(out)
    assert _strides(go) == _strides(out)
    go.copy_(torch.from_numpy(go_np))
    gf, parent = _like_feat(f, layout, SENTINEL)
    ops.voxel_maxpool_bwd(f, _ind(ind, dtype), out, go, gf, case.size, case.scale)
    win = cases.winners(feat, cell, want)
    expect = np.where(win, cases.grad_ref(feat, cell, want, go_np), SENTINEL)
    assert win.any() and (case.n == 1 or not win.all())
    assert cases.same(gf.cpu().numpy(), expect)
    if parent is not gf:
        gf.fill_(SENTINEL)
        assert bool((parent == SENTINEL).all())


# ------------------------------------------------------------------------------------------
# forward, float32: sign modes x C x layouts, and the shape cases
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("sign,c", cases.matrix_keys())
def test_forward_float32_matrix(sign, c, layout):
    """voxel_max_idx rides along in (a) and (b) -- (a) is chunked from C = 16 on -- and is left out in (c) and (d)."""
    _forward(cases.matrix_case(sign, c), layout, with_idx=layout in ("nchw", "cl"))


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("name", sorted(cases.SHAPE_CASES))
def test_forward_float32_shapes(name, layout):
    _forward(cases.shape_case(name), layout)


# ------------------------------------------------------------------------------------------
# the float32 product, the edges of the keep rule, special values
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mapping", ["f32-nchw", "f32-cl", "f64-nchw", "f64-cl"])
@pytest.mark.parametrize("name", ["scale_rounding_relu", "scale_rounding_mixed", "edge_coords_relu", "edge_coords_mixed", "edge_coords_neg"])
def test_cell_of_a_point(name, mapping):
    """cell_offset: the product is the float32 one (scale_rounding: a float64 or fused product moves the seeded points, which
    carry the largest features, into a neighbouring cell or keeps the ones the float32 product drops at the far edge), and
    -1.0, size, NaN, +-inf, +-1e30 and the padding coordinate are dropped while nextafter(-1, 0), -0.0 and nextafter(size, 0)
    are kept.  Forward with voxel_max_idx, and backward."""
    dtype, layout = mapping.split("-")
    case = SMALL[name]()
    _forward(case, layout, DTYPES[dtype])
    _backward(case, layout, DTYPES[dtype])


@pytest.mark.parametrize("mapping", ["f32-nchw", "f32-cl", "f64-nchw", "f64-cl"])
@pytest.mark.parametrize("sign", ["relu", "mixed"])
def test_special_values(sign, mapping):
    """+inf, the largest finite number and the smallest denormal as a lone member and as the maximum of a shared cell (the
    denormal also above zeros only: the fast kernels' ``v > 0`` has to hold for it), with "mixed" their negatives and -0.0 above
    negatives.  THE NaN THAT IS THE SOLE MEMBER OF A CELL COMES OUT AS NaN ON EVERY PATH, inside the all-non-negative tensor
    ("relu": only the NaN itself can raise the flag) and inside the mixed one."""
    dtype, layout = mapping.split("-")
    case = cases.special_values(sign, DTYPES[dtype])
    got = _forward(case, layout, DTYPES[dtype])
    assert np.isnan(got[:, :, 0, 3]).all() and np.isnan(got).sum() == 2 * case.c
    _backward(case, layout, DTYPES[dtype])


# ------------------------------------------------------------------------------------------
# destination inside a wider, poisoned buffer
# ------------------------------------------------------------------------------------------
def _pattern(shape, dtype):
    """A buffer of ``shape`` whose bits are a recognisable function of the element index (NaN patterns included)."""
    size = torch.empty((), dtype=dtype).element_size()
    k = torch.arange(int(np.prod(shape)), dtype=torch.int64, device=DEV) * 2654435761 + 12345
    if size < 8:
        k = k % (1 << (8 * size - 1))
    return k.to(INT_VIEW[size]).view(dtype).view(shape)


@pytest.mark.parametrize("kind", ["cl_slice", "window"])
@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
@pytest.mark.parametrize("name", ["scale_rounding_relu", "scale_rounding_mixed", "m_relu_c17", "m_mixed_c17"])
def test_destination_inside_a_poisoned_buffer(name, dtype, kind):
    """cl_slice: ``out`` is the channel slice [3, 3 + C) of a channels-last grid of an odd number of channels (out_c == 1,
    sstride != C: the rows mapping in float32); window: ``out`` is a spatial window of a wider NCHW grid of odd width, starting
    at an odd element offset (the points mapping).  In both, rows of the slice start at odd and at even element offsets, so in
    float16 the two halves of a 32-bit word belong to different owners and the CAS takes both branches.  The parent is filled
    with a pattern and only the slice zeroed; afterwards the slice equals the reference and everything around it is bit-identical
    to the pattern."""
    dtype = DTYPES[dtype]
    case = SMALL[name]()
    feat, ind, want, cell = cases.rounded(case, dtype)
    bs, c, size = case.bs, case.c, case.size
    if kind == "cl_slice":
        cw = c + 5 + (c % 2)                       # odd
        parent = _pattern((bs,) + size + (cw,), dtype)
        out = parent[..., 3:3 + c].movedim(-1, 1)
        f, _ = cases.place(feat, size, "cl", dtype, DEV)
        assert out.stride(1) == 1 and out.stride(-1) == cw and cw % 2 == 1
    else:
        wide = size[-1] + 4 + (1 - size[-1] % 2)   # odd
        parent = _pattern((bs, c, size[0] + 3, wide), dtype)
        out = parent[:, :, 1:1 + size[0], 2:2 + size[1]]
        f, _ = cases.place(feat, size, "nchw", dtype, DEV)
        assert wide % 2 == 1 and out.storage_offset() % 2 == 1
    if dtype == torch.float32:
        assert cases.launch_path(dtype, c, bs * case.n, f.stride(1), out.stride(1))[0] == ("rows" if kind == "cl_slice" else "points")
    out.zero_()
    before = parent.clone()
    idx = _idx(cell)
    ops.voxel_maxpool_fwd(f, _ind(ind, dtype), out, size, case.scale, voxel_max_idx=idx)
    assert cases.same(out.cpu().numpy(), want)
    assert np.array_equal(idx.cpu().numpy(), cases.cell_offsets(cell, size, out))
    out.zero_()
    ints = INT_VIEW[parent.element_size()]
    assert torch.equal(parent.view(ints), before.view(ints))


# ------------------------------------------------------------------------------------------
# float16 / float64: the generic kernels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "cl", "sliced"])
@pytest.mark.parametrize("sign", ["mixed", "neg"])
@pytest.mark.parametrize("c", cases.C_GENERIC)
@pytest.mark.parametrize("dtype", ["f16", "f64"])
def test_half_and_double_forward_and_backward(dtype, c, sign, layout):
    case = cases.matrix_case(sign, c)
    _forward(case, layout, DTYPES[dtype])
    _backward(case, layout, DTYPES[dtype])


# ------------------------------------------------------------------------------------------
# backward, float32
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "cl", "sliced"])
@pytest.mark.parametrize("sign", ["relu", "mixed", "neg"])
@pytest.mark.parametrize("c", [1, 9, 20, 71])
def test_backward_float32(c, sign, layout):
    """In (b) grad_out has out's channels-last strides and grad_feat feat's point-major ones.  grad_feat starts as a sentinel,
    not 0: the kernel writes winners only, which is the contract VoxelMaxPoolFunction.backward relies on when it zero-fills."""
    _backward(cases.matrix_case(sign, c), layout)


@pytest.mark.parametrize("name", ["d1", "d3", "d4", "n1", "sparse"])
def test_backward_float32_shapes(name):
    _backward(cases.shape_case(name), "nchw")
    _backward(cases.shape_case(name), "cl")


# ------------------------------------------------------------------------------------------
# grid-stride sweeps
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
def test_sweep_of_1_1_million_points_forward(dtype):
    """More points than one sweep of vmp_fwd_points (1 048 576) and two of vmp_fwd_signed / vmp_fwd_generic (524 288)."""
    _forward(cases.sweep_case("sweep_points"), "nchw", DTYPES[dtype])


def test_sweep_of_1_1_million_points_backward():
    _backward(cases.sweep_case("sweep_points"), "nchw")


def test_sweep_of_the_rows_kernel():
    """vmp_fwd_rows<64> covers 16 384 points per sweep: 40 000 points, all-negative cells, with voxel_max_idx."""
    case = cases.sweep_case("sweep_rows")
    assert cases.path_of(case, "cl") == ("rows", 64, None)
    _forward(case, "cl")


# ------------------------------------------------------------------------------------------
# the autograd function
# ------------------------------------------------------------------------------------------
def _point_major_inputs(case):
    buf = torch.from_numpy(np.ascontiguousarray(case.feat.transpose(0, 2, 1))).to(DEV)          # [BS,N,C]
    ind = _ind(case.ind, torch.float32).unsqueeze(-1)
    go_np = cases._rng(case.name + "/grad").normal(0.0, 1.0, case.out.shape).astype(np.float32)
    return buf, ind, go_np


def test_autograd_function_on_a_non_contiguous_view():
    case = cases.matrix_case("mixed", 20)
    buf, ind, go_np = _point_major_inputs(case)
    buf.requires_grad_(True)
    f = buf.permute(0, 2, 1).unsqueeze(-1)                                # [BS,C,N,1] view of the point-major buffer
    assert not f.is_contiguous()
    y = deep_point.VoxelMaxPool(f, ind, case.size, case.scale)
    assert y.requires_grad and cases.same(y.detach().cpu().numpy(), case.out)
    y.backward(torch.from_numpy(go_np).to(DEV))
    want = cases.grad_ref(case.feat, case.cell, case.out, go_np)
    assert cases.same(buf.grad.permute(0, 2, 1).cpu().numpy(), want)     # losers and dropped points: exactly 0
    y2 = deep_point.VoxelMaxPool(buf.detach().permute(0, 2, 1).unsqueeze(-1), ind, case.size, case.scale)
    assert not y2.requires_grad and y2.grad_fn is None and torch.equal(y2.view(torch.int32), y.detach().view(torch.int32))


def test_autograd_function_returns_no_gradient_nobody_needs():
    """needs_input_grad[0] == False (only the coordinates ask for a gradient, which the operator does not have): backward
    returns None for every input."""
    case = cases.matrix_case("mixed", 20)
    buf, ind, go_np = _point_major_inputs(case)
    ind.requires_grad_(True)
    f = buf.permute(0, 2, 1).unsqueeze(-1)
    y = deep_point.VoxelMaxPool(f, ind, case.size, case.scale)
    assert y.requires_grad
    y.backward(torch.from_numpy(go_np).to(DEV))
    assert ind.grad is None and buf.grad is None
    ctx = type("Ctx", (), {"needs_input_grad": (False, False, False, False)})()
    assert deep_point.VoxelMaxPoolFunction.backward(ctx, None) == (None, None, None, None)


def test_autograd_function_is_bit_identical_from_run_to_run():
    """Fast kernel + exact path on a chunked case, forward and backward twice.  (float32: the second pass of the exact path
    ends a cell whose largest member is a zero as +0 whichever member the racing store of the first pass left.)"""
    case = cases.matrix_case("mixed", 20)
    runs = []
    for _ in range(2):
        f = torch.from_numpy(case.feat).to(DEV).unsqueeze(-1).requires_grad_(True)
        y = deep_point.VoxelMaxPool(f, _ind(case.ind, torch.float32).unsqueeze(-1), case.size, case.scale)
        y.backward(torch.from_numpy(cases._rng("again").normal(0.0, 1.0, case.out.shape).astype(np.float32)).to(DEV))
        runs.append((y.detach().view(torch.int32).clone(), f.grad.view(torch.int32).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert cases.same(runs[0][0].view(torch.float32).cpu().numpy(), case.out)


# ------------------------------------------------------------------------------------------
# bindings and refusals
# ------------------------------------------------------------------------------------------
def _binding(kind):
    if kind == "pybind":
        from streammos_amd.refapi import compiled
        return compiled.load("point_deep_cuda_kernel")
    from streammos_amd.refapi.point_deep import cuda_kernel
    return cuda_kernel


@pytest.mark.parametrize("binding", ["ctypes", "pybind"])
def test_point_deep_cuda_kernel_on_a_chunked_case(binding):
    """C = 20, mixed signs, with voxel_max_idx, through both spellings of point_deep.cuda_kernel with the reference's argument
    lists (caller-allocated zero / -1 filled buffers, the four small meta tensors on the device)."""
    cuda_kernel = _binding(binding)
    case = cases.matrix_case("mixed", 20)
    pcds_feat = torch.from_numpy(case.feat).to(DEV).unsqueeze(-1)
    pcds_ind = _ind(case.ind, torch.float32).unsqueeze(-1)
    voxel_out_shape = [pcds_feat.size(0), pcds_feat.size(1)] + list(case.size)
    voxel_out = torch.zeros(voxel_out_shape, dtype=pcds_feat.dtype, device=pcds_feat.device)
    voxel_max_idx = torch.full([pcds_ind.size(0), pcds_ind.size(1)], -1, dtype=torch.int64, device=pcds_feat.device)
    voxel_out_size_pt = torch.LongTensor(voxel_out_shape).to(pcds_feat.device)
    voxel_out_stride_pt = torch.LongTensor(voxel_out.stride()).to(pcds_feat.device)
    output_size_pt = voxel_out_size_pt[2:]
    scale_rate_pt = torch.FloatTensor(list(case.scale)).to(pcds_feat.device)
    cuda_kernel.voxel_maxpooling_forward(pcds_feat, pcds_ind, voxel_out, voxel_max_idx, voxel_out_size_pt, voxel_out_stride_pt,
                                         output_size_pt, scale_rate_pt)
    assert cases.same(voxel_out.cpu().numpy(), case.out)
    assert np.array_equal(voxel_max_idx.cpu().numpy(), cases.cell_offsets(case.cell, case.size, voxel_out))
    go_np = cases._rng(case.name + "/grad").normal(0.0, 1.0, case.out.shape).astype(np.float32)
    grad_voxel_out = torch.from_numpy(go_np).to(DEV)
    grad_pcds_feat = torch.zeros(pcds_feat.shape, dtype=grad_voxel_out.dtype, device=grad_voxel_out.device)
    cuda_kernel.voxel_maxpooling_backward(pcds_feat, pcds_ind, voxel_out, voxel_max_idx, grad_pcds_feat, grad_voxel_out,
                                          voxel_out_size_pt, voxel_out_stride_pt, output_size_pt, scale_rate_pt)
    assert cases.same(grad_pcds_feat[..., 0].cpu().numpy(), cases.grad_ref(case.feat, case.cell, case.out, go_np))


def test_refusals_leave_the_output_untouched():
    case = cases.matrix_case("mixed", 9)
    f, ind = torch.from_numpy(case.feat).to(DEV), _ind(case.ind, torch.float32)
    for shape, idx_dtype in (((case.bs, case.c) + case.size[::-1], torch.int64), ((case.bs, case.c) + case.size, torch.int32)):
        out = torch.full(shape, SENTINEL, device=DEV)
        with pytest.raises(RuntimeError):
            ops.voxel_maxpool_fwd(f, ind, out, case.size, case.scale, voxel_max_idx=torch.full(case.cell.shape, -1, dtype=idx_dtype, device=DEV))
        assert bool((out == SENTINEL).all())
    ind5 = torch.ones((case.bs, case.n, 5), device=DEV)                   # D = 5: every point would land in cell (1, 1, 1, 1, 1)
    out = torch.full((case.bs, case.c, 2, 2, 2, 2, 2), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="D=5"):
        ops.voxel_maxpool_fwd(f, ind5, out, (2,) * 5, (1.0,) * 5)
    gf = torch.full(f.shape, SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="D=5"):
        ops.voxel_maxpool_bwd(f, ind5, out, out.clone(), gf, (2,) * 5, (1.0,) * 5)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((gf == SENTINEL).all())

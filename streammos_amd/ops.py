"""Tensor-level entry points of the HIP kernels (torch tensors in, C ABI underneath).

torch is used for device memory and streams only: every function launches on
``torch.cuda.current_stream`` of the tensors' device and returns without synchronising.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _lib, profiling
from .scratch import _NO_GUARD, _dev_index, _on, _raw_stream, _stream, shared       # noqa: F401 (tests and tools use them by these names)
from .scratch import release as release_stream_workspaces       # noqa: F401 (the public name: StreamRunner.close() calls it)

_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.float64: 2}


def env_on(text):
    """The one spelling rule of the boolean switches: None (unset) or empty -> None (not set); 0 / false / off / no, whatever
    the case or surrounding whitespace -> False; anything else -> True."""
    text = (text or "").strip().lower()
    return None if text == "" else text not in ("0", "false", "off", "no")


class Switch:
    """A process-wide A/B switch, resolved on every call: the explicit ``set`` setting if there is one, else the environment
    variable if it is set (``env_on``), else ``fallback()`` if there is one, else the default."""
    __slots__ = ("var", "default", "fallback", "explicit")

    def __init__(self, var, default, fallback=None):
        self.var, self.default, self.fallback, self.explicit = var, default, fallback, None

    def __call__(self):
        if self.explicit is not None:
            return self.explicit
        on = env_on(os.environ.get(self.var))
        if on is None:
            on = bool(self.fallback()) if self.fallback is not None else self.default
        return on

    def set(self, flag):
        """True / False, or None to hand the decision back to the environment.  Returns the previous explicit setting."""
        prev, self.explicit = self.explicit, (None if flag is None else bool(flag))
        return prev


# Whether bilinear_gather_backward and msda_bwd (and so the autograd nodes over them) sum in a fixed order (csrc/segsum.hip)
# when their ``deterministic`` argument is None; torch's own flag (looked up at call time) speaks where nothing else does.
is_deterministic = Switch("SMOS_DETERMINISTIC", False, lambda: torch.are_deterministic_algorithms_enabled())
# Whether PointNetStacker.forward (refapi/networks/backbone.py) may route a supported configuration to point_mlp_train,
point_mlp_fused = Switch("SMOS_POINT_MLP", False)
# backbone.point_head a supported CatFusion + PredBranch pair to point_head_train,
point_head_fused = Switch("SMOS_POINT_HEAD_TRAIN", False)
# and CENet_Transformer.forward (refapi/networks/multi_view_encoder.py) the decoder's conv_1 to upconv3x3_train.
conv1_fused = Switch("SMOS_CONV1_TRAIN", False)
# Whether BilinearSample trains through the own backward kernel (off: an A/B against F.grid_sample).
bilinear_bwd_own = Switch("SMOS_BILINEAR_BWD", True)
set_deterministic, set_point_mlp_fused, set_point_head_fused = is_deterministic.set, point_mlp_fused.set, point_head_fused.set
# Whether CENet_Transformer._cross_view may send its four transfers (BilinearSample -> VoxelMaxPool) to gather_scatter_train.
cross_view_fused = Switch("SMOS_CROSS_VIEW_TRAIN", False)
set_conv1_fused, set_bilinear_bwd_own, set_cross_view_fused = conv1_fused.set, bilinear_bwd_own.set, cross_view_fused.set


def _require_cuda(name, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("%s: expected a tensor in GPU memory, got device=%s (no CPU path here)" % (name, t.device))


def _ptr(t):
    """address of an optional tensor (None where it is absent)"""
    return None if t is None else t.data_ptr()


def _live_ptr(name, n_live):
    """address of the optional ``n_live`` count of a wrapper: a device int32 tensor whose first element is read"""
    if n_live is None:
        return None
    if n_live.dtype != torch.int32 or n_live.numel() < 1:
        raise RuntimeError("%s: n_live must be a device int32 tensor" % name)
    return n_live.data_ptr()


def _dtype_code(name, t):
    code = _DTYPE_CODE.get(t.dtype)
    if code is None:
        raise RuntimeError("%s: unsupported dtype %s" % (name, t.dtype))
    return code


def voxel_maxpool_fwd(feat, ind, out, out_size, scale, voxel_max_idx=None):
    """feat [BS,C,N(,1)] any strides, ind [BS,N,D(,1)] contiguous, out [BS,C,*out_size] zero-filled."""
    _require_cuda("voxel_maxpool_fwd", feat, ind, out, voxel_max_idx)
    if feat.dtype != ind.dtype or feat.dtype != out.dtype:
        raise RuntimeError("voxel_maxpool_fwd: feat/ind/out dtypes differ (%s, %s, %s)" % (feat.dtype, ind.dtype, out.dtype))
    if not ind.is_contiguous():
        raise RuntimeError("voxel_maxpool_fwd: pcds_ind must be contiguous")
    bs, c, n = feat.shape[0], feat.shape[1], feat.shape[2]
    d = ind.shape[2]
    if len(out_size) != d or len(scale) != d or ind.shape[0] != bs or ind.shape[1] != n:
        raise RuntimeError("voxel_maxpool_fwd: shape mismatch feat %s ind %s out_size %s" % (tuple(feat.shape), tuple(ind.shape), tuple(out_size)))
    if tuple(out.shape) != (bs, c) + tuple(int(s) for s in out_size):
        raise RuntimeError("voxel_maxpool_fwd: out has shape %s" % (tuple(out.shape),))
    if voxel_max_idx is not None and (voxel_max_idx.dtype != torch.int64 or not voxel_max_idx.is_contiguous()):
        raise RuntimeError("voxel_maxpool_fwd: voxel_max_idx must be contiguous int64")
    label = "voxel_maxpool_fwd[%dx%dx%d->%s]" % (bs, c, n, "x".join(str(int(s)) for s in out_size))
    flag = shared.get("maxpool_flag", (4,), torch.int32, feat.device, zero=True)    # the scatter's "saw a negative feature" word
    with _on(feat.device), profiling.span(label):
        _lib.call("smos_voxel_maxpool_fwd", feat.data_ptr(), _lib.i64_array(feat.stride()[:3]), ind.data_ptr(), out.data_ptr(),
                  _lib.i64_array(out.stride()), _ptr(voxel_max_idx), bs, c, n, d, _lib.i64_array(out_size), _lib.f32_array(scale),
                  _dtype_code("voxel_maxpool_fwd", feat), flag.data_ptr(), _stream(feat))
    return out


def voxel_maxpool_bwd(feat, ind, out, grad_out, grad_feat, out_size, scale):
    _require_cuda("voxel_maxpool_bwd", feat, ind, out, grad_out, grad_feat)
    # grad_out is read with out's strides and grad_feat written with feat's: same logical layout required
    # (strides of size-1 dims are arbitrary, so compare through contiguity / explicit equality on real dims)
    def _same_layout(a, b):
        return all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)
    if not _same_layout(grad_out, out):
        grad_out = grad_out.contiguous()
        if not _same_layout(grad_out, out):
            raise RuntimeError("voxel_maxpool_bwd: grad_out layout must match out")
    if not _same_layout(grad_feat, feat):
        raise RuntimeError("voxel_maxpool_bwd: grad_feat layout must match feat")
    bs, c, n = feat.shape[0], feat.shape[1], feat.shape[2]
    with _on(feat.device):
        _lib.call("smos_voxel_maxpool_bwd", feat.data_ptr(), _lib.i64_array(feat.stride()[:3]), ind.data_ptr(), out.data_ptr(),
                  grad_out.data_ptr(), _lib.i64_array(out.stride()), grad_feat.data_ptr(), bs, c, n, ind.shape[2],
                  _lib.i64_array(out_size), _lib.f32_array(scale), _dtype_code("voxel_maxpool_bwd", feat), _stream(feat))
    return grad_feat


def segsum_chunk():
    """Terms per chunk of the fixed-order sums (tests place their edge cases around it)."""
    return _lib.query("smos_segsum_chunk")


def _bilinear_gather_fwd(grid, coord, scale, out, point_major):
    if coord.dim() == 4:
        coord = coord[..., 0]
    if not coord.is_contiguous():
        coord = coord.contiguous()
    b, c, h, w = grid.shape
    n, k = coord.shape[1], coord.shape[2]
    if out is None:
        if point_major:
            out = torch.empty((b, n, c), dtype=torch.float32, device=grid.device).permute(0, 2, 1)
        else:
            out = torch.empty((b, c, n), dtype=torch.float32, device=grid.device)
    with _on(grid.device), profiling.span_f("bilinear_gather[%dx%dx%dx%d->%d]", (b, c, h, w, n)):
        _lib.call("smos_bilinear_gather_fwd", grid.data_ptr(), _lib.i64_array(grid.stride()), coord.data_ptr(), k, out.data_ptr(),
                  _lib.i64_array(out.stride()[:3]), b, c, h, w, n, _lib.f32_array(scale), _stream(grid))
    return out


def bilinear_gather_backward(grad_out, coord, scale, grid_shape, channels_last=True, deterministic=None):
    """Gradient of ``bilinear_gather`` with respect to its grid (csrc/bilinear_gather.hip, smos_bilinear_gather_bwd).

    grad_out [B,C,N] (any strides: channel-major from the module graph, point-major from a point-major forward),
    coord [B,N,K(,1)], grid_shape (B,C,H,W) or (H,W) -> grad_grid [B,C,H,W].  With ``channels_last`` the result is a
    permuted view of a [B,H,W,C] buffer, which the kernel adds to in whole rows; otherwise it is NCHW-contiguous and
    every (point, tap, channel) is a 4-byte atomic.  The kernel zeroes the result itself.  The sums are float atomics:
    their last bits depend on arrival order.

    ``deterministic`` (None: ``is_deterministic()``): the store-and-sum form smos_bilinear_gather_bwd_det of csrc/segsum.hip
    instead, for either layout of the result: no atomics, a defined float32 sum per element, the same bits on every run."""
    _require_cuda("bilinear_gather_backward", grad_out, coord)
    if grad_out.dtype != torch.float32 or coord.dtype != torch.float32:
        raise RuntimeError("bilinear_gather_backward: float32 only (got %s, %s)" % (grad_out.dtype, coord.dtype))
    if coord.dim() == 4:
        coord = coord[..., 0]
    if grad_out.dim() == 4:
        grad_out = grad_out[..., 0]
    if not coord.is_contiguous():
        coord = coord.contiguous()
    b, c, n = grad_out.shape
    h, w = int(grid_shape[-2]), int(grid_shape[-1])
    k = coord.shape[2]
    if coord.shape[0] != b or coord.shape[1] != n or (len(grid_shape) == 4 and (int(grid_shape[0]), int(grid_shape[1])) != (b, c)):
        raise RuntimeError("bilinear_gather_backward: shape mismatch grad_out %s coord %s grid %s"
                           % (tuple(grad_out.shape), tuple(coord.shape), tuple(grid_shape)))
    if channels_last:
        grad_grid = torch.empty((b, h, w, c), dtype=torch.float32, device=grad_out.device).permute(0, 3, 1, 2)
    else:
        grad_grid = torch.empty((b, c, h, w), dtype=torch.float32, device=grad_out.device)
    if is_deterministic() if deterministic is None else deterministic:
        need = _lib.query("smos_bilinear_gather_bwd_det_work_bytes", b, c, h, w, n)
        if need < 0:
            raise RuntimeError("bilinear_gather_backward: the deterministic form takes B * N < 2^29 points and B * H * W < 2^31 - 1 "
                               "pixels (got %d, %d)" % (b * n, b * h * w))
        with _on(grad_out.device), profiling.span_f("bilinear_gather_bwd_det[%dx%dx%dx%d<-%d]", (b, c, h, w, n)):
            work = torch.empty((need,), dtype=torch.uint8, device=grad_out.device)     # on the current stream, like grad_grid
            _lib.call("smos_bilinear_gather_bwd_det", grad_out.data_ptr(), _lib.i64_array(grad_out.stride()), coord.data_ptr(), k,
                      grad_grid.data_ptr(), _lib.i64_array(grad_grid.stride()), b, c, h, w, n, _lib.f32_array(scale),
                      work.data_ptr(), need, _stream(grad_out))
        return grad_grid
    with _on(grad_out.device), profiling.span_f("bilinear_gather_bwd[%dx%dx%dx%d<-%d]", (b, c, h, w, n)):
        _lib.call("smos_bilinear_gather_bwd", grad_out.data_ptr(), _lib.i64_array(grad_out.stride()), coord.data_ptr(), k,
                  grad_grid.data_ptr(), _lib.i64_array(grad_grid.stride()), b, c, h, w, n, _lib.f32_array(scale), _stream(grad_out))
    return grad_grid


class _BilinearGather(torch.autograd.Function):
    """bilinear_gather, differentiable in grid.  ``out`` travels inside a tuple: autograd then sees no tensor that is both an
    input and modified, and the result is an alias of it that carries the graph."""

    @staticmethod
    def forward(ctx, grid, coord, scale, out_box, point_major):
        ctx.save_for_backward(coord)
        ctx.scale, ctx.grid_shape = tuple(float(v) for v in scale), tuple(grid.shape)
        res = _bilinear_gather_fwd(grid, coord, scale, out_box[0], point_major)
        return res.detach() if out_box[0] is not None else res

    @staticmethod
    def backward(ctx, grad_out):
        coord, = ctx.saved_tensors
        # handed on channels-last-strided, as written: an NCHW copy made the training step longer
        return bilinear_gather_backward(grad_out, coord, ctx.scale, ctx.grid_shape, channels_last=True), None, None, None, None


def bilinear_gather(grid, coord, scale, out=None, point_major=False):
    """grid [B,C,H,W] (any strides), coord [B,N,K(,1)] -> out [B,C,N] (a view of a [B,N,C] buffer when
    point_major).  Differentiable in ``grid`` (``bilinear_gather_backward``); with ``out=`` the returned tensor shares
    ``out``'s memory and is the one that carries the graph.  There is no gradient with respect to ``coord``."""
    grad_mode = torch.is_grad_enabled()
    if grad_mode and coord.requires_grad:
        raise RuntimeError("bilinear_gather: no gradient with respect to coord (the coordinates are data); detach it")
    _require_cuda("bilinear_gather", grid, coord, out)
    if grid.dtype != torch.float32 or coord.dtype != torch.float32:
        raise RuntimeError("bilinear_gather: float32 only (got %s, %s)" % (grid.dtype, coord.dtype))
    if grad_mode and grid.requires_grad:
        return _BilinearGather.apply(grid, coord, scale, (out,), point_major)
    return _bilinear_gather_fwd(grid, coord, scale, out, point_major)


def _gst_coord(t):
    """[B,N,K(,1)] coordinates as the contiguous [B,N,K] the kernels read"""
    if t.dim() == 4:
        t = t[..., 0]
    return t if t.is_contiguous() else t.contiguous()


def _gst_common(grid, gcoord, gscale, scoord, sscale, out):
    """The leading arguments of the three smos_gather_scatter_train_* entries up to out's strides, and their trailing sizes."""
    b, c, hg, wg = grid.shape
    head = (grid.data_ptr(), _lib.i64_array(grid.stride()), gcoord.data_ptr(), gcoord.shape[2], _lib.f32_array(gscale),
            scoord.data_ptr(), scoord.shape[2], _lib.f32_array(sscale), out.data_ptr(), _lib.i64_array(out.stride()))
    return head, (b, c, hg, wg, gcoord.shape[1], out.shape[2], out.shape[3])


def _gst_strides(t):
    return None if t is None else _lib.i64_array(t.stride())


def _gather_scatter_train_fwd(grid, gcoord, gscale, scoord, out_size, sscale, want_points):
    b, c = grid.shape[:2]
    n = gcoord.shape[1]
    out = torch.zeros((b, c) + out_size, dtype=torch.float32, device=grid.device)
    pts = torch.empty((b, c, n), dtype=torch.float32, device=grid.device) if want_points else None
    flag = shared.get("maxpool_flag", (4,), torch.int32, grid.device, zero=True)
    head, sizes = _gst_common(grid, gcoord, gscale, scoord, sscale, out)
    with _on(grid.device), profiling.span_f("gather_scatter_train_fwd[%dx%dx%dx%d->%d->%dx%d]", sizes):
        _lib.call("smos_gather_scatter_train_fwd", *head, _ptr(pts), _gst_strides(pts), *sizes, flag.data_ptr(), _stream(grid))
    return out, pts


def gather_scatter_train_point_grad(grid, gcoord, gscale, scoord, sscale, out, grad_out, grad_pts=None, x=None):
    """The gradient of the point values of ``gather_scatter_train`` as a tensor x [B,C,N] (smos_gather_scatter_train_point_grad):
    grad_out at the point's cell where the point is kept and its recomputed value equals ``out`` there, else 0, plus
    ``grad_pts``.  x: where to write it (any strides), else a fresh tensor."""
    _require_cuda("gather_scatter_train_point_grad", grid, gcoord, scoord, out, grad_out, grad_pts, x)
    gcoord, scoord = _gst_coord(gcoord), _gst_coord(scoord)
    head, sizes = _gst_common(grid, gcoord, gscale, scoord, sscale, out)
    if x is None:
        x = torch.empty((sizes[0], sizes[1], sizes[4]), dtype=torch.float32, device=grid.device)
    with _on(grid.device), profiling.span_f("gather_scatter_train_point_grad[%dx%dx%dx%d->%d->%dx%d]", sizes):
        _lib.call("smos_gather_scatter_train_point_grad", *head, grad_out.data_ptr(), _lib.i64_array(grad_out.stride()),
                  _ptr(grad_pts), _gst_strides(grad_pts), x.data_ptr(), _lib.i64_array(x.stride()), *sizes, _stream(grid))
    return x


def gather_scatter_train_backward(grid, gcoord, gscale, scoord, sscale, out, grad_out, grad_pts=None, channels_last=True,
                                  deterministic=None):
    """Gradient of ``gather_scatter_train`` with respect to its grid, [B,C,Hg,Wg]: channels-last strides (row atomics) or
    NCHW-contiguous (4-byte atomics), as ``bilinear_gather_backward``.  One launch (smos_gather_scatter_train_bwd; a run of
    points whose sum is exactly 0 issues no atomic), or with ``deterministic`` (None: ``is_deterministic()``) the point
    gradient into scratch (``gather_scatter_train_point_grad``) and the fixed-order sum of ``bilinear_gather_backward``: the
    bits of the module path in that mode."""
    _require_cuda("gather_scatter_train_backward", grid, gcoord, scoord, out, grad_out, grad_pts)
    gcoord, scoord = _gst_coord(gcoord), _gst_coord(scoord)
    head, sizes = _gst_common(grid, gcoord, gscale, scoord, sscale, out)
    b, c, hg, wg, n = sizes[:5]
    if is_deterministic() if deterministic is None else deterministic:
        x = shared.get("cross_view_point_grad", (b, c, n), torch.float32, grid.device)
        gather_scatter_train_point_grad(grid, gcoord, gscale, scoord, sscale, out, grad_out, grad_pts, x=x)
        return bilinear_gather_backward(x, gcoord, gscale, (b, c, hg, wg), channels_last=channels_last, deterministic=True)
    if channels_last:
        grad_grid = torch.empty((b, hg, wg, c), dtype=torch.float32, device=grid.device).permute(0, 3, 1, 2)
    else:
        grad_grid = torch.empty((b, c, hg, wg), dtype=torch.float32, device=grid.device)
    with _on(grid.device), profiling.span_f("gather_scatter_train_bwd[%dx%dx%dx%d<-%d<-%dx%d]", sizes):
        _lib.call("smos_gather_scatter_train_bwd", *head, grad_out.data_ptr(), _lib.i64_array(grad_out.stride()), _ptr(grad_pts),
                  _gst_strides(grad_pts), grad_grid.data_ptr(), _lib.i64_array(grad_grid.stride()), *sizes, _stream(grid))
    return grad_grid


class _GatherScatterTrain(torch.autograd.Function):
    """ops.gather_scatter_train.  Kept for the backward: the source grid, the two coordinate tensors and out -- never a
    [B,C,N] tensor; nothing at all where grid needs no gradient."""

    @staticmethod
    def forward(ctx, grid, gcoord, scoord, gscale, out_size, sscale, want_points):
        out, pts = _gather_scatter_train_fwd(grid, gcoord, gscale, scoord, out_size, sscale, want_points)
        ctx.set_materialize_grads(False)           # a result nobody used arrives as None, not as a [B,C,N] tensor of zeros
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(grid, gcoord, scoord, out)
            ctx.scales = (gscale, sscale)
        return (out, pts) if want_points else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, grad_pts=None):
        if grad_out is None and grad_pts is None:
            return (None,) * 7
        grid, gcoord, scoord, out = ctx.saved_tensors
        gscale, sscale = ctx.scales
        if grad_out is None:                       # only the point values were used
            grad_out = torch.zeros_like(out)
        return (gather_scatter_train_backward(grid, gcoord, gscale, scoord, sscale, out, grad_out, grad_pts),
                None, None, None, None, None, None)


def gather_scatter_train(grid, gcoord, gscale, scoord, out_size, sscale, want_points=False):
    """One cross-view transfer of training as one autograd op: ``BilinearSample(scale_rate=gscale)(grid,
    gcoord)`` followed by ``VoxelMaxPool(., scoord, out_size, sscale)``, to the bit, without the [B,C,N] tensor between them.

    grid [B,C,Hg,Wg] float32 on the GPU, any strides; gcoord, scoord [B,N,K>=2(,1)] float32, without gradient; out_size
    (Ho, Wo).  Returns out [B,C,Ho,Wo] (NCHW-contiguous), or (out, pts [B,C,N]) with ``want_points``: the gathered values,
    which carry the graph too.  The backward recomputes each point's value from the saved grid, takes the gradient of the
    cells the point wins and adds the rows of winners only (``gather_scatter_train_backward``); it returns the gradient of
    grid with channels-last strides, like ``bilinear_gather``'s."""
    name = "gather_scatter_train"
    _require_cuda(name, grid, gcoord, scoord)
    if grid.dtype != torch.float32 or gcoord.dtype != torch.float32 or scoord.dtype != torch.float32:
        raise RuntimeError("%s: float32 only (got %s, %s, %s)" % (name, grid.dtype, gcoord.dtype, scoord.dtype))
    if gcoord.requires_grad or scoord.requires_grad:
        raise RuntimeError("%s: no gradient with respect to the coordinates (they are data); detach them" % name)
    gcoord, scoord = _gst_coord(gcoord), _gst_coord(scoord)
    out_size = tuple(int(v) for v in out_size)
    gscale, sscale = tuple(float(v) for v in gscale), tuple(float(v) for v in sscale)
    if (grid.dim() != 4 or gcoord.dim() != 3 or scoord.dim() != 3 or gcoord.shape[0] != grid.shape[0] or gcoord.shape[2] < 2
            or scoord.shape[2] < 2 or tuple(scoord.shape[:2]) != tuple(gcoord.shape[:2]) or len(out_size) != 2 or len(gscale) != 2
            or len(sscale) != 2 or min(out_size) < 1 or grid.shape[2] < 1 or grid.shape[3] < 1):
        raise RuntimeError("%s: shape mismatch grid %s gcoord %s scoord %s out_size %s"
                           % (name, tuple(grid.shape), tuple(gcoord.shape), tuple(scoord.shape), out_size))
    if gcoord.device != grid.device or scoord.device != grid.device:
        raise RuntimeError("%s: coordinates on %s / %s, grid on %s" % (name, gcoord.device, scoord.device, grid.device))
    if torch.is_grad_enabled() and grid.requires_grad:
        return _GatherScatterTrain.apply(grid, gcoord, scoord, gscale, out_size, sscale, bool(want_points))
    out, pts = _gather_scatter_train_fwd(grid, gcoord, gscale, scoord, out_size, sscale, bool(want_points))
    return (out, pts) if want_points else out


def seg_loss_tile():
    """Elements per block of the scan kernels of ``seg_loss`` (tests place their edge cases around it)."""
    return _lib.query("smos_seg_loss_tile")


def _seg_loss_args(name, pred, target):
    """-> pred as [B, C, P] (a view, strides kept), target as contiguous int64 [B, P]."""
    _require_cuda(name, pred, target)
    if pred.dtype != torch.float32:
        raise RuntimeError("%s: float32 logits only (got %s)" % (name, pred.dtype))
    if target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
        raise RuntimeError("%s: integer labels only (got %s)" % (name, target.dtype))
    if pred.dim() == 4 and pred.shape[3] == 1:
        pred = pred[..., 0]
    if target.dim() == 3 and target.shape[2] == 1:
        target = target[..., 0]
    if pred.dim() != 3 or target.dim() != 2 or pred.shape[0] != target.shape[0] or pred.shape[2] != target.shape[1]:
        raise RuntimeError("%s: shape mismatch pred %s target %s (want [B,C,P(,1)] and [B,P(,1)])"
                           % (name, tuple(pred.shape), tuple(target.shape)))
    if pred.shape[1] not in (2, 3):
        raise RuntimeError("%s: %d classes; the kernels are built for C = 2 and C = 3" % (name, pred.shape[1]))
    if pred.shape[0] * pred.shape[2] == 0:
        raise RuntimeError("%s: no positions (pred %s)" % (name, tuple(pred.shape)))
    if target.device != pred.device:
        raise RuntimeError("%s: pred on %s, target on %s" % (name, pred.device, target.device))
    return pred, target.to(torch.int64).contiguous()        # labels are small next to the logits; no copy in the usual case


class _SegLoss(torch.autograd.Function):
    """ops.seg_loss: two foreign calls, one per direction.  What the backward needs beyond pred and target is the
    [C + 1, n] coefficient table and the present-class count, both left on the device by the forward."""

    @staticmethod
    def forward(ctx, pred, target, k, top_weight, ignore_index, lovasz_weight):
        p3 = pred[..., 0] if pred.dim() == 4 else pred
        b, c, p = p3.shape
        n = b * p
        need = _lib.query("smos_seg_loss_work_bytes", n, c)
        if need <= 0:
            raise RuntimeError("seg_loss: %d positions x %d classes is more than the sort is set up for" % (n, c))
        dev = pred.device
        work = shared.get("seg_loss", (need,), torch.uint8, dev)
        coef = torch.empty((c + 1, n), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.float32, device=dev)
        with _on(dev), profiling.span_f("seg_loss[%dx%dx%d]", (b, c, p)):
            _lib.call("smos_seg_loss_fwd", p3.data_ptr(), _lib.i64_array(p3.stride()), target.data_ptr(), b, c, p, k, top_weight,
                      lovasz_weight, ignore_index, coef.data_ptr(), loss.data_ptr(), stats.data_ptr(), work.data_ptr(), need,
                      _stream(pred))
        ctx.save_for_backward(pred, target, coef, stats)
        ctx.args = (k, float(top_weight), int(ignore_index), float(lovasz_weight))
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        pred, target, coef, stats = ctx.saved_tensors
        k, top_weight, ignore_index, lovasz_weight = ctx.args
        grad = torch.empty_like(pred)                 # pred's layout where pred is dense (the point head's view is)
        p3, g3 = (pred[..., 0], grad[..., 0]) if pred.dim() == 4 else (pred, grad)
        b, c, p = p3.shape
        go = grad_out.to(torch.float32).contiguous()
        with _on(pred.device), profiling.span_f("seg_loss_bwd[%dx%dx%d]", (b, c, p)):
            _lib.call("smos_seg_loss_bwd", p3.data_ptr(), _lib.i64_array(p3.stride()), target.data_ptr(), coef.data_ptr(),
                      stats.data_ptr(), go.data_ptr(), b, c, p, k, top_weight, lovasz_weight, ignore_index, g3.data_ptr(),
                      _lib.i64_array(g3.stride()), _stream(pred))
        return grad, None, None, None, None, None


def seg_loss(pred, target, top_ratio=0.2, top_weight=4.0, ignore_index=0, lovasz_weight=3.0):
    """``ohem_cross_entropy(pred, target, top_ratio, top_weight, ignore_index) + lovasz_weight * lovasz_softmax(pred, target,
    ignore=ignore_index)`` of refapi/models/losses.py as one 0-dim device tensor, differentiable in ``pred``
    (csrc/seg_loss.hip).  pred [B,C,P(,1)] float32 with any strides (read in place), C = 2 or 3; target [B,P(,1)] integer.
    Nothing is read back to the host in either direction: where every label is ignored the result is a zero tensor (the
    torch formulation returns the int 0 there) and the gradient is all zeros."""
    pred3, tgt = _seg_loss_args("seg_loss", pred, target)
    k = max(int(top_ratio * (pred3.shape[0] * pred3.shape[2])), 1)
    if torch.is_grad_enabled() and pred.requires_grad:
        return _SegLoss.apply(pred, tgt, k, float(top_weight), int(ignore_index), float(lovasz_weight))
    with torch.no_grad():
        return _SegLoss.apply(pred3, tgt, k, float(top_weight), int(ignore_index), float(lovasz_weight))


def point_mlp_chunk():
    """Points per chunk of partial sums of ``point_mlp_train`` (tests place their shapes around it)."""
    return _lib.query("smos_point_mlp_chunk")


# ---- what the two fused training ops (point_mlp_train, point_head_train) share; ``op`` is the prefix of their messages ----
def _ptr_array(tensors):
    return (_lib.vp * len(tensors))(*[_ptr(t) for t in tensors])


def _train_work(tag, query, points, dev):
    """(work buffer from the scratch registry, its bytes) for ``points`` points; (None, need <= 0) past the kernels' range."""
    need = _lib.query(query, points)
    return (shared.get(tag, (need,), torch.uint8, dev) if need > 0 else None), need


def _train_fold_dstat(abi, dev):
    """The folded block and the float64 statistics a forward leaves for its backward, sized by ``abi``'s two queries."""
    return (torch.empty(_lib.query(abi + "_fold_floats"), dtype=torch.float32, device=dev),
            torch.empty(_lib.query(abi + "_stat_doubles"), dtype=torch.float64, device=dev))


def _train_check_bns(op, pairs, first):
    for i, (bn, c) in enumerate(pairs, first):
        if bn.weight is None or bn.bias is None or bn.running_mean is None or bn.running_var is None or bn.momentum is None:
            raise RuntimeError("%s: bn%d must be affine, track running statistics and have a momentum" % (op, i))
        if bn.weight.numel() != c:
            raise RuntimeError("%s: bn%d has %d channels, want %d" % (op, i, bn.weight.numel(), c))


def _train_conv1x1(op, name, m, shape, rule, bias=False, allow_tensor=False):
    """The weight of the 1x1 convolution ``m`` [cout, cin(,1,1)] with or without a bias; ``rule`` ends the bias message."""
    is_module = isinstance(m, torch.nn.Module)
    if not is_module and not allow_tensor:
        raise RuntimeError("%s: %s must be the convolution module" % (op, name))
    if is_module and (getattr(m, "bias", None) is not None) != bias:
        raise RuntimeError("%s: %s %s a bias; %s" % (op, name, "lacks" if bias else "has", rule))
    w = m.weight if is_module else m
    if tuple(w.shape[:2]) != shape or w.numel() != shape[0] * shape[1]:
        raise RuntimeError("%s: %s is %s, want a 1x1 convolution %d -> %d" % (op, name, tuple(w.shape), shape[1], shape[0]))
    return w


def _train_check_tensors(op, tensors, dev):
    for t in tensors:
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("%s: parameters and buffers must be contiguous float32 tensors on %s" % (op, dev))


def _bn_eps_mom(bns):
    return tuple(float(bn.eps) for bn in bns) + tuple(float(bn.momentum) for bn in bns)


def _bn_count_batch(bns):
    for bn in bns:
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)


class _PointMlpTrain(torch.autograd.Function):
    """ops.point_mlp_train: one foreign call per direction.  Kept for the backward: x, the parameters, and the folded
    statistics the forward leaves on the device (a few thousand floats) -- no activation."""

    @staticmethod
    def forward(ctx, x, g0, b0, w1, g1, b1, w2, g2, b2, buffers, eps_mom, training):
        s, _, n = x.shape[:3]
        dev = x.device
        work, need = _train_work("point_mlp", "smos_point_mlp_work_bytes", s * n, dev)
        if need <= 0:
            raise RuntimeError("point_mlp_train: %d x %d points is more than the kernels are set up for" % (s, n))
        y = torch.empty((s, 64, n, 1), dtype=torch.float32, device=dev)
        fold, dstat = _train_fold_dstat("smos_point_mlp", dev)
        rm0, rv0, rm1, rv1, rm2, rv2 = buffers
        params = (g0, b0, rm0, rv0, w1, g1, b1, rm1, rv1, w2, g2, b2, rm2, rv2)
        with _on(dev), profiling.span_f("point_mlp_%s[%dx%d]", ("train" if training else "eval", s, n)):
            _lib.call("smos_point_mlp_fwd", x.data_ptr(), s, n, int(training), _ptr_array(params), _lib.f64_array(eps_mom),
                      y.data_ptr(), fold.data_ptr(), dstat.data_ptr(), work.data_ptr(), need, _stream(x))
        ctx.save_for_backward(x, g0, b0, w1, g1, b1, w2, g2, b2, fold, dstat)
        ctx.buffers, ctx.eps_mom, ctx.training = buffers, eps_mom, bool(training)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, g0, b0, w1, g1, b1, w2, g2, b2, fold, dstat = ctx.saved_tensors
        s, _, n = x.shape[:3]
        dev = x.device
        gy = grad_y.to(torch.float32).contiguous()
        rm0, rv0, rm1, rv1, rm2, rv2 = ctx.buffers
        params = (g0, b0, rm0, rv0, w1, g1, b1, rm1, rv1, w2, g2, b2, rm2, rv2)
        grads = [torch.empty_like(p) if ctx.needs_input_grad[1 + i] else None for i, p in enumerate((g0, b0, w1, g1, b1, w2, g2, b2))]
        if any(g is not None for g in grads):
            work, need = _train_work("point_mlp", "smos_point_mlp_work_bytes", s * n, dev)
            with _on(dev), profiling.span_f("point_mlp_bwd[%dx%d]", (s, n)):
                _lib.call("smos_point_mlp_bwd", x.data_ptr(), gy.data_ptr(), s, n, int(ctx.training), _ptr_array(params),
                          _lib.f64_array(ctx.eps_mom), fold.data_ptr(), dstat.data_ptr(), _ptr_array(grads), work.data_ptr(),
                          need, _stream(x))
        return (None, *grads, None, None, None)


def point_mlp_train(x, bn0, conv1, bn1, conv2, bn2, training=None):
    """BN0 -> 1x1 conv 7->64 -> BN1 -> ReLU -> 1x1 conv 64->64 -> BN2 -> ReLU of ``PointNetStacker(7, 64, pre_bn=True,
    stack_num=2)`` as one autograd op on the HIP kernels of csrc/point_mlp_train.hip.

    x [S,7,N(,1)] float32 on the GPU (no gradient flows to it); bn0/bn1/bn2 the BatchNorm modules (affine, with running
    statistics and a momentum); conv1/conv2 the bias-free 1x1 convolutions or their weights.  ``training`` (None:
    ``bn0.training``): batch statistics over all S*N points, the six running buffers and ``num_batches_tracked`` updated in
    place as the modules would; otherwise the running statistics.  Returns [S,64,N,1] float32; differentiable in the eight
    parameters.  Every sum runs in a fixed order (the bits do not depend on the grid or the run) and nothing is read back
    to the host."""
    _require_cuda("point_mlp_train", x)
    if x.dtype != torch.float32:
        raise RuntimeError("point_mlp_train: float32 only (got %s)" % x.dtype)
    if x.dim() == 3:
        x = x[..., None]
    if x.dim() != 4 or x.shape[1] != 7 or x.shape[3] != 1 or x.shape[0] * x.shape[2] == 0:
        raise RuntimeError("point_mlp_train: x is %s, want [S,7,N(,1)] with S*N > 0" % (tuple(x.shape),))
    training = bool(bn0.training if training is None else training)
    bns = (bn0, bn1, bn2)
    _train_check_bns("point_mlp_train", zip(bns, (7, 64, 64)), 0)
    rule = "the point MLP's convolutions have none"
    w1 = _train_conv1x1("point_mlp_train", "conv1", conv1, (64, 7), rule, allow_tensor=True)
    w2 = _train_conv1x1("point_mlp_train", "conv2", conv2, (64, 64), rule, allow_tensor=True)
    tensors = [bn0.weight, bn0.bias, w1, bn1.weight, bn1.bias, w2, bn2.weight, bn2.bias]
    buffers = tuple(b for bn in bns for b in (bn.running_mean, bn.running_var))
    _train_check_tensors("point_mlp_train", tensors + list(buffers), x.device)
    if training and x.shape[0] * x.shape[2] < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (x.shape,))
    y = _PointMlpTrain.apply(x.detach().contiguous(), *tensors, buffers, _bn_eps_mom(bns), training)
    if training:
        _bn_count_batch(bns)
    return y


def point_head_train_chunk():
    """Points per chunk of partial sums of ``point_head_train`` (tests place their shapes around it)."""
    return _lib.query("smos_point_head_train_chunk")


def _point_head_pitch(x):
    """floats between two channels of a [B,64,N,1] input the kernels can read in place, else None: points unit-strided, the
    channels of a sample and the samples equally spaced (a dense tensor, or one cut out of a longer point axis)."""
    b, c, n = x.shape[:3]
    sb, sc, sn = x.stride()[:3]
    pitch = sc if n > 1 or c > 1 else n
    if (n > 1 and sn != 1) or pitch < n or (b > 1 and sb != c * pitch):
        return None
    return pitch


class _PointHeadTrain(torch.autograd.Function):
    """ops.point_head_train: one foreign call per direction.  Kept for the backward: the three inputs, the packed keep bits
    (32 bytes per point) and the folded block (weights as the forward saw them and the statistics) -- no activation."""

    @staticmethod
    def forward(ctx, a, b, c, w1, g1, b1, w2, g2, b2, w3, bias3, buffers, eps_mom, training, masks, scale):
        bs, _, n = a.shape[:3]
        dev = a.device
        work, need = _train_work("point_head_train", "smos_point_head_train_work_bytes", bs * n, dev)
        logits = torch.empty((bs, 3, n, 1), dtype=torch.float32, device=dev)
        fold, dstat = _train_fold_dstat("smos_point_head_train", dev)
        rm1, rv1, rm2, rv2 = buffers
        params = (w1, g1, b1, rm1, rv1, w2, g2, b2, rm2, rv2, w3, bias3)
        pitch = _lib.i64_array([_point_head_pitch(t) for t in (a, b, c)])
        with _on(dev), profiling.span_f("point_head_%s[%dx%d]", ("train" if training else "eval", bs, n)):
            _lib.call("smos_point_head_train_fwd", a.data_ptr(), b.data_ptr(), c.data_ptr(), pitch, _ptr(masks), scale, bs, n,
                      int(training), _ptr_array(params), _lib.f64_array(eps_mom), logits.data_ptr(), fold.data_ptr(),
                      dstat.data_ptr(), work.data_ptr(), need, _stream(a))
        ctx.save_for_backward(a, b, c, fold, masks)
        ctx.param_like = (w1, g1, b1, w2, g2, b2, w3, bias3)
        ctx.scale, ctx.training = scale, bool(training)
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logits):
        a, b, c, fold, masks = ctx.saved_tensors
        bs, _, n = a.shape[:3]
        dev = a.device
        gl = grad_logits.to(torch.float32).contiguous()
        want_x = any(ctx.needs_input_grad[:3])
        dx = [torch.empty((bs, 64, n, 1), dtype=torch.float32, device=dev) for _ in range(3)] if want_x else [None] * 3
        dp = [torch.empty_like(p) if ctx.needs_input_grad[3 + i] else None for i, p in enumerate(ctx.param_like)]
        if want_x or any(g is not None for g in dp):
            work, need = _train_work("point_head_train", "smos_point_head_train_work_bytes", bs * n, dev)
            pitch = _lib.i64_array([_point_head_pitch(t) for t in (a, b, c)])
            with _on(dev), profiling.span_f("point_head_bwd[%dx%d]", (bs, n)):
                _lib.call("smos_point_head_train_bwd", a.data_ptr(), b.data_ptr(), c.data_ptr(), pitch, _ptr(masks), ctx.scale,
                          gl.data_ptr(), bs, n, int(ctx.training), fold.data_ptr(), _ptr_array(dx + dp), work.data_ptr(),
                          need, _stream(a))
        dx = [g if ctx.needs_input_grad[i] else None for i, g in enumerate(dx)]
        return (*dx, *dp, None, None, None, None, None)


def point_head_train(a, b, c, conv1, bn1, conv2, bn2, conv3, p=0.2, training=None, keep=None):
    """``PredBranch(CatFusion(a, b, c))`` -- cat -> dropout p -> 1x1 192->96 -> BN -> ReLU -> 1x1 96->64 -> BN -> ReLU ->
    dropout p -> 1x1 64->3 + bias -- as one autograd op on the HIP kernels of csrc/point_head_train.hip.

    a, b, c [B,64,N,1] float32 on the GPU, dense or cut out of a longer point axis; conv1/conv2 the bias-free 1x1
    convolutions, conv3 the one with a bias, bn1/bn2 the batch norms (affine, with running statistics and a momentum).
    ``training`` (None: ``bn1.training``): batch statistics over all B*N points, the four running buffers and
    ``num_batches_tracked`` updated in place as the modules would, and both dropouts applied; otherwise the running
    statistics and no dropout.  ``p`` is 0.2 (the kernels' keep threshold) or 0.0 (no dropout).  ``keep = (keep1 [B,192,N]
    bool, keep2 [B,64,N] bool)`` gives the dropout masks; without it they are drawn on the device from two seed words taken
    from torch's generator of that device, so ``torch.manual_seed`` reproduces them (against themselves, not against
    torch's dropout stream).  ``point_head_keep_bits(result)`` returns the masks a call used.  Returns logits [B,3,N,1],
    differentiable in the inputs and the eight parameters; a gradient nobody needs is not computed.  Every sum runs in a
    fixed order (the bits do not depend on the grid or the run) and nothing is read back to the host."""
    _require_cuda("point_head_train", a, b, c)
    xs = [a, b, c]
    for i, x in enumerate(xs):
        if x.dtype != torch.float32:
            raise RuntimeError("point_head_train: float32 only (input %d is %s)" % (i, x.dtype))
        if x.dim() == 3:
            xs[i] = x = x[..., None]
        if x.dim() != 4 or x.shape[1] != 64 or x.shape[3] != 1 or x.shape != xs[0].shape or x.shape[0] * x.shape[2] == 0:
            raise RuntimeError("point_head_train: input %d is %s, want three equal [B,64,N(,1)] with B*N > 0" % (i, tuple(x.shape)))
        if x.device != xs[0].device:
            raise RuntimeError("point_head_train: inputs on %s and %s" % (xs[0].device, x.device))
        if _point_head_pitch(x) is None:
            raise RuntimeError("point_head_train: input %d has strides %s; want unit-strided points and equally spaced channels "
                               "(make it contiguous)" % (i, x.stride()))
    bs, _, n = xs[0].shape[:3]
    dev = xs[0].device
    training = bool(bn1.training if training is None else training)
    bns = (bn1, bn2)
    _train_check_bns("point_head_train", zip(bns, (96, 64)), 1)
    rule = "conv1 and conv2 have none, conv3 has one"
    w1 = _train_conv1x1("point_head_train", "conv1", conv1, (96, 192), rule)
    w2 = _train_conv1x1("point_head_train", "conv2", conv2, (64, 96), rule)
    w3 = _train_conv1x1("point_head_train", "conv3", conv3, (3, 64), rule, bias=True)
    tensors = [w1, bn1.weight, bn1.bias, w2, bn2.weight, bn2.bias, w3, conv3.bias]
    buffers = (bn1.running_mean, bn1.running_var, bn2.running_mean, bn2.running_var)
    _train_check_tensors("point_head_train", tensors + list(buffers), dev)
    if _lib.query("smos_point_head_train_work_bytes", bs * n) <= 0:
        raise RuntimeError("point_head_train: %d x %d points is more than the kernels are set up for" % (bs, n))
    if training and bs * n < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (torch.Size((bs, 96, n, 1)),))
    p = float(p)
    if p not in (0.0, 0.2):
        raise RuntimeError("point_head_train: p = %g; the kernels keep with probability 0.8 (p = 0.2) or everything (p = 0)" % p)
    masks = seed = None
    if training and p > 0.0:
        masks = torch.empty(_lib.query("smos_point_head_train_mask_words", bs * n), dtype=torch.int32, device=dev)
        k1 = k2 = None
        if keep is not None:
            k1, k2 = keep
            for k, ch in ((k1, 192), (k2, 64)):
                if k.dtype != torch.bool or k.device != dev or tuple(k.shape[:3]) != (bs, ch, n) or k.numel() != bs * ch * n:
                    raise RuntimeError("point_head_train: keep must be bool (keep1 [B,192,N], keep2 [B,64,N]) on %s" % dev)
            k1, k2 = k1.contiguous(), k2.contiguous()
        else:
            seed = torch.randint(-2 ** 63, 2 ** 63 - 1, (2,), dtype=torch.int64, device=dev)
        with _on(dev), profiling.span_f("point_head_masks[%dx%d]", (bs, n)):
            _lib.call("smos_point_head_train_masks", _ptr(k1), _ptr(k2), _ptr(seed), bs, n, masks.data_ptr(), _stream(xs[0]))
    elif keep is not None and training:
        raise RuntimeError("point_head_train: keep masks given with p = 0")
    need_grad = torch.is_grad_enabled()
    xin = [x if need_grad and x.requires_grad else x.detach() for x in xs]
    out = _PointHeadTrain.apply(*xin, *tensors, buffers, _bn_eps_mom(bns), training, masks, 1.0 / (1.0 - p))
    if training:
        _bn_count_batch(bns)
    out._smos_point_head = (masks, seed, bs, n)
    return out


def point_head_keep_bits(out):
    """(keep1 [B,192,N] bool, keep2 [B,64,N] bool) of the ``point_head_train`` call that returned ``out``, unpacked from the
    packed words its kernels read; None when that call dropped nothing (eval, or p = 0)."""
    masks, _, bs, n = out._smos_point_head
    if masks is None:
        return None
    words = masks.view(8, bs, n)                                   # word planes: [w][b][n]
    shifts = torch.arange(32, device=masks.device, dtype=torch.int32)
    bits = ((words[:, None] >> shifts[None, :, None, None]) & 1).bool()      # [w][bit][b][n]
    bits = bits.reshape(256, bs, n).permute(1, 0, 2)               # channel = 32 w + bit
    return bits[:, :192].contiguous(), bits[:, 192:].contiguous()


def msda_fwd(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    """value [N,S,M,D], shapes [L,2] int64 (device), level_start [L] int64 (device), loc [N,Lq,M,L,P,2],
    attn [N,Lq,M,L,P] -> [N,Lq,M*D]."""
    _require_cuda("ms_deform_attn_forward", value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    for name, t in (("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
                    ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)):
        if not t.is_contiguous():
            raise RuntimeError("%s tensor has to be contiguous" % name)
    n, s, m, d = value.shape
    lq, l, p = sampling_loc.shape[1], sampling_loc.shape[3], sampling_loc.shape[4]
    out = torch.empty((n, lq, m * d), dtype=value.dtype, device=value.device)
    with _on(value.device), profiling.span_f("msda_fwd[%dx%dx%dx%d]", (n, lq, m, d)):
        _lib.call("smos_msda_fwd", value.data_ptr(), spatial_shapes.data_ptr(), level_start_index.data_ptr(),
                  sampling_loc.data_ptr(), attn_weight.data_ptr(), out.data_ptr(), n, s, m, d, l, lq, p,
                  _dtype_code("ms_deform_attn_forward", value), _stream(value))
    return out


def msda_bwd(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, deterministic=None):
    """Returns (grad_value, grad_sampling_loc, grad_attn_weight).

    ``deterministic`` (None: ``is_deterministic()``): grad_value summed in a fixed order by smos_msda_bwd_det
    (csrc/segsum.hip) instead of float atomics; the other two gradients are the same bits either way.  The fixed-order
    form is float32 only: float64 inputs stay on the atomic kernel under an ambient setting (None), and raise when
    ``deterministic=True`` is asked for explicitly."""
    det = is_deterministic() if deterministic is None else bool(deterministic)
    if det and value.dtype != torch.float32:
        if deterministic is not None:
            raise RuntimeError("ms_deform_attn_backward: the deterministic form is float32 only (got %s)" % value.dtype)
        det = False
    _require_cuda("ms_deform_attn_backward", value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output)
    for name, t in (("value", value), ("sampling_loc", sampling_loc), ("attn_weight", attn_weight), ("grad_output", grad_output)):
        if not t.is_contiguous():
            raise RuntimeError("%s tensor has to be contiguous" % name)
    n, s, m, d = value.shape
    lq, l, p = sampling_loc.shape[1], sampling_loc.shape[3], sampling_loc.shape[4]
    g_value = torch.empty_like(value) if det else torch.zeros_like(value)      # the fixed-order form writes every element
    g_loc = torch.empty_like(sampling_loc)
    g_attn = torch.empty_like(attn_weight)
    if det:
        for name, t in (("sampling_loc", sampling_loc), ("attn_weight", attn_weight), ("grad_output", grad_output)):
            if t.dtype != torch.float32:
                raise RuntimeError("ms_deform_attn_backward: %s is %s, value float32" % (name, t.dtype))
        need = _lib.query("smos_msda_bwd_det_work_bytes", n, s, m, d, l, lq, p)
        if need < 0:
            raise RuntimeError("ms_deform_attn_backward: the deterministic form takes fewer than 2^29 samples and 2^31 - 1 value "
                               "rows (got %d, %d)" % (n * lq * m * l * p, n * s * m))
        with _on(value.device), profiling.span_f("msda_bwd_det[%dx%dx%dx%d]", (n, lq, m, d)):
            work = torch.empty((need,), dtype=torch.uint8, device=value.device)
            _lib.call("smos_msda_bwd_det", grad_output.data_ptr(), value.data_ptr(), spatial_shapes.data_ptr(),
                      level_start_index.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(), g_value.data_ptr(),
                      g_loc.data_ptr(), g_attn.data_ptr(), n, s, m, d, l, lq, p, work.data_ptr(), need, _stream(value))
        return g_value, g_loc, g_attn
    with _on(value.device), profiling.span_f("msda_bwd[%dx%dx%dx%d]", (n, lq, m, d)):
        _lib.call("smos_msda_bwd", grad_output.data_ptr(), value.data_ptr(), spatial_shapes.data_ptr(),
                  level_start_index.data_ptr(), sampling_loc.data_ptr(), attn_weight.data_ptr(), g_value.data_ptr(),
                  g_loc.data_ptr(), g_attn.data_ptr(), n, s, m, d, l, lq, p, _dtype_code("ms_deform_attn_backward", value),
                  _stream(value))
    return g_value, g_loc, g_attn


def tta_argmax(pred, want_prob=False):
    """pred [B,K,N(,1)] float32 -> labels [N] uint8 (and prob [N,K])."""
    _require_cuda("tta_argmax", pred)
    if pred.dim() == 4:
        pred = pred[..., 0]
    pred = pred.contiguous().float()
    b, k, n = pred.shape
    labels = torch.empty(n, dtype=torch.uint8, device=pred.device)
    prob = torch.empty((n, k), dtype=torch.float32, device=pred.device) if want_prob else None
    with _on(pred.device):
        _lib.call("smos_tta_argmax", pred.data_ptr(), b, k, n, labels.data_ptr(), _ptr(prob), _stream(pred))
    return (labels, prob) if want_prob else labels


def vote_clear(table):
    _require_cuda("vote_clear", table)
    with _on(table.device):
        _lib.call("smos_vote_clear", table.data_ptr(), _stream(table))


def vote_accumulate(points, labels, table, pose_diff=None, recip_quantize=False):
    """points [n, >=3] float32 rows, labels [n] uint8, pose_diff 4x4 (numpy float64) or None."""
    _require_cuda("vote_accumulate", points, labels, table)
    if points.dtype != torch.float32 or labels.dtype != torch.uint8 or points.stride(1) != 1:
        raise RuntimeError("vote_accumulate: points must be float32 rows and labels uint8")
    pose = None
    if pose_diff is not None:
        pose = _lib.f64_array([float(v) for v in pose_diff.reshape(-1)[:16]])
    with _on(points.device):
        _lib.call("smos_vote_accumulate", points.data_ptr(), points.shape[0], points.stride(0), labels.data_ptr(), pose,
                  1 if recip_quantize else 0, table.data_ptr(), _stream(points))


def vote_accumulate_frames(frames, table, recip_quantize=False):
    """The whole voting window in one launch.  frames: list of (points [n, >=3] float32 rows, labels [n] uint8, pose_diff
    4x4 numpy float64 or None for the current frame)."""
    if not frames:
        return
    count = len(frames)
    pts, lab = (ctypes.c_void_p * count)(), (ctypes.c_void_p * count)()
    n, stride = (ctypes.c_int64 * count)(), (ctypes.c_int64 * count)()
    pose = (_lib.c_f64p * count)()
    keep = []
    for f, (points, labels, pose_diff) in enumerate(frames):
        _require_cuda("vote_accumulate_frames", points, labels, table)
        if points.dtype != torch.float32 or labels.dtype != torch.uint8 or points.stride(1) != 1 or points.device != table.device:
            raise RuntimeError("vote_accumulate_frames: points must be float32 rows and labels uint8, on the table's device")
        if labels.shape[0] != points.shape[0] or not labels.is_contiguous():
            raise RuntimeError("vote_accumulate_frames: one contiguous label per point")
        pts[f], lab[f], n[f], stride[f] = points.data_ptr(), labels.data_ptr(), points.shape[0], points.stride(0)
        if pose_diff is not None:
            arr = np.ascontiguousarray(pose_diff, dtype=np.float64).reshape(-1)
            if arr.size < 16:
                raise RuntimeError("vote_accumulate_frames: pose_diff must be 4x4")
            keep.append(arr)                          # the numpy buffer is read during the call
            pose[f] = arr.ctypes.data_as(_lib.c_f64p)
    with _on(table.device), profiling.span_f("vote_accumulate[%dx%d]", (count, max(n))):
        _lib.call("smos_vote_accumulate_frames", count, pts, n, stride, lab, pose, 1 if recip_quantize else 0, table.data_ptr(),
                  _stream(table))


def vote_resolve(points, labels, table, lut=None, recip_quantize=False):
    _require_cuda("vote_resolve", points, labels, table, lut)
    out = torch.empty(points.shape[0], dtype=torch.int32, device=points.device)
    with _on(points.device):
        _lib.call("smos_vote_resolve", points.data_ptr(), points.shape[0], points.stride(0), labels.data_ptr(),
                  1 if recip_quantize else 0, table.data_ptr(), _ptr(lut), out.data_ptr(), _stream(points))
    return out


def dbscan(points, eps, min_samples, max_sweeps=4096):
    """sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(points[:, :3]) on the device (voxel_instance_voting.py:150-153).
    points [n, >=3] float32 rows.  Returns int32 [n]: the index of the cluster's lowest-index core point, -1 for noise
    (rank the distinct values to get scikit-learn's 0,1,2.. numbering).  Synchronises the stream."""
    _require_cuda("dbscan", points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3 or points.stride(1) != 1:
        raise RuntimeError("dbscan: points must be float32 rows [n, >=3]")
    n = points.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=points.device)
    if n == 0:
        return labels
    need = _lib.query("smos_dbscan_work_bytes", n)
    if need <= 0:
        raise RuntimeError("dbscan: workspace query failed for n=%d" % n)
    work = torch.empty(need + 256, dtype=torch.uint8, device=points.device)
    base = (work.data_ptr() + 255) // 256 * 256
    with _on(points.device):
        _lib.call("smos_dbscan", points.data_ptr(), n, points.stride(0), float(eps), int(min_samples), labels.data_ptr(), base,
                  need, int(max_sweeps), _stream(points))
    return labels


def box_vote(points, labels, boxes, counts, pose_diff=None):
    """counts [K,3] uint32/int32 (zero-filled by the caller) += per-box class counts of one frame's kept points
    (voxel_instance_voting.py:170-179).  boxes [K,6] float32 (lo xyz, hi xyz), closed intervals."""
    _require_cuda("box_vote", points, labels, boxes, counts)
    if points.dtype != torch.float32 or labels.dtype != torch.uint8 or points.stride(1) != 1:
        raise RuntimeError("box_vote: points must be float32 rows and labels uint8")
    if boxes.dtype != torch.float32 or not boxes.is_contiguous() or boxes.dim() != 2 or boxes.shape[1] != 6:
        raise RuntimeError("box_vote: boxes must be a contiguous float32 [K, 6] tensor")
    if counts.dtype not in (torch.int32, torch.uint32) or not counts.is_contiguous() or counts.numel() != boxes.shape[0] * 3:
        raise RuntimeError("box_vote: counts must be a contiguous 32-bit [K, 3] tensor")
    pose = None
    if pose_diff is not None:
        pose = _lib.f64_array([float(v) for v in pose_diff.reshape(-1)[:16]])
    with _on(points.device):
        _lib.call("smos_box_vote", points.data_ptr(), points.shape[0], points.stride(0), labels.data_ptr(), pose, boxes.data_ptr(),
                  boxes.shape[0], counts.data_ptr(), _stream(points))
    return counts


MAX_BOXES = 2048        # upper bound of max_boxes (the LDS of the box vote)


def instance_work_bytes(n):
    """Device scratch smos_instance_cluster needs for a scan of n points (256 bytes of slack for the alignment included)."""
    need = _lib.query("smos_instance_work_bytes", int(n))
    if need < 0:
        raise RuntimeError("instance_cluster: workspace query failed for n=%d" % n)
    return need + 256


def instance_cluster(points, bf, eps, min_samples, min_points, floor_lift, max_boxes=MAX_BOXES, work=None, out=None):
    """DBSCAN of the scan's foreground points (bf == 2) and the boxes of InstanceVoter.cluster_boxes, with nothing read
    back.  points [n, >=3] float32 rows (the whole scan), bf [n] uint8.  Returns dict(names int32 [n] (scan index of the
    cluster's lowest core point; -1 for noise and non-foreground), boxes float32 [max_boxes, 6], slot_of int32 [n] (name ->
    row of boxes, -1), k int32 [1] (rows used), status int32 [1] (bit 0: more than max_boxes clusters)).  work: a uint8
    device tensor of >= instance_work_bytes(n) bytes to reuse (its contents do not matter); out: a dict of such tensors
    to write into."""
    _require_cuda("instance_cluster", points, bf, work)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3 or points.stride(1) != 1:
        raise RuntimeError("instance_cluster: points must be float32 rows [n, >=3]")
    n = points.shape[0]
    if bf.dtype != torch.uint8 or bf.dim() != 1 or bf.shape[0] != n or not bf.is_contiguous() or bf.device != points.device:
        raise RuntimeError("instance_cluster: bf must be a contiguous uint8 [n] tensor on the points' device")
    max_boxes = int(max_boxes)
    if not 1 <= max_boxes <= MAX_BOXES:
        raise RuntimeError("instance_cluster: max_boxes must be in 1..%d, got %d" % (MAX_BOXES, max_boxes))
    dev = points.device
    if out is None:
        out = {"names": torch.empty(n, dtype=torch.int32, device=dev), "slot_of": torch.empty(n, dtype=torch.int32, device=dev),
               "boxes": torch.empty((max_boxes, 6), dtype=torch.float32, device=dev),
               "k": torch.empty(1, dtype=torch.int32, device=dev), "status": torch.empty(1, dtype=torch.int32, device=dev)}
    for key, dtype, numel in (("names", torch.int32, n), ("slot_of", torch.int32, n), ("boxes", torch.float32, max_boxes * 6),
                              ("k", torch.int32, 1), ("status", torch.int32, 1)):
        t = out[key]
        if t.dtype != dtype or t.numel() != numel or not t.is_contiguous() or t.device != dev:
            raise RuntimeError("instance_cluster: out[%r] must be a contiguous %s tensor of %d elements on the points' device"
                               % (key, dtype, numel))
    need = instance_work_bytes(n)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    base = (work.data_ptr() + 255) // 256 * 256
    room = work.numel() - (base - work.data_ptr())
    if work.dtype != torch.uint8 or not work.is_contiguous() or work.device != dev or room < need - 256:
        raise RuntimeError("instance_cluster: work must be a contiguous uint8 tensor of >= %d bytes on the points' device" % need)
    with _on(dev), profiling.span_f("instance_cluster[%d]", (n,)):
        _lib.call("smos_instance_cluster", points.data_ptr(), n, points.stride(0), bf.data_ptr(), float(eps), int(min_samples),
                  int(min_points), float(floor_lift), max_boxes, out["names"].data_ptr(), out["boxes"].data_ptr(),
                  out["slot_of"].data_ptr(), out["k"].data_ptr(), out["status"].data_ptr(), base, room, _stream(points))
    return out


def box_vote_dev(frames, boxes, k, counts):
    """box_vote for a whole window in one launch on the first k[0] rows of boxes, k a DEVICE int32 [1] tensor.  frames: list
    of (points [n, >=3] float32 rows, labels [n] uint8, pose_diff 4x4 numpy float64 or None).  boxes [max_boxes, 6] float32;
    counts [max_boxes, 3] uint32/int32, zero-filled by the caller."""
    _require_cuda("box_vote_dev", boxes, k, counts)
    if boxes.dtype != torch.float32 or not boxes.is_contiguous() or boxes.dim() != 2 or boxes.shape[1] != 6 \
            or not 1 <= boxes.shape[0] <= MAX_BOXES:
        raise RuntimeError("box_vote_dev: boxes must be a contiguous float32 [max_boxes <= %d, 6] tensor" % MAX_BOXES)
    if counts.dtype not in (torch.int32, torch.uint32) or not counts.is_contiguous() or counts.numel() != boxes.shape[0] * 3:
        raise RuntimeError("box_vote_dev: counts must be a contiguous 32-bit [max_boxes, 3] tensor")
    if k.dtype != torch.int32 or k.numel() != 1 or k.device != boxes.device or counts.device != boxes.device:
        raise RuntimeError("box_vote_dev: k must be an int32 [1] tensor on the boxes' device, counts on it too")
    if not frames:
        return counts
    count = len(frames)
    pts, lab = (ctypes.c_void_p * count)(), (ctypes.c_void_p * count)()
    n, stride = (ctypes.c_int64 * count)(), (ctypes.c_int64 * count)()
    pose = (_lib.c_f64p * count)()
    keep = []
    for f, (points, labels, pose_diff) in enumerate(frames):
        _require_cuda("box_vote_dev", points, labels)
        if points.dtype != torch.float32 or labels.dtype != torch.uint8 or points.stride(1) != 1 or points.device != boxes.device:
            raise RuntimeError("box_vote_dev: points must be float32 rows and labels uint8, on the boxes' device")
        if labels.shape[0] != points.shape[0] or not labels.is_contiguous():
            raise RuntimeError("box_vote_dev: one contiguous label per point")
        pts[f], lab[f], n[f], stride[f] = points.data_ptr(), labels.data_ptr(), points.shape[0], points.stride(0)
        if pose_diff is not None:
            arr = np.ascontiguousarray(pose_diff, dtype=np.float64).reshape(-1)
            if arr.size < 16:
                raise RuntimeError("box_vote_dev: pose_diff must be 4x4")
            keep.append(arr)                          # the numpy buffer is read during the call
            pose[f] = arr.ctypes.data_as(_lib.c_f64p)
    with _on(boxes.device), profiling.span_f("box_vote_dev[%dx%d]", (count, max(n))):
        _lib.call("smos_box_vote_dev", count, pts, n, stride, lab, pose, boxes.data_ptr(), k.data_ptr(), boxes.shape[0],
                  counts.data_ptr(), _stream(boxes))
    return counts


def instance_apply(names, slot_of, counts, k, labels):
    """labels (int32 [n], in place): 2 if 2 * counts[s, 2] > counts[s, 1] else 1 for every point whose cluster names[i] has
    a slot s = slot_of[names[i]] (voxel_instance_voting.py:178-183); every other label is kept."""
    _require_cuda("instance_apply", names, slot_of, counts, k, labels)
    n = labels.shape[0]
    for what, t in (("names", names), ("slot_of", slot_of), ("labels", labels)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous() or t.device != labels.device:
            raise RuntimeError("instance_apply: %s must be a contiguous int32 [n] tensor on the labels' device" % what)
    if counts.dtype not in (torch.int32, torch.uint32) or not counts.is_contiguous() or counts.dim() != 2 or counts.shape[1] != 3 \
            or counts.device != labels.device:
        raise RuntimeError("instance_apply: counts must be a contiguous 32-bit [max_boxes, 3] tensor on the labels' device")
    if k.dtype != torch.int32 or k.numel() != 1 or k.device != labels.device:
        raise RuntimeError("instance_apply: k must be an int32 [1] tensor on the labels' device")
    with _on(labels.device):
        _lib.call("smos_instance_apply", names.data_ptr(), slot_of.data_ptr(), counts.data_ptr(), k.data_ptr(), counts.shape[0],
                  labels.data_ptr(), n, _stream(labels))
    return labels


def _label_args(name, words, gt, gt_map, counts, n, device):
    """Checks shared by label_words / voted_label_counts; returns the raw pointers (None where absent)."""
    _require_cuda(name, words, gt, gt_map, counts)
    if words is not None and (words.dtype != torch.int32 or not words.is_contiguous() or words.numel() < n
                              or words.data_ptr() % 16 or words.device != device):
        raise RuntimeError("%s: words must be a contiguous, 16-byte aligned int32 tensor of >= n elements on the labels' device" % name)
    if gt is None:
        return _ptr(words), None, None, 0, None
    if gt_map is None or counts is None:
        raise RuntimeError("%s: counting needs gt_map and counts" % name)
    if gt.dtype not in (torch.int32, torch.uint32) or not gt.is_contiguous() or gt.numel() != n or gt.data_ptr() % 16:
        raise RuntimeError("%s: gt must be a contiguous, 16-byte aligned 32-bit tensor with one word per label" % name)
    if gt_map.dtype != torch.int32 or not gt_map.is_contiguous() or gt_map.dim() != 1:
        raise RuntimeError("%s: gt_map must be a contiguous int32 vector" % name)
    if counts.dtype not in (torch.int64, torch.uint64) or not counts.is_contiguous() or counts.numel() != 6:
        raise RuntimeError("%s: counts must be a contiguous 64-bit tensor of 6 counters" % name)
    if not (gt.device == gt_map.device == counts.device == device):
        raise RuntimeError("%s: every tensor must be on the labels' device" % name)
    return _ptr(words), gt.data_ptr(), gt_map.data_ptr(), gt_map.numel(), counts.data_ptr()


def label_words(labels, words=None, lut=True, gt=None, gt_map=None, counts=None):
    """One frame's prediction words and moving-IoU counts in one launch (csrc/labels.hip).  labels [n] uint8 in {0,1,2};
    words [>=n] int32 (allocated when None) gets the learning_map_inv value 0 / 9 / 251 per point (lut=True, predictions/)
    or the label itself (lut=False, predictions_bf/).  With gt ([n] 32-bit SemanticKITTI label words), gt_map
    (kitti.learning_map_lut() as int32 on the device) and counts ([6] int64): counts += tp[1:3], pred[1:3], gt[1:3] of
    kitti.MovingIoU.add(gt_map[gt & 0xFFFF], labels).  Returns words."""
    _require_cuda("label_words", labels)
    if labels.dtype != torch.uint8 or labels.dim() != 1 or not labels.is_contiguous() or labels.data_ptr() % 4:
        raise RuntimeError("label_words: labels must be a contiguous, 4-byte aligned uint8 vector")
    n = labels.shape[0]
    if words is None:
        words = torch.empty(n, dtype=torch.int32, device=labels.device)
    w, g, gm, mn, c = _label_args("label_words", words, gt, gt_map, counts, n, labels.device)
    with _on(labels.device):
        _lib.call("smos_label_words", labels.data_ptr(), n, 1 if lut else 0, w, g, gm, mn, c, _stream(labels))
    return words


def voted_label_counts(voted, gt, gt_map, counts, words=None):
    """The same for a voted frame: voted [n] int32 LUT words (vote_resolve with the LUT) count as class 2 for 251, 1 for 9,
    0 otherwise (run_sequence's refined IoU); words (optional, [>=n] int32) gets a copy of them."""
    _require_cuda("voted_label_counts", voted)
    if voted.dtype != torch.int32 or voted.dim() != 1 or not voted.is_contiguous() or voted.data_ptr() % 16:
        raise RuntimeError("voted_label_counts: voted must be a contiguous, 16-byte aligned int32 vector")
    n = voted.shape[0]
    w, g, gm, mn, c = _label_args("voted_label_counts", words, gt, gt_map, counts, n, voted.device)
    with _on(voted.device):
        _lib.call("smos_label_count_voted", voted.data_ptr(), n, w, g, gm, mn, c, _stream(voted))
    return words


# ---------------------------------------------------------------------------------------------
# activation codes of the fused epilogues (inference engine)
# ---------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


# ---------------------------------------------------------------------------------------------
# fused point-side kernels (inference engine)
# ---------------------------------------------------------------------------------------------
def _rows(name, t, c):
    """(batch pitch, row pitch) of a point-row view [B, N, c] whose last dim is contiguous."""
    if t.dim() != 3 or t.shape[2] != c or t.stride(2) != 1:
        raise RuntimeError("%s: expected point rows [B, N, %d] with contiguous channels, got %s / %s" % (name, c, tuple(t.shape), t.stride()))
    return t.stride(0), t.stride(1)


def pointnet_scatter(xyzi, coord, w1, b1, w2, b2, bev, pts_out=None, zero_fill=False):
    """xyzi [B,T,7,N(,1)], coord [B,T,N,K(,1)], bev [B,H,W,T*64] zero-filled channels-last (zero_fill=True clears it
    here, inside the profiled span), pts_out [B,N,64] rows."""
    _require_cuda("pointnet_scatter", xyzi, coord, w1, b1, w2, b2, bev, pts_out)
    b, t, cin, n = xyzi.shape[:4]
    k = coord.shape[3]
    if not (xyzi.is_contiguous() and coord.is_contiguous() and bev.is_contiguous()):
        raise RuntimeError("pointnet_scatter: xyzi, coord and bev must be contiguous")
    h, w = bev.shape[1], bev.shape[2]
    cout = w2.shape[0]
    if bev.shape[3] != t * cout:
        raise RuntimeError("pointnet_scatter: bev has %d channels, expected %d" % (bev.shape[3], t * cout))
    po_b = po_n = 0
    if pts_out is not None:
        po_b, po_n = _rows("pointnet_scatter", pts_out, cout)
    with _on(xyzi.device), profiling.span_f("pointnet_scatter[%dx%dx%d->%dx%d]", (b, t, n, h, w)):
        if zero_fill:
            bev.zero_()
        _lib.call("smos_pointnet_scatter", xyzi.data_ptr(), coord.data_ptr(), k, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                  b2.data_ptr(), bev.data_ptr(), _ptr(pts_out), po_b, po_n, b, t, n, h, w, cin, w1.shape[0], cout, _stream(xyzi))
    return bev


def point_head_k_order():
    """[96, 2] int64: the input channel k-step s of layer 1 feeds to lane half h.  A row is three 64-channel segments (point
    MLP | BEV | range view); steps [32 t, 32 t + 32) walk segment t, lane half h its channels [32 h, 32 h + 32) -- the same walk
    for both halves, so that one segment (the BEV one, smos_point_head_gather) can come from somewhere else than the row."""
    s = torch.arange(96)[:, None]
    h = torch.arange(2)[None, :]
    return 64 * (s >> 5) + 32 * h + (s & 31)


def point_head_prepare(l1, l2, l3):
    """(W1 [96,192(,1,1)], b1), (W2 [64,96], b2), (W3 [M3,64], b3) -> the flat weight block smos_point_head expects."""
    w1, b1 = l1[0].reshape(l1[0].shape[0], -1).float(), l1[1].float()
    w2, b2 = l2[0].reshape(l2[0].shape[0], -1).float(), l2[1].float()
    w3, b3 = l3[0].reshape(l3[0].shape[0], -1).float(), l3[1].float()
    if tuple(w1.shape) != (96, 192) or tuple(w2.shape) != (64, 96) or w3.shape[1] != 64 or w3.shape[0] > 32:
        raise RuntimeError("point_head_prepare: expected 192 -> 96 -> 64 -> (<=32), got %s %s %s" % (tuple(w1.shape), tuple(w2.shape), tuple(w3.shape)))
    dev = w1.device
    lane = torch.arange(64, device=dev)
    m, h = lane & 31, lane >> 5
    a1 = w1.view(3, 32, 192)[:, :, point_head_k_order().to(dev)].permute(0, 2, 3, 1).reshape(3, 96, 64)   # (mt, s, h*32 + m)

    def acc_order(n_steps):                                                               # ch(s, h) for s < n_steps
        s = torch.arange(n_steps, device=dev)[:, None]
        return 32 * (s >> 4) + 8 * ((s & 15) >> 2) + 4 * h[None, :] + (s & 3)            # [n_steps, 64]
    ch2 = acc_order(48)
    a2 = torch.stack([w2[mt * 32 + m[None, :].expand(48, 64), ch2] for mt in range(2)])  # (mt, s, lane)
    w3p = torch.zeros((32, 64), device=dev)
    w3p[:w3.shape[0]] = w3
    a3 = w3p[m[None, :].expand(32, 64), acc_order(32)]
    b3p = torch.zeros(32, device=dev)
    b3p[:b3.shape[0]] = b3
    flat = torch.cat([a1.reshape(-1), a2.reshape(-1), a3.reshape(-1), b1, b2, b3p]).contiguous()
    if flat.numel() != _lib.query("smos_point_head_weight_floats"):
        raise RuntimeError("point_head_prepare: weight block has %d floats" % flat.numel())
    return flat, int(w3.shape[0])


def point_head(rows, wprep, m3, out=None, n_live=None, gather=None):
    """rows [B, N, >=192] float32 (row stride a multiple of 4 floats) -> logits [B, m3, N].
    n_live: optional device int32 tensor (its first element is read): the number of REAL points at the front of every sample;
    the logits of the scan's padding tail [n_live, N) come back as zeros without being computed (the streaming runner's form:
    val_StreamMOS.py:113 cuts them off).
    gather = (grid, gcoord, gscale): channels [64, 128) of every row are not read from `rows` but gathered by the kernel itself
    from the channels-last [B, 64, Hg, Wg] view `grid` at gcoord * gscale -- gather_scatter_cl(grid, gcoord, gscale,
    pts_out=rows[:, :, 64:128]) followed by point_head(rows, ...), bit for bit, in one launch and without that pass over the rows."""
    _require_cuda("point_head", rows, wprep, out, n_live)
    if rows.dtype != torch.float32 or rows.dim() != 3 or rows.stride(2) != 1 or rows.stride(0) != rows.shape[1] * rows.stride(1):
        raise RuntimeError("point_head: rows must be a float32 [B, N, C] tensor with dense point rows")
    live = _live_ptr("point_head", n_live)
    b, n = rows.shape[0], rows.shape[1]
    if gather is not None:
        grid, gcoord, gscale = gather
        _require_cuda("point_head", grid, gcoord)
        if grid.dtype != torch.float32 or grid.shape[0] != b or grid.shape[1] != 64:
            raise RuntimeError("point_head: the gathered map must be a float32 channels-last [B, 64, Hg, Wg] view, got %s" % (tuple(grid.shape),))
        gp = _cl("point_head", grid)
        kg, gbs = _coord_view("point_head", gcoord, b, n)
    if out is None:
        out = torch.empty((b, m3, n), dtype=torch.float32, device=rows.device)
    head = (rows.data_ptr(), rows.stride(1), wprep.data_ptr(), out.data_ptr(), b, n, 192, 96, 64, m3, live)
    with _on(rows.device), profiling.span_f("point_head[%dx%d]", (b, n)):
        if gather is None:
            _lib.call("smos_point_head", *head, _stream(rows))
        else:
            _lib.call("smos_point_head_gather", *head, grid.data_ptr(), gp, grid.shape[2], grid.shape[3], gcoord.data_ptr(), kg, gbs,
                      _lib.f32_array(gscale), _stream(rows))
    return out


def conv_prepare(w, mt, order="taps"):
    """w [Cout, Cin, KH, KW] (BatchNorm folded) -> the weight block of smos_conv_cl in MFMA operand order for `mt`
    32-channel output blocks per wave (include/smos.h): [cout tile][stage = (ky, kx, cin chunk)][k-step / 4][mt][lane][k-step % 4]
    with lane = h * 32 + m holding w[ct*32*mt + mt_i*32 + m][chunk*32 + 8*i4 + 4*h + c][ky][kx].
    order="rows" (smos_conv_rows_cl, mt <= 2): stage = (ky, cin chunk, kx) -- the kx taps of a staged input row together."""
    cout, cin, kh, kw = w.shape
    if cin % 32 or cout % (32 * mt) or mt not in (1, 2, 4) or order not in ("taps", "rows") or (order == "rows" and mt > 2):
        raise RuntimeError("conv_prepare: Cin %% 32 == 0 and Cout %% (32 * mt) == 0 required (got %s, mt=%d, order=%s)" % (tuple(w.shape), mt, order))
    #           ct                mt_i  m   chunk      i4  h  c   ky  kx
    v = w.float().reshape(cout // (32 * mt), mt, 32, cin // 32, 4, 2, 4, kh, kw)
    if order == "rows":
        v = v.permute(0, 7, 3, 8, 4, 1, 5, 2, 6)     # -> [ct, ky, chunk, kx, i4, mt_i, h, m, c]
    else:
        v = v.permute(0, 7, 8, 3, 4, 1, 5, 2, 6)     # -> [ct, ky, kx, chunk, i4, mt_i, h, m, c]
    return v.reshape(-1).contiguous()


def conv_cl_supported(x, cout, kernel, stride=1, residual=None, out=None):
    """The hard limits of smos_conv_cl / smos_conv_rows_cl (the SMOS_REQUIREs of smos_conv_cl and of conv_check_operands, csrc/conv_common.h), as a
    predicate the engine asks BEFORE it routes a layer to the own kernels: Cin / Cout multiples of 32, Cout <= 2048,
    kernel <= 7x7, stride 1 or 2, and every operand below 2 GiB (the kernels address through 32-bit buffer offsets; a
    16-stream batch of 128-channel 256x256 maps is 2.1 GB).  Shapes only: works on meta tensors."""
    kh, kw = kernel
    b, cin, h, w = x.shape
    if cin % 32 or cout % 32 or cout > 2048 or not (1 <= kh <= 7 and 1 <= kw <= 7) or stride not in (1, 2):
        return False
    ho, wo = (h + 2 * (kh // 2) - kh) // stride + 1, (w + 2 * (kw // 2) - kw) // stride + 1
    if ho <= 0 or wo <= 0:
        return False

    def pitch(t, c):
        return t.stride(3) if t is not None and t.dim() == 4 and t.stride(1) == 1 else c
    limit = 1 << 31
    if b * h * w * pitch(x, cin) * 4 >= limit or b * ho * wo * pitch(out, cout) * 4 >= limit:
        return False
    if residual is not None and b * ho * wo * pitch(residual, cout) * 4 >= limit:
        return False
    return True


def conv_rows_ok(kernel, stride, cin, cout):
    """Shapes smos_conv_rows_cl covers (stride 1, "same" padding, KW in {3, 5, 7})."""
    kh, kw = kernel
    return stride == 1 and kw in (3, 5, 7) and kh in (1, 3, 5, 7) and cin % 32 == 0 and cout % 32 == 0


def _conv_operands(name, x, wprep, bias, cout, ho, wo, residual=None, out=None, chan_sums=None, sum_chunks=None):
    """What the conv wrappers share: the operands live in GPU memory, `out` is allocated (or has the output's shape), `residual`
    has it too, `chan_sums` is the contiguous float32 [B, sum_chunks(Ho, Wo), Cout] table of the kernel family and comes without
    a residual.  Returns (out, head): the arguments every conv entry point starts with -- x, x pitch, wprep, bias, res,
    res pitch, out, out pitch."""
    _require_cuda(name, x, wprep, bias, residual, out, chan_sums)
    b = x.shape[0]
    if out is None:
        out = empty_cl(b, cout, ho, wo, x.device)
    elif tuple(out.shape) != (b, cout, ho, wo):
        raise RuntimeError("%s: out has shape %s, expected %s" % (name, tuple(out.shape), (b, cout, ho, wo)))
    if residual is not None and tuple(residual.shape) != (b, cout, ho, wo):
        raise RuntimeError("%s: residual has shape %s" % (name, tuple(residual.shape)))
    if chan_sums is not None and (residual is not None or not chan_sums.is_contiguous() or chan_sums.dtype != torch.float32 or
                                  tuple(chan_sums.shape) != (b, sum_chunks(ho, wo), cout)):
        raise RuntimeError("%s: chan_sums must be contiguous float32 [B, %s(Ho, Wo), Cout], without a residual"
                           % (name, sum_chunks.__name__))
    return out, (x.data_ptr(), _cl(name, x), wprep.data_ptr(), _ptr(bias), _ptr(residual),
                 _cl(name, residual) if residual is not None else 0,
                 out.data_ptr(), _cl(name, out))


def _conv_label(name, x, cout, ho, wo, kernel, residual=None):
    return "%s[%dx%dx%dx%d->%dx%dx%dk%dx%d%s]" % ((name,) + tuple(x.shape) + (cout, ho, wo) + tuple(kernel) +
                                                ("+res" if residual is not None else "",))


def _conv_launch(fn_name, family, args, keep, x, label_fn):
    """One conv launch of the C function `fn_name` on x's device and torch's current stream.  While nothing is profiled that is
    all (no label, no span: a label is a string format of ~10 numbers); otherwise the launch carries label_fn() under the
    kernel family, and a requested replay gets a closure over args (`keep`: the operand tensors, alive as long as it is)."""
    dev = x.device
    if not profiling.enabled():
        fn = _lib.entry(fn_name)             # not _lib.call: its frame and second argument tuple show in the per-launch cost
        with _on(dev):
            rc = fn(*args, _raw_stream(_dev_index(dev)))
        if rc:
            _lib.check(rc, fn_name)
        return
    label = label_fn()
    with _on(dev), profiling.span(label, family):
        _lib.call(fn_name, *args, _stream(x))
    if profiling._replay_label == label:
        def again(keep=keep):
            with _on(keep[0].device), profiling.span(label, family):
                _lib.call(fn_name, *args, _stream(keep[0]))
        profiling.offer_replay(label, again)


def conv_rows_cl(x, wprep, bias, act, cout, kernel, mt=1, residual=None, out=None, chan_sums=None):
    """conv_cl for stride 1 / "same" padding / KW in {3, 5, 7} at 32 * mt (mt in {1, 2}) output channels per block, with the
    input rows staged through LDS once per kernel row instead of one global request per tap (csrc/conv_rows.hip).
    wprep = conv_prepare(w, mt, order="rows")."""
    b, cin, h, w = x.shape
    kh, kw = kernel
    if not conv_rows_ok(kernel, 1, cin, cout) or wprep.numel() != cout * cin * kh * kw or mt not in (1, 2) or cout % (32 * mt):
        raise RuntimeError("conv_rows_cl: unsupported shape %s k%dx%d -> %d" % (tuple(x.shape), kh, kw, cout))
    out, head = _conv_operands("conv_rows_cl", x, wprep, bias, cout, h, w, residual, out, chan_sums, conv_sum_chunks)
    args = head + (b, h, w, cin, cout, kh, kw, int(mt), int(act), _ptr(chan_sums))
    _conv_launch("smos_conv_rows_cl", "conv_rows", args, (x, wprep, bias, residual, out, chan_sums), x,
                 lambda: _conv_label("conv_cl", x, cout, h, w, kernel, residual))
    return out


_CONV_MIN_WAVE_TILES = int(os.environ.get("SMOS_CONV_MIN_WAVE_TILES", "2048"))   # tuning knob (tools/ubench_conv.py)


def conv_mt(cout, n_pixels, residual=False):
    """Output blocks per wave for smos_conv_cl: wider waves re-use each activation load more often, narrower ones give
    more wave tiles; aim at >= 2 waves for each of the 1024 SIMDs.  With a residual input the kernel holds the residual
    tile in registers, which limits it to mt <= 2."""
    tiles32 = (n_pixels + 31) // 32
    for mt in ((2, 1) if residual else (4, 2, 1)):
        if cout % (32 * mt) == 0 and tiles32 * (cout // (32 * mt)) >= _CONV_MIN_WAVE_TILES:
            return mt
    return 1


def conv_sum_chunks(ho, wo):
    """Row segments per sample in the channel-sum table of conv_cl(..., chan_sums=...)."""
    return ((ho + 3) // 4) * ((wo + 31) // 32) * 4


def conv_cl(x, wprep, bias, act, cout, kernel, stride=1, padding=None, mt=1, residual=None, out=None, chan_sums=None):
    """act(conv(x) + bias [+ residual]) on channels-last [B,C,H,W] views in one launch (csrc/conv_igemm.hip).
    wprep = conv_prepare(w, mt); kernel = (KH, KW); padding defaults to "same" for odd kernels.
    chan_sums: optional float32 [B, conv_sum_chunks(Ho, Wo), Cout] that receives the per-row-segment channel sums of the
    output (the average-pool input of a ChannelAtt block); not together with a residual."""
    b, cin, h, w = x.shape
    kh, kw = kernel
    ph, pw = padding if padding is not None else (kh // 2, kw // 2)
    ho, wo = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
    if wprep.numel() != cout * cin * kh * kw:
        raise RuntimeError("conv_cl: weight block has %d floats, expected %d" % (wprep.numel(), cout * cin * kh * kw))
    out, head = _conv_operands("conv_cl", x, wprep, bias, cout, ho, wo, residual, out, chan_sums, conv_sum_chunks)
    args = head + (b, h, w, cin, cout, kh, kw, stride, ph, pw, mt, int(act), _ptr(chan_sums))
    _conv_launch("smos_conv_cl", "conv_igemm", args, (x, wprep, bias, residual, out, chan_sums), x,
                 lambda: _conv_label("conv_cl", x, cout, ho, wo, kernel, residual))
    return out


def conv_bf16_prepare(w):
    """w [Cout, Cin, KH, KW] (BatchNorm folded, fp32) -> the bf16 weight block of smos_conv_bf16_cl (include/smos.h): rounded
    once to nearest even (torch's .to(torch.bfloat16)), in MFMA operand order [cin chunk][ky][kx][Cout / 32][k-step][lane][8]
    with lane = h * 32 + m holding w[32 q + m][32 chunk + 16 s + 8 h + j][ky][kx], j = 0..7."""
    cout, cin, kh, kw = w.shape
    if cin % 32 or cout % 32:
        raise RuntimeError("conv_bf16_prepare: Cin %% 32 == 0 and Cout %% 32 == 0 required (got %s)" % (tuple(w.shape),))
    #                q          m   chunk    s  h  j  ky  kx
    v = w.detach().float().reshape(cout // 32, 32, cin // 32, 2, 2, 8, kh, kw)
    v = v.permute(2, 6, 7, 0, 3, 4, 1, 5)           # -> [chunk, ky, kx, q, s, h, m, j]
    return v.to(torch.bfloat16).reshape(-1).contiguous()


_bf16_shape_ok = {}


def conv_bf16_ok(x, cout, kernel, stride=1, residual=None, out=None, chan_sums=None):
    """Shapes smos_conv_bf16_cl covers, as a predicate the engine asks before it routes a layer to it: the limits of
    conv_cl_supported (channel multiples of 32, Cout <= 2048, kernel <= 7x7, stride 1 or 2, every operand below 2 GiB) plus a
    block shape whose staged input region fits (smos_conv_bf16_cl_supported); channel sums never with a residual.
    Shapes only: works on meta tensors."""
    if chan_sums is not None and residual is not None:
        return False
    if not conv_cl_supported(x, cout, kernel, stride, residual, out):
        return False
    kh, kw = kernel
    key = (x.shape[1], cout, kh, kw, stride, residual is not None)
    ok = _bf16_shape_ok.get(key)
    if ok is None:
        ok = _bf16_shape_ok[key] = bool(_lib.query("smos_conv_bf16_cl_supported", *key[:5], int(key[5])))
    return ok


def conv_bf16_cl(x, wprep, bias, act, cout, kernel, stride=1, padding=None, residual=None, out=None, chan_sums=None):
    """conv_cl with bf16 operands on the bf16 matrix cores (csrc/conv_bf16.hip): act(sum bf16(w) * bf16(x) + bias [+ residual])
    with fp32 sums, bias, residual, activation and output.  wprep = conv_bf16_prepare(w); kernel = (KH, KW); padding defaults
    to "same" for odd kernels; chan_sums: float32 [B, conv_sum_chunks(Ho, Wo), Cout] (the layout of conv_cl), not together
    with a residual."""
    b, cin, h, w = x.shape
    kh, kw = kernel
    ph, pw = padding if padding is not None else (kh // 2, kw // 2)
    ho, wo = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
    if wprep.dtype != torch.bfloat16 or wprep.numel() != cout * cin * kh * kw:
        raise RuntimeError("conv_bf16_cl: weight block must hold %d bf16 (conv_bf16_prepare), got %d %s" %
                           (cout * cin * kh * kw, wprep.numel(), wprep.dtype))
    if x.dtype != torch.float32 or (bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout)):
        raise RuntimeError("conv_bf16_cl: x and bias must be float32 (bias of Cout entries)")
    if (out is not None and out.dtype != torch.float32) or (residual is not None and residual.dtype != torch.float32):
        raise RuntimeError("conv_bf16_cl: out and residual must be float32")
    out, head = _conv_operands("conv_bf16_cl", x, wprep, bias, cout, ho, wo, residual, out, chan_sums, conv_sum_chunks)
    args = head + (b, h, w, cin, cout, kh, kw, stride, ph, pw, int(act), _ptr(chan_sums))
    _conv_launch("smos_conv_bf16_cl", "conv_bf16", args, (x, wprep, bias, residual, out, chan_sums), x,
                 lambda: _conv_label("conv_bf16", x, cout, ho, wo, kernel, residual))
    return out


_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def conv_wino_prepare(w, mb):
    """w [Cout, Cin, 3, 3] (BatchNorm folded) -> the weight block of smos_conv_wino_cl: U = G w G^T per (cout, cin) in
    float64, rounded once to float32, in MFMA operand order [cout tile][cin chunk of 16][k-step i][mb][xi][lane][nu] with
    lane = q * 16 + m holding U[xi][nu] of w[ct*16*mb + mb_i*16 + m][chunk*16 + 4*q + i] (include/smos.h)."""
    cout, cin, kh, kw = w.shape
    if (kh, kw) != (3, 3) or cin % 16 or mb not in (1, 2) or cout % (16 * mb):
        raise RuntimeError("conv_wino_prepare: 3x3 kernel, Cin %% 16 == 0 and Cout %% (16 * mb) == 0 required (got %s, mb=%d)"
                           % (tuple(w.shape), mb))
    g = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    u = (g @ w.double() @ g.t()).float()                       # [Cout, Cin, xi, nu]
    #          ct               mb_i m   chunk     q  i  xi nu
    v = u.reshape(cout // (16 * mb), mb, 16, cin // 16, 4, 4, 4, 4)
    v = v.permute(0, 3, 5, 1, 6, 4, 2, 7)                      # -> [ct, chunk, i, mb_i, xi, q, m, nu]
    return v.reshape(-1).contiguous()


def conv_wino_ok(kernel, stride, cin, cout):
    """Shapes smos_conv_wino_cl covers: 3x3, stride 1, "same" padding, Cin and Cout multiples of 16."""
    return tuple(kernel) == (3, 3) and stride == 1 and cin % 16 == 0 and cout % 16 == 0


def conv_wino_mb(cout, n_items16=None):
    """16-channel output blocks per wave: 2 wherever Cout allows it -- half the operand traffic per multiply-add, and faster
    on every layer of the network, the ones with fewer items than resident blocks included (tools/ubench_wino.py)."""
    return 2 if cout % 32 == 0 else 1


def conv_wino_sum_chunks(h, w):
    """Chunks per sample in the channel-sum table of conv_wino_cl(..., chan_sums=...)."""
    return ((h + 7) // 8) * ((w + 31) // 32) * 4


def conv_wino_cl(x, wprep, bias, act, cout, mb=2, residual=None, out=None, chan_sums=None):
    """act(conv3x3(x) + bias [+ residual]) (stride 1, "same" padding) on channels-last [B,C,H,W] views in one launch of the
    Winograd F(2x2, 3x3) kernel (csrc/conv_wino.hip).  wprep = conv_wino_prepare(w, mb).
    chan_sums: optional float32 [B, conv_wino_sum_chunks(H, W), Cout]; not together with a residual."""
    b, cin, h, w = x.shape
    if not conv_wino_ok((3, 3), 1, cin, cout) or mb not in (1, 2) or cout % (16 * mb) or wprep.numel() != 16 * cout * cin:
        raise RuntimeError("conv_wino_cl: unsupported shape %s -> %d (mb=%d)" % (tuple(x.shape), cout, mb))
    out, head = _conv_operands("conv_wino_cl", x, wprep, bias, cout, h, w, residual, out, chan_sums, conv_wino_sum_chunks)
    args = head + (b, h, w, cin, cout, int(mb), int(act), _ptr(chan_sums))
    _conv_launch("smos_conv_wino_cl", "conv_wino", args, (x, wprep, bias, residual, out, chan_sums), x,
                 lambda: _conv_label("conv_cl", x, cout, h, w, (3, 3), residual))
    return out


class BasicBlockPlan:
    """Operands of one BasicBlock (networks/backbone.py:136-159) for smos_basic_block_cl: the two Winograd weight blocks, the
    biases and, for a ChannelAtt block, the gate MLP -- device addresses taken once (the tensors are kept alive here)."""
    __slots__ = ("c", "mb", "gated", "cr", "ptrs", "_keep")

    def __init__(self, w1, b1, w2, b2, gate=None):
        c = w1.shape[0]
        if tuple(w1.shape) != (c, c, 3, 3) or tuple(w2.shape) != (c, c, 3, 3) or c % 16:
            raise RuntimeError("BasicBlockPlan: two [C, C, 3, 3] weights with C %% 16 == 0 expected, got %s / %s"
                               % (tuple(w1.shape), tuple(w2.shape)))
        _require_cuda("BasicBlockPlan", w1, b1, w2, b2, *(gate or ()))
        self.c, self.mb = c, conv_wino_mb(c)
        u1, u2 = conv_wino_prepare(w1, self.mb), conv_wino_prepare(w2, self.mb)
        b1, b2 = b1.float().contiguous(), b2.float().contiguous()
        self.gated = gate is not None
        g = [t.float().contiguous() for t in gate] if self.gated else []
        if self.gated and (tuple(g[0].shape) != (g[0].shape[0], c) or tuple(g[2].shape) != (c, g[0].shape[0])):
            raise RuntimeError("BasicBlockPlan: gate MLP must be [Cr, C], [Cr], [C, Cr], [C]")
        self.cr = g[0].shape[0] if self.gated else 0
        self._keep = (u1, b1, u2, b2, g)
        self.ptrs = (u1.data_ptr(), b1.data_ptr(), u2.data_ptr(), b2.data_ptr()) + \
            (tuple(t.data_ptr() for t in g) if self.gated else (None, None, None, None)) + (self.cr,)


class UnbalanceBlockPlan:
    """Operands of one Unbalance_BasicBlock (networks/multi_view_encoder.py:478-497) for smos_unbalance_block_cl."""
    __slots__ = ("c", "mb", "ptrs_a", "ptrs_b", "ptrs_c", "_keep")

    def __init__(self, wa, ba, wb, bb, wc, bc):
        c = wa.shape[0]
        ka, kb = tuple(wa.shape[2:]), tuple(wb.shape[2:])
        if (tuple(wa.shape[:2]) != (c, c) or tuple(wb.shape[:2]) != (c, c) or tuple(wc.shape) != (c, 2 * c, 3, 3) or
                not conv_wino1d_ok(ka, 1, c, c) or not conv_wino1d_ok(kb, 1, c, c)):
            raise RuntimeError("UnbalanceBlockPlan: unexpected weights %s %s %s" % (tuple(wa.shape), tuple(wb.shape), tuple(wc.shape)))
        _require_cuda("UnbalanceBlockPlan", wa, ba, wb, bb, wc, bc)
        self.c, self.mb = c, conv_wino_mb(c)
        ua, ub = conv_wino1d_prepare(wa, self.mb), conv_wino1d_prepare(wb, self.mb)
        uc = conv_wino_prepare(wc, self.mb)
        ba, bb, bc = (t.float().contiguous() for t in (ba, bb, bc))
        self._keep = (ua, ub, uc, ba, bb, bc)
        self.ptrs_a = (ua.data_ptr(), ba.data_ptr(), ka[0], ka[1])
        self.ptrs_b = (ub.data_ptr(), bb.data_ptr(), kb[0], kb[1])
        self.ptrs_c = (uc.data_ptr(), bc.data_ptr())


def unbalance_block_cl(x, plan, both=None, out=None):
    """Unbalance_BasicBlock.forward on a channels-last [B,C,H,W] view in one foreign call (csrc/blocks.hip): conv_wino1d_cl x 2
    into the halves of `both` [B,2C,H,W], conv_wino_cl over it + x.  Bit-identical to the separate calls."""
    _require_cuda("unbalance_block_cl", x, both, out)
    b, c, h, w = x.shape
    if c != plan.c:
        raise RuntimeError("unbalance_block_cl: %d channels, the block has %d" % (c, plan.c))
    dev = x.device
    if both is None:
        both = empty_cl(b, 2 * c, h, w, dev)
    if out is None:
        out = empty_cl(b, c, h, w, dev)
    if both.shape != (b, 2 * c, h, w) or out.shape != x.shape:
        raise RuntimeError("unbalance_block_cl: both must be [B,2C,H,W] and out have x's shape %s" % (tuple(x.shape),))
    with _on(dev):
        _lib.call("smos_unbalance_block_cl", x.data_ptr(), _cl("unbalance_block_cl", x), *plan.ptrs_a, *plan.ptrs_b, *plan.ptrs_c,
                  both.data_ptr(), _cl("unbalance_block_cl", both), out.data_ptr(), _cl("unbalance_block_cl", out), b, h, w, c,
                  plan.mb, _raw_stream(_dev_index(dev)))
    return out


def gate_channels_ok(c):
    """Channel counts the ChannelAtt gate kernels take where the conv epilogue leaves the pool sums (channel_gate_apply_cl)."""
    return c % 32 == 0 and c <= 256 and 1024 % c == 0


def basic_block_ok(c, gated):
    """Channel counts smos_basic_block_cl takes in the engine (those of the gate kernel where the block has one)."""
    return c % 16 == 0 and (not gated or gate_channels_ok(c))


def basic_block_cl(x, plan, y=None, out=None, ws=None):
    """BasicBlock.forward on a channels-last [B,C,H,W] view in one foreign call (csrc/blocks.hip): the launches of
    conv_wino_cl, conv_wino_cl [, channel_gate_apply_cl] with the same arguments, bit-identical results.  y: scratch map for the
    first conv (allocated if None); ws: >= smos_basic_block_ws_floats floats for a gated block."""
    _require_cuda("basic_block_cl", x, y, out, ws)
    b, c, h, w = x.shape
    if c != plan.c:
        raise RuntimeError("basic_block_cl: %d channels, the block has %d" % (c, plan.c))
    dev = x.device
    if y is None:
        y = empty_cl(b, c, h, w, dev)
    if out is None:
        out = empty_cl(b, c, h, w, dev)
    if y.shape != x.shape or out.shape != x.shape:
        raise RuntimeError("basic_block_cl: y / out must have x's shape %s" % (tuple(x.shape),))
    wsp = None
    if plan.gated:
        if (ws is None or ws.dtype != torch.float32 or not ws.is_contiguous() or
                ws.numel() < _lib.query("smos_basic_block_ws_floats", b, h, w, c)):
            raise RuntimeError("basic_block_cl: a gated block needs smos_basic_block_ws_floats floats of contiguous scratch")
        wsp = ws.data_ptr()
    with _on(dev):
        _lib.call("smos_basic_block_cl", x.data_ptr(), _cl("basic_block_cl", x), *plan.ptrs, y.data_ptr(), _cl("basic_block_cl", y),
                  out.data_ptr(), _cl("basic_block_cl", out), wsp, b, h, w, c, plan.mb, _raw_stream(_dev_index(dev)))
    return out


def msda_fwd_qp(value, qp, h, w, points):
    """value [N, H*W, M, 32] contiguous, qp [N, H*W, M*P*3] contiguous (offsets | logits) -> [N, H*W, M*32]."""
    _require_cuda("msda_fwd_qp", value, qp)
    n, s, m, d = value.shape
    if not (value.is_contiguous() and qp.is_contiguous()) or s != h * w or qp.shape[-1] != m * points * 3 or value.dtype != torch.float32:
        raise RuntimeError("msda_fwd_qp: expected contiguous float32 value [N,H*W,M,D] and qp [N,H*W,M*P*3]")
    out = torch.empty((n, s, m * d), dtype=torch.float32, device=value.device)
    with _on(value.device), profiling.span_f("msda_fwd[%dx%dx%dx%d]", (n, s, m, d)):
        _lib.call("smos_msda_fwd_qp", value.data_ptr(), qp.data_ptr(), out.data_ptr(), n, h, w, m, d, points, _stream(value))
    return out


def add_layer_norm(x, res, gamma, beta, eps=1e-5):
    """LayerNorm(x + res) over the last dimension; x / res contiguous float32 [..., C]."""
    _require_cuda("add_layer_norm", x, res, gamma, beta)
    if not x.is_contiguous() or (res is not None and (not res.is_contiguous() or res.shape != x.shape)):
        raise RuntimeError("add_layer_norm: x and res must be contiguous and of equal shape")
    c = x.shape[-1]
    out = torch.empty_like(x)
    with _on(x.device):
        _lib.call("smos_add_layer_norm", x.data_ptr(), _ptr(res), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), x.numel() // c,
                  c, float(eps), _stream(x))
    return out


# ---------------------------------------------------------------------------------------------
# temporal fusion (csrc/tfusion.hip): the token-wise Linear / LayerNorm / FFN chain of a DeformAttnLayer on the matrix cores
# ---------------------------------------------------------------------------------------------
def _tf_pairs(w):
    """w [O, K] (O, K multiples of 16) -> [O/16, K/16, 64, 4]: pair (o, t) = 64 lanes x float4, lane q * 16 + m holding
    w[16 o + m][16 t + 4 q + 0..3] -- the A operands of the four v_mfma_f32_16x16x4_f32 that multiply k-tile t into output tile o."""
    o, k = w.shape
    v = w.float().reshape(o // 16, 16, k // 16, 4, 4)          # [o, m, t, q, r]
    return v.permute(0, 2, 3, 1, 4).reshape(o // 16, k // 16, 64, 4)


def tfusion_pack_linear(w):
    """w [cout, 128] -> the weight stream of one smos_tfusion_project job: cout zero-padded to a multiple of 64, slot o = the
    eight pairs (o, t = 0..7)."""
    cout, k = w.shape
    if k != 128 or cout > 2048:
        raise RuntimeError("tfusion_pack_linear: expected [<=2048, 128], got %s" % (tuple(w.shape),))
    pad = (cout + 63) // 64 * 64
    wp = torch.zeros((pad, k), dtype=torch.float32, device=w.device)
    wp[:cout] = w
    return _tf_pairs(wp).reshape(-1).contiguous()


class TfusionLayer:
    """Weights of one DeformAttnLayer behind its sampler in the order smos_tfusion_layer streams them, plus (optionally) the
    NEXT layer's [sampling_offsets | attention_weights] projection, which the kernel applies to its fresh output."""

    def __init__(self, out, norm1, lin1, lin2, norm2, next_qproj=None):
        wo, bo = out
        w1, b1 = lin1
        w2, b2 = lin2
        ffn = w1.shape[0]
        if tuple(wo.shape) != (128, 128) or w1.shape[1] != 128 or tuple(w2.shape) != (128, ffn) or ffn % 32:
            raise RuntimeError("TfusionLayer: built for d_model 128 and an FFN width that is a multiple of 32")
        dev = wo.device
        po, p1, p2 = _tf_pairs(wo), _tf_pairs(w1), _tf_pairs(w2)          # [8,8,..], [F/16,8,..], [8,F/16,..]
        slots = [po.reshape(8, 8, 64, 4)]
        # the kernel runs one hidden tile ahead with linear1: linear1(0), then [linear1(j + 1), linear2(j)] ..., linear2(last)
        l2 = p2.permute(1, 0, 2, 3)                                         # [F/16, 8 output tiles, 64, 4]
        n_t = ffn // 16
        slots.append(p1[0:1])
        if n_t > 1:
            slots.append(torch.stack((p1[1:], l2[:-1]), 1).reshape(-1, 8, 64, 4))
        slots.append(l2[-1:])
        self.nq = 0
        bq = torch.zeros(64, dtype=torch.float32, device=dev)
        if next_qproj is not None:
            wq, bqv = next_qproj
            self.nq = int(wq.shape[0])
            if self.nq > 64 or self.nq % 4 or wq.shape[1] != 128:
                raise RuntimeError("TfusionLayer: the next projection must have 4..64 output channels (multiple of 4)")
            wqp = torch.zeros((64, 128), dtype=torch.float32, device=dev)
            wqp[:self.nq] = wq
            bq[:self.nq] = bqv
            slots.append(_tf_pairs(wqp).reshape(4, 8, 64, 4))
        self.stream = torch.cat(slots).reshape(-1).contiguous()
        self.params = torch.cat([bo.float(), norm1[0].float(), norm1[1].float(), b1.float(), b2.float(), norm2[0].float(),
                                 norm2[1].float(), bq]).contiguous()
        self.ffn = int(ffn)
        self.eps1 = float(norm1[2]) if len(norm1) > 2 else 1e-5
        self.eps2 = float(norm2[2]) if len(norm2) > 2 else 1e-5
        if (self.stream.numel() != _lib.query("smos_tfusion_layer_stream_floats", self.ffn, 1 if self.nq else 0) or
                self.params.numel() != _lib.query("smos_tfusion_layer_param_floats", self.ffn)):
            raise RuntimeError("TfusionLayer: packed sizes disagree with the kernel's")


def _token_rows(name, t):
    """(tokens, pitch) of a token matrix [..., C] with contiguous channels and evenly pitched rows."""
    c = t.shape[-1]
    if t.dtype != torch.float32 or t.stride(-1) != 1:
        raise RuntimeError("%s: float32 rows with contiguous channels expected" % name)
    rows = t.reshape(-1, c) if t.is_contiguous() else t
    if rows.dim() != 2:
        raise RuntimeError("%s: a dense [..., C] tensor or a pitched [tokens, C] view expected, got %s / %s" % (name, tuple(t.shape), t.stride()))
    return rows.shape[0], rows.stride(0)


def tfusion_project(jobs):
    """jobs: up to eight (x [..., 128] token rows, wstream = tfusion_pack_linear(W), bias [cout] -- or an int cout for a Linear
    without bias[, out: a [tokens, cout] view with contiguous channels, e.g. a column range of a wider matrix]) -> list of
    [tokens, cout] outputs, ONE launch (csrc/tfusion.hip): the fusion's projections that depend on no previous layer; the
    decoder's tap products.  The jobs may have different token counts."""
    n = len(jobs)
    if not 1 <= n <= 8:
        raise RuntimeError("tfusion_project: 1..8 jobs")
    xs, pit, ws, bs, outs, ops_, couts, toks = ((ctypes.c_void_p * n)(), (ctypes.c_int64 * n)(), (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(),
                                                (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)())
    res = []
    for j, job in enumerate(jobs):
        x, w, b = job[0], job[1], job[2]
        bias = None if isinstance(b, int) else b
        _require_cuda("tfusion_project", x, w, bias)
        tk, pitch = _token_rows("tfusion_project", x)
        if x.shape[-1] != 128:
            raise RuntimeError("tfusion_project: 128-channel token rows expected")
        cout = int(b) if bias is None else int(bias.shape[0])
        if w.numel() != (cout + 63) // 64 * 64 * 128:
            raise RuntimeError("tfusion_project: weight stream of %d floats for %d outputs" % (w.numel(), cout))
        if len(job) > 3 and job[3] is not None:
            out = job[3]
            _require_cuda("tfusion_project", out)
            if out.dim() != 2 or tuple(out.shape) != (tk, cout) or out.stride(1) != 1 or out.dtype != torch.float32:
                raise RuntimeError("tfusion_project: out must be a float32 [tokens, cout] view with contiguous channels")
        else:
            out = torch.empty((tk, cout), dtype=torch.float32, device=x.device)
        res.append(out)
        xs[j], pit[j], ws[j], outs[j], ops_[j], couts[j], toks[j] = x.data_ptr(), pitch, w.data_ptr(), out.data_ptr(), out.stride(0), cout, tk
        bs[j] = _ptr(bias)
    x0 = jobs[0][0]
    label = ("tfusion_project[%s]" % ",".join("%dx128->%d" % (int(toks[j]), int(couts[j])) for j in range(n))
             if profiling.enabled() else None)
    with _on(x0.device), profiling.span(label):
        _lib.call("smos_tfusion_project", n, xs, pit, ws, bs, outs, ops_, couts, toks, _stream(x0))
    return res


def tfusion_layer(sampled, query, prep, out=None):
    """One DeformAttnLayer behind its sampler (multi_view_encoder.py:314-320) in one launch: norm2(q1 + FFN(q1)) with q1 =
    norm1(query + output_proj(sampled)); returns (out [tokens, 128], qp_next [tokens, nq] or None).  sampled: dense
    [..., 128]; query: token rows (may be pitched); prep: TfusionLayer."""
    _require_cuda("tfusion_layer", sampled, query, out)
    tokens, sp = _token_rows("tfusion_layer", sampled)
    tq, qp = _token_rows("tfusion_layer", query)
    if sp != 128 or tq != tokens or sampled.shape[-1] != 128 or query.shape[-1] != 128:
        raise RuntimeError("tfusion_layer: sampled must be dense [tokens, 128] and query hold as many 128-channel rows")
    if out is None:
        out = torch.empty((tokens, 128), dtype=torch.float32, device=sampled.device)
    to, op = _token_rows("tfusion_layer", out)
    if to != tokens or out.shape[-1] != 128:
        raise RuntimeError("tfusion_layer: out must hold [tokens, 128]")
    nxt = torch.empty((tokens, prep.nq), dtype=torch.float32, device=sampled.device) if prep.nq else None
    with _on(sampled.device), profiling.span_f("tfusion_layer[%dx128x%d%s]", (tokens, prep.ffn, "+q%d" % prep.nq if prep.nq else "")):
        _lib.call("smos_tfusion_layer", sampled.data_ptr(), query.data_ptr(), qp, prep.stream.data_ptr(), prep.params.data_ptr(),
                  out.data_ptr(), op, _ptr(nxt), prep.nq, tokens, prep.ffn, prep.eps1, prep.eps2, _stream(sampled))
    return out, nxt


def tap_limbs_split(w):
    """float32 w -> (lo, mid, hi) bfloat16 with hi + mid + lo == w exactly: hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi -
    mid), round-to-nearest-even; both subtractions are exact in float32 (csrc/tap_bf16x3.hip splits the activations the same way)."""
    w = w.float()
    hi = w.to(torch.bfloat16)
    r = w - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return lo, mid, hi


def tap_limbs_pack(w):
    """w [cout, 128] -> the bfloat16 weight stream of one smos_tap_products_bf16x3 job (include/smos.h): cout zero-padded to a
    multiple of 32, [tile of 32 outputs][k step 0..7][lo, mid, hi][lane = 32 h + r][8] with lane (r, h), element j =
    limb[32 tile + r][16 step + 8 h + j]: the B fragments of v_mfma_f32_32x32x16_bf16 in the order the kernel consumes them.
    Works on CPU and GPU tensors."""
    cout, k = w.shape
    if k != 128 or cout > 2048:
        raise RuntimeError("tap_limbs_pack: expected [<=2048, 128], got %s" % (tuple(w.shape),))
    pad = (cout + 31) // 32 * 32
    wp = torch.zeros((pad, k), dtype=torch.float32, device=w.device)
    wp[:cout] = w
    v = torch.stack(tap_limbs_split(wp)).reshape(3, pad // 32, 32, 8, 2, 8)         # [limb, tile, r, step, h, j]
    return v.permute(1, 3, 0, 4, 2, 5).reshape(-1).contiguous()                     # [tile, step, limb, h, r, j]


def tap_limbs_unpack(stream, cout):
    """The inverse of tap_limbs_pack: (lo, mid, hi) float32 [cout, 128] of a packed stream."""
    pad = (cout + 31) // 32 * 32
    v = stream.reshape(pad // 32, 8, 3, 2, 32, 8).permute(2, 0, 4, 1, 3, 5)         # [limb, tile, r, step, h, j]
    return tuple(v.reshape(3, pad, 128)[:, :cout].float())


def tap_products_bf16x3(jobs):
    """jobs: up to eight (x [..., 128] float32 token rows, wlimbs = tap_limbs_pack(W), cout[, out: a [tokens, cout] view with
    contiguous channels, e.g. a column range of a wider matrix]) -> list of [tokens, cout] outputs x W^T, ONE launch
    (csrc/tap_bf16x3.hip): float32 in and out at float32 accuracy, computed as six bf16 limb products per term on the bf16 matrix
    pipe.  The job tuple of tfusion_project without a bias; the jobs may have different token counts."""
    n = len(jobs)
    if not 1 <= n <= 8:
        raise RuntimeError("tap_products_bf16x3: 1..8 jobs")
    xs, pit, ws, outs, ops_, couts, toks = ((ctypes.c_void_p * n)(), (ctypes.c_int64 * n)(), (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(),
                                            (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)())
    res = []
    for j, job in enumerate(jobs):
        x, w, cout = job[0], job[1], int(job[2])
        _require_cuda("tap_products_bf16x3", x, w)
        tk, pitch = _token_rows("tap_products_bf16x3", x)
        if x.shape[-1] != 128:
            raise RuntimeError("tap_products_bf16x3: 128-channel token rows expected")
        if w.dtype != torch.bfloat16 or w.numel() != (cout + 31) // 32 * 32 * 128 * 3 or not w.is_contiguous():
            raise RuntimeError("tap_products_bf16x3: limb stream of %d %s elements for %d outputs" % (w.numel(), w.dtype, cout))
        if len(job) > 3 and job[3] is not None:
            out = job[3]
            _require_cuda("tap_products_bf16x3", out)
            if out.dim() != 2 or tuple(out.shape) != (tk, cout) or out.stride(1) != 1 or out.dtype != torch.float32:
                raise RuntimeError("tap_products_bf16x3: out must be a float32 [tokens, cout] view with contiguous channels")
        else:
            out = torch.empty((tk, cout), dtype=torch.float32, device=x.device)
        res.append(out)
        xs[j], pit[j], ws[j], outs[j], ops_[j], couts[j], toks[j] = x.data_ptr(), pitch, w.data_ptr(), out.data_ptr(), out.stride(0), cout, tk
    x0 = jobs[0][0]
    # the label of the fp32 form: bench.py's byte / FLOP model and profiles/label_durations.py price the launch as before
    label = ("tfusion_project[%s]" % ",".join("%dx128->%d" % (int(toks[j]), int(couts[j])) for j in range(n))
             if profiling.enabled() else None)
    with _on(x0.device), profiling.span(label):
        _lib.call("smos_tap_products_bf16x3", n, xs, pit, ws, outs, ops_, couts, toks, _stream(x0))
    return res


class TapWeights:
    """The per-tap matrices of a 3x3 convolution's input channels [c0, c1) in the forms upconv3x3 uses.  Everything
    derived from the weights lives in this object (owned by the engine that folded them) -- never in a cache keyed by
    the weights' address: a freed model's address is handed to the next model."""

    def __init__(self, w, c0, c1):
        cout = w.shape[0]
        self.cout, self.cin = cout, c1 - c0
        self.nk = w[:, c0:c1].permute(2, 3, 0, 1).reshape(9 * cout, c1 - c0).float().contiguous()   # tap-major, t = 3 ky + kx
        self.kn = self.nk.t().contiguous()                      # [Cin, 9*Cout]: the layout the library GEMM is fastest in
        self.zero = torch.zeros(9 * cout, dtype=torch.float32, device=w.device)
        self._conv = None
        self._stream = None
        self._limbs = None

    def stream(self, parts=1):
        """the tap matrices in the operand order of smos_tfusion_project (Cin = 128), cut into `parts` equal output ranges"""
        if self._stream is None:
            self._stream = {}
        if parts not in self._stream:
            n = self.nk.shape[0] // parts
            self._stream[parts] = [tfusion_pack_linear(self.nk[i * n:(i + 1) * n]) for i in range(parts)]
        return self._stream[parts]

    def limb_stream(self, parts=1):
        """the same column ranges as bf16 limb streams, the operand of smos_tap_products_bf16x3 (Cin = 128)"""
        if self._limbs is None:
            self._limbs = {}
        if parts not in self._limbs:
            n = self.nk.shape[0] // parts
            self._limbs[parts] = [tap_limbs_pack(self.nk[i * n:(i + 1) * n]) for i in range(parts)]
        return self._limbs[parts]

    def conv_operand(self):
        if self._conv is None:
            self._conv = conv_prepare(self.nk.view(9 * self.cout, self.cin, 1, 1), 4)
        return self._conv


def upconv_tap_weights(w, c0, c1):
    """w [Cout, Cin, 3, 3] -> TapWeights of input channels [c0, c1)."""
    return TapWeights(w, c0, c1)


# The nine tap products: library GEMM by default; "conv" runs them on the own kernel as one 1x1 convolution with 9*C outputs
# (measured in the step: 236.6 vs 238.8 scans/s -- K = 128 is only four stages per tile, so the epilogue dominates).
# "tf" (default since round 4): the token-wise Linear kernel of the temporal fusion (csrc/tfusion.hip), both sources in one launch:
# 0.26 -> 0.2x ms per step against the library GEMMs ("mm").  "x3" (default): the same jobs on the bf16 matrix pipe as three
# exact bf16 limbs per fp32 operand (csrc/tap_bf16x3.hip), fp32 accuracy kept (profiles/tap_bf16x3.txt)
_TAP_GEMM = os.environ.get("SMOS_TAP_GEMM", "x3")
_TAP_GEMM_OWN = _TAP_GEMM == "conv"
_TAP_PARTS = int(os.environ.get("SMOS_TAP_PARTS", "3"))      # column ranges per source in the tap-product launch (tuning knob)
# x pass and y pass in one launch (smos_upconv_xy) where the geometry allows; "0": always the two launches (A/B, same results)
_UPCONV_XY = os.environ.get("SMOS_UPCONV_XY", "1") != "0"
# bytes of a tap-product matrix one smos_tfusion_project job may cover (it addresses its operands with 32-bit buffer offsets) and
# the most rows of one job (the kernel takes fewer than 2^22 tokens); upconv3x3 cuts larger sources into row ranges of 64n rows
_TAP_JOB_BYTES = (1 << 31) - 4096
_TAP_JOB_ROWS = (1 << 22) - 64


def upconv_tap_products(x, wt):
    """z [B*Hs*Ws, 9*C]: the nine tap products W_t x of a channels-last source map x [B,Cin,Hs,Ws] at its own resolution."""
    b, cin, hs, ws = x.shape
    if _TAP_GEMM_OWN and cin % 32 == 0 and (9 * wt.cout) % 128 == 0:
        return conv_cl(x, wt.conv_operand(), None, 0, 9 * wt.cout, (1, 1), mt=4).permute(0, 2, 3, 1).reshape(b * hs * ws, 9 * wt.cout)
    rows = x.permute(0, 2, 3, 1).reshape(b * hs * ws, cin)     # no copy for a dense channels-last map
    # addmm with a zero bias on the [Cin, 9*C] copy of the weights: the library picks a faster kernel for this form than
    # for mm(rows, nk.t()) (tools/ubench_tapgemm.py: 0.182 vs 0.207 ms at 65536 x 128 x 1152); adding 0 changes no value
    return torch.addmm(wt.zero, rows, wt.kn)


def upconv3x3(conv_a, bias, sources, act, out=None):
    """act(conv_a + bias + sum over sources of conv3x3(bilinear_up(x_src), W_src)) without upsampling (csrc/upconv.hip).
    conv_a: channels-last [B,C,Ho,Wo] view (direct conv of the non-upsampled channels); sources: list of (x_cl
    [B,Cin,Hs,Ws] channels-last view with dense rows, tap weights from upconv_tap_weights[, tap products from
    upconv_tap_products: computed here when absent]) -- one or two."""
    _require_cuda("upconv3x3", conv_a, bias, out)
    b, c, ho, wo = conv_a.shape
    if out is None:
        out = conv_a
    st = _stream(conv_a)
    if not 1 <= len(sources) <= 2:
        raise RuntimeError("upconv3x3: one or two upsampled sources, got %d" % len(sources))
    fused = _UPCONV_XY and all(_lib.query("smos_upconv_xy_ok", src[0].shape[2], ho) for src in sources)
    zs, ts = [], []
    pre = {}
    if _TAP_GEMM in ("tf", "x3"):
        # the tap products of every source that has none yet, as jobs of the token-wise Linear kernel: one launch for the usual
        # sizes; a product matrix of 2 GiB and more (8 and more concurrent streams) is cut into row ranges below 2 GiB (a job
        # addresses its operands with 32-bit buffer offsets) and takes as many launches of up to 8 jobs as that needs
        todo = [i for i, src in enumerate(sources) if (len(src) < 3 or src[2] is None) and src[0].shape[1] == 128 and 9 * src[1].cout <= 2048]
        if todo:
            # every source's outputs in `parts` column ranges = parts x len(todo) jobs of 64-token blocks:
            # column ranges shorten the last, partly empty round of resident blocks (tools/ubench_taps.py: 0.230 / 0.213 / 0.211 ms for 1 / 2 / 3 ranges; library GEMMs 0.278)
            x3 = _TAP_GEMM == "x3"        # the bf16 limb kernel walks 32-output tiles, the fp32 one slots of 64
            parts = _TAP_PARTS if len(todo) * _TAP_PARTS <= 8 and (9 * sources[todo[0]][1].cout) % ((32 if x3 else 64) * _TAP_PARTS) == 0 else 1
            jobs = []
            for i in todo:
                x, wt = sources[i][0], sources[i][1]
                rows = x.permute(0, 2, 3, 1).reshape(-1, 128)
                z = torch.empty((rows.shape[0], 9 * wt.cout), dtype=torch.float32, device=x.device)
                pre[i] = z
                n = 9 * wt.cout // parts
                limit = min(_TAP_JOB_ROWS, _TAP_JOB_BYTES // (9 * wt.cout * 4) // 64 * 64)    # rows whose z (and x) slice stays below 2 GiB
                for r0 in range(0, rows.shape[0], limit):
                    r1 = min(r0 + limit, rows.shape[0])
                    for k, ws_k in enumerate(wt.limb_stream(parts) if x3 else wt.stream(parts)):
                        jobs.append((rows[r0:r1], ws_k, n, z[r0:r1, k * n:(k + 1) * n]))
            for j0 in range(0, len(jobs), 8):
                (tap_products_bf16x3 if x3 else tfusion_project)(jobs[j0:j0 + 8])
    with _on(conv_a.device):
        for i_src, src in enumerate(sources):
            x, wt = src[0], src[1]
            hs, ws, cin = x.shape[2], x.shape[3], x.shape[1]
            if wt.cin != cin or wt.cout != c:
                raise RuntimeError("upconv3x3: tap weights are for %d -> %d channels, got %d -> %d" % (wt.cin, wt.cout, cin, c))
            z = src[2] if len(src) > 2 and src[2] is not None else (pre[i_src] if i_src in pre else upconv_tap_products(x, wt))
            if tuple(z.shape) != (b * hs * ws, 9 * c) or not z.is_contiguous():
                raise RuntimeError("upconv3x3: tap products must be a contiguous [B*Hs*Ws, 9*C] matrix, got %s" % (tuple(z.shape),))
            zs.append((z, hs, ws))
            if fused:
                continue
            t = torch.empty((b, 3, hs, wo, c), dtype=torch.float32, device=conv_a.device)
            with profiling.span_f("upconv_xpass[%dx%dx%dx%d->%d]", (b, hs, ws, c, wo)):
                _lib.call("smos_upconv_xpass", z.data_ptr(), t.data_ptr(), b, hs, ws, c, wo, st)
            ts.append((t, hs))
        if fused:
            z1, h1, w1 = zs[0]
            z2, h2, w2 = zs[1] if len(zs) > 1 else (None, 0, 0)
            with profiling.span("upconv_xy[%dx%dx%dx%d<-%s]" % (b, ho, wo, c, "+".join("%dx%d" % (h, w) for _, h, w in zs))
                                if profiling.enabled() else None):
                _lib.call("smos_upconv_xy", conv_a.data_ptr(), _cl("upconv3x3", conv_a), bias.data_ptr(), z1.data_ptr(), h1, w1,
                          _ptr(z2), h2, w2, out.data_ptr(), _cl("upconv3x3", out), b, ho, wo, c, int(act), st)
            return out
        t1, h1 = ts[0]
        t2, h2 = ts[1] if len(ts) > 1 else (None, 0)
        with profiling.span_f("upconv_ypass[%dx%dx%dx%d]", (b, ho, wo, c)):
            _lib.call("smos_upconv_ypass", conv_a.data_ptr(), _cl("upconv3x3", conv_a), bias.data_ptr(), t1.data_ptr(), h1,
                      _ptr(t2), h2, out.data_ptr(), _cl("upconv3x3", out), b, ho, wo, c, int(act), st)
    return out


def upconv_xy_units(conv_a, bias, z1, z2, act, strip, max_blocks=0, out=None):
    """smos_upconv_xy_units: the one-launch interpolation of upconv3x3 from given tap products, with the unit geometry
    given -- `strip` output rows per unit of work (8, 16 or 32) and at most `max_blocks` blocks (0: no cap).  z1, z2: (z
    [B*Hs*Ws, 9*C] contiguous, Hs, Ws) or None (at least one).  conv_a, out: channels-last [B,C,Ho,Wo] views (out=None:
    in place).  Same results for every strip and cap (tests, tools/ubench_upconv.py)."""
    _require_cuda("upconv_xy_units", conv_a, bias, out, z1 and z1[0], z2 and z2[0])
    b, c, ho, wo = conv_a.shape
    if out is None:
        out = conv_a
    for z in (z1, z2):
        if z is not None and (tuple(z[0].shape) != (b * z[1] * z[2], 9 * c) or not z[0].is_contiguous()):
            raise RuntimeError("upconv_xy_units: tap products must be a contiguous [B*Hs*Ws, 9*C] matrix, got %s" % (tuple(z[0].shape),))
    (p1, h1, w1), (p2, h2, w2) = ((z[0].data_ptr(), z[1], z[2]) if z is not None else (None, 0, 0) for z in (z1, z2))
    with _on(conv_a.device):
        _lib.call("smos_upconv_xy_units", conv_a.data_ptr(), _cl("upconv_xy_units", conv_a), bias.data_ptr(), p1, h1, w1, p2, h2,
                  w2, out.data_ptr(), _cl("upconv_xy_units", out), b, ho, wo, c, int(act), int(strip), int(max_blocks),
                  _stream(conv_a))
    return out


# the layout upconv3x3_train returns: "cl" the channels-last-strided map its kernels write, "nchw" a contiguous copy of it
# (a development knob for that one A/B, read once at import -- unlike conv1_fused, which is read per call; DESIGN.md
# 4.9b has the measurement behind the default)
_CONV1_OUT = os.environ.get("SMOS_CONV1_OUT", "cl")


def _as_cl(t, dense=False):
    """t [B,C,H,W] as a channels-last view the kernels can read (``_cl``; dense: rows of exactly C floats): t itself where
    its strides already say so, else a channels-last copy."""
    b, c, h, w = t.shape
    s0, s1, s2, pitch = t.stride()
    if s1 == 1 and s2 == w * pitch and (b == 1 or s0 == h * w * pitch) and (pitch == c if dense else pitch >= c) and pitch % 4 == 0 \
            and t.data_ptr() % 16 == 0:
        return t
    out = empty_cl(b, c, h, w, t.device)
    out.copy_(t)
    return out


def upconv_adjoint(g, hs, ws, max_blocks=0, out=None, scratch=None):
    """The adjoint of upconv3x3's two passes for one source of Hs x Ws pixels (csrc/upconv_bwd.hip): g, the gradient of the
    output as a channels-last [B,C,Ho,Wo] view, -> G [B*Hs*Ws, 9*C], the gradient of that source's tap products, in the
    layout of the forward's z.  Two launches (y adjoint into ``scratch`` [B,3,Hs,Wo,C], x adjoint into ``out``), each element
    summed by one thread in a fixed order: the same bits on every run and for every ``max_blocks`` (a cap on both grids, 0:
    none).  out: a float32 [B*Hs*Ws, 9*C] view with contiguous channels (e.g. a column range of a wider matrix)."""
    _require_cuda("upconv_adjoint", g, out, scratch)
    if g.dim() != 4 or g.dtype != torch.float32:
        raise RuntimeError("upconv_adjoint: g must be a float32 [B,C,Ho,Wo] map, got %s %s" % (tuple(g.shape), g.dtype))
    b, c, ho, wo = g.shape
    hs, ws = int(hs), int(ws)
    gp = _cl("upconv_adjoint", g)
    if scratch is None:
        scratch = torch.empty((b, 3, hs, wo, c), dtype=torch.float32, device=g.device)
    elif scratch.dtype != torch.float32 or scratch.numel() != b * 3 * hs * wo * c or not scratch.is_contiguous():
        raise RuntimeError("upconv_adjoint: scratch must be a contiguous float32 [B,3,Hs,Wo,C] tensor")
    if out is None:
        out = torch.empty((b * hs * ws, 9 * c), dtype=torch.float32, device=g.device)
    elif out.dim() != 2 or tuple(out.shape) != (b * hs * ws, 9 * c) or out.stride(1) != 1 or out.dtype != torch.float32:
        raise RuntimeError("upconv_adjoint: out must be a float32 [B*Hs*Ws, 9*C] view with contiguous channels")
    zp = out.stride(0) if out.shape[0] > 1 else max(out.stride(0), 9 * c)
    with _on(g.device):
        st = _stream(g)
        with profiling.span_f("upconv_bwd_ypass[%dx%dx%dx%d->%d]", (b, ho, wo, c, hs)):
            _lib.call("smos_upconv_bwd_ypass", g.data_ptr(), gp, scratch.data_ptr(), b, ho, wo, c, hs, int(max_blocks), st)
        with profiling.span_f("upconv_bwd_xpass[%dx%dx%dx%d<-%d]", (b, hs, ws, c, wo)):
            _lib.call("smos_upconv_bwd_xpass", scratch.data_ptr(), out.data_ptr(), zp, b, hs, ws, c, wo, int(max_blocks), st)
    return out


def _upconv_dx(gz, w, shape):
    """dX = G nk: the data gradient of one source, [B,128,Hs,Ws] (channels-last strides), from G [P, 9*C] and w [C,128,3,3]."""
    b, cin, hs, ws = shape
    nk = w.permute(2, 3, 0, 1).reshape(-1, cin).float()           # [9*C, Cin], tap-major: TapWeights.nk
    return torch.mm(gz, nk).view(b, hs, ws, cin).permute(0, 3, 1, 2)


def _upconv_dw(gz, x):
    """dW from dNK = G^T X: the weight gradient of one source, [C,128,3,3], from G [P, 9*C] and x [B,128,Hs,Ws]."""
    cin = x.shape[1]
    rows = _as_cl(x, dense=True).permute(0, 2, 3, 1).reshape(-1, cin)
    return torch.mm(gz.t(), rows).view(3, 3, -1, cin).permute(2, 3, 0, 1)


class _Upconv3x3Train(torch.autograd.Function):
    """ops.upconv3x3_train.  Kept for the backward: the sources and their weights as they came in -- no activation, no tap
    product, no resized map."""

    @staticmethod
    def forward(ctx, conv_a, *xw):
        b, c, ho, wo = conv_a.shape
        a = _as_cl(conv_a)
        out = a if a is not conv_a else empty_cl(b, c, ho, wo, conv_a.device)      # a fresh copy is finished in place
        srcs = [(_as_cl(xw[i], dense=True), TapWeights(xw[i + 1], 0, xw[i + 1].shape[1])) for i in range(0, len(xw), 2)]
        upconv3x3(a, torch.zeros(c, dtype=torch.float32, device=conv_a.device), srcs, 0, out=out)
        ctx.save_for_backward(*xw)
        return out.contiguous() if _CONV1_OUT == "nchw" else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xw = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = [g if need[0] else None]
        gcl = None
        for i in range(0, len(xw), 2):
            x, w = xw[i], xw[i + 1]
            dx = dw = None
            if need[1 + i] or need[2 + i]:
                if gcl is None:
                    gcl = _as_cl(g.float())
                gz = upconv_adjoint(gcl, x.shape[2], x.shape[3])
                if need[1 + i]:
                    dx = _upconv_dx(gz, w, x.shape)
                if need[2 + i]:
                    dw = _upconv_dw(gz, x)
            grads += [dx, dw]
        return tuple(grads)


def upconv3x3_train(conv_a, sources):
    """``conv_a + sum over sources of conv3x3(bilinear_up(x_src, align_corners=True), w_src, padding 1)`` as one autograd op
    that never builds the resized maps: the training form of ``upconv3x3``.

    conv_a [B,C,Ho,Wo]: the ordinary convolution of the channels that are not upsampled, computed by the caller; sources: one
    or two (x_src [B,128,Hs,Ws], w_src [C,128,3,3]); float32 on the GPU, any strides (what is not a channels-last view is
    copied into one).  No bias and no activation.  The forward IS ``upconv3x3`` (tap products at source resolution, then the
    interpolation launch), with the tap weights rebuilt from w_src on the device at every call.  The backward returns the
    output gradient itself for conv_a and, per source, runs the adjoint of the interpolation in HIP (``upconv_adjoint``)
    followed by two library matrix products at source resolution, dX = G nk and dW from G^T X; a gradient nobody needs is
    not computed.  Returns a logical [B,C,Ho,Wo] tensor with channels-last strides."""
    _require_cuda("upconv3x3_train", conv_a)
    if conv_a.dim() != 4 or conv_a.dtype != torch.float32 or conv_a.numel() == 0:
        raise RuntimeError("upconv3x3_train: conv_a must be a non-empty float32 [B,C,Ho,Wo] map, got %s %s" % (tuple(conv_a.shape), conv_a.dtype))
    b, c = conv_a.shape[:2]
    if c % 4 or 9 * c > 2048:
        raise RuntimeError("upconv3x3_train: %d output channels; the tap-product kernels take multiples of 4 up to 224" % c)
    sources = list(sources)
    if not 1 <= len(sources) <= 2:
        raise RuntimeError("upconv3x3_train: one or two upsampled sources, got %d" % len(sources))
    flat = []
    for i, src in enumerate(sources):
        if len(src) != 2:
            raise RuntimeError("upconv3x3_train: source %d must be (x_src, w_src)" % i)
        x, w = src
        _require_cuda("upconv3x3_train", x, w)
        if x.dim() != 4 or x.dtype != torch.float32 or x.shape[0] != b or x.shape[1] != 128 or x.numel() == 0:
            raise RuntimeError("upconv3x3_train: source %d is %s %s, want float32 [%d,128,Hs,Ws]" % (i, tuple(x.shape), x.dtype, b))
        if tuple(w.shape) != (c, 128, 3, 3) or w.dtype != torch.float32:
            raise RuntimeError("upconv3x3_train: weights of source %d are %s %s, want float32 [%d,128,3,3]" % (i, tuple(w.shape), w.dtype, c))
        if x.device != conv_a.device or w.device != conv_a.device:
            raise RuntimeError("upconv3x3_train: source %d on %s / %s, conv_a on %s" % (i, x.device, w.device, conv_a.device))
        flat += [x, w]
    return _Upconv3x3Train.apply(conv_a, *flat)


STEM_TAPS = (1, 2, 2, 4)      # 3x3 taps that reach an output pixel under stride 2, per parity class (y&1)*2 + (x&1)
_STEM_Y = ("stem_y0", "stem_y1", "stem_y2", "stem_y3")      # scratch tags of the per-class GEMM outputs


def stem_prepare_weights(wa, wp):
    """wa [Cout,Cin,3,3], wp [Cout,Cin,1,1] (BatchNorm folded) -> 4 tensors in the MFMA operand order smos_stem_gemm
    expects: [(taps+1), Cin/2, 64], entry (mt, s, lane) = W[mt*32 + (lane & 31)][(lane >> 5) * (Cin/2) + s]."""
    cout, cin = wa.shape[0], wa.shape[1]
    out = []
    for cls in range(4):
        ey, ex = cls >> 1, cls & 1
        kys, kxs = ((0, 2) if ey else (1,)), ((0, 2) if ex else (1,))
        w = torch.cat([wa[:, :, ky, kx] for ky in kys for kx in kxs] + [wp[:, :, 0, 0]], 0).float()      # [(taps+1)*Cout, Cin]
        km = w.shape[0] // 32
        out.append(w.view(km, 32, 2, cin // 2).permute(0, 3, 2, 1).reshape(km, cin // 2, 64).contiguous())
    return out


class StemPlan:
    """Occupancy of the input grid of one frame (csrc/stem.hip): which cells hold points, in which compact row.
    meta (device, 12 x int32): [4..7] first row of each parity class, [8..11] one past its last row; meta[11] = rows."""

    def __init__(self, b, h, w, row_cell, row_of, meta, rows):
        self.b, self.h, self.w = b, h, w
        self.row_cell, self.row_of, self.meta, self.rows = row_cell, row_of, meta, rows

    def class_rows(self):
        """device tensor [4]: occupied cells per parity class (y & 1) * 2 + (x & 1)"""
        return self.meta[8:12] - self.meta[4:8]


def stem_plan(coord, h, w, row_floats=0):
    """coord [B,T,N,K(,1)] float32 contiguous -> StemPlan: marks the cells the points fall into and compacts them (rows
    ordered by parity class, sample, position) in two launches (mark, single-pass scan).  row_floats > 0 also provides the
    compact row table ``plan.rows`` [min(B*H*W, B*T*N), row_floats] with its existing rows zero-filled (by the scan kernel).
    Everything stays on the device; every buffer is per-stream scratch, valid until the next plan on the stream."""
    _require_cuda("stem_plan", coord)
    if coord.dtype != torch.float32 or not coord.is_contiguous():
        raise RuntimeError("stem_plan: coord must be contiguous float32")
    b, t, n, k = coord.shape[:4]
    dev = coord.device
    cells = b * h * w
    words = _lib.query("smos_stem_scan_state_words", cells)
    if words < 0:
        raise RuntimeError("stem_plan: grid too large for the scan")
    flags = shared.get("stem_flags", (cells,), torch.int32, dev, zero=True)      # left all-zero by the scan
    state = shared.get("stem_scan_state", (words,), torch.int64, dev)
    row_cell = shared.get("stem_row_cell", (cells,), torch.int32, dev)
    row_of = shared.get("stem_row_of", (cells,), torch.int32, dev)
    meta = shared.get("stem_meta", (12,), torch.int32, dev, zero=True)
    rows = None
    if row_floats:
        # capacity: an occupied cell holds at least one point, so min(cells, points) rows always suffice
        rows = shared.get("stem_rows", (min(cells, b * t * n), row_floats), torch.float32, dev)
    st = _stream(coord)
    with _on(dev), profiling.span_f("stem_mark+scan[%dx%dx%d]", (b, h, w)):
        _lib.call("smos_stem_mark", coord.data_ptr(), k, b, t, n, h, w, flags.data_ptr(), state.data_ptr(), st)
        _lib.call("smos_stem_scan", flags.data_ptr(), b, h, w, state.data_ptr(), row_cell.data_ptr(), row_of.data_ptr(),
                  meta.data_ptr(), _ptr(rows), row_floats, st)
    return StemPlan(b, h, w, row_cell, row_of, meta, rows)


def pointnet_scatter_rows(xyzi, coord, w1, b1, w2, b2, plan, pts_out=None, n_live=None):
    """pointnet_scatter into the COMPACT row table of `plan` (stem_plan(..., row_floats=T*64)): returns plan.rows, a view of
    this stream's scratch (valid until the next plan on the stream); only the first plan.meta[11] rows exist (zero-filled by
    the plan's scan) -- the dense grid is never materialised."""
    _require_cuda("pointnet_scatter_rows", xyzi, coord, w1, b1, w2, b2, pts_out, n_live)
    live = _live_ptr("pointnet_scatter_rows", n_live)
    b, t, cin, n = xyzi.shape[:4]
    k = coord.shape[3]
    if not (xyzi.is_contiguous() and coord.is_contiguous()):
        raise RuntimeError("pointnet_scatter_rows: xyzi and coord must be contiguous")
    cout = w2.shape[0]
    rows = plan.rows
    if rows is None or rows.shape[1] != t * cout:
        raise RuntimeError("pointnet_scatter_rows: the plan carries no row table of %d floats per row" % (t * cout))
    po_b = po_n = 0
    if pts_out is not None:
        po_b, po_n = _rows("pointnet_scatter_rows", pts_out, cout)
    st = _stream(xyzi)
    # the span holds exactly ONE kernel, so its HIP-event mean is comparable with rocprofv3's per-kernel mean
    with _on(xyzi.device), profiling.span_f("pointnet_scatter[%dx%dx%d->%dx%d]", (b, t, n, plan.h, plan.w)):
        _lib.call("smos_pointnet_scatter_rows", xyzi.data_ptr(), coord.data_ptr(), k, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                  b2.data_ptr(), rows.data_ptr(), plan.row_of.data_ptr(), _ptr(pts_out), po_b, po_n, b, t, n, plan.h, plan.w, cin,
                  w1.shape[0], cout, live, st)
    return rows


def sparse_downsample(src, plan, wprep, bias, compact, out=None):
    """DownSample2D(stride 2) on the occupied cells only (csrc/stem.hip): per-class MFMA GEMM + per-pixel assembly.
    src: the compact row table of pointnet_scatter_rows (compact=True) or the dense channels-last grid [B,H,W,Cin]
    (compact=False).  Returns the channels-last [B,Cout,H/2,W/2] view.  No host synchronisation."""
    _require_cuda("sparse_downsample", src, bias, out, *wprep)
    b, h, w = plan.b, plan.h, plan.w
    cin = src.shape[-1]
    dev = src.device
    if src.dtype != torch.float32 or not src.is_contiguous() or (not compact and src.numel() != b * h * w * cin):
        raise RuntimeError("sparse_downsample: src must be contiguous float32 with B*H*W rows of Cin")
    if compact and src.dim() != 2:
        raise RuntimeError("sparse_downsample: the compact row table is [rows, Cin]")
    cout = bias.shape[0]
    per = b * (h // 2) * (w // 2)
    ys = [shared.get(tag, (per, (taps + 1) * cout), torch.float32, dev)                # worst-case capacity
          for tag, taps in zip(_STEM_Y, STEM_TAPS)]
    if out is None:
        out = empty_cl(b, cout, (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1, dev)
    y_ptrs = (ctypes.c_void_p * 4)(*[y.data_ptr() for y in ys])
    w_ptrs = (ctypes.c_void_p * 4)(*[wt.data_ptr() for wt in wprep])
    st = _stream(src)
    tag = "[%dx%dx%dx%d]" % (b, h, w, cin) if profiling.enabled() else ""
    with _on(dev):
        with profiling.span("stem_gemm" + tag):
            _lib.call("smos_stem_gemm", src.data_ptr(), None if compact else plan.row_cell.data_ptr(), plan.meta.data_ptr(), w_ptrs,
                      y_ptrs, cin, cout, st)
        with profiling.span("stem_epilogue" + tag):
            _lib.call("smos_stem_epilogue", y_ptrs, plan.meta.data_ptr(), plan.row_of.data_ptr(), bias.data_ptr(), out.data_ptr(),
                      _cl("sparse_downsample", out), b, h, w, cout, st)
    return out


# ---------------------------------------------------------------------------------------------
# channels-last engine kernels: tensors are logical [B, C, H, W] with channels_last strides (possibly a channel
# slice of a wider channels-last buffer)
# ---------------------------------------------------------------------------------------------
_WINO1D_KERNELS = ((5, 3), (7, 3), (3, 5), (3, 7))


def conv_wino1d_ok(kernel, stride, cin, cout, residual=None, chan_sums=None):
    """Shapes smos_conv_wino1d_cl covers: 5x3 / 7x3 / 3x5 / 3x7, stride 1, "same" padding, Cin and Cout multiples of 16, no
    residual / channel sums (the Unbalance branches have neither)."""
    return (tuple(kernel) in _WINO1D_KERNELS and stride == 1 and cin % 16 == 0 and cout % 16 == 0 and residual is None and
            chan_sums is None)


def conv_wino1d_prepare(w, mb):
    """w [Cout, Cin, KH, KW] (BatchNorm folded; one extent 3, the other 5 or 7) -> the weight block of smos_conv_wino1d_cl:
    U = G g along the 3-tap axis per (cout, cin, long-axis tap) in float64, rounded once to float32, in MFMA operand order
    [cout tile][cin chunk of 16][k-step i][long tap][mb][lane][position], lane = q * 16 + m holding the four positions of
    w[ct*16*mb + mb_i*16 + m][chunk*16 + 4*q + i] (include/smos.h)."""
    cout, cin, kh, kw = w.shape
    if (kh, kw) not in _WINO1D_KERNELS or cin % 16 or mb not in (1, 2) or cout % (16 * mb):
        raise RuntimeError("conv_wino1d_prepare: 5x3 / 7x3 / 3x5 / 3x7 kernel, Cin %% 16 == 0 and Cout %% (16 * mb) == 0 required "
                           "(got %s, mb=%d)" % (tuple(w.shape), mb))
    g = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    wl = w.double() if kw == 3 else w.double().transpose(2, 3)      # [Cout, Cin, long tap, short tap]
    kl = wl.shape[2]
    u = (wl @ g.t()).float()                                        # [Cout, Cin, long tap, position]
    #          ct               mb_i m   chunk     q  i  kl  pos
    v = u.reshape(cout // (16 * mb), mb, 16, cin // 16, 4, 4, kl, 4)
    v = v.permute(0, 3, 5, 6, 1, 4, 2, 7)                           # -> [ct, chunk, i, kl, mb_i, q, m, pos]
    return v.reshape(-1).contiguous()


def conv_wino1d_cl(x, wprep, bias, act, cout, kernel, mb=2, out=None):
    """act(conv(x) + bias) (stride 1, "same" padding) for a 5x3 / 7x3 / 3x5 / 3x7 kernel on channels-last [B,C,H,W] views in
    one launch of the 1-D Winograd F(2, 3) kernel (csrc/conv_wino1d.hip).  wprep = conv_wino1d_prepare(w, mb)."""
    b, cin, h, w = x.shape
    kh, kw = kernel
    if not conv_wino1d_ok(kernel, 1, cin, cout) or mb not in (1, 2) or cout % (16 * mb) or wprep.numel() != 4 * max(kh, kw) * cout * cin:
        raise RuntimeError("conv_wino1d_cl: unsupported shape %s -> %d k%dx%d (mb=%d)" % (tuple(x.shape), cout, kh, kw, mb))
    out, head = _conv_operands("conv_wino1d_cl", x, wprep, bias, cout, h, w, out=out)
    args = head[:4] + head[6:] + (b, h, w, cin, cout, kh, kw, int(mb), int(act))      # this kernel takes no residual
    _conv_launch("smos_conv_wino1d_cl", "conv_wino1d", args, (x, wprep, bias, out), x,
                 lambda: _conv_label("conv_cl", x, cout, h, w, kernel))
    return out


ConvSwitches = collections.namedtuple("ConvSwitches", "wino wino1d conv_rows conv_rows_mt", defaults=(True, True, 3, 1))


def conv_route(cin, cout, kernel, stride, n_out_pixels, has_residual, has_sums, switches):
    """(family, tile) of the fp32 kernel a conv layer runs on, from its shape alone -- the caller has settled that the own
    kernels cover it (conv_cl_supported).  family "wino" / "wino1d" (tile = mb, 16-channel output blocks per wave) or "rows" /
    "igemm" (tile = mt, 32-channel blocks); `switches`: anything with the A/B attributes of ConvSwitches (InferenceEngine has
    them).  Plain numbers in, no library call: the table is pinned in tests/test_host_conv_route.py."""
    if switches.wino and conv_wino_ok(kernel, stride, cin, cout):
        return "wino", conv_wino_mb(cout)
    if switches.wino1d and not has_residual and not has_sums and conv_wino1d_ok(kernel, stride, cin, cout):
        return "wino1d", conv_wino_mb(cout)
    mt = conv_mt(cout, n_out_pixels, has_residual)
    if switches.conv_rows and mt <= switches.conv_rows_mt and conv_rows_ok(kernel, stride, cin, cout) and kernel[1] >= switches.conv_rows:
        return "rows", mt
    return "igemm", mt


class ConvLayer:
    """One folded conv weight w [Cout, Cin, KH, KW] with its operand-ordered copies, each made on first use: keyed by what
    conv_route returns, plus "bf16".  Its owner keys it by id(w); it holds w, so that id stays w's.
    ran_bf16: bf16 engines note here whether the layer's last launch ran on the bf16 kernel (None: not launched)."""
    __slots__ = ("w", "packed", "ran_bf16")
    _PREPARE = {"wino": conv_wino_prepare, "wino1d": conv_wino1d_prepare, "igemm": conv_prepare,
                "rows": lambda w, mt: conv_prepare(w, mt, order="rows")}

    def __init__(self, w):
        self.w, self.packed, self.ran_bf16 = w, {}, None

    def operand(self, key):
        wp = self.packed.get(key)
        if wp is None:
            wp = self.packed[key] = conv_bf16_prepare(self.w) if key == "bf16" else self._PREPARE[key[0]](self.w, key[1])
        return wp


def empty_cl(b, c, h, w, device, zero=False):
    """logical [B, C, H, W] with channels-last strides (one allocation call; the explicit strides keep C innermost also where a
    size-1 dimension would let torch's channels_last format choose others)"""
    if zero:
        return torch.zeros((b, h, w, c), dtype=torch.float32, device=device).permute(0, 3, 1, 2)
    return torch.empty_strided((b, c, h, w), (h * w * c, 1, w * c, c), dtype=torch.float32, device=device)


def _cl(name, t):
    """row pitch of a channels-last [B,C,H,W] view (C innermost, rows back to back over B*H*W)."""
    b, c, h, w = t.shape
    s0, s1, s2, pitch = t.stride()
    if s1 != 1 or s2 != w * pitch or (b > 1 and s0 != h * w * pitch) or pitch < c:
        raise RuntimeError("%s: expected a channels-last [B,C,H,W] view, got shape %s strides %s" % (name, tuple(t.shape), t.stride()))
    return pitch


def bias_act_cl(x, bias, act, out=None, residual=None):
    _require_cuda("bias_act_cl", x, bias, out, residual)
    b, c, h, w = x.shape
    if out is None:
        out = empty_cl(b, c, h, w, x.device)
    with _on(x.device):
        _lib.call("smos_bias_act_cl", x.data_ptr(), _cl("bias_act_cl", x), _ptr(bias), _ptr(residual),
                  _cl("bias_act_cl", residual) if residual is not None else 0, out.data_ptr(), _cl("bias_act_cl", out), b * h * w,
                  c, act, _stream(x))
    return out


def downsample_epilogue_cl(a, p, bias, stride, out=None):
    _require_cuda("downsample_epilogue_cl", a, p, bias, out)
    b, c, h, w = p.shape
    if out is None:
        out = empty_cl(b, c, a.shape[2], a.shape[3], a.device)
    with _on(a.device):
        _lib.call("smos_downsample_epilogue_cl", a.data_ptr(), _cl("downsample_epilogue_cl", a), p.data_ptr(),
                  _cl("downsample_epilogue_cl", p), bias.data_ptr(), out.data_ptr(), _cl("downsample_epilogue_cl", out), b, c, h, w,
                  stride, _stream(a))
    return out


def pool_branch_prepare(w):
    """1x1 pool-branch weights [Cout, Cin(, 1, 1)] (BatchNorm folded) -> the operand block of smos_downsample_pool_branch."""
    w2 = w.reshape(w.shape[0], -1)
    if w2.shape[0] != w2.shape[1] or w2.shape[0] not in (32, 64, 128):
        raise RuntimeError("pool_branch_prepare: Cin == Cout in {32, 64, 128} expected, got %s" % (tuple(w.shape),))
    return _tf_pairs(w2).reshape(-1).contiguous()


def pool_branch_ok(cin, cout, stride):
    """Shapes smos_downsample_pool_branch covers."""
    return cin == cout and cin in (32, 64, 128) and stride in (1, 2) and not (cin == 128 and stride == 1)


def downsample_pool_branch(x, wpairs, a, bias, stride, out=None):
    """relu(a + bias + maxpool3x3(conv1x1(x); stride, pad 1)) on channels-last views in one launch (csrc/downsample.hip): the
    DownSample2D tail with its pool branch computed on the fly; wpairs = pool_branch_prepare(w)."""
    _require_cuda("downsample_pool_branch", x, wpairs, a, bias, out)
    b, c, h, w = x.shape
    ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
    if tuple(a.shape) != (b, c, ho, wo) or wpairs.numel() != c * c or not pool_branch_ok(c, c, stride):
        raise RuntimeError("downsample_pool_branch: unsupported shapes x %s a %s stride %d" % (tuple(x.shape), tuple(a.shape), stride))
    if out is None:
        out = empty_cl(b, c, ho, wo, x.device)
    elif tuple(out.shape) != (b, c, ho, wo):
        raise RuntimeError("downsample_pool_branch: out has shape %s" % (tuple(out.shape),))
    with _on(x.device), profiling.span_f("downsample_pool_branch[%dx%dx%dx%d/s%d]", (b, c, h, w, stride)):
        _lib.call("smos_downsample_pool_branch", x.data_ptr(), _cl("downsample_pool_branch", x), wpairs.data_ptr(), a.data_ptr(),
                  _cl("downsample_pool_branch", a), bias.data_ptr(), out.data_ptr(), _cl("downsample_pool_branch", out), b, h, w, c,
                  c, int(stride), _stream(x))
    return out


def channel_gate_residual_cl(y, bias, w1, b1, w2, b2, xres, ws, out=None):
    _require_cuda("channel_gate_residual_cl", y, bias, w1, b1, w2, b2, xres, ws, out)
    b, c, h, w = y.shape
    if out is None:
        out = empty_cl(b, c, h, w, y.device)
    with _on(y.device):
        _lib.call("smos_channel_gate_residual_cl", y.data_ptr(), _cl("channel_gate_residual_cl", y), bias.data_ptr(), w1.data_ptr(),
                  b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), xres.data_ptr(), _cl("channel_gate_residual_cl", xres),
                  out.data_ptr(), _cl("channel_gate_residual_cl", out), ws.data_ptr(), ws.numel(), b, c, w1.shape[0], h * w,
                  _stream(y))
    return out


def channel_gate_apply_cl(y, bias, w1, b1, w2, b2, xres, chan_sums, gate_ws, out=None):
    """ChannelAtt + residual + ReLU from the channel sums conv_cl left in chan_sums [B, chunks, C]: gate MLP, then
    out = relu((y + bias) * gate + xres).  gate_ws: >= B*C floats of scratch."""
    _require_cuda("channel_gate_apply_cl", y, bias, w1, b1, w2, b2, xres, chan_sums, gate_ws, out)
    b, c, h, w = y.shape
    if chan_sums.dim() != 3 or chan_sums.shape[0] != b or chan_sums.shape[2] != c or not chan_sums.is_contiguous() or gate_ws.numel() < b * c:
        raise RuntimeError("channel_gate_apply_cl: chan_sums must be contiguous [B, chunks, C] and gate_ws hold B*C floats")
    if out is None:
        out = empty_cl(b, c, h, w, y.device)
    with _on(y.device):
        _lib.call("smos_channel_gate_apply_cl", y.data_ptr(), _cl("channel_gate_apply_cl", y), bias.data_ptr(), w1.data_ptr(),
                  b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), xres.data_ptr(), _cl("channel_gate_apply_cl", xres), out.data_ptr(),
                  _cl("channel_gate_apply_cl", out), chan_sums.data_ptr(), chan_sums.shape[1], gate_ws.data_ptr(), b, c,
                  w1.shape[0], h * w, _stream(y))
    return out


def upsample_concat_cl(sources, size):
    import ctypes
    _require_cuda("upsample_concat_cl", *sources)
    b = sources[0].shape[0]
    ctot = sum(s.shape[1] for s in sources)
    out = empty_cl(b, ctot, size[0], size[1], sources[0].device)
    ptrs = (ctypes.c_void_p * len(sources))(*[s.data_ptr() for s in sources])
    with _on(out.device):
        _lib.call("smos_upsample_concat_cl", ptrs, _lib.i64_array([s.shape[1] for s in sources]),
                  _lib.i64_array([s.shape[2] for s in sources]), _lib.i64_array([s.shape[3] for s in sources]),
                  _lib.i64_array([_cl("upsample_concat_cl", s) for s in sources]), len(sources), out.data_ptr(), b, size[0],
                  size[1], _stream(out))
    return out


def zero_views_cl(views):
    """Zero fill of up to four channels-last [B,C,H,W] views (dense maps or channel slices of wider ones) in one launch."""
    if not 1 <= len(views) <= 4:
        raise RuntimeError("zero_views_cl: 1 .. 4 views")
    _require_cuda("zero_views_cl", *views)
    k = len(views)
    ptrs, rows, rf, pit = (ctypes.c_void_p * k)(), (ctypes.c_int64 * k)(), (ctypes.c_int64 * k)(), (ctypes.c_int64 * k)()
    for i, v in enumerate(views):
        b, c, h, w = v.shape
        if v.dtype != torch.float32 or v.device != views[0].device:
            raise RuntimeError("zero_views_cl: float32 views on one device")
        ptrs[i], rows[i], rf[i], pit[i] = v.data_ptr(), b * h * w, c, _cl("zero_views_cl", v)
    with _on(views[0].device):
        _lib.call("smos_zero_views_cl", k, ptrs, rows, rf, pit, _stream(views[0]))


def _coord_view(name, t, b, n):
    """(floats per point, floats per sample) of a coordinate view [B, N, K >= 2] whose last dimension is dense -- contiguous or a
    slice of a wider tensor such as pcds_coord[:, 0, :, :, 0] of the reference's [B, T, N, 3, 1] layout."""
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != b or (n is not None and t.shape[1] != n) or t.shape[2] < 2:
        raise RuntimeError("%s: coordinates must be float32 [B, N, K >= 2], got %s %s" % (name, tuple(t.shape), t.dtype))
    s0, s1, s2 = t.stride()
    if s2 != 1 or s1 < 2 or s0 < 0:
        raise RuntimeError("%s: coordinate view with strides %s (the last dimension must be dense)" % (name, t.stride()))
    return s1, s0


def gather_scatter_cl(grid, gcoord, gscale, scoord=None, sscale=None, out=None, pts_out=None, n_live=None):
    """grid: channels-last [B,C,Hg,Wg] view; out: channels-last [B,C,Ho,Wo] view, zero-filled (or None);
    pts_out: [B,N,C] rows (or None).  gcoord / scoord: [B,N,K>=2] float32 views with a dense last dimension (strided slices of
    the reference's coordinate tensors are taken as they lie).  n_live (device int32 tensor, optional): real points at the front
    of every sample; point rows of the padding tail are not written.  The scatter is max(0, .) into the zero-filled target -- a
    cell whose members are all negative stays 0, where VoxelMaxPool keeps the true maximum -- and is meant for the engine's
    non-negative maps; the point rows carry the signed gathered values."""
    _require_cuda("gather_scatter_cl", grid, gcoord, scoord, out, pts_out, n_live)
    live = _live_ptr("gather_scatter_cl", n_live)
    b, c, hg, wg = grid.shape
    n = gcoord.shape[1]
    kg, gbs = _coord_view("gather_scatter_cl", gcoord, b, None)
    ho = wo = ks = op = sbs = 0
    sc = ss = None                        # the scatter's coordinates and scale: only with a target
    if out is not None:
        ho, wo, op = out.shape[2], out.shape[3], _cl("gather_scatter_cl", out)
        ks, sbs = _coord_view("gather_scatter_cl", scoord, b, n)
        sc, ss = scoord.data_ptr(), _lib.f32_array(sscale)
    po_b = po_n = 0
    if pts_out is not None:
        po_b, po_n = _rows("gather_scatter_cl", pts_out, c)
    label = ("gather_scatter_cl[%dx%dx%dx%d->%d->%dx%d%s]" % (b, c, hg, wg, n, ho, wo,
                                                           "+pts" if pts_out is not None and out is not None else "")
             if profiling.enabled() else None)
    with _on(grid.device), profiling.span(label):
        _lib.call("smos_gather_scatter_cl", grid.data_ptr(), _cl("gather_scatter_cl", grid), gcoord.data_ptr(), kg, gbs,
                  _lib.f32_array(gscale), sc, ks, sbs, ss, _ptr(out), op, _ptr(pts_out), po_b, po_n, b, c, hg, wg, n, ho, wo, live,
                  _stream(grid))

"""Building blocks of the StreamMOS BEV / range-view encoder (mirror of networks/backbone.py).

Only the blocks reachable from the shipped configuration are provided.
Sub-module names and registration order reproduce the reference's ``state_dict`` keys exactly, which
is what makes the 474-tensor checkpoint loadable with ``strict=True``; cited per class.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops


def _bn(c):
    return nn.BatchNorm2d(c)


def conv3x3(in_planes, out_planes, stride=1, dilation=1, bias=False):
    return nn.Conv2d(in_planes, out_planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=bias)


def conv1x1(in_planes, out_planes, bias=False):
    return nn.Conv2d(in_planes, out_planes, 1, bias=bias)


class DownSample2D(nn.Module):
    """relu(bn(conv3x3 stride s) + maxpool3x3 stride s(bn(conv1x1)))  -- networks/backbone.py:14-34."""

    def __init__(self, in_planes, out_planes, stride=1):
        super().__init__()
        self.conv_branch = nn.Sequential(conv3x3(in_planes, out_planes, stride=stride), _bn(out_planes))
        self.pool_branch = nn.Sequential(conv1x1(in_planes, out_planes), _bn(out_planes),
                                         nn.MaxPool2d(3, stride=stride, padding=1))

    def forward(self, x):
        return F.relu(self.conv_branch(x) + self.pool_branch(x))


class ChannelAtt(nn.Module):
    """Squeeze-excite gate -- networks/backbone.py:87-102 (keys cnet.1 / cnet.3)."""

    def __init__(self, channels, reduction=4):
        super().__init__()
        self.cnet = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(channels, channels // reduction, 1), nn.ReLU(),
                                  nn.Conv2d(channels // reduction, channels, 1), nn.Sigmoid())

    def forward(self, x):
        return x * self.cnet(x)


class BasicBlock(nn.Module):
    """Two conv3x3+BN with a residual, optional channel gate -- networks/backbone.py:136-159."""

    def __init__(self, inplanes, reduction=1, dilation=1, use_att=True):
        super().__init__()
        mid = inplanes // reduction
        self.layer = nn.Sequential(conv3x3(inplanes, mid), _bn(mid), nn.ReLU(),
                                   conv3x3(mid, inplanes, dilation=dilation), _bn(inplanes))
        self.use_att = use_att
        if use_att:
            self.channel_att = ChannelAtt(inplanes, reduction=4)

    def forward(self, x):
        y = self.layer(x)
        if self.use_att:
            y = self.channel_att(y)
        return F.relu(y + x)


class PredBranch(nn.Module):
    """Dropout(0.2, train only) + 1x1 classifier with bias -- networks/backbone.py:188-196."""

    def __init__(self, cin, cout):
        super().__init__()
        self.pred_layer = nn.Sequential(nn.Conv2d(cin, cout, 1))

    def forward(self, x):
        return self.pred_layer(F.dropout(x, p=0.2, training=self.training))


class PointNet(nn.Module):
    """[BN] -> 1x1 conv -> BN -> [ReLU] over (B, C, N, 1) -- networks/backbone.py:199-231."""

    def __init__(self, cin, cout, pre_bn=False, post_act=True):
        super().__init__()
        mods = [_bn(cin)] if pre_bn else []
        mods += [conv1x1(cin, cout), _bn(cout)]
        if post_act:
            mods.append(nn.ReLU())
        self.layer = nn.Sequential(*mods)

    def forward(self, x):
        return self.layer(x)


def _is_conv1x1(conv, cin, cout, bias, device):
    """A plain float32 1x1 ``nn.Conv2d`` cin -> cout on ``device``, with a bias or without as ``bias`` says."""
    return (type(conv) is nn.Conv2d and conv.in_channels == cin and conv.out_channels == cout and (conv.bias is not None) == bias
            and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
            and conv.weight.dtype == torch.float32 and conv.weight.device == device)


def _bn_single_process(bn, channels, training, device):
    """A float32 ``nn.BatchNorm2d`` -- or an ``nn.SyncBatchNorm`` whose process group is one process -- over ``channels`` on
    ``device``: affine, with running statistics and a momentum, in the mode ``training``."""
    if type(bn) is nn.SyncBatchNorm:
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(bn.process_group) > 1:
            return False
    elif type(bn) is not nn.BatchNorm2d:
        return False
    return (bn.num_features == channels and bn.affine and bn.track_running_stats and bn.momentum is not None
            and bn.running_mean is not None and bn.training == training
            and bn.weight.dtype == torch.float32 and bn.weight.device == device)


class PointNetStacker(nn.Module):
    """networks/backbone.py:233-250."""

    def __init__(self, cin, cout, pre_bn=False, post_act=True, stack_num=1):
        super().__init__()
        if stack_num == 1:
            mods = [PointNet(cin, cout, pre_bn, post_act)]
        else:
            mods = [PointNet(cin, cout, pre_bn, True)]
            mods += [PointNet(cout, cout, False, True) for _ in range(stack_num - 2)]
            mods.append(PointNet(cout, cout, False, post_act))
        self.layer = nn.Sequential(*mods)

    def _fused_modules(self, x):
        """(bn0, conv1, bn1, conv2, bn2) where ops.point_mlp_train computes this forward, else None: the switch is on
        (ops.point_mlp_fused, SMOS_POINT_MLP, default 0), x is a CUDA float32 [S,7,N,1] that needs no gradient, the stack is
        exactly pre_bn 7 -> 64 -> 64 with ReLU, no autocast, the module is training or gradients are enabled, and the batch
        norms are single-process.  Everything else stays on the module path."""
        if not ops.point_mlp_fused():
            return None
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and x.dim() == 4
                and x.shape[1] == 7 and x.shape[3] == 1 and x.shape[0] * x.shape[2] > 0):
            return None
        if torch.is_autocast_enabled() or not (self.training or torch.is_grad_enabled()):
            return None
        if len(self.layer) != 2:
            return None
        a, b = list(self.layer[0].layer), list(self.layer[1].layer)
        if len(a) != 4 or len(b) != 3:
            return None
        bn0, conv1, bn1, conv2, bn2 = a[0], a[1], a[2], b[0], b[1]
        if not all(type(m) is nn.ReLU for m in (a[3], b[2])):
            return None
        if not all(_is_conv1x1(conv, cin, 64, False, x.device) for conv, cin in ((conv1, 7), (conv2, 64))):
            return None
        if not all(_bn_single_process(bn, c, self.training, x.device) for bn, c in ((bn0, 7), (bn1, 64), (bn2, 64))):
            return None
        return bn0, conv1, bn1, conv2, bn2

    def forward(self, x):
        fused = self._fused_modules(x)
        if fused is not None:
            return ops.point_mlp_train(x, *fused, training=self.training)
        return self.layer(x)


class CatFusion(nn.Module):
    """concat -> dropout(0.2, train only) -> two 1x1 conv+BN+ReLU -- networks/backbone.py:387-413."""

    def __init__(self, in_channel_list, out_channel):
        super().__init__()
        assert len(in_channel_list) >= 2
        self.in_channel_list, self.out_channel = in_channel_list, out_channel
        s = sum(in_channel_list)
        self.merge_layer = nn.Sequential(conv1x1(s, s // 2), _bn(s // 2), nn.ReLU(),
                                         conv1x1(s // 2, out_channel), _bn(out_channel), nn.ReLU())

    def forward(self, *x_list):
        x = F.dropout(torch.cat(x_list, dim=1), p=0.2, training=self.training)
        return self.merge_layer(x)


def _point_head_modules(fusion, pred, xs):
    """(conv1, bn1, conv2, bn2, conv3) where ops.point_head_train computes ``pred(fusion(*xs))``, else None: the switch is on
    (ops.point_head_fused, SMOS_POINT_HEAD_TRAIN, default 0), xs are three CUDA float32 [B,64,N,1] the kernels can read in
    place, no autocast, the modules are exactly 192 -> 96 -> 64 -> 3 with the expected types, the batch norms are
    single-process, fusion and pred are in the same mode, and either they train or gradients are enabled and an input or
    a parameter needs one.  Everything else stays on the modules."""
    if not ops.point_head_fused():
        return None
    if type(fusion) is not CatFusion or type(pred) is not PredBranch or len(xs) != 3 or fusion.training != pred.training:
        return None
    for x in xs:
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape == xs[0].shape
                and x.device == xs[0].device and x.shape[1] == 64 and x.shape[3] == 1 and x.shape[0] * x.shape[2] > 0
                and ops._point_head_pitch(x) is not None):
            return None
    if torch.is_autocast_enabled():
        return None
    merge, head = list(fusion.merge_layer), list(pred.pred_layer)
    if len(merge) != 6 or len(head) != 1 or not all(type(m) is nn.ReLU for m in (merge[2], merge[5])):
        return None
    conv1, bn1, conv2, bn2, conv3 = merge[0], merge[1], merge[3], merge[4], head[0]
    dev = xs[0].device
    if not all(_is_conv1x1(conv, cin, cout, bias, dev)
               for conv, cin, cout, bias in ((conv1, 192, 96, False), (conv2, 96, 64, False), (conv3, 64, 3, True))):
        return None
    if not all(_bn_single_process(bn, c, fusion.training, dev) for bn, c in ((bn1, 96), (bn2, 64))):
        return None
    if not fusion.training:
        params = [conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias, conv3.weight, conv3.bias]
        if not (torch.is_grad_enabled() and any(t.requires_grad for t in list(xs) + params)):
            return None
    return conv1, bn1, conv2, bn2, conv3


def point_head(fusion, pred, *xs):
    """``pred(fusion(*xs))``, the point head of AttNet.stage_forward and of Refine.forward: through ops.point_head_train
    where ``_point_head_modules`` allows it, else through the two modules as they are."""
    fused = _point_head_modules(fusion, pred, xs)
    if fused is not None:
        return ops.point_head_train(*xs, *fused, p=0.2, training=fusion.training)
    return pred(fusion(*xs))


class BilinearSample(nn.Module):
    """Grid -> point bilinear gather, parameter-free -- networks/backbone.py:453-475.

    grid_feat (BS, C, H, W), grid_coord (BS, N, 2, S) -> (BS, C, N, S).  GPU float32 tensors with S = 1 use the HIP
    gather: directly when nothing needs a gradient, and through its autograd node (``ops.bilinear_gather``, backward
    kernel ``smos_bilinear_gather_bwd``) when ``grid_feat`` does.  Anything else -- CPU tensors, other dtypes, a
    ``grid_coord`` that requires a gradient, or ``SMOS_BILINEAR_BWD=0`` for a ``grid_feat`` that does -- goes through
    ``F.grid_sample`` with the reference's exact formulation.
    """

    def __init__(self, in_dim, scale_rate):
        super().__init__()
        self.scale_rate = scale_rate

    def forward(self, grid_feat, grid_coord):
        grad_mode = torch.is_grad_enabled()
        coord_grad = grad_mode and grid_coord.requires_grad
        # ops.bilinear_bwd_own (SMOS_BILINEAR_BWD) is asked only where a backward would run; off = training through F.grid_sample
        own = not coord_grad and (not (grad_mode and grid_feat.requires_grad) or ops.bilinear_bwd_own())
        if grid_feat.is_cuda and own and grid_coord.shape[-1] == 1 and grid_feat.dtype == torch.float32:
            return ops.bilinear_gather(grid_feat, grid_coord.float(), self.scale_rate).unsqueeze(-1)
        h, w = grid_feat.shape[2], grid_feat.shape[3]
        gx = (2 * grid_coord[:, :, 1] * self.scale_rate[1] / (w - 1)) - 1
        gy = (2 * grid_coord[:, :, 0] * self.scale_rate[0] / (h - 1)) - 1
        return F.grid_sample(grid_feat, torch.stack((gx, gy), dim=-1), mode="bilinear", padding_mode="zeros",
                             align_corners=True)


_REGISTRY = {"BilinearSample": BilinearSample, "CatFusion": CatFusion, "BasicBlock": BasicBlock}


def get_module(param_dic, **kwargs):
    """Config dict -> module (networks/backbone.py:37-44; a lookup table instead of ``eval``)."""
    for key, val in param_dic.items():
        if key != "type" and val is not None:
            kwargs[key] = val
    return _REGISTRY[param_dic["type"]](**kwargs)

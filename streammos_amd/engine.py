"""Fused inference engine for ``AttNet`` (eval mode, fp32, one GPU).

``AttNet.infer`` / ``stage_forward`` keep the reference's module graph for training and for CPU
tensors; on a GPU in eval mode they hand over to this engine, which computes the same function
(models/StreamMOS.py:86-113, networks/multi_view_encoder.py:390-458) with far fewer passes over HBM:

* every feature map is channels-last, which is also the layout of the scatters and of the attention tokens: nothing is transposed;
* BatchNorm is folded into the preceding conv's weights once (float64 on the host), and every conv -> BN -> ReLU (-> add -> ReLU)
  chain is one launch of an own convolution kernel with the epilogue fused (csrc/conv_wino.hip, conv_wino1d.hip, conv_igemm.hip,
  conv_rows.hip; opt-in bf16: conv_bf16.hip); MIOpen is only the fallback for shapes those kernels do not cover (``_conv``);
* the first BEV stage runs on the occupied cells only (csrc/stem.hip): the dense input grid is never built;
* concatenations never run: producers write straight into channel slices of the destination buffer
  (conv epilogues, scatters and gathers all take output strides);
* ``conv_1`` takes the two coarser maps as tap GEMMs at source resolution (csrc/upconv.hip) instead of three bilinear
  resizes + ``torch.cat``;
* temporal fusion is the deformable-attention sampler plus one fused kernel per layer (csrc/tfusion.hip);
* ``encode`` holds everything that does not depend on the previous frame, ``decode_memory`` the part that is serial across
  frames and ``decode_heads`` the rest, so the streaming runner can overlap them.

The engine holds *copies* of the folded weights: it is rebuilt whenever the module's parameters may have
changed (``load_state_dict``, ``.to()``, ``.train()``), see ``AttNet._engine_for``.
"""
import itertools
import os

import torch
import torch.nn.functional as F

from . import ops, profiling, scratch

RELU, LEAKY, NONE = ops.ACT_RELU, ops.ACT_LEAKY, ops.ACT_NONE
_gated_tags = itertools.count()         # BasicBlock.tag: a small integer per gated block built


def _fold(conv_w, conv_b, bn, pre=None):
    """(w', b') with BatchNorm `bn` (eval statistics) applied AFTER the conv and, optionally, a BatchNorm
    `pre` applied BEFORE it (PointNet's input BN, networks/backbone.py:205-210).  w' is channels-last, the memory format of
    the maps (for a 1x1 kernel that is the plain contiguous tensor)."""
    w = conv_w.detach().double()
    b = conv_b.detach().double() if conv_b is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    if pre is not None:
        s_in = pre.weight.detach().double() / torch.sqrt(pre.running_var.detach().double() + pre.eps)
        o_in = pre.bias.detach().double() - pre.running_mean.detach().double() * s_in
        b = b + (w.flatten(2).sum(2) * o_in[None, :]).sum(1)
        w = w * s_in[None, :, None, None]
    if bn is not None:
        s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        w = w * s[:, None, None, None]
        b = (b - bn.running_mean.detach().double()) * s + bn.bias.detach().double()
    return w.float().contiguous(memory_format=torch.channels_last), b.float().contiguous()


def _block_call(eng):
    """The switches every block call depends on, read per call: a block's two or three launches behind ONE foreign call
    (csrc/blocks.hip; same launches, same arguments).  Profiled runs go launch by launch so that every launch keeps its label."""
    return eng.block_call and eng.own_conv and eng.wino and not profiling.enabled()


class DownBlock:
    """DownSample2D (networks/backbone.py): conv3x3 (stride) + BN next to conv1x1 + BN + maxpool3x3 (stride), + , ReLU."""
    kind = "down"
    __slots__ = ("wa", "wp", "bias", "stride", "pool_ok", "pool_pack")

    def __init__(self, m):
        self.wa, ba = _fold(m.conv_branch[0].weight, None, m.conv_branch[1])
        self.wp, bp = _fold(m.pool_branch[0].weight, None, m.pool_branch[1])
        # maxpool(y + b) == maxpool(y) + b for a per-channel constant b: both biases move behind the pool
        self.bias = (ba + bp).contiguous()
        self.stride = m.conv_branch[0].stride[0]
        cout, cin = self.wp.shape[0], self.wp.shape[1]
        # the 1x1 pool-branch conv, the 3x3 max pool and the tail in one launch (csrc/downsample.hip): the full-resolution
        # branch map is never written.  Measured (tools/ubench_pool.py): 64 ch @256^2 /2 0.044 vs 0.047 ms for the two
        # launches, 32 ch @32x1024 /1 0.019 vs 0.023, 64 ch @16x512 /1 0.014 vs 0.020 -- and 128 ch @128^2 /2 0.043 vs
        # 0.037: the 1x1 conv is not as HBM-bound as it looks (2.1 GFLOP x 1.29 halo recompute = 19 us at the matrix
        # peak), so the 128-channel block keeps the two launches
        self.pool_ok = cin <= 64 and ops.pool_branch_ok(cin, cout, self.stride)
        self.pool_pack = None           # ops.pool_branch_prepare(wp), made by the first call that takes the fused launch

    def run(self, eng, x, out=None):
        a = eng._conv(x, self.wa, None, NONE, stride=self.stride)
        if (self.pool_ok and eng.pool_fused and eng.own_conv and
                x.shape[0] * x.shape[2] * x.shape[3] * x.stride(3) * 4 < (1 << 31)):
            if self.pool_pack is None:
                self.pool_pack = ops.pool_branch_prepare(self.wp)
            return ops.downsample_pool_branch(x, self.pool_pack, a, self.bias, self.stride, out=out if out is not None else a)
        q = eng._conv(x, self.wp, None, NONE)
        return ops.downsample_epilogue_cl(a, q, self.bias, self.stride, out=out if out is not None else a)


class UnbalanceBlock:
    """Unbalance_BasicBlock (networks/multi_view_encoder.py:478-497): conv k x 3 and conv 3 x k side by side, conv3x3 over
    both, + x, ReLU."""
    kind = "unbalance"
    __slots__ = ("wa", "ba", "pa", "wb", "bb", "pb", "wc", "bc", "plan_ok", "plan")

    def __init__(self, m):
        self.wa, self.ba = _fold(m.layer7x3[0].weight, None, m.layer7x3[1])
        self.wb, self.bb = _fold(m.layer3x7[0].weight, None, m.layer3x7[1])
        self.wc, self.bc = _fold(m.layer3x3[0].weight, None, m.layer3x3[1])
        self.pa, self.pb = m.layer7x3[0].padding, m.layer3x7[0].padding
        c = self.wa.shape[0]
        self.plan_ok = (c % 16 == 0 and tuple(self.wa.shape[:2]) == (c, c) and tuple(self.wb.shape[:2]) == (c, c) and
                        tuple(self.wc.shape) == (c, 2 * c, 3, 3) and ops.conv_wino1d_ok(tuple(self.wa.shape[2:]), 1, c, c) and
                        ops.conv_wino1d_ok(tuple(self.wb.shape[2:]), 1, c, c))
        self.plan = None                # ops.UnbalanceBlockPlan, made by the first block call (a bf16 engine makes none)

    def run(self, eng, x, out=None):
        if self.plan_ok and _block_call(eng) and eng.wino1d and 2 * x.numel() <= (1 << 26):
            if self.plan is None:
                self.plan = ops.UnbalanceBlockPlan(self.wa, self.ba, self.wb, self.bb, self.wc, self.bc)
            return ops.unbalance_block_cl(x, self.plan, out=out)
        b, c, h, w = x.shape
        both = ops.empty_cl(b, 2 * c, h, w, x.device)
        eng._conv(x, self.wa, self.ba, RELU, out=both[:, :c])
        eng._conv(x, self.wb, self.bb, RELU, out=both[:, c:])
        return eng._conv(both, self.wc, self.bc, RELU, residual=x, out=out)


class BasicBlock:
    """BasicBlock (networks/backbone.py:136-159): conv3x3 + BN + ReLU, conv3x3 + BN [, ChannelAtt gate], + x, ReLU."""
    kind = "basic"
    __slots__ = ("w1", "b1", "w2", "b2", "att", "cw1", "cb1", "cw2", "cb2", "plan_ok", "plan", "tag")

    def __init__(self, m):
        self.w1, self.b1 = _fold(m.layer[0].weight, None, m.layer[1])
        self.w2, self.b2 = _fold(m.layer[3].weight, None, m.layer[4])
        self.att = m.use_att
        self.cw1 = self.cb1 = self.cw2 = self.cb2 = None            # the gate MLP of a ChannelAtt block
        if m.use_att:
            c1, c2 = m.channel_att.cnet[1], m.channel_att.cnet[3]
            self.cw1 = c1.weight.detach().reshape(c1.weight.shape[0], -1).contiguous()
            self.cb1 = c1.bias.detach().contiguous()
            self.cw2 = c2.weight.detach().reshape(c2.weight.shape[0], -1).contiguous()
            self.cb2 = c2.bias.detach().contiguous()
        c = self.w1.shape[0]
        self.plan_ok = tuple(self.w1.shape) == (c, c, 3, 3) and tuple(self.w2.shape) == (c, c, 3, 3) and ops.basic_block_ok(c, self.att)
        self.plan = None                # ops.BasicBlockPlan, made by the first block call (a bf16 engine makes none)
        self.tag = next(_gated_tags) if m.use_att else None        # gated blocks: names the plane sums in the engine's scratch table

    def run(self, eng, x, out=None):
        # a gated block call takes its pool sums from the conv epilogue: without fused_gate_sums it goes launch by launch
        if (self.plan_ok and _block_call(eng) and (eng.fused_gate_sums or not self.att) and x.numel() <= (1 << 26)):
            if self.plan is None:
                self.plan = ops.BasicBlockPlan(self.w1, self.b1, self.w2, self.b2,
                                               (self.cw1, self.cb1, self.cw2, self.cb2) if self.att else None)
            ws = None
            if self.att:
                bsz, c, h, w = x.shape
                ws = eng._block_ws(self, bsz * c * (ops.conv_wino_sum_chunks(h, w) + 1))
            return ops.basic_block_cl(x, self.plan, out=out, ws=ws)
        y = eng._conv(x, self.w1, self.b1, RELU)
        if not self.att:
            return eng._conv(y, self.w2, self.b2, RELU, residual=x, out=out)
        bsz, c, h, w = y.shape
        k2 = tuple(self.w2.shape[2:])
        if (eng.own_conv and eng.fused_gate_sums and ops.gate_channels_ok(c) and ops.conv_cl_supported(y, c, k2) and
                (not eng._bf16 or ops.conv_bf16_ok(y, c, k2, chan_sums=True))):
            # the conv's epilogue leaves the per-row-segment channel sums behind: no pass over y2 for the average pool
            # (bf16 mode: the bf16 kernel writes them, in the table layout of conv_cl)
            # the table's layout is the kernel's, so the function that picks the kernel in _conv picks it here
            family = "bf16" if eng._bf16 else ops.conv_route(c, c, k2, 1, bsz * h * w, False, True, eng)[0]
            chunks = ops.conv_wino_sum_chunks(h, w) if family == "wino" else ops.conv_sum_chunks(h, w)
            ws = eng._block_ws(self, bsz * c * (chunks + 1))
            sums = ws[:bsz * chunks * c].view(bsz, chunks, c)
            y2 = eng._conv(y, self.w2, None, NONE, chan_sums=sums)
            return ops.channel_gate_apply_cl(y2, self.b2, self.cw1, self.cb1, self.cw2, self.cb2, x, sums, ws[bsz * chunks * c:],
                                             out=out if out is not None else y2)
        y2 = eng._conv(y, self.w2, None, NONE)
        need = (y2.shape[2] * y2.shape[3] // 512 + 2) * y2.shape[0] * y2.shape[1]
        return ops.channel_gate_residual_cl(y2, self.b2, self.cw1, self.cb1, self.cw2, self.cb2, x, eng._block_ws(self, need),
                                            out=out if out is not None else y2)


class FusionLayer:
    """One DeformAttnLayer of the temporal fusion (multi_view_encoder.py:245-321): its weights as (W, b) pairs, and what the
    own kernels stream (tf, wv_stream, wq_stream: filled in by InferenceEngine.__init__ where csrc/tfusion.hip covers the layer)."""
    __slots__ = ("heads", "points", "value", "qproj", "out", "norm1", "lin1", "lin2", "norm2", "tf", "wv_stream", "wq_stream")

    def __init__(self, lyr):
        ca = lyr.cross_attn
        self.heads, self.points = ca.n_heads, ca.n_points
        self.value = (ca.value_proj.weight.detach(), ca.value_proj.bias.detach())
        # one GEMM for offsets and attention logits
        self.qproj = (torch.cat((ca.sampling_offsets.weight.detach(), ca.attention_weights.weight.detach()), 0).contiguous(),
                      torch.cat((ca.sampling_offsets.bias.detach(), ca.attention_weights.bias.detach()), 0).contiguous())
        self.out = (ca.output_proj.weight.detach(), ca.output_proj.bias.detach())
        self.norm1 = (lyr.norm1.weight.detach(), lyr.norm1.bias.detach(), lyr.norm1.eps)
        self.lin1 = (lyr.linear1.weight.detach(), lyr.linear1.bias.detach())
        self.lin2 = (lyr.linear2.weight.detach(), lyr.linear2.bias.detach())
        self.norm2 = (lyr.norm2.weight.detach(), lyr.norm2.bias.detach(), lyr.norm2.eps)
        self.tf = self.wv_stream = self.wq_stream = None


CONV_PRECISIONS = ("fp32", "bf16")

# The A/B switches: (attribute, environment variable, default, kind); kind "bool" parses by ops.env_on, "int" as int().  Each is a
# plain attribute read on every call, so setting one on a live engine selects the other route from the next call on.
SWITCHES = (
    ("sparse_stem", "SMOS_SPARSE_STEM", True, "bool"),        # first BEV stage on the occupied cells (AttNet.engine_sparse_stem overrides)
    # temporal fusion on the own MFMA kernels (csrc/tfusion.hip): value_proj of every layer + the first layer's offset /
    # logit projection as ONE launch, then per layer the sampler and ONE kernel for output_proj -> +query -> LayerNorm ->
    # FFN -> + -> LayerNorm (-> the next layer's projection).  0: the library-GEMM form
    ("tfusion", "SMOS_TFUSION", True, "bool"),
    # conv_1 without the upsampled concatenation (csrc/upconv.hip): direct conv on the fine map's channels, tap GEMMs
    # at source resolution for the two coarser maps; the aux heads likewise run before the (linear) upsampling
    ("upconv", "SMOS_UPCONV", True, "bool"),
    ("fused_head", "SMOS_FUSED_HEAD", True, "bool"),          # fused point head (csrc/point_head.hip) for the 192 -> 96 -> 64 -> 3 head
    ("head_gather", "SMOS_HEAD_GATHER", True, "bool"),        # the fused head gathers the decoder's BEV rows itself: no gather launch
    # every 2-D convolution runs on the library's own kernels with the epilogue fused.  0: MIOpen convs + separate
    # epilogue passes (kept for A/B runs; tools/ubench_conv.py compares the two per layer)
    ("own_conv", "SMOS_OWN_CONV", True, "bool"),
    ("conv_rows_mt", "SMOS_CONV_ROWS_MT", 1, "int"),          # largest mt the row-staging conv is used for
    ("conv_rows", "SMOS_CONV_ROWS", 3, "int"),                # n > 0: row-staging conv for KW >= n at mt = 1; 0: off
    ("fused_gate_sums", "SMOS_GATE_SUMS", True, "bool"),      # ChannelAtt pool sums from the conv epilogue
    ("wino", "SMOS_WINO", True, "bool"),                      # Winograd F(2x2,3x3) for the stride-1 3x3 layers
    ("wino1d", "SMOS_WINO1D", True, "bool"),                  # 1-D Winograd F(2,3) for the k x 3 / 3 x k layers
    ("pool_fused", "SMOS_POOL_FUSED", True, "bool"),          # DownSample2D pool branch + tail in one launch
    ("block_call", "SMOS_BLOCK_CALL", True, "bool"),          # a residual block = one foreign call (same launches)
)

# Switches of the training step, in the same row format.  The engine above is inference only, so these become attributes
# of the model (AttNet.__init__ -> read_switches) and are read there on every call, like the engine's on the engine.
TRAIN_SWITCHES = (
    # the "ohem" loss of AttNet._seg_loss as ops.seg_loss (csrc/seg_loss.hip): one fused OHEM-CE + Lovasz value with its own
    # backward and no host read of a device value.  0: the torch formulation of refapi/models/losses.py
    ("seg_loss_own", "SMOS_SEG_LOSS", True, "bool"),
)


def read_switches(obj, table):
    """Set every switch of `table` on `obj` from the environment (or its default)."""
    for attr, var, default, kind in table:
        v = os.environ.get(var)
        v = ops.env_on(v) if kind == "bool" else (None if v is None else int(v))
        setattr(obj, attr, default if v is None else v)


class InferenceEngine:
    def __init__(self, net, layout="cl", conv_precision="fp32"):
        """layout: "cl" (every feature map channels-last) is the only layout; the argument and the attribute remain because
        AttNet.engine_layout and bench.py name it.  The first-generation NCHW / MIOpen engine was removed: any other value raises.
        conv_precision "fp32" (default: exact fp32 everywhere) or "bf16" (opt-in): every layer that goes
        through _conv -- the BasicBlock, Unbalance and DownSample2D convs and the decoder's conv_1a / conv_2 -- runs on the
        bf16 matrix-core kernel (csrc/conv_bf16.hip: bf16-rounded weights and activations, fp32 sums and epilogue); a layer
        the kernel does not cover stays on the fp32 path and is counted (conv_precision_stats)."""
        if layout != "cl":        # before anything touches net
            raise ValueError("layout=%r: the NCHW engine was removed, 'cl' (channels-last) is the only layout" % (layout,))
        if conv_precision not in CONV_PRECISIONS:
            raise ValueError("conv_precision must be one of %s, got %r" % (CONV_PRECISIONS, conv_precision))
        self.layout = layout
        self.conv_precision = conv_precision
        self._bf16 = conv_precision == "bf16"
        self._conv_layers = {}          # id(folded weight) -> ops.ConvLayer (which holds the weight): see _conv
        self.scratch = scratch.Table()      # the gated blocks' plane sums: see _block_ws
        self.device = next(net.parameters()).device
        read_switches(self, SWITCHES)
        if self._bf16:
            # the block calls launch fp32 kernels: bf16 mode takes the launch-by-launch path
            self.block_call = False
        self.bev_hw = tuple(net.bev_wl_shape)
        enc = net.bev_net

        l0, l1 = net.point_pre.layer[0].layer, net.point_pre.layer[1].layer
        self.pp1 = _fold(l0[1].weight, None, l0[2], pre=l0[0])
        self.pp2 = _fold(l1[0].weight, None, l1[1])

        self.header_bev = [self._block(m) for m in enc.header_bev]
        # sparse first stage (csrc/stem.hip): per parity class of the input cell, the kernel taps that can reach an
        # output pixel under stride 2, stacked with the 1x1 pool-branch weights, in MFMA operand order
        self.stem_w = None
        p0 = self.header_bev[0]
        if (p0.kind == "down" and p0.stride == 2 and p0.wa.shape[0] == 32 and p0.wa.shape[1] == 192 and
                tuple(p0.wa.shape[2:]) == (3, 3)):
            self.stem_w = ops.stem_prepare_weights(p0.wa, p0.wp)
        self.header_rv = [self._block(m) for m in enc.header_rv]
        self.res1_bev = [self._block(m) for m in enc.res1_bev]
        self.res1_rv = [self._block(m) for m in enc.res1_rv]
        self.res2 = [self._block(m) for m in enc.res2]

        self.query_embed = enc.query_embed.weight.detach()
        self.layers = [FusionLayer(lyr) for lyr in enc.deformattn_module.deformattn_layers]

        # what the own temporal-fusion kernels stream (the tfusion switch)
        self._tf_ok = False
        try:
            for i, L in enumerate(self.layers):
                nxt = self.layers[i + 1].qproj if i + 1 < len(self.layers) else None
                L.tf = ops.TfusionLayer(L.out, L.norm1, L.lin1, L.lin2, L.norm2, next_qproj=nxt)
                L.wv_stream = ops.tfusion_pack_linear(L.value[0])
                L.wq_stream = ops.tfusion_pack_linear(L.qproj[0]) if i == 0 else None
            self._tf_ok = all(L.value[0].shape[0] // L.heads == 32 and L.points <= 8 and L.qproj[0].shape[0] % 4 == 0 for L in self.layers)
        except RuntimeError:
            self._tf_ok = False

        self.conv_1 = _fold(enc.conv_1.conv.weight, None, enc.conv_1.bn)
        self.conv_2 = _fold(enc.conv_2.conv.weight, None, enc.conv_2.bn)
        # the three 1x1 aux heads as ONE block-diagonal 1x1 conv over the 320-channel decoder input
        heads = (enc.aux_head1, enc.aux_head2, enc.aux_head3)
        ncls = heads[0].weight.shape[0]
        cin = [h.weight.shape[1] for h in heads]
        w = torch.zeros((3 * ncls, sum(cin), 1, 1), device=self.device)
        off = 0
        for i, h in enumerate(heads):
            w[i * ncls:(i + 1) * ncls, off:off + cin[i]] = h.weight.detach()
            off += cin[i]
        self.aux = (w.contiguous(), torch.cat([h.bias.detach() for h in heads]).contiguous(), ncls)
        self.grid2point_scale = tuple(net.bev_grid2point.scale_rate)
        # the operands of the upconv switch: conv_1 cut into the fine map's channels and the two coarser maps' tap matrices
        w1 = self.conv_1[0]
        self.conv_1a = w1[:, :cin[0]].contiguous(memory_format=torch.channels_last)
        self.conv_1z = (ops.upconv_tap_weights(w1, cin[0], cin[0] + cin[1]), ops.upconv_tap_weights(w1, cin[0] + cin[1], sum(cin)))
        self.aux_split = [(h.weight.detach().contiguous(), h.bias.detach().contiguous()) for h in heads]

        m = net.point_post.merge_layer
        self.post1 = _fold(m[0].weight, None, m[1])
        self.post2 = _fold(m[3].weight, None, m[4])
        p = net.pred_layer.pred_layer[0]
        self.pred = (p.weight.detach().contiguous(), p.bias.detach().contiguous())
        self.refine = None                  # stage-2 model (models/StreamMOS_seg.py:21-30): a second point head
        if hasattr(net, "refine"):
            rm = net.refine.bf_point_post.merge_layer
            rp = net.refine.bf_pred_layer.pred_layer[0]
            self.refine = (_fold(rm[0].weight, None, rm[1]), _fold(rm[3].weight, None, rm[4]),
                           (rp.weight.detach().contiguous(), rp.bias.detach().contiguous()))
        # the fused point head's operands, where the head has the reference's 192 -> 96 -> 64 -> 3 shape
        self.head_w = self.refine_w = None
        try:
            self.head_w = ops.point_head_prepare(self.post1, self.post2, self.pred)
            if self.refine is not None:
                self.refine_w = ops.point_head_prepare(*self.refine)
        except RuntimeError:
            self.head_w = self.refine_w = None
        self._shapes = None
        self._lsi = None
        self._hw = None
        self.miopen_search = True

    # ---- parameter extraction -----------------------------------------------------------
    def _block(self, m):
        from .refapi.networks import backbone as bb
        from .refapi.networks import multi_view_encoder as mve
        for cls, module in ((DownBlock, bb.DownSample2D), (UnbalanceBlock, mve.Unbalance_BasicBlock), (BasicBlock, bb.BasicBlock)):
            if isinstance(m, module):
                return cls(m)
        raise RuntimeError("InferenceEngine: unexpected module %s" % type(m).__name__)

    # ---- blocks ---------------------------------------------------------------------------
    @staticmethod
    def _linear_relu(x, wb):
        """relu(x @ W^T + b) for a folded 1x1 conv (W [Cout, Cin, 1, 1]) on point rows; the bias + ReLU epilogue
        is fused into the hipBLASLt GEMM where the runtime offers it."""
        w = wb[0].view(wb[0].shape[0], -1)
        try:
            return torch._addmm_activation(wb[1], x, w.t(), use_gelu=False)
        except (RuntimeError, AttributeError):
            return torch.relu_(torch.addmm(wb[1], x, w.t()))

    def _head_gathers(self, fuse, bev_feat, o1, o2):
        """True where the fused head may gather the BEV third of the point rows itself: it is the only reader of that third
        (stage-1 model: no refine head; the aux heads read maps, not rows) and the kernel's layout holds."""
        return (self.head_gather and self.fused_head and self.head_w is not None and self.refine is None
                and (o1, o2) == (64, 128) and fuse.shape[2] == 192 and fuse.stride(1) % 4 == 0
                and bev_feat.data_ptr() % 16 == 0 and bev_feat.stride(3) % 4 == 0)

    def _point_heads(self, fuse, aux, k, x2, n_live=None, gather=None):
        """CatFusion + PredBranch as point-major GEMMs: [B*N, 192] -> 96 -> 64 -> 3 (and the stage-2 refine head).
        n_live (device int32, runner only): real points at the front of every sample; the padding tail's logits are zeros.
        gather (see ops.point_head; only where _head_gathers() holds): the BEV third of `fuse` has not been written."""
        bs, n = fuse.shape[0], fuse.shape[1]
        rows = fuse.view(bs * n, -1)
        a3 = tuple(aux) if isinstance(aux, (tuple, list)) else (aux[:, :k], aux[:, k:2 * k], aux[:, 2 * k:])

        def head(l1, l2, pr, fused):
            if self.fused_head and fused is not None and fuse.stride(1) % 4 == 0:
                return ops.point_head(fuse, fused[0], fused[1], n_live=n_live, gather=gather).unsqueeze(-1)
            if gather is not None:
                raise RuntimeError("InferenceEngine: the BEV rows were left to the fused point head, which does not run")
            z = self._linear_relu(self._linear_relu(rows, l1), l2)
            out = torch.addmm(pr[1], z, pr[0].view(pr[0].shape[0], -1).t())
            return out.view(bs, n, -1).permute(0, 2, 1).contiguous().unsqueeze(-1)

        pred = head(self.post1, self.post2, self.pred, self.head_w)
        if self.refine is not None:
            return (pred, head(*self.refine, self.refine_w)) + a3 + (x2,)
        return (pred,) + a3 + (x2,)

    def _block_ws(self, p, n_floats):
        """Scratch of one channel-attention block (plane sums written by one kernel, read by the next), from this engine's
        table (scratch.py): blocks of different pipeline stages run concurrently on different streams, the same block may
        run on two streams at once (encode(t) on the main stream next to encode(t+1) on the side stream), and hipGraphs
        captured from one engine for several TTA groups replay concurrently with the addresses baked in (a namespace per
        group, StreamRunner._capture_groups) -- a shared scratch would be a data race in each case."""
        return self.scratch.get(p.tag, (n_floats,), torch.float32, self.device, zero=True)

    @staticmethod
    def _add_norm(a, b, norm, c):
        """LayerNorm(a + b) in one pass (csrc/epilogue.hip) for the token widths that kernel is built for."""
        if c in (64, 128, 256, 512):
            return ops.add_layer_norm(a.contiguous(), b.contiguous(), norm[0], norm[1], norm[2] if len(norm) > 2 else 1e-5)
        return F.layer_norm(a + b, (c,), norm[0], norm[1], norm[2] if len(norm) > 2 else 1e-5)

    def _temporal_fusion(self, x2, memory):
        """DeformAttnModule (multi_view_encoder.py:426-439, 245-321): the memory stream queries the current map."""
        b, c, hh, ww = x2.shape
        dev = x2.device
        if self._shapes is None or self._hw != (hh, ww):
            self._hw = (hh, ww)
            self._shapes = torch.tensor([[hh, ww]], dtype=torch.long, device=dev)
            self._lsi = torch.zeros((1,), dtype=torch.long, device=dev)
            ys = (torch.arange(hh, dtype=torch.float32, device=dev) + 0.5) / hh
            xs = (torch.arange(ww, dtype=torch.float32, device=dev) + 0.5) / ww
            self._ref = torch.stack((xs[None, :].expand(hh, ww), ys[:, None].expand(hh, ww)), -1).reshape(1, hh * ww, 1, 1, 1, 2)
            self._norm = torch.tensor([ww, hh], dtype=torch.float32, device=dev)
        # a channels-last [B,C,H,W] map is already the [B, H*W, C] token matrix: the permute + reshape below is a view
        src = x2.permute(0, 2, 3, 1).reshape(b, hh * ww, c)
        if memory is None:
            query = self.query_embed.unsqueeze(0).expand(b, -1, -1)
        else:
            query = memory.permute(0, 2, 3, 1).reshape(b, hh * ww, c)
        lq = hh * ww
        if self.tfusion and self._tf_ok and c == 128:
            # five launches: projections | (sampler, layer) x 2
            query = query if query.is_contiguous() else query.contiguous()
            jobs = [(src, L.wv_stream, L.value[1]) for L in self.layers] + [(query, self.layers[0].wq_stream, self.layers[0].qproj[1])]
            outs = []
            for k in range(0, len(jobs), 8):
                outs += ops.tfusion_project(jobs[k:k + 8])
            qp = outs[-1]
            for i, L in enumerate(self.layers):
                sampled = ops.msda_fwd_qp(outs[i].view(b, lq, L.heads, 32), qp.view(b, lq, -1), hh, ww, L.points)
                query, qp = ops.tfusion_layer(sampled, query, L.tf)
            return query.view(b, hh, ww, c).permute(0, 3, 1, 2)
        for L in self.layers:
            h, p = L.heads, L.points
            value = F.linear(src, *L.value).view(b, lq, h, c // h)
            qp = F.linear(query, *L.qproj)
            if c // h == 32 and p <= 8:
                # softmax over the points, offset normalisation and reference points folded into the sampler
                sampled = ops.msda_fwd_qp(value.contiguous(), qp.contiguous(), hh, ww, p)
            else:
                off = qp[..., :h * p * 2].reshape(b, lq, h, 1, p, 2)
                attn = F.softmax(qp[..., h * p * 2:].reshape(b, lq, h, p), -1).view(b, lq, h, 1, p)
                loc = (self._ref + off / self._norm).contiguous()
                sampled = ops.msda_fwd(value.contiguous(), self._shapes, self._lsi, loc, attn.contiguous())
            query = self._add_norm(query, F.linear(sampled, *L.out), L.norm1, c)
            ffn = F.linear(self._linear_relu(query.view(b * lq, c), L.lin1).view(b, lq, -1), *L.lin2)
            query = self._add_norm(query, ffn, L.norm2, c)
        return query.contiguous().view(b, hh, ww, c).permute(0, 3, 1, 2)

    # ---- the network ------------------------------------------------------------------------
    @torch.no_grad()
    def stage_forward(self, point_feat, pcds_coord, pcds_sphere_coord, memory=None):
        return self.decode(self.encode(point_feat, pcds_coord, pcds_sphere_coord), memory)

    def _conv_flags(self):
        """MIOpen solver search (measure every applicable solver once per conv shape, then reuse the fastest) --
        what the reference's own test scripts switch on (test_StreamMOS.py:20-23).  +7 % scans/s at the val shape;
        scoped to the engine's calls instead of flipping the process-wide flag."""
        if self.own_conv:
            return ops._NO_GUARD          # every convolution of this engine is an own kernel: nothing for MIOpen to search
        return torch.backends.cudnn.flags(enabled=True, benchmark=self.miopen_search)

    def encode(self, point_feat, pcds_coord, pcds_sphere_coord, n_live=None):
        """n_live (device int32 tensor, runner only): see decode(); the point rows of the padding tail are not produced."""
        with torch.no_grad(), self._conv_flags():
            return self._encode_cl(point_feat, pcds_coord, pcds_sphere_coord, n_live)

    def decode(self, enc, memory=None, want_aux=True, n_live=None):
        """want_aux=False: the three BEV aux maps (training-time supervision heads, models/StreamMOS.py:106-111) are not
        computed and come back as None -- the streaming runner throws them away (val_StreamMOS.py:97 uses pred_cls only);
        AttNet.infer always returns them.  n_live (device int32 tensor, runner only): the number of real points at the front
        of every sample of the current scan; the point head leaves the padding tail's logits at zero (val_StreamMOS.py:113
        cuts that tail off; datasets/data_StreamMOS.py:568-571 creates it).  AttNet.infer computes all N."""
        return self.decode_heads(enc, self.decode_memory(enc, memory), want_aux, n_live)

    def decode_memory(self, enc, memory=None):
        """The only part that is serial across frames: third BEV stage + deformable-attention fusion with the previous
        frame's memory.  Returns the new memory (= the fused 1/8-resolution map)."""
        with torch.no_grad(), self._conv_flags():
            return self._temporal_fusion(self._stage_cl(enc["x1cat"], self.res2), memory)

    def decode_heads(self, enc, x2, want_aux=True, n_live=None):
        """Decoder convs, aux heads, bev->point gather and the point heads; nothing here feeds the next frame."""
        with torch.no_grad(), self._conv_flags():
            return self._decode_cl(enc, x2, want_aux, n_live)

    # ---- convolutions and blocks ------------------------------------------------------------------
    def conv_precision_stats(self):
        """bf16 mode: {"bf16": layers whose last launch ran on the bf16 kernel, "fallback": layers that stayed on the fp32
        path (shapes the bf16 kernel does not cover)}; one entry per layer, so after a step these are that step's counts.
        fp32 mode: both 0."""
        ran = [layer.ran_bf16 for layer in self._conv_layers.values() if layer.ran_bf16 is not None]
        return {"bf16": sum(ran), "fallback": len(ran) - sum(ran)}

    def _conv_layer(self, w):
        """The ops.ConvLayer of a folded weight, made on first use.  Keyed by id(w): the layer holds w, so the id stays w's."""
        layer = self._conv_layers.get(id(w))
        if layer is None:
            layer = self._conv_layers[id(w)] = ops.ConvLayer(w)
        return layer

    def _conv(self, x, w, bias, act, stride=1, residual=None, out=None, chan_sums=None):
        """act(conv(x, w) + bias [+ residual]) for a folded weight w [Cout, Cin, KH, KW] ("same" padding for odd kernels)
        on channels-last maps: one launch of the kernel ops.conv_route names; the operand-ordered copies of w are made once,
        in the weight's ops.ConvLayer.  With SMOS_OWN_CONV=0: MIOpen conv + the separate bias / activation / residual pass.
        conv_precision "bf16": csrc/conv_bf16.hip where it covers the shape, else the fp32 path below (counted in
        conv_precision_stats)."""
        cout, cin, kh, kw = w.shape
        layer = self._conv_layer(w)
        if self._bf16:
            layer.ran_bf16 = self.own_conv and ops.conv_bf16_ok(x, cout, (kh, kw), stride, residual, out, chan_sums)
            if layer.ran_bf16:
                return ops.conv_bf16_cl(x, layer.operand("bf16"), bias, act, cout, (kh, kw), stride=stride, residual=residual,
                                        out=out, chan_sums=chan_sums)
        # fast accept (no per-launch predicate walk): channel counts the MFMA tiling covers and operands far below the 2 GiB of the
        # 32-bit buffer offsets (<= 2^26 input floats; a slice's pitch is at most twice its channels, Cout at most four times Cin)
        easy = (cin % 32 == 0 and cout % 32 == 0 and cout <= 4 * cin and kh <= 7 and kw <= 7 and (stride == 1 or stride == 2) and
                x.numel() <= (1 << 26))
        if not self.own_conv or not (easy or ops.conv_cl_supported(x, cout, (kh, kw), stride, residual, out)):
            # MIOpen + the separate epilogue pass: channel counts the MFMA tiling does not cover, operands of 2 GiB and more
            if chan_sums is not None:
                raise RuntimeError("InferenceEngine._conv: channel sums need the own conv kernel")
            y = F.conv2d(x, w, None, stride, (kh // 2, kw // 2))
            if bias is None and act == NONE and residual is None and out is None:
                return y
            return ops.bias_act_cl(y, bias, act, out=out if out is not None else y, residual=residual)
        b, _, h, wd = x.shape
        ho, wo = (h + 2 * (kh // 2) - kh) // stride + 1, (wd + 2 * (kw // 2) - kw) // stride + 1
        route = ops.conv_route(cin, cout, (kh, kw), stride, b * ho * wo, residual is not None, chan_sums is not None, self)
        family, tile = route
        wp = layer.operand(route)
        if family == "wino":
            # stride-1 3x3: Winograd F(2x2, 3x3) on the matrix cores (csrc/conv_wino.hip): 4 instead of 9 multiply-adds per
            # output and channel pair, fp32 throughout (weights transformed in float64 on the host); 1.35-1.7x the direct
            # kernels per layer (tools/ubench_wino.py), logits within 2e-6 of the reference's (tests/test_gpu_e2e.py)
            return ops.conv_wino_cl(x, wp, bias, act, cout, mb=tile, residual=residual, out=out, chan_sums=chan_sums)
        if family == "wino1d":
            # the k x 3 / 3 x k branches of the Unbalance blocks: 1-D Winograd F(2, 3) along the 3-tap axis (csrc/conv_wino1d.hip)
            return ops.conv_wino1d_cl(x, wp, bias, act, cout, (kh, kw), mb=tile, out=out)
        if family == "rows":
            # the row-staging variant (csrc/conv_rows.hip): per layer within 0 .. -5 % of conv_igemm alone on the GPU, +1 % in the
            # two-stream step (241.9 vs 239.1 scans/s: a fifth of the L1 requests leaves more of the memory path to the other stream)
            return ops.conv_rows_cl(x, wp, bias, act, cout, (kh, kw), mt=tile, residual=residual, out=out, chan_sums=chan_sums)
        return ops.conv_cl(x, wp, bias, act, cout, (kh, kw), stride=stride, mt=tile, residual=residual, out=out, chan_sums=chan_sums)

    def _block_cl(self, x, p, out=None):
        return p.run(self, x, out)

    def _stage_cl(self, x, blocks, out=None):
        for i, p in enumerate(blocks):
            x = p.run(self, x, out if i == len(blocks) - 1 else None)
        return x

    def _cross_view_cl(self, cat_buf, c, bev_xy, sphere, rv_blocks, rv_hw, scale, point_rows=None, n_live=None, rv=None):
        """B2P gather + P2R scatter, range-view convs, R2P gather + P2B scatter straight into cat_buf[:, c:]
        (multi_view_encoder.py:395-405 / :410-420); everything channels-last, nothing transposed."""
        b = cat_buf.shape[0]
        back = cat_buf[:, c:]
        if rv is None:
            rv = ops.empty_cl(b, c, rv_hw[0], rv_hw[1], cat_buf.device)
            ops.zero_views_cl([rv, back])                 # the two scatter-max targets
        ops.gather_scatter_cl(cat_buf[:, :c], bev_xy, scale, sphere, scale, out=rv)
        rv = self._stage_cl(rv, rv_blocks)
        ops.gather_scatter_cl(rv, sphere, scale, bev_xy, scale, out=back, pts_out=point_rows, n_live=n_live)

    def _stem_sparse_cl(self, bev_cl, pcds_coord):
        """header_bev[0] on the occupied cells of a DENSE channels-last grid (csrc/stem.hip); the engine itself scatters
        into compact rows and never builds the dense grid (_encode_cl), this entry serves tests and A/B runs."""
        plan = ops.stem_plan(pcds_coord, bev_cl.shape[1], bev_cl.shape[2])
        return ops.sparse_downsample(bev_cl, plan, self.stem_w, self.header_bev[0].bias, compact=False)

    def _encode_cl(self, point_feat, pcds_coord, pcds_sphere_coord, n_live=None):
        bs, t, cin, n, _ = point_feat.shape
        dev = point_feat.device
        # views, not copies: the cross-view kernels take the strided slices as they lie (smos_gather_scatter_cl)
        bev_xy = pcds_coord[:, 0, :, :2, 0]
        sphere = pcds_sphere_coord[:, 0, :, :, 0]
        cpt = self.pp2[0].shape[0]
        hb, wb = self.bev_hw
        c_dec, c1 = self.conv_2[0].shape[0], self.res1_bev[-1].w2.shape[0]
        o1, o2 = cpt, cpt + c_dec
        fuse = torch.empty((bs, n, cpt + c_dec + c1), dtype=torch.float32, device=dev)
        c0 = self.header_bev[-1].w2.shape[0]
        x0cat = ops.empty_cl(bs, 2 * c0, hb // 2, wb // 2, dev)
        x1cat = ops.empty_cl(bs, 2 * c1, hb // 4, wb // 4, dev)
        # the four zero-initialised scatter-max targets of the frame's two cross-view transfers (two range-view maps, the upper
        # channel halves of the two concatenation buffers) in one launch instead of four torch fills
        hw0, hw1 = (32, 1024), (16, 512)               # range-view maps of the two cross-view transfers
        rv0, rv1 = ops.empty_cl(bs, c0, hw0[0], hw0[1], dev), ops.empty_cl(bs, c1, hw1[0], hw1[1], dev)
        ops.zero_views_cl([rv0, x0cat[:, c0:], rv1, x1cat[:, c1:]])
        if self.sparse_stem and self.stem_w is not None:
            # sparse first stage: the occupancy of the grid follows from the coordinates alone, so the point MLP scatters
            # into a compact row table (one row per occupied cell) and the 805 MB dense grid is never built
            plan = ops.stem_plan(pcds_coord, hb, wb, row_floats=t * cpt)
            rows = ops.pointnet_scatter_rows(point_feat.float(), pcds_coord, self.pp1[0], self.pp1[1], self.pp2[0], self.pp2[1],
                                             plan, pts_out=fuse[:, :, :o1], n_live=n_live)
            x = ops.sparse_downsample(rows, plan, self.stem_w, self.header_bev[0].bias, compact=True)
            self._stage_cl(x, self.header_bev[1:], out=x0cat[:, :c0])
        else:
            bev_cl = torch.empty((bs, hb, wb, t * cpt), dtype=torch.float32, device=dev)
            ops.pointnet_scatter(point_feat.float(), pcds_coord, self.pp1[0], self.pp1[1], self.pp2[0], self.pp2[1], bev_cl,
                                 pts_out=fuse[:, :, :o1], zero_fill=True)
            self._stage_cl(bev_cl.permute(0, 3, 1, 2), self.header_bev, out=x0cat[:, :c0])
        self._cross_view_cl(x0cat, c0, bev_xy, sphere, self.header_rv, hw0, (0.5, 0.5), rv=rv0)
        self._stage_cl(x0cat, self.res1_bev, out=x1cat[:, :c1])
        self._cross_view_cl(x1cat, c1, bev_xy, sphere, self.res1_rv, hw1, (0.25, 0.25), point_rows=fuse[:, :, o2:], n_live=n_live,
                            rv=rv1)
        # res2 (the third BEV stage) is independent of the past too, but it runs in decode(): that keeps the two pipeline
        # stages balanced so both HIP streams stay busy (re-measured after the sparse first stage shortened the encoder:
        # res2 on the encode side 158.6 vs 167.5 scans/s)
        return {"x0cat": x0cat, "x1cat": x1cat, "fuse": fuse, "bev_xy": bev_xy, "o1": o1, "o2": o2}

    def _decode_cl(self, enc, x2, want_aux=True, n_live=None):
        x0cat, x1cat, fuse, bev_xy, o1, o2 = enc["x0cat"], enc["x1cat"], enc["fuse"], enc["bev_xy"], enc["o1"], enc["o2"]
        k = self.aux[2]
        if self.upconv:
            y = ops.upconv3x3(self._conv(x0cat, self.conv_1a, None, NONE), self.conv_1[1],
                              [(x1cat, self.conv_1z[0]), (x2, self.conv_1z[1])], LEAKY)
            size = tuple(x0cat.shape[2:])

            def head1x1(src, wb):
                # 3 output channels: as a conv MIOpen falls back to its naive kernel; on channels-last rows it is a GEMM
                bb, cc, hh, ww = src.shape
                rows = src.permute(0, 2, 3, 1).reshape(bb * hh * ww, cc)
                return torch.addmm(wb[1], rows, wb[0].reshape(wb[0].shape[0], -1).t()).view(bb, hh, ww, -1).permute(0, 3, 1, 2)

            aux = (None, None, None)
            if want_aux:
                aux = [head1x1(x0cat, self.aux_split[0])]
                for src, wb in ((x1cat, self.aux_split[1]), (x2, self.aux_split[2])):
                    # a 1x1 convolution commutes with the (linear, weights summing to 1) bilinear resize
                    aux.append(F.interpolate(head1x1(src, wb), size=size, mode="bilinear", align_corners=True))
        else:
            dec_in = ops.upsample_concat_cl([x0cat, x1cat, x2], tuple(x0cat.shape[2:]))
            y = self._conv(dec_in, self.conv_1[0], self.conv_1[1], LEAKY)
            aux = F.conv2d(dec_in, self.aux[0], self.aux[1]) if want_aux else (None, None, None)
        bev_feat = self._conv(y, self.conv_2[0], self.conv_2[1], LEAKY)
        if self._head_gathers(fuse, bev_feat, o1, o2):
            return self._point_heads(fuse, aux, k, x2, n_live, gather=(bev_feat, bev_xy, self.grid2point_scale))
        ops.gather_scatter_cl(bev_feat, bev_xy, self.grid2point_scale, pts_out=fuse[:, :, o1:o2], n_live=n_live)
        return self._point_heads(fuse, aux, k, x2, n_live)

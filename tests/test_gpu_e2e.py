"""End-to-end parity of AttNet.infer on the GPU (HIP kernels + PyTorch-ROCm convs) against the golden
vectors of the real reference and against the CPU oracle, plus the streaming runner with voting."""
import contextlib
from unittest import mock

import numpy as np
import pytest
import torch

from oracle import net_torch, ops_np
from streammos_amd import preprocess, scratch, streaming, synth
from streammos_amd.refapi.config import StreamMOS as cfg
from streammos_amd.refapi.models import StreamMOS
from tests import cases
from tests.util import check_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    m = StreamMOS.AttNet(cfg.get_config()[2])
    m.load_state_dict(synth.seeded_state_dict(m.state_dict()), strict=True)
    return m.to(DEV).eval()


def test_infer_matches_reference_golden(golden, model):
    g = golden("e2e")
    memory = None
    with torch.no_grad():
        for i, batch in enumerate(cases.e2e_frames()):
            check_inputs(g, "e2e_f%d_in_sha" % i, batch["pcds_xyzi"], batch["pcds_coord"], batch["pcds_sphere_coord"])
            tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
            pred, a0, a1, a2, memory = model.infer(tb, i, memory)
            ref = g["e2e_f%d_pred" % i]
            got = pred.cpu().numpy()
            # fp32 on both sides; what differs is the summation order of ~40 conv layers (own MFMA convs / MIOpen vs
            # MKL-DNN) and the float64 BatchNorm folding.  Observed on MI355X: ~1.5e-6 of the logit range, all labels
            # equal; the bars are ~10x that, so a wrong tap or channel in any fused kernel fails.
            err = np.abs(got - ref).max() / np.abs(ref).max()
            agree = (got.argmax(1) == ref.argmax(1)).mean()
            mem_ref = g["e2e_f%d_mem_sub" % i]
            mem_err = np.abs(memory[:, ::8, ::4, ::4].cpu().numpy() - mem_ref).max() / np.abs(mem_ref).max()
            aux = torch.stack((a0, a1, a2))[:, :, :, ::8, ::8].cpu().numpy()
            ref_aux = g["e2e_f%d_aux_sub" % i]
            aux_err = np.abs(aux - ref_aux).max() / np.abs(ref_aux).max()
            print("golden frame %d: logits %.2e of range, labels %.6f, memory %.2e, aux %.2e" % (i, err, agree, mem_err, aux_err))
            assert err <= 2e-5 and agree >= 0.9999, (i, err, agree)
            assert mem_err <= 5e-5 and aux_err <= 2e-5, (i, mem_err, aux_err)
            stats = g["e2e_f%d_mem_stats" % i]
            assert abs(memory.double().abs().sum().item() - stats[1]) <= 1e-5 * stats[1]


def test_stream_runner_with_voting_matches_oracle(model):
    """6 frames of a small synthetic sequence through StreamRunner (window shortened to 4 so that both the
    look-ahead start-up phase and the steady state run), predictions and voted labels vs the CPU oracle."""
    spec = preprocess.VoxelSpec()
    n_frames = 6
    scans = [synth.synthetic_scan(k, 16, 120) for k in range(n_frames + 2)]
    poses = [synth.synthetic_pose(k) for k in range(n_frames + 2)]
    runner = streaming.StreamRunner(model, DEV, vote=True)
    runner.voter.window = 4
    oracle = net_torch.OracleNet({k: v.cpu() for k, v in model.state_dict().items()})
    memory = None
    raw_preds, voted = [], {}
    for i in range(n_frames):
        idx = preprocess.window_indices(i, n_frames + 2, 3)
        sample = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True)
        out = runner.step(runner.upload(sample, scans[i]), poses[i])
        want, _, _, _, memory = oracle.stage_forward(*(torch.from_numpy(sample[k]) for k in
                                                       ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord")), memory)
        want_lab, _ = net_torch.tta_labels(want)
        # the runner leaves the scan's padding tail to the point head as zeros (StreamRunner(skip_padding=True): the reference
        # cuts that tail off, val_StreamMOS.py:113); everything in front of it is compared
        nv = int(sample["valid_mask"].sum())
        assert nv < 2048 and float(out["pred_cls"][:, :, nv:].abs().max()) == 0.0
        agree = (out["labels"].cpu().long()[:nv] == want_lab[:nv]).float().mean().item()
        err = (out["pred_cls"].cpu()[:, :, :nv] - want[:, :, :nv]).abs().max().item() / want.abs().max().item()
        print("runner frame %d vs oracle: logits %.2e of range, TTA labels %.6f" % (i, err, agree))
        # ~10x the observed error (fp32 on both sides, summation order only); 2048 points: one flipped label = 4.9e-4
        assert err <= 2e-5 and agree >= 0.9995, (i, err, agree)
        raw_preds.append(out["raw_labels"].cpu().numpy())
        for fid, lab in out["voted"]:
            voted[fid] = lab.cpu().numpy()
    assert sorted(voted) == list(range(n_frames))
    # voting is integer work: given the SAME per-point predictions it must be bit-exact with the oracle
    lut = np.zeros(256, dtype=np.int32)
    lut[1], lut[2] = 9, 251
    for fid in range(n_frames):
        hist_ids = streaming.vote_history_ids(fid, 4)
        inv_cur = np.linalg.inv(poses[fid])
        hp = np.concatenate([preprocess.pose_align(scans[h], inv_cur.dot(poses[h])) for h in hist_ids], 0)
        hl = np.concatenate([raw_preds[h] for h in hist_ids], 0)
        want = ops_np.vote_frame(scans[fid], raw_preds[fid], hp, hl)
        assert np.array_equal(voted[fid], lut[want]), fid


def test_model_survives_reference_val_wrapping(model):
    """val_StreamMOS.py:188-195: SyncBatchNorm conversion + optimizer construction around the net."""
    import copy
    m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(model)).to(DEV).eval()
    torch.optim.SGD(m.parameters(), lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-3)
    assert list(m.state_dict().keys()) == list(model.state_dict().keys())
    batch = next(iter(cases.e2e_frames(1)))
    tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
    with torch.no_grad():
        a = m.infer(tb, 0)[0]
        b = model.infer(tb, 0)[0]
    assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item()


def test_fused_engine_equals_module_graph(model):
    """The fused engine (folded BN, fused epilogues, no concatenations) against the plain module graph with the
    same weights on the same GPU: identical function, differences only from BN folding / summation order."""
    frames = list(cases.e2e_frames(2))
    outs = {}
    for fast in (False, True):
        model.fast_inference = fast
        memory = None
        res = []
        with torch.no_grad():
            for i, batch in enumerate(frames):
                tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
                pred, a0, a1, a2, memory = model.infer(tb, i, memory)
                res.append((pred, a0, a1, a2, memory))
        outs[fast] = res
    assert model._engine is not None and model._engine.layout == "cl"
    for slow, fast in zip(outs[False], outs[True]):
        for a, b in zip(slow, fast):
            assert a.shape == b.shape
            assert (a - b).abs().max().item() <= 2e-4 * a.abs().max().item()


def test_engine_variants_agree(model):
    """The engine's A/B switches select other kernels for the same function: row-staging convolution on / off / also at 64
    outputs per block, ChannelAtt pool sums from the conv epilogue or from their own pass, the temporal fusion on the own
    MFMA kernels (csrc/tfusion.hip) or as library GEMMs + add_layer_norm, the DownSample2D pool branch fused (csrc/downsample.hip)
    or as 1x1 conv + epilogue pass.  Same fp32 products, other
    summation orders: 1e-5 of the range; every variant leaves the default flags behind."""
    frames = list(cases.e2e_frames(2))
    model.fast_inference, model.engine_layout = True, "cl"
    with torch.no_grad():
        eng = model._engine_for(torch.zeros(1, device=DEV))
    assert eng is not None and eng.layout == "cl"
    assert eng.pool_fused
    default = (eng.conv_rows, eng.conv_rows_mt, eng.fused_gate_sums, eng.tfusion, eng.pool_fused)
    assert eng.tfusion and eng._tf_ok                     # the fused temporal-fusion kernels are what runs by default
    outs = []
    try:
        for variant in (default, (0, 1, True, True, True), (3, 2, True, True, True), (3, 1, False, True, True),
                        default[:3] + (False, True), default[:4] + (False,)):
            eng.conv_rows, eng.conv_rows_mt, eng.fused_gate_sums, eng.tfusion, eng.pool_fused = variant
            memory, res = None, []
            with torch.no_grad():
                for i, batch in enumerate(frames):
                    tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
                    pred, a0, a1, a2, memory = model.infer(tb, i, memory)
                    res.append((pred.clone(), memory.clone()))
            outs.append(res)
    finally:
        eng.conv_rows, eng.conv_rows_mt, eng.fused_gate_sums, eng.tfusion, eng.pool_fused = default
    for other in outs[1:]:
        for (p0, m0), (p1, m1) in zip(outs[0], other):
            assert (p0 - p1).abs().max().item() <= 1e-5 * p0.abs().max().item()
            assert (m0 - m1).abs().max().item() <= 5e-5 * m0.abs().max().item()      # observed 1.5e-5 (behind two LayerNorms)


def test_block_call_is_bit_identical(model):
    """BasicBlocks enqueued by one foreign call each (smos_basic_block_cl, csrc/blocks.hip) against the launch-by-launch path:
    the same launches with the same arguments -- logits and recurrent memory equal bit for bit over two streamed frames."""
    frames = list(cases.e2e_frames(2))
    model.fast_inference, model.engine_layout = True, "cl"
    with torch.no_grad():
        eng = model._engine_for(torch.zeros(1, device=DEV))
    assert eng.block_call                                   # the default
    outs = []
    try:
        for on in (True, False):
            eng.block_call = on
            memory, res = None, []
            with torch.no_grad():
                for i, batch in enumerate(frames):
                    tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
                    pred, a0, a1, a2, memory = model.infer(tb, i, memory)
                    res.append((pred.clone(), memory.clone()))
            outs.append(res)
    finally:
        eng.block_call = True
    plans = [p.plan for p in eng.res2 if p.kind == "basic"]
    assert plans and all(plans) and any(pl.gated for pl in plans)        # the third stage did go through the block call
    unb = [p.plan for stage in (eng.header_bev, eng.header_rv, eng.res1_bev, eng.res1_rv, eng.res2)
           for p in stage if p.kind == "unbalance"]
    assert unb and all(unb)                                              # and so did the Unbalance blocks
    for (p0, m0), (p1, m1) in zip(*outs):
        assert torch.equal(p0, p1) and torch.equal(m0, m1)


@contextlib.contextmanager
def _block_launches():
    """Counts the calls of the three wrappers a residual block's routes differ in."""
    from streammos_amd import ops
    seen = {}

    def counted(name):
        fn = getattr(ops, name)
        seen[name] = 0

        def call(*args, **kw):
            seen[name] += 1
            return fn(*args, **kw)
        return mock.patch.object(ops, name, call)

    with counted("basic_block_cl"), counted("unbalance_block_cl"), counted("channel_gate_residual_cl"):
        yield seen


def _run_block(eng, p, x):
    with _block_launches() as seen, torch.no_grad(), eng._conv_flags():
        y = eng._block_cl(x, p).clone()
    return y, (seen["basic_block_cl"], seen["unbalance_block_cl"], seen["channel_gate_residual_cl"])


def _block_input(seed):
    """[2, 32, 9, 33] channels-last: two samples, one row and one column past the 8 x 32 chunk of the Winograd sum table."""
    x = torch.randn((2, 32, 9, 33), generator=torch.Generator().manual_seed(seed))
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def test_gated_block_follows_the_switches_per_call(model):
    """One gated BasicBlock (C = 32, the smallest width the gate kernels take) on a live engine: the switches are read on
    every call, so after a block call with the default switches, fused_gate_sums = False takes the same block through
    channel_gate_residual_cl (1e-5 of the range, the bar of test_engine_variants_agree for this pair of paths), and
    block_call = False through the separate launches of the block call (bit-identical, as test_block_call_is_bit_identical)."""
    with torch.no_grad():
        eng = model._engine_for(torch.zeros(1, device=DEV))
    p = next(b for b in eng.header_bev if b.kind == "basic" and b.att)
    assert p.w1.shape[0] == 32 and eng.block_call and eng.fused_gate_sums
    x = _block_input(5)
    try:
        a, calls = _run_block(eng, p, x)
        assert calls == (1, 0, 0) and p.plan is not None and p.plan.gated
        eng.fused_gate_sums = False
        b, calls = _run_block(eng, p, x)
        assert calls == (0, 0, 1), calls
        err = (a - b).abs().max().item() / a.abs().max().item()
        print("gated block, pool sums from their own pass: %.2e of range" % err)
        assert err <= 1e-5
        eng.fused_gate_sums, eng.block_call = True, False
        c, calls = _run_block(eng, p, x)
        assert calls == (0, 0, 0) and torch.equal(a, c)
    finally:
        eng.fused_gate_sums, eng.block_call = True, True


def test_unbalance_block_follows_the_switches_per_call(model):
    """The same for one Unbalance block (C = 32, 7 x 3 / 3 x 7) and wino1d: off, the branches run on the direct kernels, within
    the bar tests/test_gpu_ops.py::test_conv_wino_cl_against_float64 holds a Winograd and a direct kernel to against each other
    (4e-6 of the range)."""
    with torch.no_grad():
        eng = model._engine_for(torch.zeros(1, device=DEV))
    p = next(b for b in eng.header_bev if b.kind == "unbalance")
    assert p.wa.shape[0] == 32 and eng.block_call and eng.wino1d
    x = _block_input(6)
    try:
        a, calls = _run_block(eng, p, x)
        assert calls == (0, 1, 0) and p.plan is not None
        eng.wino1d = False
        b, calls = _run_block(eng, p, x)
        assert calls == (0, 0, 0), calls
        err = (a - b).abs().max().item() / a.abs().max().item()
        print("unbalance block, branches on the direct kernels: %.2e of range" % err)
        assert err <= 4e-6
        eng.wino1d, eng.block_call = True, False
        c, calls = _run_block(eng, p, x)
        assert calls == (0, 0, 0) and torch.equal(a, c)
    finally:
        eng.wino1d, eng.block_call = True, True


@pytest.mark.parametrize("fill", ["lidar", "empty_sample", "dense_corner"])
def test_sparse_stem_equals_dense_downsample(model, fill):
    """header_bev[0] computed on the occupied cells only (stem_mark + per-parity-class GEMMs + stem_epilogue) against
    the dense conv3x3 s2 / conv1x1 + maxpool formulation on the same grid.  fp32 both ways, different summation order:
    1e-5 of the output range.  Covers image borders, all four parity classes, a sample without points and a fully
    occupied region."""
    from streammos_amd import ops
    gen = torch.Generator(device="cpu").manual_seed(31)
    b, t, n, h, w = 2, 3, 6000, 512, 512
    eng = model._engine_for(torch.zeros(1, device=DEV)) if False else None
    with torch.no_grad():
        eng = model._engine_for(torch.zeros(1, device=DEV))
    assert eng is not None and eng.stem_w is not None
    coord = torch.rand((b, t, n, 3, 1), generator=gen) * 540.0 - 14.0          # some points outside the grid
    coord[0, :, :200, 0] = torch.rand((t, 200, 1), generator=gen) * 1.9 - 0.95   # rows -1 < y < 1 (top border, cell 0)
    coord[0, :, 200:400, 1] = 511.0 + torch.rand((t, 200, 1), generator=gen) * 0.99
    if fill == "empty_sample":
        coord[1] = -100.0
    if fill == "dense_corner":
        yy, xx = torch.meshgrid(torch.arange(40.0), torch.arange(50.0), indexing="ij")
        blockc = torch.stack((yy.reshape(-1) + 0.5, xx.reshape(-1) + 0.5, torch.zeros(2000)), 1)
        coord[1, 0, :2000, :, 0] = blockc
    coord = coord.to(DEV)
    xyzi = torch.randn((b, t, 7, n, 1), generator=gen).to(DEV)
    bev_cl = torch.zeros((b, h, w, t * 64), device=DEV)
    ops.pointnet_scatter(xyzi, coord, eng.pp1[0], eng.pp1[1], eng.pp2[0], eng.pp2[1], bev_cl)
    with torch.no_grad(), eng._conv_flags():
        want = eng._block_cl(bev_cl.permute(0, 3, 1, 2), eng.header_bev[0])
        got = eng._stem_sparse_cl(bev_cl, coord)
    assert got.shape == want.shape
    scale = want.abs().max().item()
    assert scale > 0
    assert (got - want).abs().max().item() <= 1e-5 * scale
    assert ((got > 0) == (want > 0)).float().mean().item() > 0.9999
    # the engine's own route: the point MLP scatters into compact rows, the dense grid is never built
    plan = ops.stem_plan(coord, h, w, row_floats=t * 64)
    assert not bool(scratch.shared.get("stem_flags", (b * h * w,), torch.int32, coord.device).any())    # scan cleared the flags
    rows = ops.pointnet_scatter_rows(xyzi, coord, eng.pp1[0], eng.pp1[1], eng.pp2[0], eng.pp2[1], plan)
    n_rows = int(plan.meta[11])
    row_of = plan.row_of.long()
    occupied = row_of >= 0
    assert int(occupied.sum()) == n_rows == int(plan.class_rows().sum()) and int(plan.meta[4]) == 0
    # rows are numbered in parity-class-major order, each exactly once
    assert torch.equal(torch.sort(row_of[occupied])[0], torch.arange(n_rows, device=DEV))
    cells = plan.row_cell[:n_rows].long()
    assert torch.equal(row_of[cells], torch.arange(n_rows, device=DEV))
    cy, cx = (cells // w) % h, cells % w
    cls = ((cy & 1) * 2 + (cx & 1))
    assert bool((cls[1:] >= cls[:-1]).all())
    dense_rows = bev_cl.view(b * h * w, -1)
    assert torch.equal(rows[row_of[occupied]], dense_rows[occupied])          # same maxima, bit for bit
    assert not bool(dense_rows[~occupied].any())                              # and nothing outside the marked cells
    with torch.no_grad():
        got2 = ops.sparse_downsample(rows, plan, eng.stem_w, eng.header_bev[0].bias, compact=True)
    assert torch.equal(got2, got)


def test_engine_is_dropped_when_weights_change(model):
    import copy
    m = copy.deepcopy(model)
    batch = next(iter(cases.e2e_frames(1)))
    tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
    with torch.no_grad():
        a = m.infer(tb, 0)[0]
        assert m._engine is not None
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        sd["pred_layer.pred_layer.0.bias"] += 1.0
        m.load_state_dict(sd)
        assert m._engine is None
        b = m.infer(tb, 0)[0]
    assert abs((b - a).mean().item() - 1.0) < 1e-3


def test_full_size_scan_against_cpu_oracle(model):
    """BASELINE.json configs[1] shape (B=4 TTA, T=3, N=160000, 120k-point synthetic scans): two chained frames on
    the GPU engine vs the CPU oracle.  fp32 both sides, different summation order (MFMA implicit GEMM vs MKL-DNN direct)
    and BN folding: 2e-5 of the logit range, >= 99.99 % identical labels."""
    import bench
    frames = bench.make_frames(2, seq_seed=7)
    oracle = net_torch.OracleNet({k: v.cpu() for k, v in model.state_dict().items()})
    torch.set_num_threads(bench.host_cores())
    mem_gpu = mem_cpu = None
    with torch.no_grad():
        for i, (sample, raw, pose) in enumerate(frames):
            tb = {k: torch.from_numpy(sample[k]).unsqueeze(0).to(DEV) for k in ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord")}
            pred, a0, a1, a2, mem_gpu = model.infer(tb, i, mem_gpu)
            want, w0, w1, w2, mem_cpu = oracle.stage_forward(*(torch.from_numpy(sample[k]) for k in
                                                              ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord")), mem_cpu)
            got = pred.cpu()
            err = (got - want).abs().max().item() / want.abs().max().item()
            n_valid = int(sample["valid_mask"].sum())
            agree = (got.argmax(1)[:, :n_valid] == want.argmax(1)[:, :n_valid]).float().mean().item()
            tta_g = (torch.softmax(got, 1).mean(0).argmax(0)[:n_valid, 0])
            tta_c = net_torch.tta_labels(want)[0][:n_valid]
            tta_agree = (tta_g == tta_c).float().mean().item()
            mem_err = (mem_gpu.cpu() - mem_cpu).abs().max().item() / mem_cpu.abs().max().item()
            aux_err = max((g_.cpu() - c_).abs().max().item() / c_.abs().max().item() for g_, c_ in ((a0, w0), (a1, w1), (a2, w2)))
            print("full-size frame %d: logits %.2e of range, labels %.6f, TTA labels %.6f, memory %.2e, aux %.2e"
                  % (i, err, agree, tta_agree, mem_err, aux_err))
            # ~10x the error observed on MI355X (summation order only: fp32 on both sides)
            assert err <= 2e-5 and agree >= 0.9999 and tta_agree >= 0.9999, (i, err, agree, tta_agree)
            assert mem_err <= 1e-4 and aux_err <= 5e-5, (i, mem_err, aux_err)     # observed 1.6e-5 / 8.6e-6 on frame 1


def test_run_sequence_writes_reference_file_formats(tmp_path):
    """A 10-scan synthetic sequence in SemanticKITTI layout through streammos_amd.run_sequence: prediction and
    refined files exist for every scan, have one 32-bit LUT word per raw point, and the IoU report is filled."""
    from streammos_amd import kitti, run_sequence
    seq = tmp_path / "sequences" / "08"
    (seq / "velodyne").mkdir(parents=True)
    (seq / "labels").mkdir()
    n = 10
    for k in range(n):
        scan, lab = synth.synthetic_scan(k, 16, 120, with_labels=True)
        scan.tofile(seq / "velodyne" / ("%06d.bin" % k))
        np.where(lab == 2, 252, 40).astype(np.uint32).tofile(seq / "labels" / ("%06d.label" % k))
    kitti.write_poses(seq / "poses.txt", [synth.synthetic_pose(k) for k in range(n)])
    kitti.write_calibration(seq / "calib.txt")
    model = run_sequence.load_model(None, DEV)
    out = tmp_path / "out"
    res = run_sequence.run_sequence(model, str(seq), str(out), DEV, vote=True, frame_point_num=2048)
    assert res["scans"] == n and set(res["network"]) == {"static_iou", "moving_iou", "mean_iou"} and "voted" in res
    for k in range(n):
        npts = kitti.read_scan(seq / "velodyne" / ("%06d.bin" % k)).shape[0]
        for sub in ("predictions", "refined"):
            words = np.fromfile(out / sub / ("%06d.label" % k), dtype=np.uint32)
            assert words.shape[0] == npts and set(np.unique(words)) <= {0, 9, 251}


def test_graph_replay_equals_eager(model):
    """StreamRunner(graph=True) replays captured hipGraphs; labels and logits must equal the eager engine's."""
    spec = preprocess.VoxelSpec()
    scans = [synth.synthetic_scan(k, 16, 120) for k in range(6)]
    poses = [synth.synthetic_pose(k) for k in range(6)]
    res = {}
    import copy
    for graph in (False, True, 2):
        # graph capture reconfigures the engine of the model it is given: use a private copy
        # (skip_padding=False: the graphs capture AttNet.infer, which computes the padding tail's logits too)
        runner = streaming.StreamRunner(copy.deepcopy(model), DEV, vote=False, graph=bool(graph), split=2 if graph == 2 else 1,
                                        skip_padding=False)
        outs = []
        for i in range(4):
            idx = preprocess.window_indices(i, 6, 3)
            sample = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True)
            o = runner.step(runner.upload(sample, scans[i]), poses[i])
            outs.append((o["pred_cls"].clone(), o["labels"].clone(), o["raw_labels"].clone()))
        res[graph] = outs
    for other in (True, 2):
        for (p0, l0, r0), (p1, l1, r1) in zip(res[False], res[other]):
            # the same channels-last engine, replayed instead of launched: own convs are deterministic and batch-independent,
            # only the library GEMMs of the attention block may choose another kernel for the half batch of split=2
            assert (p0 - p1).abs().max().item() <= 1e-5 * p0.abs().max().item()
            assert torch.equal(l0, l1) and torch.equal(r0, r1)


def test_graph_scratch_is_per_group_and_released_by_owner(model):
    """StreamRunner(graph=True, split=2): the two groups' graphs replay concurrently, so no scratch buffer of one group may
    overlap the same tag's buffer of the other -- in the wrappers' shared table and in the engine's own.  close() drops exactly
    that runner's graph scratch: an eager runner on another stream keeps its entries and computes what a fresh one computes."""
    import copy
    spec = preprocess.VoxelSpec()
    scans = [synth.synthetic_scan(k, 16, 120) for k in range(6)]
    poses = [synth.synthetic_pose(k) for k in range(6)]

    def step(runner, i):
        idx = preprocess.window_indices(i, 6, 3)
        sample = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True)
        o = runner.step(runner.upload(sample, scans[i]), poses[i])
        return o["pred_cls"].clone(), o["labels"].clone()

    def graph_entries(table, owner):
        return [(key, buf) for key, buf in table.entries()
                if isinstance(key.namespace, scratch.GraphNamespace) and key.namespace.owner == owner]
    runner = streaming.StreamRunner(copy.deepcopy(model), DEV, vote=False, graph=True, split=2, skip_padding=False)
    for i in range(2):
        step(runner, i)
    owner, eng = runner._ws_owner, runner._g_engine
    for table in (scratch.shared, eng.scratch):
        mine = graph_entries(table, owner)
        assert mine and {key.namespace.group for key, _ in mine} == {0, 1}
        spans = {}
        for key, buf in mine:
            span = (buf.data_ptr(), buf.data_ptr() + buf.numel() * buf.element_size())
            spans.setdefault(key.tag, {0: [], 1: []})[key.namespace.group].append(span)
        both = [tag for tag, groups in spans.items() if groups[0] and groups[1]]
        assert both
        for tag in both:
            for lo0, hi0 in spans[tag][0]:
                for lo1, hi1 in spans[tag][1]:
                    assert hi0 <= lo1 or hi1 <= lo0, (tag, lo0, hi0, lo1, hi1)

    main, side = torch.cuda.current_stream(DEV), torch.cuda.Stream(DEV)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        eager = streaming.StreamRunner(model, DEV, vote=False, skip_padding=False)
        step(eager, 0)
        kept = {key for key, _ in scratch.entries() if key.stream == side.cuda_stream and key.namespace == 0}
        assert kept and any(type(key.tag) is int for key in kept) and any(type(key.tag) is str for key in kept)
    runner.close()
    left = {key for key, _ in scratch.entries()}
    assert not any(isinstance(key.namespace, scratch.GraphNamespace) and key.namespace.owner == owner for key in left)
    assert kept <= left
    with torch.cuda.stream(side):
        got = step(eager, 1)
    main.wait_stream(side)
    fresh = streaming.StreamRunner(model, DEV, vote=False, skip_padding=False)
    step(fresh, 0)
    want = step(fresh, 1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_concurrent_streams_equal_separate_streams(model):
    """configs[2] in small: two sequences batched through MultiStreamRunner give each stream the labels it gets
    when streamed alone.  The network is batch-independent and the own kernels are deterministic; only the library GEMMs
    of the attention block (hipBLASLt) may pick another kernel for the doubled token count, hence a (tight) tolerance on the
    logits; the labels must be identical."""
    spec = preprocess.VoxelSpec()
    seqs = []
    for q in range(2):
        scans = [synth.synthetic_scan(50 * q + k, 16, 120) for k in range(6)]
        poses = [synth.synthetic_pose(k) for k in range(6)]
        seqs.append((scans, poses))
    solo = []
    for scans, poses in seqs:
        r = streaming.StreamRunner(model, DEV, vote=False, skip_padding=False)     # MultiStreamRunner computes every logit
        outs = []
        for i in range(3):
            idx = preprocess.window_indices(i, 6, 3)
            sample = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True)
            o = r.step(r.upload(sample, scans[i]), poses[i])
            outs.append((o["pred_cls"].clone(), o["raw_labels"].clone()))
        solo.append(outs)
    ms = streaming.MultiStreamRunner(model, DEV, n_streams=2, vote=False)
    msp = streaming.MultiStreamRunner(model, DEV, n_streams=2, vote=False, pipeline=True)      # two HIP streams, one batch of look-ahead
    declared = set(vars(msp))
    up = streaming.StreamRunner(model, DEV, vote=False)
    uploads, batches, kept = [], [], []
    for i in range(3):
        devs = []
        for scans, poses in seqs:
            idx = preprocess.window_indices(i, 6, 3)
            sample = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True)
            devs.append(up.upload(sample, scans[i]))
        uploads.append(devs)
        batches.append(ms.batch_inputs(devs))
    for i in range(3):
        pred, outs = ms.step(batches[i], [seqs[q][1][i] for q in range(2)])
        pred_p, outs_p = msp.step(batches[i], [seqs[q][1][i] for q in range(2)], next_batched=batches[i + 1] if i + 1 < 3 else None)
        assert torch.equal(pred_p, pred) and all(torch.equal(a["raw_labels"], b["raw_labels"]) for a, b in zip(outs_p, outs))
        kept.append((pred.clone(), [o["raw_labels"].clone() for o in outs]))
        for q in range(2):
            want_pred, want_raw = solo[q][i]
            err = (pred[4 * q:4 * q + 4] - want_pred).abs().max().item() / want_pred.abs().max().item()
            flips = int((outs[q]["raw_labels"] != want_raw).sum().item())
            print("2 streams, frame %d, stream %d: batched vs solo %.2e of range, %d labels differ" % (i, q, err, flips))
            assert err <= 1e-5 and flips == 0, (i, q, err, flips)
    # the same sequences once more after reset(); batch 1 arrives re-made (another object than the one announced), so its
    # encoder issued ahead is dropped and it is encoded again on the main stream
    assert msp.frame == 3 and set(vars(msp)) == declared
    msp.reset()
    assert msp.frame == 0 and msp.memory is None and set(vars(msp)) == declared
    for i in range(3):
        cur = ms.batch_inputs(uploads[i]) if i == 1 else batches[i]
        pred_p, outs_p = msp.step(cur, [seqs[q][1][i] for q in range(2)], next_batched=batches[i + 1] if i + 1 < 3 else None)
        pred, raws = kept[i]
        assert torch.equal(pred_p, pred) and all(torch.equal(a["raw_labels"], b) for a, b in zip(outs_p, raws))


def test_pipelined_runner_equals_plain_runner(model):
    """pipeline=True overlaps the encoder of frame t+1 with the decoder of frame t on a second HIP stream; results
    must equal the serial runner's (same kernels, same inputs), frame after frame, including the voting output.
    Second pass ("miss"): frame 2 arrives as a fresh upload of the sample that was announced, another dict object -- the
    encoder issued ahead is dropped and the frame is encoded again on the main stream; same results.  Every pass is given
    the next frame's inputs: the serial runner must not look ahead."""
    spec = preprocess.VoxelSpec()
    n_frames = 6
    scans = [synth.synthetic_scan(k, 16, 120) for k in range(n_frames + 2)]
    poses = [synth.synthetic_pose(k) for k in range(n_frames + 2)]
    samples = []
    for i in range(n_frames):
        idx = preprocess.window_indices(i, n_frames + 2, 3)
        samples.append(preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True))
    res = {}
    # which encodes run on the main stream: all of the serial runner's; frame 0 of the pipelined one; frame 2 again on a miss
    on_main = {"plain": [True] * 6, "ahead": [True] + [False] * 5, "miss": [True, False, False, True, False, False, False]}
    for mode in ("plain", "ahead", "miss"):
        runner = streaming.StreamRunner(model, DEV, vote=True, pipeline=mode != "plain")
        runner.voter.window = 3
        devs = [runner.upload(samples[i], scans[i]) for i in range(n_frames)]
        with torch.no_grad():
            eng = model._engine_for(devs[0]["pcds_xyzi"])
        encode, streams = eng.encode, []

        def spy(*args, **kwargs):
            streams.append(torch.cuda.current_stream().cuda_stream)
            return encode(*args, **kwargs)
        main = torch.cuda.current_stream().cuda_stream
        outs = []
        with mock.patch.object(eng, "encode", spy):
            for i in range(n_frames):
                cur = runner.upload(samples[i], scans[i]) if (mode, i) == ("miss", 2) else devs[i]
                o = runner.step(cur, poses[i], next_dev=devs[i + 1] if i + 1 < n_frames else None)
                outs.append((o["pred_cls"].clone(), o["raw_labels"].clone(), [(f, l.clone()) for f, l in o["voted"]]))
        torch.cuda.synchronize()
        assert [s == main for s in streams] == on_main[mode], (mode, streams, main)
        res[mode] = outs
    for mode in ("ahead", "miss"):
        for (p0, r0, v0), (p1, r1, v1) in zip(res["plain"], res[mode]):
            assert torch.equal(p0, p1) or (p0 - p1).abs().max().item() <= 1e-6 * p0.abs().max().item()
            assert torch.equal(r0, r1)
            assert [f for f, _ in v0] == [f for f, _ in v1] and all(torch.equal(a[1], b[1]) for a, b in zip(v0, v1))


def test_reset_with_a_look_ahead_pending_starts_a_clean_sequence(model):
    """Three frames of sequence A through a pipelined runner, the last of which wrongly announces a successor, so an
    encoder is pending on the side stream; reset(); three frames of sequence B.  B's logits, raw labels and votes equal a
    fresh pipelined runner's bit for bit, the runner restarts at frame 0 without memory, and it holds the same attributes
    after construction, after the steps and after reset()."""
    spec = preprocess.VoxelSpec()
    seqs = []
    for q in range(2):
        scans = [synth.synthetic_scan(70 * q + k, 16, 120) for k in range(4)]
        poses = [synth.synthetic_pose(k) for k in range(4)]
        samples = []
        for i in range(4):
            idx = preprocess.window_indices(i, 4, 3)
            samples.append(preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True))
        seqs.append((scans, poses, samples))

    def run(runner, seq, announce_past_the_end):
        scans, poses, samples = seq
        devs = [runner.upload(samples[i], scans[i]) for i in range(4)]
        outs = []
        for i in range(3):
            o = runner.step(devs[i], poses[i], next_dev=devs[i + 1] if i < 2 or announce_past_the_end else None)
            outs.append((o["pred_cls"].clone(), o["raw_labels"].clone(), [(f, l.clone()) for f, l in o["voted"]]))
        return outs

    runner = streaming.StreamRunner(model, DEV, vote=True, pipeline=True)
    runner.voter.window = 3
    declared = set(vars(runner))
    run(runner, seqs[0], True)
    assert runner.frame == 3 and runner.memory is not None and set(vars(runner)) == declared
    runner.reset()
    assert runner.frame == 0 and runner.memory is None and set(vars(runner)) == declared
    got = run(runner, seqs[1], False)
    fresh = streaming.StreamRunner(model, DEV, vote=True, pipeline=True)
    fresh.voter.window = 3
    want = run(fresh, seqs[1], False)
    torch.cuda.synchronize()
    for (p0, r0, v0), (p1, r1, v1) in zip(want, got):
        assert torch.equal(p0, p1) and torch.equal(r0, r1)
        assert [f for f, _ in v0] == [f for f, _ in v1] and all(torch.equal(a[1], b[1]) for a, b in zip(v0, v1))
    assert len(got[2][2]) == 3                # the window of 3 voted: B's votes saw none of A's frames


def test_seg_variant_engine_matches_reference_golden(golden):
    """Stage-2 model (refine head) on the GPU engine: both point heads against the reference's outputs, two chained frames,
    and through StreamRunner (which also emits the `_bf` labels of val_StreamMOS_seg.py)."""
    from streammos_amd.refapi.config import StreamMOS_seg as seg_cfg
    from streammos_amd.refapi.models import StreamMOS_seg
    g = golden("seg")
    m = StreamMOS_seg.AttNet(seg_cfg.get_config()[2])
    m.load_state_dict(synth.seeded_state_dict(m.state_dict()), strict=True)
    m = m.to(DEV).eval()
    memory = None
    with torch.no_grad():
        for i, batch in enumerate(cases.e2e_frames(2)):
            check_inputs(g, "seg_f%d_in_sha" % i, batch["pcds_xyzi"], batch["pcds_coord"], batch["pcds_sphere_coord"])
            tb = {k: torch.from_numpy(v).unsqueeze(0).to(DEV) for k, v in batch.items()}
            pred, bf, a0, a1, a2, memory = m.infer(tb, i, memory)
            for got, key in ((pred, "seg_f%d_pred" % i), (bf, "seg_f%d_bf_pred" % i)):
                ref = g[key]
                err = np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max()
                agree = (got.cpu().numpy().argmax(1) == ref.argmax(1)).mean()
                print("seg golden frame %d %s: %.2e of range, labels %.6f" % (i, key, err, agree))
                # the stage-1 bar (test_infer_matches_reference_golden): ~10x the error observed on MI355X
                assert err <= 2e-5 and agree >= 0.9999, (i, key, err, agree)
    spec = preprocess.VoxelSpec()
    scans = [synth.synthetic_scan(k, 16, 120) for k in range(4)]
    poses = [synth.synthetic_pose(k) for k in range(4)]
    runner = streaming.StreamRunner(m, DEV, vote=False, pipeline=True)
    idx = preprocess.window_indices(0, 4, 3)
    sample = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True)
    out = runner.step(runner.upload(sample, scans[0]), poses[0])
    assert out["bf_raw_labels"].shape == out["raw_labels"].shape and int(out["bf_raw_labels"].max()) <= 2


def test_eight_concurrent_streams_full_size(model):
    """BASELINE.json configs[2]: 8 sequences advanced in lock step as ONE batch of 32 samples at the validation shape
    (N = 160 000), every stream's memory and voting window resident.  Stream 0 is checked against the CPU oracle, every
    stream against its own solo run (logits, raw labels, voted labels), two chained frames."""
    import bench
    S, n_frames = 8, 2
    per_stream = [bench.make_frames(n_frames, seq_seed=200 + q) for q in range(S)]
    up = streaming.StreamRunner(model, DEV, vote=False)
    solo = []
    for q in range(S):
        r = streaming.StreamRunner(model, DEV, vote=True, skip_padding=False)      # MultiStreamRunner computes every logit
        r.voter.window = n_frames
        outs = []
        for f in range(n_frames):
            sample, raw, pose = per_stream[q][f]
            o = r.step(r.upload(sample, raw), pose)
            outs.append((o["pred_cls"].clone(), o["raw_labels"].clone(), [(k, l.clone()) for k, l in o["voted"]]))
        solo.append(outs)
        del r
    ms = streaming.MultiStreamRunner(model, DEV, n_streams=S, vote=True)
    for v in ms.voters:
        v.window = n_frames
    oracle = net_torch.OracleNet({k: v.cpu() for k, v in model.state_dict().items()})
    torch.set_num_threads(bench.host_cores())
    mem_cpu = None
    worst = [0.0, 1.0]
    total_raw_flips = [0] * S
    for f in range(n_frames):
        devs = [up.upload(per_stream[q][f][0], per_stream[q][f][1]) for q in range(S)]
        pred, outs = ms.step(ms.batch_inputs(devs), [per_stream[q][f][2] for q in range(S)])
        assert pred.shape[0] == 4 * S
        for q in range(S):
            want_pred, want_raw, want_voted = solo[q][f]
            err = (pred[4 * q:4 * q + 4] - want_pred).abs().max().item() / want_pred.abs().max().item()
            same = (outs[q]["raw_labels"] == want_raw).float().mean().item()
            worst = [max(worst[0], err), min(worst[1], same)]
            assert err <= 1e-5 and same >= 0.9999, (f, q, err, same)
            assert [k for k, _ in outs[q]["voted"]] == [k for k, _ in want_voted]
            for (k, a), (_, b) in zip(outs[q]["voted"], want_voted):
                # voting is integer work on the raw labels: identical raw labels -> identical voted labels; count, do not tolerate
                vote_flips = int((a != b).sum().item())
                raw_flips = int((outs[q]["raw_labels"] != want_raw).sum().item())
                if vote_flips or raw_flips:
                    print("8 streams, frame %d stream %d voted frame %d: %d voted / %d raw labels differ from the solo run"
                          % (f, q, k, vote_flips, raw_flips))
                assert vote_flips <= 2 * max(raw_flips, total_raw_flips[q]), (f, q, k, vote_flips, raw_flips)
            total_raw_flips[q] += int((outs[q]["raw_labels"] != want_raw).sum().item())
        s0 = per_stream[0][f][0]
        with torch.no_grad():
            want, _, _, _, mem_cpu = oracle.stage_forward(*(torch.from_numpy(s0[k]) for k in
                                                            ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord")), mem_cpu)
        got = pred[:4].cpu()
        err = (got - want).abs().max().item() / want.abs().max().item()
        n_valid = int(s0["valid_mask"].sum())
        agree = (got.argmax(1)[:, :n_valid] == want.argmax(1)[:, :n_valid]).float().mean().item()
        print("8 streams, frame %d: stream 0 vs oracle %.2e of range, labels %.6f; batched vs solo worst %.2e / %.6f"
              % (f, err, agree, worst[0], worst[1]))
        assert err <= 2e-5 and agree >= 0.9999, (f, err, agree)
    print("8 streams: peak HBM allocated %.1f GB" % (torch.cuda.max_memory_allocated() / 1e9))


def test_pipelined_runner_on_a_warm_engine_at_full_size(model):
    """Two sequences back to back through ONE pipelined runner at the validation shape (reset() in between, engine and
    scratch warm): on frame 0 of the second sequence encode(t) has just been issued on the main stream when encode(t+1)
    starts on the side stream -- both through the same engine.  Must equal the serial runner frame for frame."""
    import bench
    seqs = [bench.make_frames(3, seq_seed=300 + q) for q in range(2)]
    res = {}
    for pipe in (False, True):
        runner = streaming.StreamRunner(model, DEV, vote=False, pipeline=pipe)
        outs = []
        for frames in seqs:
            runner.reset()
            devs = [runner.upload(s, raw) for s, raw, _ in frames]
            for i in range(len(frames)):
                o = runner.step(devs[i], frames[i][2], next_dev=devs[i + 1] if i + 1 < len(frames) else None)
                outs.append((o["pred_cls"].clone(), o["raw_labels"].clone()))
        torch.cuda.synchronize()
        res[pipe] = outs
        runner.close()
    for k, ((p0, r0), (p1, r1)) in enumerate(zip(res[False], res[True])):
        # same kernels on the same inputs; a library conv that splits K with atomic adds may differ in the last bits
        assert torch.equal(p0, p1) or (p0 - p1).abs().max().item() <= 1e-6 * p0.abs().max().item(), k
        assert (r0 == r1).float().mean().item() >= 0.99999, k


@pytest.mark.parametrize("pipe", [False, True])
def test_runner_skipping_the_padding_tail_changes_no_real_point(model, pipe):
    """StreamRunner(skip_padding=True) (the default) tells the point head how many points of the scan are real
    (datasets/data_StreamMOS.py:568-571 pads to frame_point_num, val_StreamMOS.py:113 cuts the tail off): the logits of every
    real point, the TTA labels, the raw-scan labels and the votes are BIT-identical to the runner that computes the tail too;
    the tail's logits are zeros.  Host-preprocessed and device-preprocessed frames (the count lives on the device), plain and
    two-stream."""
    spec = preprocess.VoxelSpec()
    n_frames = 4
    scans = [synth.synthetic_scan(300 + k, 16, 120) for k in range(n_frames + 2)]
    poses = [synth.synthetic_pose(k) for k in range(n_frames + 2)]
    res = {}
    for skip in (False, True):
        runner = streaming.StreamRunner(model, DEV, vote=True, pipeline=pipe, skip_padding=skip)
        runner.voter.window = 3
        outs, devs, nvs = [], [], []
        for i in range(n_frames):
            idx = preprocess.window_indices(i, n_frames + 2, 3)
            sample = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], 2048, spec, tta=True)
            devs.append(runner.upload(sample, scans[i]))
            nvs.append(int(sample["valid_mask"].sum()))
        for i in range(n_frames):
            o = runner.step(devs[i], poses[i], next_dev=devs[i + 1] if pipe and i + 1 < n_frames else None)
            outs.append((o["pred_cls"].clone(), o["labels"].clone(), o["raw_labels"].clone(), [(f, l.clone()) for f, l in o["voted"]]))
        # the same through step_raw: the in-range count never leaves the device
        raw_runner = streaming.StreamRunner(model, DEV, vote=False, pipeline=pipe, skip_padding=skip)
        raws = []
        for i in range(2):
            idx = preprocess.window_indices(i, n_frames + 2, 3)
            o = raw_runner.step_raw([scans[j] for j in idx], [poses[j] for j in idx], frame_point_num=2048)
            raws.append((o["pred_cls"].clone(), o["raw_labels"].clone()))
        res[skip] = (outs, nvs, raws)
    (full, nvs, raw_full), (lean, _, raw_lean) = res[False], res[True]
    for (p0, l0, r0, v0), (p1, l1, r1, v1), nv in zip(full, lean, nvs):
        assert 0 < nv < 2048
        assert torch.equal(p0[:, :, :nv], p1[:, :, :nv]) and float(p1[:, :, nv:].abs().max()) == 0.0 and float(p0[:, :, nv:].abs().max()) > 0
        assert torch.equal(l0[:nv], l1[:nv]) and torch.equal(r0, r1)
        assert [f for f, _ in v0] == [f for f, _ in v1] and all(torch.equal(a, b) for (_, a), (_, b) in zip(v0, v1))
    for (p0, r0), (p1, r1), nv in zip(raw_full, raw_lean, nvs):
        assert torch.equal(p0[:, :, :nv], p1[:, :, :nv]) and float(p1[:, :, nv:].abs().max()) == 0.0 and torch.equal(r0, r1)

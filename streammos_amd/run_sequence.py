"""Stream one SemanticKITTI-format sequence through the MI355X path and write the reference's files.

    python -m streammos_amd.run_sequence --seq-dir .../sequences/08 --out-dir results/sequences/08 \
        [--checkpoint 40-model.pth] [--no-vote] [--device cuda:0]

Writes ``<out>/predictions/NNNNNN.label`` (network output, the files val_StreamMOS.py:121-126 writes) and, with
voting, ``<out>/refined/NNNNNN.label`` (the files voxel_voting.py:244-249 writes).  If the sequence has
``labels/``, the static / moving IoU of both is printed (utils/metric.py formula).  Several sequences are
sharded over ranks with ``streaming.shard_sequences``: under ``torch.distributed.run`` the ranks are the launcher's;
with ``--gpus N`` and no launcher around it the program starts its N ranks itself (``launch.self_launch``, the
reference's README.md:97 launch line folded in; the parent never touches the GPU).
"""
import argparse
import json
import os

import numpy as np
import torch

from . import kitti, launch, preprocess, streaming, synth


def load_model(checkpoint=None, device="cuda:0", seg=False):
    """seg=True: the stage-2 model (models/StreamMOS_seg.py) whose refine head also yields the `_bf` labels."""
    if seg:
        from .refapi.config import StreamMOS_seg as cfg
        from .refapi.models import StreamMOS_seg as StreamMOS
    else:
        from .refapi.config import StreamMOS as cfg
        from .refapi.models import StreamMOS
    model = StreamMOS.AttNet(cfg.get_config()[2])
    if checkpoint:
        state = torch.load(checkpoint, map_location="cpu", weights_only=True)
        state = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state.items()}
        model.load_state_dict(state, strict=True)
    else:
        model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    return model.to(device).eval()


def run_sequence(model, seq_dir, out_dir, device="cuda:0", vote=True, frame_point_num=160000, limit=None, seq_num=3,
                 device_preprocess=False, conv_precision=None):
    """device_preprocess=True: only the raw scans are uploaded (each once) and the validation preprocessing runs on
    the GPU (identical to the host path except the last ulp of asinf / atan2f) -- in the overlapped loop
    of ``_run_overlapped``: file reads and label writes on threads of their own, nothing read back per frame.  The
    default host-preprocessing loop is serial and reproduces the reference's numpy numerics to the last ulp.
    conv_precision "fp32" / "bf16": the engine's convolution precision (streaming.set_conv_precision; None: the model's)."""
    streaming.set_conv_precision(model, conv_precision)
    spec = preprocess.VoxelSpec()
    files = sorted(f for f in os.listdir(os.path.join(seq_dir, "velodyne")) if f.endswith(".bin"))
    if limit:
        files = files[:limit]
    poses = kitti.read_poses(os.path.join(seq_dir, "poses.txt"), kitti.read_calibration(os.path.join(seq_dir, "calib.txt")))
    has_gt = os.path.isdir(os.path.join(seq_dir, "labels"))
    res = {"sequence": os.path.basename(os.path.normpath(seq_dir)), "scans": len(files)}
    if device_preprocess:
        m_raw, m_ref = _run_overlapped(model, seq_dir, out_dir, files, poses, has_gt, device, vote, frame_point_num, seq_num)
    else:
        m_raw, m_ref = _run_serial(model, seq_dir, out_dir, files, poses, has_gt, device, vote, frame_point_num, seq_num, spec)
    if has_gt:
        res["network"] = m_raw.result()
        if vote:
            res["voted"] = m_ref.result()
    return res


def _run_serial(model, seq_dir, out_dir, files, poses, has_gt, device, vote, frame_point_num, seq_num, spec):
    runner = streaming.StreamRunner(model, device, vote=vote)
    m_raw, m_ref = kitti.MovingIoU(), kitti.MovingIoU()
    cache = {}

    def scan(i):
        if i not in cache:
            cache[i] = kitti.read_scan(os.path.join(seq_dir, "velodyne", files[i]))
            for k in [k for k in cache if k < i - 12]:
                del cache[k]
        return cache[i]

    def gt(i):
        return kitti.read_label(os.path.join(seq_dir, "labels", files[i][:-4] + ".label"))

    def emit_refined(voted):
        for fid, lab in voted:
            lab = lab.cpu().numpy()
            kitti.write_prediction(os.path.join(out_dir, "refined", files[fid][:-4] + ".label"), lut_labels=lab)
            if has_gt:
                m_ref.add(gt(fid), np.where(lab == 251, 2, np.where(lab == 9, 1, 0)))

    for i in range(len(files)):
        idx = [min(j, len(files) - 1) for j in preprocess.window_indices(i, len(files), seq_num)]
        sample = preprocess.build_sample([scan(j) for j in idx], [poses[j] for j in idx], frame_point_num, spec, tta=True)
        out = runner.step(runner.upload(sample, scan(i)), poses[i])
        raw = out["raw_labels"].cpu().numpy()
        kitti.write_prediction(os.path.join(out_dir, "predictions", files[i][:-4] + ".label"), labels_012=raw)
        if "bf_raw_labels" in out:          # val_StreamMOS_seg.py:141: raw 0/1/2 words, no LUT
            kitti.write_prediction(os.path.join(out_dir, "predictions_bf", files[i][:-4] + ".label"),
                                   lut_labels=out["bf_raw_labels"].cpu().numpy())
        if has_gt:
            m_raw.add(gt(i), raw)
        emit_refined(out["voted"])
    if runner.voter is not None:
        emit_refined(runner.voter.flush())
    return m_raw, m_ref


IN_FLIGHT = 4          # frames whose labels are on their way to the writer (output ring slots)
READ_AHEAD = 6         # scans the reader thread may hold (input ring slots)


def _iou_from_counts(counts):
    """Device [6] int64 counters of ops.label_words (tp1, tp2, pred1, pred2, gt1, gt2) -> the kitti.MovingIoU they stand for."""
    m = kitti.MovingIoU()
    c = counts.cpu().numpy().astype(np.float64)
    m.tp[:], m.pred[:], m.gt[:] = c[0:2], c[2:4], c[4:6]
    return m


def _run_overlapped(model, seq_dir, out_dir, files, poses, has_gt, device, vote, frame_point_num, seq_num):
    """The device-preprocessing loop, overlapped (DESIGN.md "The sequence loop").  The reader thread reads scans and ground
    truth into pinned slots; this thread uploads each once, runs StreamRunner(pipeline=True).step_raw with the next window,
    and per frame only LAUNCHES the label kernel (prediction words + IoU counts, ops.label_words / voted_label_counts) into
    the frame's device staging slot, copies the window's in-range counts there and queues one device-to-host copy of the
    slot on a copy stream; the writer thread waits for that copy, checks the counts (the host path's capacity error) and
    writes the files.  Nothing is read back per frame: the one wait is for a free output slot, IN_FLIGHT frames behind.
    The IoU counters are read once, at the end.  Instance voting (vote="instance") runs the voter's device-resident path
    (SMOS_INSTANCE_DEVICE=0: the path that reads back per voted frame): the status word of every voted frame travels in the
    slot, and the writer raises before that frame's refined file if the frame had more clusters than the voter has boxes."""
    from . import ops, sequence_io
    from .device_preprocess import check_in_range_counts
    device = torch.device(device)
    n = len(files)
    runner = streaming.StreamRunner(model, device, vote=vote, pipeline=True,
                                    instance_device=streaming.instance_device_switch(True))
    voter = runner.voter
    voter_status = voter.status if isinstance(voter, streaming.InstanceVoter) and voter.device_resident else None
    main = torch.cuda.current_stream(device)
    copier = torch.cuda.Stream(device)
    gt_map = torch.from_numpy(kitti.learning_map_lut()).to(device)
    counts_raw = torch.zeros(6, dtype=torch.int64, device=device)
    counts_ref = torch.zeros(6, dtype=torch.int64, device=device)
    reader = sequence_io.ScanReader(seq_dir, files, ring=READ_AHEAD, labels=has_gt)
    writer = None
    try:
        a4 = (reader.max_points + 3) // 4 * 4
        cap = (2 + streaming.VOTE_WINDOW) * a4 + (seq_num + 3) // 4 * 4 + 4 * streaming.VOTE_WINDOW
        dev_stage = [torch.empty(cap, dtype=torch.int32, device=device) for _ in range(IN_FLIGHT)]
        host_stage = [torch.empty(cap, dtype=torch.int32, pin_memory=True) for _ in range(IN_FLIGHT)]
        writer = sequence_io.SlotWriter(range(IN_FLIGHT))
        dev_scans, gt_dev = {}, {}
        pulled = [0]

        def dev_scan(i):
            while pulled[0] <= i:                     # frames arrive in order; each is uploaded once, from its pinned slot
                fr = reader.get()
                dev_scans[fr.index] = fr.scan.to(device, non_blocking=True)
                if fr.label is not None:
                    gt_dev[fr.index] = fr.label.to(device, non_blocking=True)
                done = torch.cuda.Event(blocking=True)
                done.record(main)
                reader.release(fr, done)
                pulled[0] += 1
                for k in [k for k in dev_scans if k < fr.index - 12]:
                    del dev_scans[k]
            return dev_scans[i]

        def launch_slot(frame, out, voted):
            """Label kernels of one frame (frame None: the voter's flush) into a free slot, its D2H, the writer's job."""
            k = writer.take()                         # back-pressure: waits while IN_FLIGHT slots are on their way
            stage, off = dev_stage[k], 0
            parts = {}

            def section(name, m):
                nonlocal off
                parts[name] = (off, m)
                off += (m + 3) // 4 * 4
                return stage[parts[name][0]:parts[name][0] + m]

            if frame is not None:
                raw = out["raw_labels"]
                ops.label_words(raw, words=section(("predictions", frame), raw.shape[0]), lut=True,
                                gt=gt_dev.get(frame) if has_gt else None, gt_map=gt_map, counts=counts_raw)
                if "bf_raw_labels" in out:
                    ops.label_words(out["bf_raw_labels"], words=section(("predictions_bf", frame), raw.shape[0]), lut=False)
                section("counts", seq_num).copy_(runner.last_in_range_counts())
                if not vote:
                    gt_dev.pop(frame, None)
            if len(voted) > streaming.VOTE_WINDOW:
                raise RuntimeError("run_sequence: the voter released %d frames at once (slots hold %d)"
                                   % (len(voted), streaming.VOTE_WINDOW))
            for fid, lab in voted:
                if voter_status is not None:          # checked by the writer before the frame's refined file
                    section(("status", fid), 1).copy_(voter_status(fid))
                ops.voted_label_counts(lab, gt_dev.pop(fid) if has_gt else None, gt_map, counts_ref,
                                       words=section(("refined", fid), lab.shape[0]))
            ready = torch.cuda.Event()
            ready.record(main)
            copier.wait_event(ready)
            with torch.cuda.stream(copier):
                host_stage[k][:off].copy_(stage[:off], non_blocking=True)
            copied = torch.cuda.Event(blocking=True)
            copied.record(copier)
            host = host_stage[k].numpy()

            def write():
                if "counts" in parts:                 # the window's capacity check comes before any file of the frame
                    o, m = parts["counts"]
                    check_in_range_counts(host[o:o + m].tolist(), frame_point_num)
                for key, (o, m) in parts.items():
                    if key != "counts":
                        sub, fid = key
                        if sub == "status":
                            if int(host[o]) & 1:
                                raise RuntimeError("instance voting: more than %d clusters in frame %s"
                                                   % (voter.max_boxes, files[fid][:-4]))
                            continue
                        kitti.write_prediction(os.path.join(out_dir, sub, files[fid][:-4] + ".label"), lut_labels=host[o:o + m])

            writer.submit(k, copied, write)

        for i in range(n):
            if writer.error is not None:
                raise writer.error
            idx = [min(j, n - 1) for j in preprocess.window_indices(i, n, seq_num)]
            nxt = [min(j, n - 1) for j in preprocess.window_indices(i + 1, n, seq_num)] if i + 1 < n else None
            out = runner.step_raw([dev_scan(j) for j in idx], [poses[j] for j in idx], frame_point_num,
                                  next_scans=[dev_scan(j) for j in nxt] if nxt else None,
                                  next_poses=[poses[j] for j in nxt] if nxt else None)
            launch_slot(i, out, out["voted"])
        if runner.voter is not None:
            voted = runner.voter.flush()
            if voted:
                launch_slot(None, None, voted)
        writer.close()                                # the files of every frame are written when this returns
        if writer.error is not None:
            raise writer.error
        m_raw = _iou_from_counts(counts_raw) if has_gt else None
        m_ref = _iou_from_counts(counts_ref) if has_gt and vote else None
        return m_raw, m_ref
    except BaseException:
        if writer is not None:
            writer.close()
        torch.cuda.synchronize(device)                # nothing of this run stays in flight once the error is raised
        raise
    finally:
        reader.close()


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq-dir", nargs="+", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--device", default=None)
    ap.add_argument("--no-vote", action="store_true")
    ap.add_argument("--seg", action="store_true", help="stage-2 model StreamMOS_seg (488-tensor checkpoint)")
    ap.add_argument("--instance-vote", action="store_true",
                    help="voxel_instance_voting.py instead of voxel_voting.py for the refined labels (needs --seg: the "
                         "clusters come from the `_bf` prediction)")
    ap.add_argument("--limit", type=int, default=None)
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks (one per GPU) the sequences are sharded over; > 1 without a launcher: started by this program")
    ap.add_argument("--frame-point-num", type=int, default=160000, help="Val.frame_point_num of config/StreamMOS.py:44")
    ap.add_argument("--device-preprocess", action="store_true",
                    help="range filter / pose alignment / TTA / quantisation on the GPU: only raw scans cross PCIe")
    ap.add_argument("--conv-precision", choices=("fp32", "bf16"), default="fp32",
                    help="convolutions of the engine in exact fp32 (default) or on the bf16 matrix cores (opt-in)")
    return ap


def main():
    ap = build_parser()
    args = ap.parse_args()
    if args.gpus > 1 and not launch.under_launcher():
        import sys
        sys.exit(launch.self_launch(args.gpus, sys.argv[1:], module="streammos_amd.run_sequence"))
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    # SMOS_BENCH_ONE_DEVICE=1 (rehearsal on a one-GPU box, as in bench.py): every rank uses cuda:0
    local = 0 if os.environ.get("SMOS_BENCH_ONE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    device = args.device or "cuda:%d" % local
    lengths = {d: len(os.listdir(os.path.join(d, "velodyne"))) for d in args.seq_dir}
    mine = streaming.shard_sequences(lengths, world)[rank]
    if args.instance_vote and not args.seg:
        ap.error("--instance-vote needs --seg")
    model = load_model(args.checkpoint, device, seg=args.seg)
    vote = False if args.no_vote else ("instance" if args.instance_vote else True)
    for d in mine:
        out = os.path.join(args.out_dir, os.path.basename(os.path.normpath(d))) if len(args.seq_dir) > 1 else args.out_dir
        res = run_sequence(model, d, out, device, vote=vote, limit=args.limit, frame_point_num=args.frame_point_num,
                           device_preprocess=args.device_preprocess, conv_precision=args.conv_precision)
        print(json.dumps(dict(res, rank=rank, world=world)), flush=True)


if __name__ == "__main__":
    main()

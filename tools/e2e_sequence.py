"""Dev: full-size end-to-end run of run_sequence on a synthetic SemanticKITTI-layout sequence (120k-point scans,
frame_point_num 160000), stage-2 model + instance voting; prints the IoU report and the wall time per scan.

    python tools/e2e_sequence.py [N]          # the three configurations on N scans (default 24), wall time incl. set-up
    python tools/e2e_sequence.py --steady N   # stage 1 + voxel voting + --device-preprocess on N >= 200 scans: a warm-up
                                              # run, then a second run_sequence call on the same model (warm page cache)
                                              # timed on its own: steady-state scans/s of the deployable loop
    python tools/e2e_sequence.py --steady N --instance [--alternate R]
                                              # the steady mode with the stage-2 model and instance voting (vote="instance",
                                              # device preprocessing); --alternate R: after the warm-up runs, R timed runs
                                              # each with SMOS_INSTANCE_DEVICE=0 and =1, alternating, in this process
    --conv-precision {fp32,bf16}              # the engine's convolution precision (default fp32)
"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from streammos_amd import kitti, run_sequence, synth
steady = "--steady" in sys.argv
prec = "fp32"
if "--conv-precision" in sys.argv:
    i = sys.argv.index("--conv-precision")
    prec = sys.argv[i + 1]
    if prec not in ("fp32", "bf16"):
        sys.exit("--conv-precision: fp32 or bf16")
    del sys.argv[i:i + 2]
instance = "--instance" in sys.argv
alternate = 0
if "--alternate" in sys.argv:
    i = sys.argv.index("--alternate")
    alternate = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
args = [a for a in sys.argv[1:] if a not in ("--steady", "--instance")]
n = int(args[0]) if args else (200 if steady else 24)
root = tempfile.mkdtemp(prefix="smos_seq_")
seq = os.path.join(root, "sequences", "08")
os.makedirs(os.path.join(seq, "velodyne")); os.makedirs(os.path.join(seq, "labels"))
for k in range(n):
    scan, lab = synth.synthetic_scan(k, with_labels=True)
    scan.tofile(os.path.join(seq, "velodyne", "%06d.bin" % k))
    kitti.write_prediction(os.path.join(seq, "labels", "%06d.label" % k), lut_labels=np.where(lab == 2, 251, 9).astype(np.uint32))
kitti.write_poses(os.path.join(seq, "poses.txt"), [synth.synthetic_pose(k) for k in range(n)])
kitti.write_calibration(os.path.join(seq, "calib.txt"))
if steady:
    import torch
    model = run_sequence.load_model(None, "cuda:0", seg=instance)
    what = "stage 2 + instance voting" if instance else "stage 1 + voxel voting"
    reps = [("warm-up", None), ("timed", None)]
    if instance and alternate:
        reps = [("warm-up", "0"), ("warm-up", "1")] + [("timed", v) for _ in range(alternate) for v in ("0", "1")]
    for rep, switch in reps:
        if switch is not None:
            os.environ["SMOS_INSTANCE_DEVICE"] = switch
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = run_sequence.run_sequence(model, seq, os.path.join(root, "out_steady"), "cuda:0", vote="instance" if instance else True,
                                        device_preprocess=True, conv_precision=prec)
        torch.cuda.synchronize()          # run_sequence returns after its last file is written; nothing is left queued
        dt = time.perf_counter() - t
        tag = " SMOS_INSTANCE_DEVICE=%s" % os.environ.get("SMOS_INSTANCE_DEVICE", "unset") if instance else ""
        print("steady %s (conv %s%s): %s + device preprocessing, %d scans: %.1f scans/s (%.2f ms/scan, disk IO "
              "and runner set-up included)" % (rep, prec, tag, what, n, n / dt, 1e3 * dt / n), res, flush=True)
    sys.exit(0)
for seg, vote, devpre in ((False, True, False), (True, "instance", False), (True, "instance", True)):
    model = run_sequence.load_model(None, "cuda:0", seg=seg)
    t = time.time()
    res = run_sequence.run_sequence(model, seq, os.path.join(root, "out_%d%d" % (seg, devpre)), "cuda:0", vote=vote, device_preprocess=devpre,
                                    conv_precision=prec)
    dt = time.time() - t
    print("seg=%s vote=%s device_preprocess=%s  %.1f ms/scan (disk IO included)" % (seg, vote, devpre, 1e3 * dt / n), res, flush=True)
import numpy as np
a = [np.fromfile(os.path.join(root, "out_10", "refined", "%06d.label" % k), dtype=np.uint32) for k in range(n)]
b = [np.fromfile(os.path.join(root, "out_11", "refined", "%06d.label" % k), dtype=np.uint32) for k in range(n)]
print("refined labels host-vs-device preprocessing agreement: %.5f" % np.mean([np.mean(x == y) for x, y in zip(a, b)]))

"""Dev: the copy-paste augmentation of one training sample on the device (device_preprocess.DeviceCopyPaste,
csrc/copy_paste.hip) against the numpy restatement on one host core (preprocess.copy_paste_sample), and build_batch with the
paste stage in front beside the stage-1 training step.

  python tools/ubench_copy_paste.py [--out profiles/ubench_copy_paste.txt] [--reps 5] [--no-step]

Sample: five synthetic scans of 64 x 1875 = 120 000 points (the ground returns carry the road id 40, the movers 252, the rest 70),
10 objects of 500 points out of a bank of 16, explicit scalar draws, noise generated in the kernels or read from the device.
Device (HIP events around 20 back-to-back calls after a warm-up, `reps` such measurements, median and min..max): host scans in,
device-resident scans in, and one call that also builds and uploads the bank; the kernels' own time and the launch count from the
profiler.  Host: the same sample and draws through the restatement in a child pinned to one core with the BLAS / OpenMP pools at
one thread; drawing the noise with numpy's generator is timed beside it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from tools.ubench_train_prep import N_POINTS, kernel_stats

DEV = "cuda:0"
ITERS = 20
OBJECTS, OBJECT_POINTS, BANK = 10, 500, 16


def sample_inputs(first=6):
    from streammos_amd import preprocess, synth
    idx = preprocess.train_window_indices(first, first + 6)
    scans, words, poses = [], [], []
    for k in idx:
        scan, lab = synth.synthetic_scan(k, with_labels=True)
        sem = np.where(lab == 2, 252, np.where(np.abs(scan[:, 2] + 1.73) < 0.05, 40, 70)).astype(np.uint32)
        scans.append(scan)
        words.append(sem | (np.arange(lab.shape[0], dtype=np.uint32) << np.uint32(16)))
        poses.append(synth.synthetic_pose(k))
    return scans, words, poses


def make_bank():
    from streammos_amd import preprocess
    rng = np.random.Generator(np.random.PCG64(77))
    bank = []
    for i in range(BANK):
        cate = preprocess.PASTE_CATEGORIES[i % len(preprocess.PASTE_CATEGORIES)]
        r, az, yaw = rng.uniform(8.0, 30.0), rng.uniform(0, 2 * np.pi), rng.uniform(-np.pi, np.pi)
        size = np.array([4.0, 1.8, 1.6])
        centre = np.array([r * np.cos(az), r * np.sin(az), -0.9])
        local = rng.uniform(-0.5, 0.5, (OBJECT_POINTS, 3)) * size
        c, s = np.cos(yaw), np.sin(yaw)
        xyz = np.stack((c * local[:, 0] - s * local[:, 1], s * local[:, 0] + c * local[:, 1], local[:, 2]), axis=1) + centre
        bank.append(preprocess.PasteObject(np.concatenate((xyz, rng.random((OBJECT_POINTS, 1))), axis=1).astype(np.float32), centre, size,
                                           yaw, cate))
    return bank


def scalar_draws(sample=0):
    """OBJECTS objects: bank index, velocity and trial order from numpy's generator."""
    from streammos_amd import preprocess
    rng = np.random.Generator(np.random.PCG64(500 + sample))
    index = rng.integers(0, BANK, OBJECTS).tolist()
    velocity = [rng.uniform(*preprocess.PASTE_VELOCITY[preprocess.PASTE_CATEGORIES[i % 8]]) for i in index]
    order = np.stack([rng.permutation(preprocess.PASTE_TRIALS) for _ in index]).astype(np.uint8)
    return index, velocity, order


def host_child(reps):
    """Pinned to one core; prints one JSON line."""
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    except (AttributeError, OSError):
        pass
    from streammos_amd import preprocess
    scans, words, poses = sample_inputs()
    bank = make_bank()
    index, velocity, order = scalar_draws()
    rng = np.random.Generator(np.random.PCG64(1))
    inv0 = np.linalg.inv(poses[0])
    draw_s, paste_s, status = [], [], None
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        noise = [rng.normal(0.0, preprocess.PASTE_NOISE_STD, (5, OBJECT_POINTS, 3)) for _ in index]
        t1 = time.perf_counter()
        aligned = [preprocess.pose_align(s, inv0.dot(p)) for s, p in zip(scans, poses)]
        t2 = time.perf_counter()
        road = aligned[0][(words[0] & np.uint32(0xFFFF)) == preprocess.PASTE_ROAD_ID]
        _, _, status = preprocess.copy_paste_sample(aligned, words, road, bank, preprocess.PasteDraws(index, velocity, order, noise))
        t3 = time.perf_counter()
        draw_s.append(t1 - t0)
        paste_s.append(t3 - t2)
    print(json.dumps({"draw_s": draw_s[1:], "paste_s": paste_s[1:], "cores": len(os.sched_getaffinity(0)), "status": status.tolist()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_copy_paste.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-child", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if args.host_child:
        return host_child(args.reps)
    import torch

    from streammos_amd import device_preprocess, preprocess, synth
    from tools.ubench_bilinear import fmt, measure
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_copy_paste.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    scans, words, poses = sample_inputs()
    objects = make_bank()
    index, velocity, order = scalar_draws()
    log("one sample: 5 scans of %d points (%d road points in scan 0), %d objects of %d points, bank of %d"
        % (scans[0].shape[0], int(((words[0] & 0xFFFF) == 40).sum()), OBJECTS, OBJECT_POINTS, BANK))
    bank = device_preprocess.DeviceObjectBank(DEV, objects)
    paste = device_preprocess.DeviceCopyPaste(bank)
    noise = [torch.empty((5, OBJECT_POINTS, 3), dtype=torch.float64, device=DEV).normal_(0.0, preprocess.PASTE_NOISE_STD) for _ in index]
    draws = preprocess.PasteDraws(index, velocity, order, noise)
    dev_scans = [torch.from_numpy(s).to(DEV) for s in scans]
    dev_words = [torch.from_numpy(w.view(np.int32)).to(DEV) for w in words]
    _, _, status = paste.apply(dev_scans, dev_words, poses, draws=draws)
    log("accepted trial per object (-1: none): %s" % status.cpu().tolist())
    with_up = measure(lambda: paste.apply(scans, words, poses, draws=draws), args.reps, iters=ITERS)
    resident = measure(lambda: paste.apply(dev_scans, dev_words, poses, draws=draws), args.reps, iters=ITERS)

    def with_bank():
        fresh = device_preprocess.DeviceCopyPaste(device_preprocess.DeviceObjectBank(DEV, objects))
        return fresh.apply(scans, words, poses, draws=draws)
    cold = measure(with_bank, args.reps, iters=ITERS)
    n_launch, k_us, names = kernel_stats(lambda: paste.apply(dev_scans, dev_words, poses, draws=draws))
    log("device paste, host scans in, bank resident (staging + 2 copies + launches)   %s  median (min..max) of %d x %d calls" % (fmt(with_up), args.reps, ITERS))
    log("device paste, scans already on the device, bank resident                     %s" % fmt(resident))
    log("device paste, host scans in, bank built and uploaded by the same call        %s" % fmt(cold))
    log("kernels of one call: %d launches (1 + 4 per object of 10 points or more), %.3f ms summed" % (n_launch, k_us / 1e3))
    for name, us in sorted(names.items(), key=lambda kv: -kv[1]):
        log("    %-60s %8.3f ms" % (name[:60], us / 1e3))
    seeded = next(i for i in range(4096) if len(preprocess.seeded_paste_scalars(1, i, bank.categories)[0]) == OBJECTS)
    t_seed = measure(lambda: paste.apply(dev_scans, dev_words, poses, seed=1, sample_index=seeded), args.reps, iters=ITERS)
    log("device paste, seeded (%d objects, noise from Philox in the kernels)            %s" % (OBJECTS, fmt(t_seed)))

    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-child", "--reps", str(max(3, args.reps))],
                          env=dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1"),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if proc.returncode != 0:
        log("host child FAILED (exit %d): %s" % (proc.returncode, proc.stderr.strip().splitlines()[-1:] or ""))
        raise SystemExit(proc.returncode)
    h = json.loads(proc.stdout.strip().splitlines()[-1])
    host_ms = [1e3 * v for v in h["paste_s"]]
    log("host restatement, %d core (numpy, BLAS pools at one thread), scans aligned     %s  of %d calls; accepted %s"
        % (h["cores"], fmt(host_ms), len(host_ms), h["status"]))
    log("    numpy's generator for the noise of the %d objects, same core              %s" % (OBJECTS, fmt([1e3 * v for v in h["draw_s"]])))
    log("host one core / device with uploads: %.1f" % (statistics.median(host_ms) / statistics.median(with_up)))
    log("no host read in the device path: the status stays on the device; launches = 1 + 4 x (objects of 10 points or more)")

    if not args.no_step:
        from streammos_amd.refapi.config import StreamMOS as cfg
        from streammos_amd.refapi.models import StreamMOS
        torch.cuda.empty_cache()
        pre = device_preprocess.DeviceTrainPreprocessor(DEV, frame_point_num=N_POINTS, paste_labels={"pcds_target": (0, 1, 2)})
        model = StreamMOS.AttNet(cfg.get_config()[2])
        model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
        model = model.to(DEV).train()
        torch.manual_seed(0)
        samples = [sample_inputs(first) for first in (6, 7, 8, 9)]
        batch = pre.alloc_batch(4)

        def build(with_paste=True):
            return pre.build_batch(samples, seed=3, out=batch, paste=paste if with_paste else None)

        def step():
            model.zero_grad(set_to_none=True)
            loss = model({k: v for k, v in batch.items() if k != "paste_status"})
            loss.backward()
            return loss
        built = build()
        counts = [int(st.shape[0]) for st in built["paste_status"]]
        loss = step()
        t_plain = measure(lambda: build(False), args.reps, iters=20, warm=2)
        t_build = measure(build, args.reps, iters=20, warm=2)
        t_step = measure(step, args.reps, iters=1, warm=2)
        log("")
        log("stage-1 training step (AttNet.forward on three chained samples + backward, train mode, B = 4, N = %d)" % N_POINTS)
        log("build_batch of 4 samples, host scans in, no paste              %s" % fmt(t_plain))
        log("build_batch of 4 samples with paste (seeded: %s objects)   %s" % (counts, fmt(t_build)))
        log("step on the built batch                                        %s   loss %.5f" % (fmt(t_step), float(loss.item())))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

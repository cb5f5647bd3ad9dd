"""Dev: one training sample built on the device (device_preprocess.DeviceTrainPreprocessor, csrc/train_prep.hip) against the
numpy restatement on one host core (preprocess.build_train_sample), and the stage-1 training step fed device-built batches.

  python tools/ubench_train_prep.py [--out profiles/ubench_train_prep.txt] [--reps 5] [--no-step]

Sample: five synthetic scans of 64 x 1875 = 120 000 points, N = 130 000, the reference's AugParam, seeded draws.
Device (HIP events around 200 back-to-back builds after a warm-up, `reps` such measurements, median and min..max): host
scans in (pinned staging + copies + the four launches) and device-resident scans in (the launches alone); the kernels' own
time and the launch count of one build from the profiler.  Host: the same sample through the restatement in a child pinned to
one core with the BLAS / OpenMP pools at one thread; drawing with numpy's generator (what the reference's np.random calls
cost) is timed beside it.  Bytes crossing PCIe per sample both ways.  Step: AttNet.forward on three chained samples +
backward (train mode, B = 4, N = 130 000) on a batch `build_batch` made, the build of that batch, and both in sequence.
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

N_POINTS = 130000
DEV = "cuda:0"
ITERS = 200          # builds per timed window: a window of a few milliseconds would measure the clock


def sample_inputs(first=6):
    from streammos_amd import preprocess, synth
    idx = preprocess.train_window_indices(first, first + 6)
    scans, words, poses = [], [], []
    for k in idx:
        scan, lab = synth.synthetic_scan(k, with_labels=True)
        scans.append(scan)
        words.append(np.where(lab == 2, 252, 40).astype(np.uint32) | (np.arange(lab.shape[0], dtype=np.uint32) << np.uint32(16)))
        poses.append(synth.synthetic_pose(k))
    return scans, words, poses


def host_child(reps):
    """Pinned to one core; prints one JSON line."""
    try:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    except (AttributeError, OSError):
        pass
    from streammos_amd import preprocess
    scans, words, poses = sample_inputs()
    spec, aug = preprocess.VoxelSpec(), preprocess.AugParam()
    rng = np.random.Generator(np.random.PCG64(1))
    draw_s, build_s = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        w = rng.integers(0, 1 << 32, (3, 3, N_POINTS), dtype=np.uint64).astype(np.uint32)
        noise = rng.normal(aug.noise_mean, aug.noise_std, (3, 3 * N_POINTS, 3))
        draws = preprocess.TrainDraws(w, noise, (1.1, -0.7, 0.2), 1.01, 1, 0, 33.0)
        t1 = time.perf_counter()
        out = preprocess.build_train_sample(scans, words, poses, N_POINTS, spec, aug, draws)
        t2 = time.perf_counter()
        draw_s.append(t1 - t0)
        build_s.append(t2 - t1)
    nbytes = sum(v.nbytes for k, v in out.items() if k != "in_range_counts")
    print(json.dumps({"draw_s": draw_s[1:], "build_s": build_s[1:], "cores": len(os.sched_getaffinity(0)), "sample_bytes": nbytes}), flush=True)


def kernel_stats(fn):
    """(launches, summed kernel microseconds) of one call of fn from the profiler's device activities."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
          and "memset" not in e.name.lower()]
    names = {}
    for e in ev:
        names[e.name] = names.get(e.name, 0.0) + e.device_time_total
    return len(ev), sum(names.values()), names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_train_prep.txt"))
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
    log("tools/ubench_train_prep.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    scans, words, poses = sample_inputs()
    n_raw = sum(s.shape[0] for s in scans)
    log("one sample: 5 scans of %d points, N = %d, 3 windows x 3 frames, seeded draws, reference AugParam" % (scans[0].shape[0], N_POINTS))
    pre = device_preprocess.DeviceTrainPreprocessor(DEV, frame_point_num=N_POINTS)
    out = pre.alloc_batch(1)
    dev_scans = [torch.from_numpy(s).to(DEV) for s in scans]
    dev_words = [torch.from_numpy(w.view(np.int32)).to(DEV) for w in words]
    with_up = measure(lambda: pre.build(scans, words, poses, seed=1, out=out), args.reps, iters=ITERS)
    resident = measure(lambda: pre.build(dev_scans, dev_words, poses, seed=1, out=out), args.reps, iters=ITERS)
    n_launch, k_us, names = kernel_stats(lambda: pre.build(dev_scans, dev_words, poses, seed=1, out=out))
    log("device build, host scans in (staging + 2 copies + launches)   %s  median (min..max) of %d x %d builds" % (fmt(with_up), args.reps, ITERS))
    log("device build, scans already on the device (launches alone)    %s" % fmt(resident))
    log("kernels of one build: %d launches, %.3f ms summed" % (n_launch, k_us / 1e3))
    for name, us in sorted(names.items(), key=lambda kv: -kv[1]):
        log("    %-60s %8.3f ms" % (name[:60], us / 1e3))
    explicit = pre.seeded_draws(1, 0)
    expl = measure(lambda: pre.build(dev_scans, dev_words, poses, draws=explicit, out=out), args.reps, iters=ITERS)
    log("device build, explicit draws read from device memory           %s" % fmt(expl))

    proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-child", "--reps", str(max(3, args.reps))],
                          env=dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1"),
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if proc.returncode != 0:
        log("host child FAILED (exit %d): %s" % (proc.returncode, proc.stderr.strip().splitlines()[-1:] or ""))
        raise SystemExit(proc.returncode)
    h = json.loads(proc.stdout.strip().splitlines()[-1])
    host_ms = [1e3 * v for v in h["build_s"]]
    log("host restatement, %d core (numpy, BLAS pools at one thread)     %s  of %d builds" % (h["cores"], fmt(host_ms), len(host_ms)))
    log("    numpy's generator for the same draws (words + noise), same core %s" % fmt([1e3 * v for v in h["draw_s"]]))
    ratio = statistics.median(host_ms) / statistics.median(with_up)
    log("host one core / device with uploads: %.1f; a loader that must deliver 25 samples/s needs %.1f such cores for this arithmetic, "
        "the device %.1f %% of its time" % (ratio, 25 * statistics.median(host_ms) / 1e3, 25 * statistics.median(with_up) / 10))
    up_dev = n_raw * 20
    log("bytes over PCIe per sample: device path %.2f MB up (scans 16 B + label words 4 B a point), 0 B down (counts stay on the device); "
        "host path %.2f MB up (the built tensors)" % (up_dev / 1e6, h["sample_bytes"] / 1e6))

    if not args.no_step:
        from streammos_amd.refapi.config import StreamMOS as cfg
        from streammos_amd.refapi.models import StreamMOS
        del out, explicit
        torch.cuda.empty_cache()
        model = StreamMOS.AttNet(cfg.get_config()[2])
        model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
        model = model.to(DEV).train()
        torch.manual_seed(0)
        samples = [sample_inputs(first) for first in (6, 7, 8, 9)]
        batch = pre.alloc_batch(4)

        def build():
            return pre.build_batch(samples, seed=3, out=batch)

        def step():
            model.zero_grad(set_to_none=True)
            loss = model(batch)
            loss.backward()
            return loss
        build()
        loss = step()
        t_build = measure(build, args.reps, iters=50, warm=2)
        t_step = measure(step, args.reps, iters=1, warm=2)
        t_both = measure(lambda: (build(), step()), args.reps, iters=1, warm=1)
        log("")
        log("stage-1 training step (AttNet.forward on three chained samples + backward, train mode, B = 4, N = %d) on device-built batches" % N_POINTS)
        log("build_batch of 4 samples, host scans in        %s" % fmt(t_build))
        log("step on the built batch                        %s   loss %.5f, peak %.1f GiB" % (fmt(t_step), float(loss.item()),
                                                                                             torch.cuda.max_memory_allocated() / 2 ** 30))
        log("build_batch + step in sequence, one stream     %s" % fmt(t_both))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

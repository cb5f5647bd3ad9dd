"""Dev: forward + backward of the grid -> point bilinear gather on the own kernels against F.grid_sample, per call site
of one training sample-forward and per stage-1 training step.

  python tools/ubench_bilinear.py [--out profiles/ubench_bilinear.txt] [--reps 5]

Per call site (batch 4, N = 130 000, the coordinates of a synthetic scan; HIP events around `iters` back-to-back
forward + backward pairs after a warm-up, `reps` such measurements, median and min..max): the module's own path
(ops.bilinear_gather + its autograd node) against the F.grid_sample formulation in the same process, and the backward
launch alone with the added bytes per second it issues after the run merge (the bytes before the merge are listed as work).
Per step: AttNet.forward on three chained samples + backward, SMOS_BILINEAR_BWD=1 (the gradient channels-last-strided as
the autograd node returns it, and made NCHW-contiguous by one more pass) and =0, each in a fresh child process
(the switch is read once per process).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn.functional as F

DEV = "cuda:0"
N_POINTS = 130000
# name, C, (H, W), scale, coordinates
SITES = (("x0", 32, (256, 256), (0.5, 0.5), "bev"), ("x0_rv", 32, (32, 1024), (0.5, 0.5), "rv"),
         ("x1", 64, (128, 128), (0.25, 0.25), "bev"), ("x1_rv", 64, (16, 512), (0.25, 0.25), "rv"),
         ("decoder", 64, (256, 256), (0.5, 0.5), "bev"))
ATOMIC_RATE = 1.3e12      # chip-wide float atomic rate of the MI355X, added bytes per second


def samples(n_samples):
    from streammos_amd import preprocess, synth
    spec = preprocess.VoxelSpec()
    total = n_samples + 2
    scans = [synth.synthetic_scan(k) for k in range(total)]
    poses = [synth.synthetic_pose(k) for k in range(total)]
    out = []
    for i in range(n_samples):
        idx = preprocess.window_indices(i, total, 3)
        out.append(preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], N_POINTS, spec, tta=True))
    return out


def measure(fn, reps, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return ms


def fmt(ms):
    return "%8.3f ms (%.3f..%.3f)" % (statistics.median(ms), min(ms), max(ms))


def issued_rows(coord, scale, h, w):
    """(taps of every point inside the map, row adds bil_bwd_rows issues per 64-channel chunk, the share of those adds that
    lands in the 1 % most-hit pixels, the adds into the most-hit pixel): runs of equal cells inside 32-point tiles, times
    the taps of the run's cell that lie inside the map."""
    from oracle import ops_np
    iy, ix = ops_np.bilinear_pixel_coords(coord, scale, h, w)
    fin = (iy > -2) & (iy < h + 1) & (ix > -2) & (ix < w + 1)
    y0 = np.where(fin, np.floor(iy), -5).astype(np.int64)
    x0 = np.where(fin, np.floor(ix), -5).astype(np.int64)
    taps = sum(((y0 + dy >= 0) & (y0 + dy < h) & (x0 + dx >= 0) & (x0 + dx < w)).astype(np.int64) for dy in (0, 1) for dx in (0, 1))
    tail = np.ones(y0.shape, dtype=bool)
    tail[:, :-1] = (y0[:, 1:] != y0[:, :-1]) | (x0[:, 1:] != x0[:, :-1])
    tail[:, 31::32] = True
    hits = np.zeros(y0.shape[0] * h * w, dtype=np.int64)
    batch = np.broadcast_to(np.arange(y0.shape[0])[:, None], y0.shape)
    for dy in (0, 1):
        for dx in (0, 1):
            ok = tail & (y0 + dy >= 0) & (y0 + dy < h) & (x0 + dx >= 0) & (x0 + dx < w)
            hits += np.bincount(((batch * h + y0 + dy) * w + x0 + dx)[ok], minlength=hits.size)
    hot = np.sort(hits)[::-1]
    return int(taps.sum()), int(taps[tail].sum()), float(hot[:max(1, hot.size // 100)].sum()) / max(1, int(hot.sum())), int(hot[0])


def call_sites(reps, log):
    from streammos_amd import ops
    s = samples(1)[0]
    coords = {"bev": torch.from_numpy(s["pcds_coord"]).to(DEV)[:, 0, :, :2].contiguous(),       # (B, N, 2, 1)
              "rv": torch.from_numpy(s["pcds_sphere_coord"]).to(DEV)[:, 0].contiguous()}
    b, n = coords["bev"].shape[:2]
    log("call sites: B = %d, N = %d, forward + backward (torch.autograd.grad), median (min..max) of %d x 10 pairs" % (b, n, reps))
    log("%-8s %-14s %-30s %-30s %s" % ("site", "C x H x W", "own (HIP gather + bwd)", "F.grid_sample", "own / grid_sample"))
    own_sum, ref_sum, rows = [0.0] * reps, [0.0] * reps, []
    for name, c, (h, w), scale, which in SITES:
        coord = coords[which]
        grid = torch.randn((b, c, h, w), device=DEV, requires_grad=True)
        go = torch.randn((b, c, n, 1), device=DEV)
        gx = (2 * coord[:, :, 1] * scale[1] / (w - 1)) - 1
        gy = (2 * coord[:, :, 0] * scale[0] / (h - 1)) - 1
        norm = torch.stack((gx, gy), dim=-1)

        def own():
            out = ops.bilinear_gather(grid, coord, scale).unsqueeze(-1)
            return torch.autograd.grad(out, grid, go)[0]

        def ref():
            out = F.grid_sample(grid, norm, mode="bilinear", padding_mode="zeros", align_corners=True)
            return torch.autograd.grad(out, grid, go)[0]
        dev = (own() - ref()).abs().max().item()
        t_own, t_ref = measure(own, reps), measure(ref, reps)
        c2 = coord[..., 0].contiguous()
        t_bwd = measure(lambda: ops.bilinear_gather_backward(go[..., 0], c2, scale, (h, w)), reps)
        taps, issued, hot_share, hottest = issued_rows(coord[..., 0].cpu().numpy(), scale, h, w)
        rows.append((name, c, h, w, t_bwd, taps * c * 4, issued * c * 4, dev, hot_share, hottest))
        own_sum = [a + t for a, t in zip(own_sum, t_own)]
        ref_sum = [a + t for a, t in zip(ref_sum, t_ref)]
        log("%-8s %-14s %-30s %-30s %.2f" % (name, "%dx%dx%d" % (c, h, w), fmt(t_own), fmt(t_ref),
                                             statistics.median(t_own) / statistics.median(t_ref)))
    log("%-8s %-14s %-30s %-30s %.2f" % ("sum", "", fmt(own_sum), fmt(ref_sum), statistics.median(own_sum) / statistics.median(ref_sum)))
    log("")
    log("backward launch alone (memset + bil_bwd_rows, grad_out channel-major): added bytes = in-map taps x C x 4")
    log("hot rows: share of the issued row adds that lands in the 1 % most-hit pixels / adds into the most-hit pixel")
    log("taps MB: w * g products before the run merge (work, not traffic); issued MB: what the atomics add, the figure the atomic rate applies to")
    log("%-8s %-28s %-10s %-10s %-25s %-14s %s" % ("site", "time", "taps MB", "issued MB", "issued rate", "hot rows", "max |own - grid_sample|"))
    for name, c, h, w, t_bwd, nominal, issued, dev, hot_share, hottest in rows:
        t = statistics.median(t_bwd) * 1e-3
        log("%-8s %-28s %-10.1f %-10.1f %-25s %-14s %.2e" % (
            name, fmt(t_bwd), nominal / 1e6, issued / 1e6, "%.3f TB/s (%.2f of 1.3)" % (issued / t / 1e12, issued / t / ATOMIC_RATE),
            "%.2f / %d" % (hot_share, hottest), dev))
    nominal, issued = sum(r[5] for r in rows), sum(r[6] for r in rows)
    log("one sample-forward: %.3f GB of taps, %.3f GB issued: the run merge removes %.1f %%" % (nominal / 1e9, issued / 1e9, 100.0 * (1 - issued / nominal)))
    return statistics.median(own_sum), statistics.median(ref_sum), max(own_sum) - min(own_sum), max(ref_sum) - min(ref_sum)


def step_child(reps, contiguous):
    """One stage-1 training step, timed; prints one JSON line."""
    from streammos_amd import ops, synth
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    model = StreamMOS.AttNet(cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(DEV).train()
    torch.manual_seed(0)      # the same dropout masks in every child: the losses are comparable
    gen = torch.Generator(device="cpu").manual_seed(5)
    batch = {}
    for i, s in enumerate(samples(3)):
        for k in ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord"):
            batch["%s_%d" % (k, i)] = torch.from_numpy(s[k]).to(DEV)
        bsz = s["pcds_xyzi"].shape[0]
        batch["pcds_target_%d" % i] = torch.randint(0, 3, (bsz, N_POINTS, 1), generator=gen).to(DEV)
        batch["pcds_bev_target_%d" % i] = torch.randint(0, 3, (bsz, 256, 256, 1), generator=gen).to(DEV)
    calls = {"bwd": 0}
    inner = ops.bilinear_gather_backward

    def counted(*a, **k):
        calls["bwd"] += 1
        return inner(*a, **k)
    ops.bilinear_gather_backward = counted
    if contiguous:      # the variant with one more pass: the node hands on an NCHW-contiguous copy
        ops._BilinearGather.backward = staticmethod(lambda ctx, g: (ops.bilinear_gather_backward(
            g, ctx.saved_tensors[0], ctx.scale, ctx.grid_shape, channels_last=True).contiguous(), None, None, None, None))

    def step():
        model.zero_grad(set_to_none=True)
        loss = model(batch)
        loss.backward()
        return loss
    loss = step()
    per_step = calls["bwd"]
    ms = measure(step, reps, iters=1, warm=2)
    print(json.dumps({"switch": int(ops.bilinear_bwd_own()), "contiguous": bool(contiguous), "ms": ms, "loss": float(loss.item()),
                      "own_backward_calls_per_step": per_step, "peak_gb": torch.cuda.max_memory_allocated() / 2 ** 30}), flush=True)


def steps(reps, log):
    log("")
    log("stage-1 training step (AttNet.forward on three chained samples + backward, train mode, B = 4, N = %d), %d steps after 2 warm-ups," % (N_POINTS, reps))
    log("each setting in a fresh process: median (min..max)")
    res = {}
    for label, switch, nchw in (("SMOS_BILINEAR_BWD=1 (gradient channels-last-strided)", "1", False),
                                ("SMOS_BILINEAR_BWD=1, gradient made NCHW-contiguous", "1", True),
                                ("SMOS_BILINEAR_BWD=0 (F.grid_sample)", "0", False)):
        env = dict(os.environ, SMOS_BILINEAR_BWD=switch)
        cmd = [sys.executable, os.path.abspath(__file__), "--step-child", "--reps", str(reps)] + (["--contiguous"] if nchw else [])
        proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        if proc.returncode != 0:
            log("%-52s FAILED (exit %d): %s" % (label, proc.returncode, proc.stderr.strip().splitlines()[-1:] or ""))
            raise SystemExit(proc.returncode)
        r = json.loads(proc.stdout.strip().splitlines()[-1])
        res[label] = r
        log("%-52s %s   loss %.5f, own backward launches per step %d, peak %.1f GiB" % (
            label, fmt(r["ms"]), r["loss"], r["own_backward_calls_per_step"], r["peak_gb"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_bilinear.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-child", action="store_true")
    ap.add_argument("--contiguous", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    if args.step_child:
        return step_child(args.reps, args.contiguous)
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_bilinear.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    call_sites(args.reps, log)
    torch.cuda.empty_cache()
    if not args.no_steps:
        steps(args.reps, log)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

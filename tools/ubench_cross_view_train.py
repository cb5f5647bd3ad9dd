"""Dev: the training form of the cross-view transfers (ops.gather_scatter_train, csrc/gather_scatter_train.hip) against the
module formulation it replaces -- BilinearSample followed by VoxelMaxPool and their backward -- per transfer, per stage-1
training step and per stage-2 step.

  python tools/ubench_cross_view_train.py [--out profiles/ubench_cross_view_train.txt] [--reps 5] [--parent DIR]

Per transfer (the four of CENet_Transformer._cross_view at B = 4, N = 130000 on the coordinates of a synthetic sample, a
post-ReLU standard-normal source map and a standard-normal incoming gradient; HIP events around 5 back-to-back calls after
a warm-up, `reps` such measurements, median and min..max) in two forms -- forward + backward, forward under no_grad -- the
module formulation and the op, EACH IN A FRESH PROCESS (--site-child), the two paths run twice in alternation so that the
run-to-run spread shows; with the kernel launches of one call counted by the profiler, max_memory_allocated over the calls
and the memory still held between forward and backward (what the autograd graph keeps; the output excluded).
Per step: the stage-1 step of tools/ubench_bilinear.py (AttNet.forward on three chained samples + backward), timed by that
tool's own child, with SMOS_CROSS_VIEW_TRAIN=0 and =1, each in a fresh process; with --parent DIR also the checkout of the
parent commit in DIR.  Stage 2: bench.py --full --train-steps 3 with the switch at 0 and at 1 (--only-stage2: these alone).
A difference counts only where it exceeds twice the larger min..max spread; the tool says which it is.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from tools.ubench_bilinear import fmt, measure, samples
from tools.ubench_seg_loss import launches, run_child

DEV = "cuda:0"
SWITCH = "SMOS_CROSS_VIEW_TRAIN"
# name, C, source (H, W), gather coordinates, target (H, W), scatter coordinates, scale of both, point values handed on
SITES = (("x0 bev->rv", 32, (256, 256), "bev", (32, 1024), "rv", (0.5, 0.5), False),
         ("x0 rv->bev", 32, (32, 1024), "rv", (256, 256), "bev", (0.5, 0.5), False),
         ("x1 bev->rv", 64, (128, 128), "bev", (16, 512), "rv", (0.25, 0.25), False),
         ("x1 rv->bev", 64, (16, 512), "rv", (128, 128), "bev", (0.25, 0.25), True))
FORMS = ("all", "forward")


def site_child(site, fused, form, reps):
    """One transfer on one path in one form; prints one JSON line."""
    from streammos_amd import ops
    from streammos_amd.refapi import deep_point
    from streammos_amd.refapi.networks import backbone
    name, c, (hg, wg), gwhich, size, swhich, scale, want_points = SITES[site]
    s = samples(1)[0]
    coords = {"bev": torch.from_numpy(s["pcds_coord"]).to(DEV)[:, 0, :, :2].contiguous(),       # (B, N, 2, 1)
              "rv": torch.from_numpy(s["pcds_sphere_coord"]).to(DEV)[:, 0].contiguous()}
    gcoord, scoord = coords[gwhich], coords[swhich]
    b, n = gcoord.shape[:2]
    torch.manual_seed(3)
    grid = torch.randn(b, c, hg, wg, device=DEV).relu_().requires_grad_(form == "all")
    g_out = torch.randn((b, c) + size, device=DEV)
    g_pts = torch.randn(b, c, n, device=DEV)
    sampler = backbone.BilinearSample(c, scale)
    held = {}

    def forward():
        if fused:
            res = ops.gather_scatter_train(grid, gcoord, scale, scoord, size, scale, want_points=want_points)
            return res if want_points else (res, None)
        pts = sampler(grid, gcoord)
        return deep_point.VoxelMaxPool(pts, scoord, size, scale), (pts[..., 0] if want_points else None)

    def call():
        grid.grad = None
        base = torch.cuda.memory_allocated()
        if form == "forward":
            with torch.no_grad():
                forward()
            held["graph_mb"] = 0.0
            return
        out, pts = forward()
        kept = out.numel() + (pts.numel() if pts is not None else 0)
        held["graph_mb"] = (torch.cuda.memory_allocated() - base - kept * 4) / 2 ** 20
        torch.autograd.backward([out] + ([pts] if pts is not None else []), [g_out] + ([g_pts] if pts is not None else []))
    call()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = measure(call, reps, iters=5, warm=2)
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({"fused": int(fused), "form": form, "ms": ms, "launches": launches(call), "peak_mb": peak / 2 ** 20,
                      "graph_mb": held["graph_mb"], "b": b, "n": n}), flush=True)


PATHS = (("module formulation", 0), ("ops.gather_scatter_train", 1))


def verdict(op, mod):
    """(ratio of the medians of the medians, difference, larger min..max spread, whether the difference exceeds twice it)"""
    op_all, mod_all = [m for r in op for m in r["ms"]], [m for r in mod for m in r["ms"]]
    op_med = statistics.median([statistics.median(r["ms"]) for r in op])
    mod_med = statistics.median([statistics.median(r["ms"]) for r in mod])
    spread = max(max(op_all) - min(op_all), max(mod_all) - min(mod_all))
    return op_med, mod_med, spread, abs(op_med - mod_med) > 2 * spread


def call_sites(reps, log):
    log("the four transfers of _cross_view, B = 4, N = 130000, each line a fresh process: median (min..max) of %d x 5 calls" % reps)
    for i, site in enumerate(SITES):
        for form in FORMS:
            log("")
            log("%s, C = %d, %dx%d -> %dx%d%s: %s" % (site[0], site[1], site[2][0], site[2][1], site[4][0], site[4][1],
                                                    ", point values handed on" if site[7] else "",
                                                    {"all": "forward + backward", "forward": "forward under no_grad"}[form]))
            log("%-28s %-30s %-10s %-26s %s" % ("path", "time", "launches", "peak above the inputs", "held between forward and backward (results excluded)"))
            res = {}
            for label, fused in PATHS * 2:
                cmd = [sys.executable, os.path.abspath(__file__), "--site-child", str(i), "--fused", str(fused), "--form", form, "--reps", str(reps)]
                r = run_child(label, cmd, dict(os.environ), ROOT, log, lambda r: r)
                res.setdefault(label, []).append(r)
                log("%-28s %-30s %-10s %-26s %.1f MB" % (label, fmt(r["ms"]), r["launches"] if r["launches"] else "not measured",
                                                        "%.1f MB" % r["peak_mb"], r["graph_mb"]))
            op_med, mod_med, spread, shown = verdict(res[PATHS[1][0]], res[PATHS[0][0]])
            log("op / module: %.3f (medians of the medians: %.3f vs %.3f ms); difference %.3f ms, larger min-max spread %.3f ms: %s"
                % (op_med / mod_med, op_med, mod_med, op_med - mod_med, spread, "difference shown" if shown else "no difference shown"))


def steps(reps, parent, log, stage1=True, stage2=True):
    if stage1:
        log("")
        log("stage-1 training step (tools/ubench_bilinear.py --step-child: AttNet.forward on three chained samples + backward, train mode,")
        log("B = 4, N = 130000), %d steps after 2 warm-ups, each setting in a fresh process: median (min..max)" % reps)
        runs = [("%s=0 (module path)" % SWITCH, "0", ROOT), ("%s=1 (ops.gather_scatter_train)" % SWITCH, "1", ROOT)]
        if parent:
            runs.append(("parent commit", None, os.path.abspath(parent)))
        runs = runs + runs[:2]            # the two settings once more, after the others: the run-to-run spread
        res = {}
        for label, switch, root in runs:
            env = dict(os.environ)
            env.pop(SWITCH, None)
            if switch is not None:
                env[SWITCH] = switch
            cmd = [sys.executable, os.path.join(root, "tools", "ubench_bilinear.py"), "--step-child", "--reps", str(reps)]
            r = run_child(label, cmd, env, root, log, lambda r: r)
            res.setdefault(label, []).append(r)
            log("%-50s %s   loss %.5f, peak %.1f GiB" % (label, fmt(r["ms"]), r["loss"], r["peak_gb"]))
        on_med, off_med, spread, shown = verdict(res[runs[1][0]], res[runs[0][0]])
        log("switch on / off: %.4f (%.3f vs %.3f ms); difference %.3f ms, larger min-max spread %.3f ms: %s"
            % (on_med / off_med, on_med, off_med, on_med - off_med, spread, "difference shown" if shown else "no difference shown"))
    if stage2:
        log("")
        log("stage-2 training step (bench.py --gpus 1 --steps 2 --warmup 1 --no-raw --full --cpu-scans 0 --train-steps 3): its stage2_training entry")
        for label, switch in (("%s=0" % SWITCH, "0"), ("%s=1" % SWITCH, "1")) * 2:
            env = dict(os.environ)
            env[SWITCH] = switch
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-raw", "--full", "--cpu-scans", "0",
                   "--train-steps", "3"]
            r = run_child(label, cmd, env, ROOT, log, lambda r: r.get("stage2_training"))
            log("%-50s %s" % (label, json.dumps({k: r.get(k) for k in ("ms_per_step", "value", "loss", "hbm_allocated_gb")})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_cross_view_train.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its stage-1 step is timed too")
    ap.add_argument("--site-child", type=int, default=None, help="internal: one transfer of the per-call measurement (index into SITES)")
    ap.add_argument("--fused", type=int, default=0, help="internal: the path a --site-child runs (0 module formulation, 1 op)")
    ap.add_argument("--form", default="all", choices=FORMS, help="internal: the form a --site-child runs")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--only-steps", action="store_true")
    ap.add_argument("--only-stage2", action="store_true", help="the bench.py runs alone")
    ap.add_argument("--no-stage2", action="store_true", help="leave the bench.py runs out")
    args = ap.parse_args()
    if args.site_child is not None:
        return site_child(args.site_child, args.fused, args.form, args.reps)
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_cross_view_train.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if not (args.only_stage2 or args.only_steps):
        call_sites(args.reps, log)
    if not args.no_steps:
        steps(args.reps, args.parent, log, stage1=not args.only_stage2, stage2=not args.no_stage2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

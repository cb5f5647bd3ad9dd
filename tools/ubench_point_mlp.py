"""Dev: the fused training point MLP (ops.point_mlp_train, csrc/point_mlp_train.hip) against the module path of
PointNetStacker(7, 64, pre_bn=True, stack_num=2), per call, per stage-1 training step and per stage-2 step.

  python tools/ubench_point_mlp.py [--out profiles/ubench_point_mlp.txt] [--reps 5] [--parent DIR]

Per call (forward + backward of point_pre on (12, 7, 130 000, 1), train mode, a standard-normal incoming gradient; HIP events
around `iters` back-to-back pairs after a warm-up, `reps` such measurements, median and min..max): the module path and the
op, EACH IN A FRESH PROCESS (--site-child), the settings run twice in alternation so that the run-to-run spread shows; with
the kernel launches of one pair counted by the profiler, max_memory_allocated over the pairs and the memory still held
between forward and backward (what the autograd graph keeps).
Per step: the stage-1 step of tools/ubench_bilinear.py (AttNet.forward on three chained samples + backward), timed by that
tool's own child, with SMOS_POINT_MLP=0 and =1, each in a fresh process; with --parent DIR also the checkout of the parent
commit in DIR.  Stage 2: bench.py --full --train-steps 3 with the switch at 0 and at 1 (--only-stage2: these runs alone).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from tools.ubench_bilinear import fmt, measure
from tools.ubench_seg_loss import launches, run_child

DEV = "cuda:0"
S, N = 12, 130000


def site_child(fused, reps):
    """Forward + backward of point_pre at the training shape on one path; prints one JSON line."""
    from streammos_amd import ops
    from streammos_amd.refapi.networks.backbone import PointNetStacker
    ops.set_point_mlp_fused(bool(fused))
    torch.manual_seed(3)
    m = PointNetStacker(7, 64, pre_bn=True, stack_num=2).to(DEV).train()
    x = torch.randn(S, 7, N, 1, device=DEV)
    x[:, 0:2] *= 20.0
    g = torch.randn(S, 64, N, 1, device=DEV)
    held = {}

    def pair():
        m.zero_grad(set_to_none=True)
        base = torch.cuda.memory_allocated()
        y = m(x)
        held["graph_mb"] = (torch.cuda.memory_allocated() - base - y.numel() * 4) / 2 ** 20
        y.backward(g)
    pair()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = measure(pair, reps, iters=5, warm=2)
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({"fused": int(fused), "ms": ms, "launches": launches(pair), "peak_mb": peak / 2 ** 20,
                      "graph_mb": held["graph_mb"]}), flush=True)


def call_sites(reps, log):
    log("point_pre forward + backward, (%d, 7, %d, 1) -> (%d, 64, %d, 1), train mode, each line a fresh process: median (min..max) of %d x 5 pairs" % (S, N, S, N, reps))
    log("%-34s %-30s %-10s %-26s %s" % ("path", "forward + backward", "launches", "peak above the inputs", "held between forward and backward (y excluded)"))
    med = {}
    for label, fused in (("module path (SMOS_POINT_MLP=0)", 0), ("ops.point_mlp_train (=1)", 1)) * 2:
        cmd = [sys.executable, os.path.abspath(__file__), "--site-child", str(fused), "--reps", str(reps)]
        r = run_child(label, cmd, dict(os.environ), ROOT, log, lambda r: r)
        med.setdefault(fused, []).append(statistics.median(r["ms"]))
        log("%-34s %-30s %-10s %-26s %.1f MB" % (label, fmt(r["ms"]), r["launches"] if r["launches"] else "not measured",
                                                "%.1f MB" % r["peak_mb"], r["graph_mb"]))
    log("op / module path: %.3f (medians of the medians)" % (statistics.median(med[1]) / statistics.median(med[0])))


def steps(reps, parent, log, stage1=True):
    if stage1:
        log("")
        log("stage-1 training step (tools/ubench_bilinear.py --step-child: AttNet.forward on three chained samples + backward, train mode,")
        log("B = 4, N = 130000), %d steps after 2 warm-ups, each setting in a fresh process: median (min..max)" % reps)
        runs = [("SMOS_POINT_MLP=0 (module path)", "0", ROOT), ("SMOS_POINT_MLP=1 (ops.point_mlp_train)", "1", ROOT)]
        if parent:
            runs.append(("parent commit", None, os.path.abspath(parent)))
        runs = runs + runs[:2]            # the two settings once more, after the others: the run-to-run spread
        for label, switch, root in runs:
            env = dict(os.environ)
            env.pop("SMOS_POINT_MLP", None)
            if switch is not None:
                env["SMOS_POINT_MLP"] = switch
            cmd = [sys.executable, os.path.join(root, "tools", "ubench_bilinear.py"), "--step-child", "--reps", str(reps)]
            r = run_child(label, cmd, env, root, log, lambda r: r)
            log("%-44s %s   loss %.5f, peak %.1f GiB" % (label, fmt(r["ms"]), r["loss"], r["peak_gb"]))
    log("")
    log("stage-2 training step (bench.py --gpus 1 --steps 2 --warmup 1 --no-raw --full --cpu-scans 0 --train-steps 3): its stage2_training entry")
    for label, switch in (("SMOS_POINT_MLP=0", "0"), ("SMOS_POINT_MLP=1", "1")):
        env = dict(os.environ, SMOS_POINT_MLP=switch)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-raw", "--full", "--cpu-scans", "0",
               "--train-steps", "3"]
        r = run_child(label, cmd, env, ROOT, log, lambda r: r.get("stage2_training"))
        log("%-44s %s" % (label, json.dumps(r)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_point_mlp.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its stage-1 step is timed too")
    ap.add_argument("--site-child", type=int, default=None, help="internal: one path of the per-call measurement (0 module path, 1 op)")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--only-steps", action="store_true")
    ap.add_argument("--only-stage2", action="store_true", help="the bench.py runs alone")
    args = ap.parse_args()
    if args.site_child is not None:
        return site_child(args.site_child, args.reps)
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_point_mlp.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if not (args.only_stage2 or args.only_steps):
        call_sites(args.reps, log)
    if not args.no_steps:
        steps(args.reps, args.parent, log, stage1=not args.only_stage2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

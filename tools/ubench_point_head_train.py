"""Dev: the fused training point head (ops.point_head_train, csrc/point_head_train.hip) against the module path of
CatFusion((64, 64, 64), 64) + PredBranch(64, 3), per call, per stage-1 training step and per stage-2 step.

  python tools/ubench_point_head_train.py [--out profiles/ubench_point_head_train.txt] [--reps 5] [--parent DIR]

Per call (the head on three (4, 64, 130 000, 1) inputs, train mode, a standard-normal incoming gradient; HIP events around
`iters` back-to-back calls after a warm-up, `reps` such measurements, median and min..max) in three forms -- stage-1 (inputs
and parameters need gradients), stage-2 (parameters only), forward only -- the module path and the op, EACH IN A FRESH
PROCESS (--site-child), the settings run twice in alternation so that the run-to-run spread shows; with the kernel launches of
one call counted by the profiler, max_memory_allocated over the calls and the memory still held between forward and
backward (what the autograd graph keeps; the logits excluded).
Per step: the stage-1 step of tools/ubench_bilinear.py (AttNet.forward on three chained samples + backward), timed by that
tool's own child, with SMOS_POINT_HEAD_TRAIN=0 and =1, each in a fresh process; with --parent DIR also the checkout of the
parent commit in DIR.  Stage 2: bench.py --full --train-steps 3 with the switch at 0 and at 1 (--only-stage2: these alone).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from tools.ubench_bilinear import fmt, measure
from tools.ubench_seg_loss import launches, run_child

DEV = "cuda:0"
B, N = 4, 130000
FORMS = ("stage1", "stage2", "forward")
SWITCH = "SMOS_POINT_HEAD_TRAIN"


def site_child(fused, form, reps):
    """The head at the training shape on one path in one form; prints one JSON line."""
    from streammos_amd import ops
    from streammos_amd.refapi.networks import backbone
    ops.set_point_head_fused(bool(fused))
    torch.manual_seed(3)
    fusion = backbone.CatFusion((64, 64, 64), 64).to(DEV).train()
    pred = backbone.PredBranch(64, 3).to(DEV).train()
    xs = [torch.randn(B, 64, N, 1, device=DEV).abs_().requires_grad_(form == "stage1") for _ in range(3)]
    g = torch.randn(B, 3, N, 1, device=DEV)
    params = list(fusion.parameters()) + list(pred.parameters())
    held = {}

    def call():
        for t in params + xs:
            t.grad = None
        base = torch.cuda.memory_allocated()
        if form == "forward":
            with torch.no_grad():
                backbone.point_head(fusion, pred, *xs)
            held["graph_mb"] = 0.0
            return
        y = backbone.point_head(fusion, pred, *xs)
        held["graph_mb"] = (torch.cuda.memory_allocated() - base - y.numel() * 4) / 2 ** 20
        y.backward(g)
    call()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = measure(call, reps, iters=5, warm=2)
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({"fused": int(fused), "form": form, "ms": ms, "launches": launches(call), "peak_mb": peak / 2 ** 20,
                      "graph_mb": held["graph_mb"]}), flush=True)


def call_sites(reps, log):
    log("point head, 3 x (%d, 64, %d, 1) -> (%d, 3, %d, 1), train mode, each line a fresh process: median (min..max) of %d x 5 calls" % (B, N, B, N, reps))
    for form in FORMS:
        log("")
        log("%s form (%s)" % (form, {"stage1": "forward + backward, inputs and parameters need gradients",
                                    "stage2": "forward + backward, parameters only", "forward": "forward under no_grad"}[form]))
        log("%-40s %-30s %-10s %-26s %s" % ("path", "time", "launches", "peak above the inputs", "held between forward and backward (logits excluded)"))
        res = {}
        for label, fused in (("module path (%s=0)" % SWITCH, 0), ("ops.point_head_train (=1)", 1)) * 2:
            cmd = [sys.executable, os.path.abspath(__file__), "--site-child", str(fused), "--form", form, "--reps", str(reps)]
            r = run_child(label, cmd, dict(os.environ), ROOT, log, lambda r: r)
            res.setdefault(fused, []).append(r)
            log("%-40s %-30s %-10s %-26s %.1f MB" % (label, fmt(r["ms"]), r["launches"] if r["launches"] else "not measured",
                                                    "%.1f MB" % r["peak_mb"], r["graph_mb"]))
        op_med = statistics.median([statistics.median(r["ms"]) for r in res[1]])
        mod_med = statistics.median([statistics.median(r["ms"]) for r in res[0]])
        mod_min = min(min(r["ms"]) for r in res[0])
        log("op / module path: %.3f (medians of the medians); op median %.3f ms %s module-path minimum %.3f ms; held %.1f MB vs %.1f MB"
            % (op_med / mod_med, op_med, "below" if op_med < mod_min else "NOT below", mod_min, res[1][0]["graph_mb"], res[0][0]["graph_mb"]))


def steps(reps, parent, log, stage1=True, stage2=True):
    if stage1:
        log("")
        log("stage-1 training step (tools/ubench_bilinear.py --step-child: AttNet.forward on three chained samples + backward, train mode,")
        log("B = 4, N = 130000), %d steps after 2 warm-ups, each setting in a fresh process: median (min..max)" % reps)
        runs = [("%s=0 (module path)" % SWITCH, "0", ROOT), ("%s=1 (ops.point_head_train)" % SWITCH, "1", ROOT)]
        if parent:
            runs.append(("parent commit", None, os.path.abspath(parent)))
        runs = runs + runs[:2]            # the two settings once more, after the others: the run-to-run spread
        for label, switch, root in runs:
            env = dict(os.environ)
            env.pop(SWITCH, None)
            if switch is not None:
                env[SWITCH] = switch
            cmd = [sys.executable, os.path.join(root, "tools", "ubench_bilinear.py"), "--step-child", "--reps", str(reps)]
            r = run_child(label, cmd, env, root, log, lambda r: r)
            log("%-50s %s   loss %.5f, peak %.1f GiB" % (label, fmt(r["ms"]), r["loss"], r["peak_gb"]))
    if stage2:
        log("")
        log("stage-2 training step (bench.py --gpus 1 --steps 2 --warmup 1 --no-raw --full --cpu-scans 0 --train-steps 3): its stage2_training entry")
        for label, switch in (("%s=0" % SWITCH, "0"), ("%s=1" % SWITCH, "1")):
            env = dict(os.environ)
            env[SWITCH] = switch
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-raw", "--full", "--cpu-scans", "0",
                   "--train-steps", "3"]
            r = run_child(label, cmd, env, ROOT, log, lambda r: r.get("stage2_training"))
            log("%-50s %s" % (label, json.dumps(r)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_point_head_train.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its stage-1 step is timed too")
    ap.add_argument("--site-child", type=int, default=None, help="internal: one path of the per-call measurement (0 module path, 1 op)")
    ap.add_argument("--form", default="stage1", choices=FORMS, help="internal: the form a --site-child runs")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--only-steps", action="store_true")
    ap.add_argument("--only-stage2", action="store_true", help="the bench.py runs alone")
    ap.add_argument("--no-stage2", action="store_true", help="leave the bench.py runs out")
    args = ap.parse_args()
    if args.site_child is not None:
        return site_child(args.site_child, args.form, args.reps)
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_point_head_train.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if not (args.only_stage2 or args.only_steps):
        call_sites(args.reps, log)
    if not args.no_steps:
        steps(args.reps, args.parent, log, stage1=not args.only_stage2, stage2=not args.no_stage2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Dev: the training form of the decoder's conv_1 (ops.upconv3x3_train, csrc/upconv_bwd.hip) against the module formulation
it replaces -- two F.interpolate(align_corners=True) + cat + conv2d 320 -> 128 and their backward -- per call, per stage-1
training step and per stage-2 step.

  python tools/ubench_conv1_train.py [--out profiles/ubench_conv1_train.txt] [--reps 5] [--parent DIR]

Per call (B = 4, x0 64 x 256^2, x1 128 x 128^2, x2 128 x 64^2, a standard-normal incoming gradient; HIP events around 5
back-to-back calls after a warm-up, `reps` such measurements, median and min..max) in three forms -- forward + backward with
all gradients, parameters only, forward only -- the module formulation, the op returning its channels-last map and the op
returning an NCHW copy (SMOS_CONV1_OUT=nchw), EACH IN A FRESH PROCESS (--site-child), the settings run twice in alternation
so that the run-to-run spread shows; with the kernel launches of one call counted by the profiler, max_memory_allocated over
the calls and the memory still held between forward and backward (what the autograd graph keeps; the output excluded).
Both paths include the x0 part (the op's caller computes it with F.conv2d on the 64-channel slice of the weights).
The two adjoint launches on their own (--adjoint-child): time, compulsory bytes (every operand once) and achieved TB/s.
Per step: the stage-1 step of tools/ubench_bilinear.py (AttNet.forward on three chained samples + backward), timed by that
tool's own child, with SMOS_CONV1_TRAIN=0 and =1, each in a fresh process; with --parent DIR also the checkout of the parent
commit in DIR.  Stage 2: bench.py --full --train-steps 3 with the switch at 0 and at 1 (--only-stage2: these alone).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

from tools.ubench_bilinear import fmt, measure
from tools.ubench_seg_loss import launches, run_child

DEV = "cuda:0"
B, C, HO = 4, 128, 256
SOURCES = ((128, 128), (64, 64))
FORMS = ("all", "params", "forward")
SWITCH = "SMOS_CONV1_TRAIN"


def site_child(fused, form, reps):
    """conv_1 at the training shape on one path in one form; prints one JSON line."""
    from streammos_amd import ops
    torch.manual_seed(3)
    w = (torch.randn(C, 320, 3, 3, device=DEV) * (2.0 / (9 * 320)) ** 0.5).requires_grad_(form != "forward")
    x0 = torch.randn(B, 64, HO, HO, device=DEV).requires_grad_(form == "all")
    xs = [torch.randn(B, 128, h, v, device=DEV).requires_grad_(form == "all") for h, v in SOURCES]
    g = torch.randn(B, C, HO, HO, device=DEV)
    leaves = [w, x0] + xs
    held = {}

    def forward():
        if fused:
            return ops.upconv3x3_train(F.conv2d(x0, w[:, :64], padding=1), [(xs[0], w[:, 64:192]), (xs[1], w[:, 192:320])])
        ups = [F.interpolate(t, size=(HO, HO), mode="bilinear", align_corners=True) for t in xs]
        return F.conv2d(torch.cat([x0] + ups, dim=1), w, padding=1)

    def call():
        for t in leaves:
            t.grad = None
        base = torch.cuda.memory_allocated()
        if form == "forward":
            with torch.no_grad():
                forward()
            held["graph_mb"] = 0.0
            return
        y = forward()
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


def adjoint_child(reps):
    """upconv_bwd_ypass and upconv_bwd_xpass alone at the training shape, per source; prints one JSON line."""
    from streammos_amd import _lib, ops
    g = ops.empty_cl(B, C, HO, HO, torch.device(DEV))
    g.normal_()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for hs, ws in SOURCES:
        s = torch.empty((B, 3, hs, HO, C), dtype=torch.float32, device=DEV)
        gz = torch.empty((B * hs * ws, 9 * C), dtype=torch.float32, device=DEV)
        y_ms = measure(lambda: _lib.call("smos_upconv_bwd_ypass", g.data_ptr(), C, s.data_ptr(), B, HO, HO, C, hs, 0, st), reps, iters=5, warm=2)
        x_ms = measure(lambda: _lib.call("smos_upconv_bwd_xpass", s.data_ptr(), gz.data_ptr(), 9 * C, B, hs, ws, C, HO, 0, st), reps, iters=5, warm=2)
        rows.append({"hs": hs, "ws": ws, "y_ms": y_ms, "x_ms": x_ms, "y_bytes": (g.numel() + s.numel()) * 4, "x_bytes": (s.numel() + gz.numel()) * 4,
                     "y_window": _lib.query("smos_upconv_bwd_window", hs, HO), "x_window": _lib.query("smos_upconv_bwd_window", ws, HO)})
    print(json.dumps({"rows": rows}), flush=True)


PATHS = (("module formulation", 0, None), ("ops.upconv3x3_train, channels-last out", 1, "cl"), ("ops.upconv3x3_train, NCHW copy out", 1, "nchw"))


def call_sites(reps, log):
    log("conv_1, B = %d, x0 64 x %d^2, x1 128 x 128^2, x2 128 x 64^2 -> 128 x %d^2, each line a fresh process: median (min..max) of %d x 5 calls"
        % (B, HO, HO, reps))
    for form in FORMS:
        log("")
        log("%s form (%s)" % (form, {"all": "forward + backward, inputs and weights need gradients", "params": "forward + backward, weights only",
                                    "forward": "forward under no_grad"}[form]))
        log("%-42s %-30s %-10s %-26s %s" % ("path", "time", "launches", "peak above the inputs", "held between forward and backward (output excluded)"))
        res = {}
        for label, fused, layout in PATHS * 2:
            env = dict(os.environ)
            env.pop("SMOS_CONV1_OUT", None)
            if layout:
                env["SMOS_CONV1_OUT"] = layout
            cmd = [sys.executable, os.path.abspath(__file__), "--site-child", str(fused), "--form", form, "--reps", str(reps)]
            r = run_child(label, cmd, env, ROOT, log, lambda r: r)
            res.setdefault(label, []).append(r)
            log("%-42s %-30s %-10s %-26s %.1f MB" % (label, fmt(r["ms"]), r["launches"] if r["launches"] else "not measured",
                                                    "%.1f MB" % r["peak_mb"], r["graph_mb"]))
        mod = res[PATHS[0][0]]
        mod_med, mod_all = statistics.median([statistics.median(r["ms"]) for r in mod]), [m for r in mod for m in r["ms"]]
        for label, _, _ in PATHS[1:]:
            op_all = [m for r in res[label] for m in r["ms"]]
            op_med = statistics.median([statistics.median(r["ms"]) for r in res[label]])
            spread = max(max(op_all) - min(op_all), max(mod_all) - min(mod_all))
            shown = abs(op_med - mod_med) >= 2 * spread
            log("%s / module: %.3f (medians of the medians: %.3f vs %.3f ms); difference %.3f ms, larger min-max spread %.3f ms: %s; held %.1f MB vs %.1f MB"
                % (label, op_med / mod_med, op_med, mod_med, op_med - mod_med, spread, "difference shown" if shown else "no difference shown",
                   res[label][0]["graph_mb"], mod[0]["graph_mb"]))


def adjoint(reps, log):
    log("")
    log("the adjoint launches alone (g %d x %d x %d^2 channels-last), a fresh process: median (min..max) of %d x 5 calls; bytes = every operand once"
        % (B, C, HO, reps))
    r = run_child("adjoint", [sys.executable, os.path.abspath(__file__), "--adjoint-child", "--reps", str(reps)], dict(os.environ), ROOT, log, lambda r: r)
    for row in r["rows"]:
        for key, name in (("y", "upconv_bwd_ypass"), ("x", "upconv_bwd_xpass")):
            ms = row[key + "_ms"]
            log("%-18s source %3d x %-3d window %2d  %-30s %7.1f MB  %.2f TB/s" % (name, row["hs"], row["ws"], row[key + "_window"], fmt(ms),
                                                                                  row[key + "_bytes"] / 1e6, row[key + "_bytes"] / statistics.median(ms) / 1e9))


def steps(reps, parent, log, stage1=True, stage2=True):
    if stage1:
        log("")
        log("stage-1 training step (tools/ubench_bilinear.py --step-child: AttNet.forward on three chained samples + backward, train mode,")
        log("B = 4, N = 130000), %d steps after 2 warm-ups, each setting in a fresh process: median (min..max)" % reps)
        runs = [("%s=0 (module path)" % SWITCH, "0", ROOT), ("%s=1 (ops.upconv3x3_train)" % SWITCH, "1", ROOT)]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_conv1_train.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its stage-1 step is timed too")
    ap.add_argument("--site-child", type=int, default=None, help="internal: one path of the per-call measurement (0 module formulation, 1 op)")
    ap.add_argument("--adjoint-child", action="store_true", help="internal: the two adjoint launches alone")
    ap.add_argument("--form", default="all", choices=FORMS, help="internal: the form a --site-child runs")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--only-steps", action="store_true")
    ap.add_argument("--only-stage2", action="store_true", help="the bench.py runs alone")
    ap.add_argument("--no-stage2", action="store_true", help="leave the bench.py runs out")
    args = ap.parse_args()
    if args.site_child is not None:
        return site_child(args.site_child, args.form, args.reps)
    if args.adjoint_child:
        return adjoint_child(args.reps)
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_conv1_train.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if not (args.only_stage2 or args.only_steps):
        call_sites(args.reps, log)
        adjoint(args.reps, log)
    if not args.no_steps:
        steps(args.reps, args.parent, log, stage1=not args.only_stage2, stage2=not args.no_stage2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

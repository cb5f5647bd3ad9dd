"""Dev: the fused training loss (ops.seg_loss, csrc/seg_loss.hip) against the torch formulation of refapi/models/losses.py,
per call site of one training sample-forward, per stage-1 training step and per stage-2 step.

  python tools/ubench_seg_loss.py [--out profiles/ubench_seg_loss.txt] [--reps 5] [--parent DIR]

Per call site (AttNet._seg_loss forward + backward at the two shapes a sample-forward calls it with: the point head's
B = 4 x P = 130 000 view of a [B, P, C] buffer and a BEV auxiliary head's B = 4 x 256^2 map; HIP events around `iters`
back-to-back pairs after a warm-up, `reps` such measurements, median and min..max): the own path against the torch path
in the same process, the kernel launches of one pair counted by the profiler, and the bytes one pair has to move at the
least (logits and labels once per direction, keys and payloads read and written once per radix pass, the coefficient table
written once and read once) with the rate that figure gives over the measured time.
Per step: the stage-1 step of tools/ubench_bilinear.py (AttNet.forward on three chained samples + backward), timed by that
tool's own child, with SMOS_SEG_LOSS=1 and =0, each in a fresh process; with --parent DIR also the checkout of the parent
commit in DIR.  Stage 2: bench.py --full --train-steps 3 with the switch at 1 and at 0 (--only-stage2: these runs alone).
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

DEV = "cuda:0"
# name, B, P, layout
SITES = (("point head", 4, 130000, "point_major"), ("BEV aux head", 4, 256 * 256, "contiguous"))
C = 3
KEY_BITS, RADIX_BITS = 33, 8          # csrc/seg_loss.hip sorts bits [0, 33); the library's passes take up to 8 bits each


def launches(fn):
    """Kernel launches of one call of fn, from the profiler's device activities (None where it records none)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def call_sites(reps, log):
    from streammos_amd import engine
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS

    def model(own):
        m = StreamMOS.AttNet.__new__(StreamMOS.AttNet)       # _seg_loss needs the config and the switch, not the network
        engine.read_switches(m, engine.TRAIN_SWITCHES)
        m.pModel = cfg.get_config()[2]
        m.seg_loss_own = own
        return m
    own_m, torch_m = model(True), model(False)
    log("call sites: AttNet._seg_loss forward + backward, C = %d, labels uniform over {0, 1, 2} (0 ignored), median (min..max) of %d x 10 pairs" % (C, reps))
    log("%-14s %-12s %-30s %-30s %-12s %s" % ("site", "B x P", "own (SMOS_SEG_LOSS=1)", "torch (SMOS_SEG_LOSS=0)", "own / torch", "launches own / torch"))
    gen = torch.Generator(device="cpu").manual_seed(11)
    rows = []
    for name, b, p, layout in SITES:
        logits = torch.randn((b, C, p), generator=gen)
        if layout == "point_major":
            pred = logits.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1).unsqueeze(-1)
        else:
            pred = logits.to(DEV).unsqueeze(-1)
        pred.requires_grad_()
        target = torch.randint(0, 3, (b, p, 1), generator=gen).to(DEV)

        def pair(m):
            def fn():
                pred.grad = None
                m._seg_loss(pred, target).backward()
            return fn
        own, ref = pair(own_m), pair(torch_m)
        own()
        g_own = pred.grad.clone()
        ref()
        dev = (g_own - pred.grad).abs().max().item() / pred.grad.abs().max().item()
        t_own, t_ref = measure(own, reps), measure(ref, reps)
        n_own, n_ref = launches(own), launches(ref)
        n = b * p
        passes = -(-KEY_BITS // RADIX_BITS)
        least = 2 * (n * C * 4 + n * 8) + n * C * 4 + passes * 2 * (C + 1) * n * 12 + 2 * (C + 1) * n * 4
        rows.append((name, least, statistics.median(t_own), statistics.median(t_ref), dev))
        log("%-14s %-12s %-30s %-30s %-12.3f %s / %s" % (name, "%d x %d" % (b, p), fmt(t_own), fmt(t_ref),
                                                       statistics.median(t_own) / statistics.median(t_ref),
                                                       n_own if n_own else "not measured", n_ref if n_ref else "not measured"))
    log("")
    log("least bytes of one own pair: logits + labels per direction, the gradient, (keys + payloads) x 2 x %d radix passes of %d bits, coef written + read"
        % (-(-KEY_BITS // RADIX_BITS), RADIX_BITS))
    for name, least, t, _, dev in rows:
        log("%-14s %8.1f MB  -> %.3f TB/s over the measured pair; max |own - torch gradient| / largest element %.2e" % (
            name, least / 1e6, least / (t * 1e-3) / 1e12, dev))
    own_ms, torch_ms = rows[0][2] + 3 * rows[1][2], rows[0][3] + 3 * rows[1][3]
    log("one sample-forward (point head + 3 aux heads): own %.3f ms, torch %.3f ms; a stage-1 step makes three: %.3f ms against %.3f ms"
        % (own_ms, torch_ms, 3 * own_ms, 3 * torch_ms))


def run_child(label, cmd, env, cwd, log, parse):
    proc = subprocess.run(cmd, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if proc.returncode != 0:
        log("%-44s FAILED (exit %d): %s" % (label, proc.returncode, proc.stderr.strip().splitlines()[-1:] or ""))
        raise SystemExit(proc.returncode)
    return parse(json.loads([l for l in proc.stdout.splitlines() if l.startswith("{")][-1]))


def steps(reps, parent, log, stage1=True):
    if not stage1:
        return stage2(log)
    log("")
    log("stage-1 training step (tools/ubench_bilinear.py --step-child: AttNet.forward on three chained samples + backward, train mode,")
    log("B = 4, N = 130000), %d steps after 2 warm-ups, each setting in a fresh process: median (min..max)" % reps)
    runs = [("SMOS_SEG_LOSS=1 (own loss kernels)", "1", ROOT), ("SMOS_SEG_LOSS=0 (torch formulation)", "0", ROOT)]
    if parent:
        runs.append(("parent commit", None, os.path.abspath(parent)))
    runs = runs + runs[:2]            # the two settings once more, after the others: the run-to-run spread
    for label, switch, root in runs:
        env = dict(os.environ)
        env.pop("SMOS_SEG_LOSS", None)
        if switch is not None:
            env["SMOS_SEG_LOSS"] = switch
        cmd = [sys.executable, os.path.join(root, "tools", "ubench_bilinear.py"), "--step-child", "--reps", str(reps)]
        r = run_child(label, cmd, env, root, log, lambda r: r)
        log("%-44s %s   loss %.5f, peak %.1f GiB" % (label, fmt(r["ms"]), r["loss"], r["peak_gb"]))
    stage2(log)


def stage2(log):
    log("")
    log("stage-2 training step (bench.py --gpus 1 --steps 2 --warmup 1 --no-raw --full --cpu-scans 0 --train-steps 3): its stage2_training entry")
    for label, switch in (("SMOS_SEG_LOSS=1", "1"), ("SMOS_SEG_LOSS=0", "0")):
        env = dict(os.environ, SMOS_SEG_LOSS=switch)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-raw", "--full", "--cpu-scans", "0",
               "--train-steps", "3"]
        r = run_child(label, cmd, env, ROOT, log, lambda r: r.get("stage2_training"))
        log("%-44s %s" % (label, json.dumps(r)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_seg_loss.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its stage-1 step is timed too")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--only-stage2", action="store_true", help="the bench.py runs alone")
    args = ap.parse_args()
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_seg_loss.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if not args.only_stage2:
        call_sites(args.reps, log)
        torch.cuda.empty_cache()
    if not args.no_steps:
        steps(args.reps, args.parent, log, stage1=not args.only_stage2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

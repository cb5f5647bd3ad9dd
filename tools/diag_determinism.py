"""Dev: which parameter gradients of a stage-1 training step are reproducible bit for bit.

  python tools/diag_determinism.py [--out profiles/determinism_step.txt] [--points 16384] [--beams 32] [--azimuth 400]

One stage-1 step (AttNet.forward on three chained samples + backward, train mode, batch 4) is run twice from the same seed
in one process, on small synthetic scans (32 beams x 400 columns padded to N = 16384), with ops.set_deterministic(False)
and (True).  Per parameter: whether the two gradients are bit-equal, and
their largest difference.  torch.use_deterministic_algorithms is NOT set (torch's interpolate backward would raise): the
backward kernels of MIOpen and torch are outside the setting, and this report is the map of what is still order-dependent
with the project's own operators fixed.  A report, not a test.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

DEV = "cuda:0"


def build(points, beams, azimuth):
    from streammos_amd import preprocess, synth
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    model = StreamMOS.AttNet(cfg.get_config()[2])
    model.load_state_dict(synth.seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(DEV).train()
    spec = preprocess.VoxelSpec()
    scans = [synth.synthetic_scan(k, beams, azimuth) for k in range(5)]
    poses = [synth.synthetic_pose(k) for k in range(5)]
    gen = torch.Generator(device="cpu").manual_seed(5)
    batch = {}
    for i in range(3):
        idx = preprocess.window_indices(i, 5, 3)
        s = preprocess.build_sample([scans[j] for j in idx], [poses[j] for j in idx], points, spec, tta=True)
        for k in ("pcds_xyzi", "pcds_coord", "pcds_sphere_coord"):
            batch["%s_%d" % (k, i)] = torch.from_numpy(s[k]).to(DEV)
        bsz = s["pcds_xyzi"].shape[0]
        batch["pcds_target_%d" % i] = torch.randint(0, 3, (bsz, points, 1), generator=gen).to(DEV)
        batch["pcds_bev_target_%d" % i] = torch.randint(0, 3, (bsz, 256, 256, 1), generator=gen).to(DEV)
    return model, batch


def step(model, batch):
    torch.manual_seed(0)                       # the same dropout masks in every run
    model.zero_grad(set_to_none=True)
    loss = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.item()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "determinism_step.txt"))
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--beams", type=int, default=32)
    ap.add_argument("--azimuth", type=int, default=400)
    args = ap.parse_args()
    from streammos_amd import ops
    model, batch = build(args.points, args.beams, args.azimuth)
    step(model, batch)                         # warm-up: MIOpen picks its kernels
    lines = ["tools/diag_determinism.py on %s, torch %s: one stage-1 training step twice from the same seed, B = 4, N = %d (%d x %d scans)"
             % (torch.cuda.get_device_name(0), torch.__version__, args.points, args.beams, args.azimuth),
             "torch.use_deterministic_algorithms is not set; per parameter: bit-equal or not, the largest |difference| and it relative to the largest |gradient|", ""]
    table = {}
    for flag in (False, True):
        ops.set_deterministic(flag)
        (la, ga), (lb, gb) = step(model, batch), step(model, batch)
        rows = []
        for name in ga:
            same = torch.equal(ga[name].view(torch.int32), gb[name].view(torch.int32))
            diff = (ga[name] - gb[name]).abs().max().item()
            rows.append((name, same, diff, diff / max(ga[name].abs().max().item(), 1e-30)))
        table[flag] = rows
        equal = sum(1 for r in rows if r[1])
        lines.append("ops.set_deterministic(%s): loss %.9g / %.9g, %d of %d parameter gradients bit-equal, largest relative difference %.3e"
                     % (flag, la, lb, equal, len(rows), max(r[3] for r in rows)))
    ops.set_deterministic(None)
    lines += ["", "%-64s %-28s %s" % ("parameter", "setting off", "setting on")]
    for off, on in zip(table[False], table[True]):
        cell = lambda r: "equal" if r[1] else "differs %.3e (%.1e)" % (r[2], r[3])
        lines.append("%-64s %-28s %s" % (off[0], cell(off), cell(on)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

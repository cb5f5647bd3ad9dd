"""Dev: the fixed-order backward sums (csrc/segsum.hip) against the atomic kernels, per call site and per training step.

  python tools/ubench_det_bwd.py [--out profiles/ubench_det_bwd.txt] [--reps 5] [--parent DIR] [--no-steps]

Method of tools/ubench_bilinear.py (whose sites, samples and timing loop are imported): HIP events around 10 back-to-back
calls after a warm-up, `reps` such measurements, median and min..max.
  - the five bilinear call sites of one sample-forward at B = 4, N = 130 000: forward + backward through the autograd node
    and the backward alone, ops.set_deterministic(False) against (True), in one process (the setting is read per call);
  - ops.msda_bwd at the network's shape (4 x 4096 queries, 4 heads of 32, one 64 x 64 level, 4 points);
  - the least bytes of the deterministic form -- emit (coordinates in; key, payload, weight out), the radix sort's passes
    (8-bit digits: one histogram read of the keys, then per pass keys and payloads in and out), the start search's output,
    the sum's index, weight and grad_out reads and its destination write -- and the rate that is of the measured time;
  - the stage-1 training step (tools/ubench_bilinear.py --step-child) with SMOS_DETERMINISTIC at 0 and at 1, each in a fresh
    process, and with --parent DIR the built checkout of the parent commit.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import ubench_bilinear as ub

DEV = ub.DEV
MSDA_SHAPE = dict(n=4, s=64 * 64, m=4, d=32, levels=((64, 64),), lq=64 * 64, p=4)


def least_bytes(pairs, rows, c, present, src_rows, coord_bytes, transposed):
    """Bytes the three steps cannot avoid, by step."""
    bits = max(1, int(rows).bit_length())
    passes = -(-bits // 8)
    emit = coord_bytes + pairs * 12
    sort = pairs * 4 + passes * pairs * 16
    copy = src_rows * c * 8 if transposed else 0
    summ = (rows + 1) * 4 + present * 8 + src_rows * c * 4 + rows * c * 4      # every grad_out row once: its four taps share it
    return emit, sort, copy, summ, passes


def bilinear_sites(reps, log):
    from oracle import ops_np
    from streammos_amd import ops
    s = ub.samples(1)[0]
    coords = {"bev": torch.from_numpy(s["pcds_coord"]).to(DEV)[:, 0, :, :2].contiguous(),
              "rv": torch.from_numpy(s["pcds_sphere_coord"]).to(DEV)[:, 0].contiguous()}
    b, n = coords["bev"].shape[:2]
    log("bilinear call sites: B = %d, N = %d, chunk L = %d; median (min..max) of %d x 10 calls" % (b, n, ops.segsum_chunk(), reps))
    log("%-8s %-12s %-30s %-30s %-30s %-30s %s" % ("site", "C x H x W", "fwd+bwd atomic", "fwd+bwd deterministic", "bwd atomic",
                                                   "bwd deterministic", "det / atomic (bwd)"))
    sums = {k: [0.0] * reps for k in ("fa", "fd", "ba", "bd")}
    rows = []
    for name, c, (h, w), scale, which in ub.SITES:
        coord = coords[which]
        grid = torch.randn((b, c, h, w), device=DEV, requires_grad=True)
        go = torch.randn((b, c, n, 1), device=DEV)
        c2 = coord[..., 0].contiguous()

        def both():
            out = ops.bilinear_gather(grid, coord, scale).unsqueeze(-1)
            return torch.autograd.grad(out, grid, go)[0]

        def bwd(det):
            return lambda: ops.bilinear_gather_backward(go[..., 0], c2, scale, (h, w), deterministic=det)
        t = {}
        for key, det in (("fa", False), ("fd", True)):
            ops.set_deterministic(det)
            t[key] = ub.measure(both, reps)
        ops.set_deterministic(None)
        t["ba"], t["bd"] = ub.measure(bwd(False), reps), ub.measure(bwd(True), reps)
        a, d1, d2 = bwd(False)(), bwd(True)(), bwd(True)()
        assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))
        dev = (a - d1).abs().max().item()
        for key in sums:
            sums[key] = [x + y for x, y in zip(sums[key], t[key])]
        iy, ix = ops_np.bilinear_pixel_coords(c2.cpu().numpy(), scale, h, w)
        fin = (iy > -2) & (iy < h + 1) & (ix > -2) & (ix < w + 1)
        y0, x0 = np.where(fin, np.floor(iy), -5), np.where(fin, np.floor(ix), -5)
        present = int(sum(((y0 + dy >= 0) & (y0 + dy < h) & (x0 + dx >= 0) & (x0 + dx < w)).sum() for dy in (0, 1) for dx in (0, 1)))
        rows.append((name, c, h, w, t["bd"], least_bytes(b * n * 4, b * h * w, c, present, b * n, b * n * c2.shape[2] * 4, True), present, dev))
        log("%-8s %-12s %-30s %-30s %-30s %-30s %.2f" % (name, "%dx%dx%d" % (c, h, w), ub.fmt(t["fa"]), ub.fmt(t["fd"]), ub.fmt(t["ba"]),
                                                        ub.fmt(t["bd"]), statistics.median(t["bd"]) / statistics.median(t["ba"])))
    log("%-8s %-12s %-30s %-30s %-30s %-30s %.2f" % ("sum", "", ub.fmt(sums["fa"]), ub.fmt(sums["fd"]), ub.fmt(sums["ba"]), ub.fmt(sums["bd"]),
                                                    statistics.median(sums["bd"]) / statistics.median(sums["ba"])))
    log("")
    log("deterministic backward alone: least bytes by step (grad_out channel-major, so one dense copy), and the rate they make of the time")
    log("%-8s %-10s %-9s %-9s %-9s %-9s %-9s %-12s %-14s %s" % ("site", "pairs in", "emit MB", "sort MB", "copy MB", "sum MB", "total MB",
                                                              "sort passes", "achieved", "max |det - atomic|"))
    for name, c, h, w, t_bd, (emit, sort, copy, summ, passes), present, dev in rows:
        total = emit + sort + copy + summ
        log("%-8s %-10d %-9.1f %-9.1f %-9.1f %-9.1f %-9.1f %-12d %-14s %.2e" % (
            name, present, emit / 1e6, sort / 1e6, copy / 1e6, summ / 1e6, total / 1e6, passes,
            "%.3f TB/s" % (total / (statistics.median(t_bd) * 1e-3) / 1e12), dev))


def msda_site(reps, log):
    from streammos_amd import ops
    from tests import util
    k = MSDA_SHAPE
    shapes, lsi = util.msda_levels(k["levels"])
    gen = torch.Generator(device="cpu").manual_seed(3)
    value = torch.randn((k["n"], k["s"], k["m"], k["d"]), generator=gen).to(DEV)
    loc = (torch.rand((k["n"], k["lq"], k["m"], 1, k["p"], 2), generator=gen) * 1.2 - 0.1).to(DEV)
    attn = torch.softmax(torch.randn((k["n"], k["lq"], k["m"], k["p"]), generator=gen), -1).view(k["n"], k["lq"], k["m"], 1, k["p"]).contiguous().to(DEV)
    go = torch.randn((k["n"], k["lq"], k["m"] * k["d"]), generator=gen).to(DEV)
    sh, ls = torch.from_numpy(shapes).to(DEV), torch.from_numpy(lsi).to(DEV)

    def run(det):
        return lambda: ops.msda_bwd(value, sh, ls, loc, attn, go, deterministic=det)
    ta, td = ub.measure(run(False), reps), ub.measure(run(True), reps)
    a, d1, d2 = run(False)(), run(True)(), run(True)()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(d1, d2))
    assert torch.equal(a[1].view(torch.int32), d1[1].view(torch.int32)) and torch.equal(a[2].view(torch.int32), d1[2].view(torch.int32))
    pairs = k["n"] * k["lq"] * k["m"] * k["p"] * 4
    rows = k["n"] * k["s"] * k["m"]
    emit, sort, _, summ, passes = least_bytes(pairs, rows, k["d"], pairs, k["n"] * k["lq"] * k["m"], 0, False)
    emit += value.numel() * 4 + go.numel() * 4 + loc.numel() * 4 + attn.numel() * 4 + loc.numel() * 4 + attn.numel() * 4   # grad_loc / grad_attn part
    total = emit + sort + summ
    log("")
    log("msda_bwd, N = %(n)d, S = Lq = %(s)d, M = %(m)d, D = %(d)d, L = 1, P = %(p)d" % k + ": %d pairs onto %d rows" % (pairs, rows))
    log("atomic         %s" % ub.fmt(ta))
    log("deterministic  %s   det / atomic %.2f; least %.1f MB (emit + grad_loc/grad_attn %.1f, sort %.1f in %d passes, sum %.1f): %.3f TB/s; "
        "max |det - atomic| on grad_value %.2e, grad_loc and grad_attn bit-equal" % (
            ub.fmt(td), statistics.median(td) / statistics.median(ta), total / 1e6, emit / 1e6, sort / 1e6, passes, summ / 1e6,
            total / (statistics.median(td) * 1e-3) / 1e12, (a[0] - d1[0]).abs().max().item()))


def steps(reps, parent, log):
    log("")
    log("stage-1 training step (tools/ubench_bilinear.py --step-child: AttNet.forward on three chained samples + backward, B = 4, N = %d)," % ub.N_POINTS)
    log("%d steps after 2 warm-ups, each setting in a fresh process: median (min..max)" % reps)
    runs = [("SMOS_DETERMINISTIC=0 (float atomics)", "0", ROOT), ("SMOS_DETERMINISTIC=1 (fixed-order sums)", "1", ROOT)]
    if parent:
        runs.append(("parent commit", None, os.path.abspath(parent)))
    for label, switch, root in runs:
        env = dict(os.environ)
        env.pop("SMOS_DETERMINISTIC", None)
        if switch is not None:
            env["SMOS_DETERMINISTIC"] = switch
        cmd = [sys.executable, os.path.join(root, "tools", "ubench_bilinear.py"), "--step-child", "--reps", str(reps)]
        proc = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        if proc.returncode != 0:
            log("%-44s FAILED (exit %d): %s" % (label, proc.returncode, proc.stderr.strip().splitlines()[-1:] or ""))
            raise SystemExit(proc.returncode)
        r = json.loads(proc.stdout.strip().splitlines()[-1])
        log("%-44s %s   loss %.5f, bilinear backward calls per step %d, peak %.1f GiB" % (
            label, ub.fmt(r["ms"]), r["loss"], r["own_backward_calls_per_step"], r["peak_gb"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubench_det_bwd.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    log("tools/ubench_det_bwd.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    bilinear_sites(args.reps, log)
    msda_site(args.reps, log)
    torch.cuda.empty_cache()
    if not args.no_steps:
        steps(args.reps, args.parent, log)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

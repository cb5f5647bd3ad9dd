"""Dev: the convolution kernels' share of one SERIAL streaming step (StreamRunner(pipeline=False), stage 1 + voting, B = 4 TTA x
N = 160 000, synthetic scans), fp32 against conv_precision="bf16": each precision runs in a child process under
`rocprofv3 --kernel-trace`, and the kernel durations of the timed steps (after the warm-up, split at the per-step tta_argmax
dispatch) are summed per family and divided by the number of steps.

    python tools/conv_family_step.py [out_dir]
"""
import collections, csv, glob, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, STEPS = 3, 10
FAMILIES = (("conv_wino1d", "conv_wino1d"), ("conv_wino", "conv_wino"), ("conv_igemm", "conv_igemm"), ("conv_rows", "conv_rows"),
            ("conv_bf16", "conv_bf16"))


def child(prec):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from streammos_amd import streaming, synth
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    m = StreamMOS.AttNet(cfg.get_config()[2])
    m.load_state_dict(synth.seeded_state_dict(m.state_dict()), strict=True)
    m = m.to("cuda:0").eval()
    r = streaming.StreamRunner(m, "cuda:0", vote=True, conv_precision=prec)
    frames = bench.make_frames(WARM + STEPS, seq_seed=3)
    devs = [r.upload(s, raw) for s, raw, _ in frames]
    for d, (_, _, pose) in zip(devs, frames):
        r.step(d, pose)
    torch.cuda.synchronize()


def family(name):
    for frag, fam in FAMILIES:
        if frag in name:
            return fam
    return None


def summarize(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "tta_argmax" in r["Kernel_Name"]]
    timed = rows[marks[WARM - 1] + 1:marks[-1] + 1]              # the STEPS steps after the warm-up
    steps = len(marks) - WARM
    fam, total = collections.Counter(), 0.0
    for r in timed:
        t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        total += t
        k = family(r["Kernel_Name"])
        if k:
            fam[k] += t
    return {k: v / steps for k, v in fam.items()}, total / steps, steps


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else "/tmp/conv_family_step"
    res = {}
    for prec in ("fp32", "bf16"):
        d = os.path.join(out, prec)
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable,
                               os.path.abspath(__file__), "--child", prec], stdout=subprocess.DEVNULL)
        res[prec] = summarize(d)
    for prec, (fam, total, steps) in res.items():
        conv = sum(fam.values())
        print("%s: serial step (mean of %d): kernels %.1f us, conv family %.1f us (%s)" % (
            prec, steps, total, conv, ", ".join("%s %.1f" % kv for kv in sorted(fam.items()))))

"""Dev: where does a wave of csrc/conv_bf16.hip spend its cycles?  Runs layers on a DIAGNOSTIC copy of the library with
in-kernel s_memtime stamps (-DSMOS_CONV_STAMPS; the shipped library has none) and prints, per layer, the block shape the host
picks, the cycles a wave spends per stage against its MFMA issue floor, and the share of each segment of the stage body.
Shares, not lengths: the stamps' own waits (lgkmcnt(0) after each) forbid overlaps the real kernel has.

    python tools/conv_bf16_stamps.py                     # builds the diagnostic library into /tmp first
    SMOS_HIP_LIB=<diagnostic .so> python tools/conv_bf16_stamps.py
"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("SMOS_HIP_LIB"):
    from streammos_amd import build
    diag, objs, procs = "/tmp/libsmos_bf16_stamps.so", [], []
    for src in build.sources():
        obj = "/tmp/bf16_stamps_" + os.path.basename(src)[:-4] + ".o"
        objs.append(obj)
        procs.append(subprocess.Popen([build.HIPCC] + build.FLAGS + ["-DSMOS_CONV_STAMPS", "-DSMOS_CONV_SCHED=0", "-c", src, "-o", obj]))
    if any(p.wait() for p in procs):
        sys.exit("diagnostic build failed")
    subprocess.check_call([build.HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", diag] + objs)
    os.environ["SMOS_HIP_LIB"] = diag
import torch
from streammos_amd import ops

dev = "cuda:0"
SEGMENTS = ["weight ring (park + request)", "region / residual requests", "fragments + MFMAs",
            "region write (barrier, wait, convert, store)", "epilogue", "end-of-stage barrier", "stage bookkeeping"]
MFMA_CYCLES = 32          # v_mfma_f32_32x32x16_bf16, back to back on one SIMD (MI355X_MICROARCH.md)


def pick_cfg(b, ho, wo, cout, kh, kw, s, res=False):
    """mirror of pick_cfg in csrc/conv_bf16.hip: (mt, wc, rw, rb, items)"""
    nq, best, key_best = cout // 32, None, -1
    for mt in (4, 2, 1):
        for wc in (1, 2, 4):
            for rw in (2, 1):
                g = mt * wc
                if g > 4 or nq % g or mt * rw > 4 or (res and mt * rw > 2):
                    continue
                rb = (4 // wc) * rw
                rr, cc = (rb - 1) * s + kh, 31 * s + kw
                if rr * cc * 4 > 2048 or (4 * g * 128 + rr * cc * 5) * 16 + cout * 4 > 80 * 1024:
                    continue
                items = b * -(-ho // rb) * -(-wo // 32) * (nq // g)
                key = ((min(items, 512)) * 8 + g) * 64 + mt * 8 + rw
                if key > key_best:
                    key_best, best = key, (mt, wc, rw, rb, items)
    return best


LAYERS = [("hdr_bev 3x3 32", 32, 32, (3, 3), 1, (256, 256)), ("hdr_bev 64->32", 64, 32, (3, 3), 1, (256, 256)),
          ("hdr_bev 7x3", 32, 32, (7, 3), 1, (256, 256)), ("conv_1a 64->128", 64, 128, (3, 3), 1, (256, 256)),
          ("conv_2 128->64", 128, 64, (3, 3), 1, (256, 256))]
for name, cin, cout, (kh, kw), stride, (h, w) in LAYERS:
    x = torch.randn(4, h, w, cin, device=dev).permute(0, 3, 1, 2)
    wt = torch.randn(cout, cin, kh, kw, device=dev) / (cin * kh * kw) ** 0.5
    bias = torch.randn(cout, device=dev)
    wp = ops.conv_bf16_prepare(wt)
    ho, wo = (h + 2 * (kh // 2) - kh) // stride + 1, (w + 2 * (kw // 2) - kw) // stride + 1
    mt, wc, rw, rb, items = pick_cfg(4, ho, wo, cout, kh, kw, stride)
    nstage = kh * kw * cin // 32
    buf = torch.zeros(4 * 11 * 2048, dtype=torch.int64, device=dev)
    os.environ["SMOS_CONV_STAMP_PTR"] = str(buf.data_ptr())
    for _ in range(3):
        ops.conv_bf16_cl(x, wp, bias, 1, cout, (kh, kw), stride=stride)
    torch.cuda.synchronize()
    st = buf.view(-1, 11).double()
    st = st[st[:, 9] > 0]
    seg = st[:, :7].sum(0)
    per_stage = st[:, 9].sum().item() / (4 * items * nstage)          # every wave of a block runs all of its block's stages
    floor = 2 * rw * mt * MFMA_CYCLES
    ghz = (st[:, 9] / st[:, 10]).mean().item() / 10.0                   # s_memrealtime runs at 100 MHz
    print("%-16s MT %d wc %d RW %d (rb %d rows, %d items, %d blocks, %d stages / item): %.0f cycles per stage per wave, "
          "MFMA issue floor %d (%.2f GHz)" % (name, mt, wc, rw, rb, items, st.shape[0] // 4, nstage, per_stage, floor, ghz))
    for k, nm in enumerate(SEGMENTS):
        print("    %-46s %5.1f %%" % (nm, 100.0 * seg[k].item() / seg.sum().item()))

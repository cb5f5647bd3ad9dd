"""Dev: one sha256 per result of ops.point_mlp_train and ops.point_head_train on shapes around a chunk and a group of the
fixed-order sums (csrc/chunk_sums.h).  Two commits that print the same lines compute the same bits.

  python tools/train_ops_digest.py [--out FILE]

Uses nothing but the two ops, ops.point_head_keep_bits, the case builders of tests/ and the grid-cap hook, so the same file
runs in a built checkout of an older commit.  Per op, with v in (2, chunk - 1, chunk, chunk + 1, 64 chunk + 1 = a second
group): the v points as one sample (v = 2: as two samples of one point), and two samples of v points (of 32 chunk + 1
for the last), where a sample boundary falls inside a chunk.  Each shape in train and eval mode, forward and backward with
all gradients, uncapped and under a grid cap of 3 blocks; the head with the case's keep masks and with masks drawn under
torch.manual_seed, and once more with inputs cut out of a longer point axis.  Hashed: the output, every gradient, the
running buffers after the call, and the head's keep bits.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from streammos_amd import _lib, ops
from tests import point_head_train_cases as head_cases
from tests import point_mlp_cases as mlp_cases

DEV = "cuda:0"
CAPS = (0, 3)


def shapes(chunk):
    one = [(2, 1)] + [(1, v) for v in (chunk - 1, chunk, chunk + 1, 64 * chunk + 1)]
    two = [(2, v) for v in (chunk - 1, chunk, chunk + 1, 32 * chunk + 1)]
    return one + two


def sha(t):
    return "-" if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def capped(cap, fn):
    lib = _lib.load()
    lib.smos_debug_set_conv_grid_cap(cap)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.smos_debug_set_conv_grid_cap(0)
    return out


def mlp(log):
    for s, n in shapes(ops.point_mlp_chunk()):
        c = mlp_cases.make_case("kitti", s, n)
        x = torch.from_numpy(c["x"]).to(device=DEV, dtype=torch.float32)
        g = torch.from_numpy(c["g"]).to(device=DEV, dtype=torch.float32)
        for mode in ("train", "eval"):
            for cap in CAPS:
                m = mlp_cases.build_modules(c, torch.float32, DEV).train(mode == "train")
                a, b = m.layer[0].layer, m.layer[1].layer

                def run():
                    y = ops.point_mlp_train(x, a[0], a[1], a[2], b[0], b[1], training=mode == "train")
                    y.backward(g)
                    return y
                y = capped(cap, run)
                params, buffers = mlp_cases.module_tensors(m)
                tag = "mlp %dx%d %s cap%d" % (s, n, mode, cap)
                log("%s y %s" % (tag, sha(y)))
                for k, p in params.items():
                    log("%s d%s %s" % (tag, k, sha(p.grad)))
                for k, buf in buffers.items():
                    log("%s %s %s" % (tag, k, sha(buf)))


def head(log):
    for bs, n in shapes(ops.point_head_train_chunk()):
        c = head_cases.make_case("plain", bs, n)
        runs = [(mode, cap, masks, False) for cap in CAPS for mode, masks in (("train", "case"), ("train", "drawn"), ("eval", "none"))]
        runs.append(("train", 0, "case", True))
        for mode, cap, masks, pitched in runs:
            fusion, pred = head_cases.build_modules(c, torch.float32, DEV)
            fusion.train(mode == "train")
            pred.train(mode == "train")
            xs, g, own = head_cases.case_tensors(c, torch.float32, DEV, grad=False)
            if pitched:       # the same values, each input a slice of a longer point axis
                xs = [torch.cat([x, x.new_full((bs, 64, 5 + i, 1), 7.0)], dim=2)[:, :, :n] for i, x in enumerate(xs)]
            xs = [x.requires_grad_(True) for x in xs]
            ml = fusion.merge_layer

            def run():
                torch.manual_seed(20)
                out = ops.point_head_train(*xs, ml[0], ml[1], ml[3], ml[4], pred.pred_layer[0], training=mode == "train",
                                           keep=own if masks == "case" else None)
                out.backward(g)
                return out
            out = capped(cap, run)
            params, buffers = head_cases.module_tensors(fusion, pred)
            tag = "head %dx%d %s cap%d masks-%s%s" % (bs, n, mode, cap, masks, " pitched" if pitched else "")
            log("%s logits %s" % (tag, sha(out)))
            for k, x in zip(head_cases.INPUTS, xs):
                log("%s d%s %s" % (tag, k, sha(x.grad)))
            for k, p in params.items():
                log("%s d%s %s" % (tag, k, sha(p.grad)))
            for k, buf in buffers.items():
                log("%s %s %s" % (tag, k, sha(buf)))
            keep = ops.point_head_keep_bits(out)
            for i, k in enumerate(keep if keep is not None else (None, None), 1):
                log("%s keep%d %s" % (tag, i, sha(k)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)
    mlp(log)
    head(log)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Dev: the fused point head alone (B=4, N=160000), and the head that gathers its BEV rows itself against the gather launch +
head pair it replaces (the decoder shapes of the bench: a 64-channel 256 x 256 map, 96 069 live points per sample)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from streammos_amd import ops
dev = "cuda:0"
g = torch.Generator(device="cpu").manual_seed(0)
rows = torch.randn((4, 160000, 192), generator=g).to(dev)
l1 = ((torch.randn((96, 192), generator=g) * 0.1).to(dev), torch.randn(96, generator=g).to(dev))
l2 = ((torch.randn((64, 96), generator=g) * 0.1).to(dev), torch.randn(64, generator=g).to(dev))
l3 = ((torch.randn((3, 64), generator=g) * 0.1).to(dev), torch.randn(3, generator=g).to(dev))
w, m3 = ops.point_head_prepare(l1, l2, l3)
for _ in range(5): ops.point_head(rows, w, m3)
torch.cuda.synchronize()
a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(30): ops.point_head(rows, w, m3)
b.record(); torch.cuda.synchronize()
ms = a.elapsed_time(b) / 30
print("point_head %.4f ms  %.1f TFLOP/s  (floor 0.2015 ms at 157.3 TFLOP/s)" % (ms, 2 * 640000 * (192 * 96 + 96 * 64 + 64 * 3) / ms / 1e9))

# the runner's form: the scan's padding tail left out (96 069 real points of 160 000 on the bench's synthetic scans)
n_live = torch.tensor([96069], dtype=torch.int32, device="cuda:0")
for _ in range(5): ops.point_head(rows, w, m3, n_live=n_live)
torch.cuda.synchronize()
a.record()
for _ in range(30): ops.point_head(rows, w, m3, n_live=n_live)
b.record(); torch.cuda.synchronize()
ms = a.elapsed_time(b) / 30
print("point_head, 96 069 live points per sample: %.4f ms  (matrix floor %.4f ms)" % (ms, 0.2015 * 96069 / 160000))

# fold mode: smos_point_head_gather against gather_scatter_cl(pts_out=rows[:, :, 64:128]) + point_head
grid = torch.randn((4, 256, 256, 64), generator=g).to(dev).permute(0, 3, 1, 2)
pcds = torch.full((4, 3, 160000, 3, 1), -1000.0)
pcds[:, :, :96069, :2, 0] = torch.rand((4, 3, 96069, 2), generator=g) * 511.0      # positions = coordinate * 0.5 over the map
xy = pcds.to(dev)[:, 0, :, :2, 0]
scale = (0.5, 0.5)


def pair():
    ops.gather_scatter_cl(grid, xy, scale, pts_out=rows[:, :, 64:128], n_live=n_live)
    return ops.point_head(rows, w, m3, n_live=n_live)


def fold():
    return ops.point_head(rows, w, m3, n_live=n_live, gather=(grid, xy, scale))


if not os.environ.get("SMOS_HIP_LIB"):          # (a diagnostic build of tools/ablate_head.sh computes nothing meaningful)
    assert torch.equal(pair()[:, :, :96069], fold()[:, :, :96069])
for name, fn in (("gather + head pair", pair), ("fold", fold), ("gather + head pair", pair), ("fold", fold)):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(30): fn()
    b.record(); torch.cuda.synchronize()
    print("%-20s 96 069 live points per sample, uniform positions: %.4f ms" % (name, a.elapsed_time(b) / 30))

"""Dev: device DBSCAN at realistic foreground sizes (cars as 200-point blobs) and a worst-case chain."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from streammos_amd import ops
dev = "cuda:0"
rng = np.random.default_rng(0)
for n_obj in (10, 50, 100, 250):
    pts = np.concatenate([rng.normal(c, (0.8, 0.35, 0.3), (200, 3)) for c in rng.uniform(-45, 45, (n_obj, 3)) * (1, 1, 0.02)]).astype(np.float32)
    x = torch.from_numpy(pts).to(dev)
    ops.dbscan(x, 0.3, 5); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(5): lab = ops.dbscan(x, 0.3, 5)
    torch.cuda.synchronize()
    print("n=%6d  %.2f ms   clusters %d" % (len(pts), (time.perf_counter() - t) / 5 * 1e3, len(torch.unique(lab[lab >= 0]))), flush=True)
chain = np.stack((np.arange(20000) * 0.05, np.zeros(20000), np.zeros(20000)), 1).astype(np.float32)   # one 1 km wall
x = torch.from_numpy(chain).to(dev)
t = time.perf_counter(); lab = ops.dbscan(x, 0.3, 5); torch.cuda.synchronize()
print("chain n=20000  %.2f ms  clusters %d" % ((time.perf_counter() - t) * 1e3, len(torch.unique(lab[lab >= 0]))))

# The device-resident path (ops.instance_cluster: names + boxes of a whole 120 000-point scan, nothing read back) beside the
# existing one (ops.dbscan on the compacted foreground + InstanceVoter.cluster_boxes) on the same points, alternating.
from streammos_amd import streaming
voter = streaming.InstanceVoter(dev)
N_SCAN = 120000
for n_fg in (2000, 20000, 50000):
    fgp = np.concatenate([rng.normal(c, (0.8, 0.35, 0.3), (200, 3)) for c in rng.uniform(-45, 45, (n_fg // 200, 3)) * (1, 1, 0.02)])
    rest = rng.uniform(-50, 50, (N_SCAN - n_fg, 3)) * (1, 1, 0.03)
    order = rng.permutation(N_SCAN)
    scan = np.concatenate((np.concatenate((fgp, rest))[order], np.zeros((N_SCAN, 1))), axis=1).astype(np.float32)
    bf = np.concatenate((np.full(n_fg, 2), np.ones(N_SCAN - n_fg)))[order].astype(np.uint8)
    scan_d, bf_d = torch.from_numpy(scan).to(dev), torch.from_numpy(bf).to(dev)
    work = torch.empty(ops.instance_work_bytes(N_SCAN), dtype=torch.uint8, device=dev)

    def old():
        fg = torch.nonzero(bf_d == 2).flatten()
        return voter.cluster_boxes(scan_d[fg][:, :3].contiguous())[2]

    def new():
        return ops.instance_cluster(scan_d, bf_d, voter.EPS, voter.MIN_SAMPLES, voter.MIN_POINTS, voter.FLOOR_LIFT, work=work)

    times = {"old": [], "new": []}
    for rep in range(6):                                  # the first round is the warm-up
        for name, fn in (("old", old), ("new", new)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(5): res = fn()
            torch.cuda.synchronize()
            if rep: times[name].append((time.perf_counter() - t) / 5 * 1e3)
    k_old, k_new = old().shape[0], int(new()["k"].item())
    print("n_fg=%6d of %d  dbscan+cluster_boxes %.2f ms (min %.2f)   instance_cluster %.2f ms (min %.2f)   boxes %d / %d"
          % (n_fg, N_SCAN, np.median(times["old"]), min(times["old"]), np.median(times["new"]), min(times["new"]), k_old, k_new), flush=True)

"""Cases and the float64 reference of ops.point_mlp_train (csrc/point_mlp_train.hip).

``restate`` writes the forward, the running-statistics update and the backward of

    BN0 -> 1x1 conv 7->64 -> BN1 -> ReLU -> 1x1 conv 64->64 -> BN2 -> ReLU         (PointNetStacker(7, 64, True, stack_num=2))

out in numpy float64, formula by formula; tests/test_host_point_mlp.py holds it against torch.autograd through the float64
modules and shows that each of its six value-only mutants moves a result by far more than the GPU test's bar.  The GPU
test compares the kernels with it.

Error metric (per tensor): max|got - ref| / max|ref|; dbeta0, whose true value is zero (a bias in front of a batch norm),
is scaled by max|dgamma0| instead.
"""
import numpy as np

SHAPES = ((1, 5), (3, 32), (3, 45), (6, 97), (2, 1000))          # (S, N): under a tile, one tile, a ragged tail, ..., several chunks
CASES = ("normal", "kitti", "bigmean", "const", "dead")
MODES = ("train", "eval")
PARAMS = ("g0", "b0", "w1", "g1", "b1", "w2", "g2", "b2")
BUFFERS = ("rm0", "rv0", "rm1", "rv1", "rm2", "rv2")
MUTANTS = ("unbiased_norm", "no_dbeta", "no_dgamma", "mask_from_z", "biased_running", "dw2_from_zhat")
EPS = (1e-5, 1e-5, 1e-5)
MOM = (0.1, 0.1, 0.1)
FLOOR = 1e-6                 # the bar is max(8 x the float32 module path's own error, FLOOR)


def _rng(*key):
    return np.random.default_rng([20240607] + [int(k) for k in key])


def make_case(name, s, n):
    """-> dict: x [S,7,N,1], g [S,64,N,1] (the incoming gradient), the eight parameters and the six running buffers, all
    float64 arrays holding float32 values (so that the float32 runs see exactly the reference's inputs)."""
    ci, si = CASES.index(name), SHAPES.index((s, n)) if (s, n) in SHAPES else 99
    r = _rng(ci, si, s, n)
    x = r.standard_normal((s, 7, n))
    if name == "kitti":
        x[:, 0:2] *= 20.0
        x[:, 2] = -1.7 + 0.5 * x[:, 2]
        x[:, 3] = np.abs(r.random((s, n)))
        x[:, 4] = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2 + x[:, 2] ** 2)
        x[:, 5:7] = r.random((s, 2, n))
    elif name == "bigmean":
        x[:, 4] = 1000.0 + 0.01 * x[:, 4]
    elif name == "const":
        x[:, 5] = 0.75
    c = {"x": x[..., None], "g": r.standard_normal((s, 64, n, 1)),
         "g0": 1.0 + 0.3 * r.standard_normal(7), "b0": 0.2 * r.standard_normal(7),
         "w1": r.standard_normal((64, 7)) / np.sqrt(7.0), "g1": 1.0 + 0.3 * r.standard_normal(64), "b1": 0.2 * r.standard_normal(64),
         "w2": r.standard_normal((64, 64)) / 8.0, "g2": 1.0 + 0.3 * r.standard_normal(64), "b2": 0.2 * r.standard_normal(64),
         "rm0": x.mean((0, 2)) + 0.1 * r.standard_normal(7), "rv0": x.var((0, 2)) * (1.0 + 0.2 * r.random(7)) + 0.05,
         "rm1": 0.3 * r.standard_normal(64), "rv1": 0.5 + r.random(64),
         "rm2": 0.3 * r.standard_normal(64), "rv2": 0.5 + r.random(64)}
    if name == "dead":
        c["b1"][11] = -50.0              # a hidden unit that never fires
        c["w1"][23, :] = 0.0             # a hidden unit with constant input (zero variance in BN1)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in c.items()}


def restate(c, training, mutant=None):
    """The float64 restatement.  -> dict: y [S,64,N,1], d<param> for the eight parameters, the six buffers after the call."""
    x4, g4 = c["x"], c["g"]
    s, _, n, _ = x4.shape
    X = x4[..., 0].transpose(1, 0, 2).reshape(7, -1)
    G = g4[..., 0].transpose(1, 0, 2).reshape(64, -1)
    P = X.shape[1]
    t = 1.0 if training else 0.0
    out = {}

    def stats(v, i):
        rm, rv = c["rm%d" % i], c["rv%d" % i]
        if not training:
            out["rm%d" % i], out["rv%d" % i] = rm.copy(), rv.copy()
            return rm, 1.0 / np.sqrt(rv + EPS[i])
        mu = v.mean(1)
        var = ((v - mu[:, None]) ** 2).mean(1)
        unbiased = var * P / (P - 1)
        out["rm%d" % i] = (1.0 - MOM[i]) * rm + MOM[i] * mu
        out["rv%d" % i] = (1.0 - MOM[i]) * rv + MOM[i] * (var if mutant == "biased_running" else unbiased)
        return mu, 1.0 / np.sqrt((unbiased if mutant == "unbiased_norm" else var) + EPS[i])

    def bn_backward(da, zh, gamma, r):
        db, dg = da.sum(1), (da * zh).sum(1)
        mean_b = 0.0 if mutant == "no_dbeta" else t * db[:, None] / P
        mean_g = 0.0 if mutant == "no_dgamma" else t * zh * dg[:, None] / P
        return db, dg, (gamma * r)[:, None] * (da - mean_b - mean_g)

    mu0, r0 = stats(X, 0)
    xt = (X - mu0[:, None]) * r0[:, None]
    xh = c["g0"][:, None] * xt + c["b0"][:, None]
    z1 = c["w1"] @ xh
    mu1, r1 = stats(z1, 1)
    zh1 = (z1 - mu1[:, None]) * r1[:, None]
    a1 = c["g1"][:, None] * zh1 + c["b1"][:, None]
    h1 = np.maximum(a1, 0.0)
    z2 = c["w2"] @ h1
    mu2, r2 = stats(z2, 2)
    zh2 = (z2 - mu2[:, None]) * r2[:, None]
    a2 = c["g2"][:, None] * zh2 + c["b2"][:, None]
    y = np.maximum(a2, 0.0)
    out["y"] = y.reshape(64, s, n).transpose(1, 0, 2)[..., None]

    da2 = G * ((z2 if mutant == "mask_from_z" else a2) > 0)
    out["db2"], out["dg2"], dz2 = bn_backward(da2, zh2, c["g2"], r2)
    out["dw2"] = dz2 @ (zh1 if mutant == "dw2_from_zhat" else h1).T
    da1 = (c["w2"].T @ dz2) * ((z1 if mutant == "mask_from_z" else a1) > 0)
    out["db1"], out["dg1"], dz1 = bn_backward(da1, zh1, c["g1"], r1)
    out["dw1"] = dz1 @ xh.T
    dxh = c["w1"].T @ dz1
    out["db0"], out["dg0"] = dxh.sum(1), (dxh * xt).sum(1)
    return out


def closed_forms(c, training):
    """The arithmetic of csrc/point_mlp_train.hip in float64: statistics of z1 from the centred second moments of x, the
    backward's lower layers from the one 64x8 sum M = sum da1 (x) (x - mu0, 1) (header of the file, `pm_fin_l1`, `pm_fin_bwd2`).
    -> the results `restate` gives, by the other route."""
    x4, g4 = c["x"], c["g"]
    s, _, n, _ = x4.shape
    X = x4[..., 0].transpose(1, 0, 2).reshape(7, -1)
    G = g4[..., 0].transpose(1, 0, 2).reshape(64, -1)
    P = X.shape[1]
    t = 1.0 if training else 0.0
    out = {}

    def running(i, mu, var):
        out["rm%d" % i] = (1.0 - MOM[i]) * c["rm%d" % i] + MOM[i] * mu if training else c["rm%d" % i].copy()
        out["rv%d" % i] = (1.0 - MOM[i]) * c["rv%d" % i] + MOM[i] * var * P / max(P - 1, 1) if training else c["rv%d" % i].copy()

    if training:
        mu0 = X[:, 0] + (X - X[:, :1]).sum(1) / P
        d = X - mu0[:, None]
        cov = d @ d.T / P
        var0 = np.diag(cov).copy()
    else:
        mu0, var0 = c["rm0"], c["rv0"]
        d = X - mu0[:, None]
        cov = np.zeros((7, 7))
    running(0, mu0, var0)
    r0 = 1.0 / np.sqrt(var0 + EPS[0])
    a0 = c["g0"] * r0
    u = c["w1"] * a0[None, :]
    m1 = c["w1"] @ c["b0"]
    mu1, var1 = (m1, np.einsum("ja,ab,jb->j", u, cov, u)) if training else (c["rm1"], c["rv1"])
    running(1, mu1, var1)
    r1 = 1.0 / np.sqrt(var1 + EPS[1])
    Z1, ZC1 = r1[:, None] * u, r1 * (m1 - mu1)
    zh1 = Z1 @ d + ZC1[:, None]
    h1 = np.maximum(c["g1"][:, None] * zh1 + c["b1"][:, None], 0.0)
    z2 = c["w2"] @ h1
    if training:
        first = z2[:, :512].mean(1)
        s1, s2 = (z2 - first[:, None]).sum(1) / P, ((z2 - first[:, None]) ** 2).sum(1) / P
        mu2, var2 = first + s1, np.maximum(s2 - s1 * s1, 0.0)
    else:
        mu2, var2 = c["rm2"], c["rv2"]
    running(2, mu2, var2)
    r2 = 1.0 / np.sqrt(var2 + EPS[2])
    cen = z2 - mu2[:, None]
    pre = (c["g2"] * r2)[:, None] * cen + c["b2"][:, None]
    out["y"] = np.maximum(pre, 0.0).reshape(64, s, n).transpose(1, 0, 2)[..., None]
    zh2 = cen * r2[:, None]
    da2 = G * (pre > 0)
    out["db2"], out["dg2"] = da2.sum(1), (da2 * zh2).sum(1)
    dz2 = (c["g2"] * r2)[:, None] * (da2 - t * out["db2"][:, None] / P - zh2 * t * out["dg2"][:, None] / P)
    out["dw2"] = dz2 @ h1.T
    da1 = (c["w2"].T @ dz2) * (h1 > 0)
    M = da1 @ np.concatenate((d, np.ones((1, P))), 0).T                  # [64, 8]
    db1 = M[:, 7]
    dg1 = (Z1 * M[:, :7]).sum(1) + ZC1 * db1
    gr = c["g1"] * r1
    D = gr[:, None] * (M[:, :7] - t * (dg1 * r1)[:, None] * (u @ cov))
    sdz1 = (1.0 - t) * gr * db1
    out["db1"], out["dg1"] = db1, dg1
    out["dw1"] = D * a0[None, :] + sdz1[:, None] * c["b0"][None, :]
    out["dg0"] = r0 * (c["w1"] * D).sum(0)
    out["db0"] = c["w1"].T @ sdz1
    return out


RESULTS = ("y",) + tuple("d" + p for p in PARAMS) + BUFFERS


def metric(got, ref, key):
    """max|got - ref| / max|ref| of one result; db0 on the scale of dg0."""
    scale = np.abs(ref["dg0"]).max() if key == "db0" else np.abs(ref[key]).max()
    return float(np.abs(np.asarray(got[key], dtype=np.float64).reshape(ref[key].shape) - ref[key]).max() / max(scale, 1e-300))


def build_modules(c, dtype, device="cpu"):
    """PointNetStacker(7, 64, pre_bn=True, stack_num=2) holding the case's parameters and buffers."""
    import torch
    from streammos_amd.refapi.networks.backbone import PointNetStacker
    m = PointNetStacker(7, 64, pre_bn=True, stack_num=2)
    a, b = m.layer[0].layer, m.layer[1].layer
    mods = {"0": a[0], "1": a[2], "2": b[1]}
    with torch.no_grad():
        for i, bn in mods.items():
            bn.weight.copy_(torch.from_numpy(c["g" + i]))
            bn.bias.copy_(torch.from_numpy(c["b" + i]))
            bn.running_mean.copy_(torch.from_numpy(c["rm" + i]))
            bn.running_var.copy_(torch.from_numpy(c["rv" + i]))
        a[1].weight.copy_(torch.from_numpy(c["w1"]).reshape(64, 7, 1, 1))
        b[0].weight.copy_(torch.from_numpy(c["w2"]).reshape(64, 64, 1, 1))
    return m.to(device=device, dtype=dtype)


def module_tensors(m):
    a, b = m.layer[0].layer, m.layer[1].layer
    params = {"g0": a[0].weight, "b0": a[0].bias, "w1": a[1].weight, "g1": a[2].weight, "b1": a[2].bias, "w2": b[0].weight,
              "g2": b[1].weight, "b2": b[1].bias}
    buffers = {"rm0": a[0].running_mean, "rv0": a[0].running_var, "rm1": a[2].running_mean, "rv1": a[2].running_var,
               "rm2": b[1].running_mean, "rv2": b[1].running_var}
    return params, buffers


def run_modules(c, training, dtype, device="cpu", module=None):
    """forward + backward through the module (the module path unless the fused switch is on) -> results as float64 numpy."""
    import torch
    m = build_modules(c, dtype, device) if module is None else module
    m.train(training)
    x = torch.from_numpy(c["x"]).to(device=device, dtype=dtype)
    g = torch.from_numpy(c["g"]).to(device=device, dtype=dtype)
    y = m(x)
    y.backward(g)
    params, buffers = module_tensors(m)
    out = {"y": y.detach().double().cpu().numpy()}
    for k, p in params.items():
        out["d" + k] = None if p.grad is None else p.grad.detach().double().cpu().numpy().reshape(c[k].shape)
    for k, b in buffers.items():
        out[k] = b.detach().double().cpu().numpy()
    return out, m

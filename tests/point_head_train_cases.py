"""Cases and the float64 reference of ops.point_head_train (csrc/point_head_train.hip).

``restate`` writes the forward, the running-statistics update and the backward of

    cat(a, b, c) -> dropout -> 1x1 192->96 -> BN1 -> ReLU -> 1x1 96->64 -> BN2 -> ReLU -> dropout -> 1x1 64->3 + bias

(CatFusion + PredBranch) out in numpy float64 with explicit keep masks, formula by formula;
tests/test_host_point_head_train.py holds it against torch.autograd through the float64 modules and shows that each of its
six mutants moves a result by more than the GPU test's bar.  The GPU test compares the kernels with it.

Error metric (per result): max|got - ref| / max|ref|; a bias gradient (dbeta1, dbeta2, db3) on the scale of its weight's
(dgamma1, dgamma2, dW3).

All inputs are non-negative, as the real ones are (each is the output of a ReLU).
"""
import numpy as np

CASES = ("plain", "bigmean", "dead", "const", "dropped")
MODES = ("train", "eval")
INPUTS = ("xa", "xb", "xc")
PARAMS = ("w1", "g1", "be1", "w2", "g2", "be2", "w3", "b3")
BUFFERS = ("rm1", "rv1", "rm2", "rv2")
RESULTS = ("logits",) + tuple("d" + k for k in INPUTS + PARAMS) + BUFFERS
SCALE_OF = {"dbe1": "dg1", "dbe2": "dg2", "db3": "dw3"}
MUTANTS = ("no_scale_bwd", "biased_running", "no_mean_term", "relu_wrong_layer", "keep2_before_bn", "dw1_unmasked_x")
EPS = (1e-5, 1e-5)
MOM = (0.1, 0.1)
SCALE = 1.25                 # 1 / (1 - 0.2), exact in float32
FLOOR = 1e-6                 # the bar is max(8 x the float32 module path's own error, FLOOR)
BIG_CHANNEL = 70             # `bigmean`: channel 6 of b
DROPPED_CHANNEL = 17         # `dropped`: this input channel is dropped at every point
DEAD1, DEAD2, CONST2 = 11, 7, 5


def shapes():
    """(B, N): two points; under a wave; a ragged tail; several samples; and 2 N just over three chunks of partial sums."""
    from streammos_amd import ops
    return ((1, 2), (2, 33), (3, 70), (6, 97), (2, (3 * ops.point_head_train_chunk()) // 2 + 1))


def dropped_point(b, n):
    """`dropped`: the (sample, point) whose 64 keep2 bits are all off"""
    return b - 1, n // 2


def _rng(*key):
    return np.random.default_rng([20250911] + [int(k) for k in key])


def _flat(x4):
    """[B,C,N,1] -> [C, B*N]"""
    return x4[..., 0].transpose(1, 0, 2).reshape(x4.shape[1], -1)


def _unflat(m, b, n):
    return m.reshape(m.shape[0], b, n).transpose(1, 0, 2)[..., None]


def make_case(name, b, n):
    """-> dict: xa, xb, xc [B,64,N,1], g [B,3,N,1] (the incoming gradient), the eight parameters, the four running buffers
    (float64 arrays holding float32 values, so that the float32 runs see exactly the reference's inputs) and keep1 [B,192,N],
    keep2 [B,64,N] bool."""
    r = _rng(CASES.index(name), b, n)
    x = np.abs(r.standard_normal((b, 192, n)))
    if name == "bigmean":
        x[:, BIG_CHANNEL] = 1000.0 + 0.01 * r.standard_normal((b, n))
    c = {"g": r.standard_normal((b, 3, n, 1)),
         "w1": r.standard_normal((96, 192)) / np.sqrt(192.0), "g1": 1.0 + 0.3 * r.standard_normal(96), "be1": 0.2 * r.standard_normal(96),
         "w2": r.standard_normal((64, 96)) / np.sqrt(96.0), "g2": 1.0 + 0.3 * r.standard_normal(64), "be2": 0.2 * r.standard_normal(64),
         "w3": r.standard_normal((3, 64)) / 8.0, "b3": 0.2 * r.standard_normal(3)}
    if name == "dead":
        c["be1"][DEAD1] = -50.0              # negative at every point: no gradient passes
        c["be2"][DEAD2] = -50.0
    if name == "const":
        c["w2"][CONST2, :] = 0.0             # z2 is 0 at every point: zero variance, eps governs
    keep1, keep2 = r.random((b, 192, n)) < 0.8, r.random((b, 64, n)) < 0.8
    if name == "dropped":
        keep1[:, DROPPED_CHANNEL] = False
        pb, pn = dropped_point(b, n)
        keep2[pb, :, pn] = False
    # running buffers near what the data gives in eval mode, so that eval activations stay in range
    X = x.transpose(1, 0, 2).reshape(192, -1)
    z1 = c["w1"] @ X
    c["rm1"] = z1.mean(1) + 0.1 * r.standard_normal(96)
    c["rv1"] = z1.var(1) * (1.0 + 0.2 * r.random(96)) + 0.05
    h1 = np.maximum(c["g1"][:, None] * (z1 - c["rm1"][:, None]) / np.sqrt(c["rv1"][:, None] + EPS[0]) + c["be1"][:, None], 0.0)
    z2 = c["w2"] @ h1
    c["rm2"] = z2.mean(1) + 0.1 * r.standard_normal(64)
    c["rv2"] = z2.var(1) * (1.0 + 0.2 * r.random(64)) + 0.05
    c["xa"], c["xb"], c["xc"] = x[:, :64, :, None], x[:, 64:128, :, None], x[:, 128:, :, None]
    c = {k: v.astype(np.float32).astype(np.float64) for k, v in c.items()}
    c["keep1"], c["keep2"] = keep1, keep2
    return c


def restate(c, training, mutant=None, keep=None):
    """The float64 restatement -> dict of RESULTS.  ``keep``: (keep1, keep2) instead of the case's own masks."""
    b, _, n, _ = c["xa"].shape
    X = np.concatenate([_flat(c[k]) for k in INPUTS], 0)
    G = _flat(c["g"])
    P = X.shape[1]
    t = 1.0 if training else 0.0
    k1, k2 = (c["keep1"], c["keep2"]) if keep is None else keep
    if training:
        K1 = k1.transpose(1, 0, 2).reshape(192, -1).astype(np.float64)
        K2 = k2.transpose(1, 0, 2).reshape(64, -1).astype(np.float64)
        s = SCALE
    else:
        K1, K2, s = np.ones((192, P)), np.ones((64, P)), 1.0
    sb = 1.0 if mutant == "no_scale_bwd" else s
    out = {}

    def stats(v, i):
        rm, rv = c["rm%d" % i], c["rv%d" % i]
        if not training:
            out["rm%d" % i], out["rv%d" % i] = rm.copy(), rv.copy()
            return rm, 1.0 / np.sqrt(rv + EPS[i - 1])
        mu = v.mean(1)
        var = ((v - mu[:, None]) ** 2).mean(1)
        # how far a two-point batch amplifies rounding (tests/test_host_point_head_train.py derives it)
        out["_amp%d" % i] = float(((var + EPS[i - 1]) / EPS[i - 1] * np.maximum(1.0, np.abs(v).max(1) / np.sqrt(var + EPS[i - 1]))).max())
        out["rm%d" % i] = (1.0 - MOM[i - 1]) * rm + MOM[i - 1] * mu
        out["rv%d" % i] = (1.0 - MOM[i - 1]) * rv + MOM[i - 1] * (var if mutant == "biased_running" else var * P / (P - 1))
        return mu, 1.0 / np.sqrt(var + EPS[i - 1])

    def bn_backward(da, zh, gamma, r):
        db, dg = da.sum(1), (da * zh).sum(1)
        mean_b = 0.0 if mutant == "no_mean_term" else t * db[:, None] / P
        return db, dg, (gamma * r)[:, None] * (da - mean_b - t * zh * dg[:, None] / P)

    xt = X * K1 * s
    z1 = c["w1"] @ xt
    mu1, r1 = stats(z1, 1)
    zh1 = (z1 - mu1[:, None]) * r1[:, None]
    a1 = c["g1"][:, None] * zh1 + c["be1"][:, None]
    h1 = np.maximum(a1, 0.0)
    z2 = c["w2"] @ h1
    if mutant == "keep2_before_bn":
        z2 = z2 * K2 * s
    mu2, r2 = stats(z2, 2)
    zh2 = (z2 - mu2[:, None]) * r2[:, None]
    a2 = c["g2"][:, None] * zh2 + c["be2"][:, None]
    h2 = np.maximum(a2, 0.0)
    h2d = h2 if mutant == "keep2_before_bn" else h2 * K2 * s
    out["logits"] = _unflat(c["w3"] @ h2d + c["b3"][:, None], b, n)

    out["dw3"], out["db3"] = G @ h2d.T, G.sum(1)
    dh2 = c["w3"].T @ G
    if mutant != "keep2_before_bn":
        dh2 = dh2 * K2 * sb
    da2 = dh2 * ((a1[:64] if mutant == "relu_wrong_layer" else a2) > 0)
    out["dbe2"], out["dg2"], dz2 = bn_backward(da2, zh2, c["g2"], r2)
    if mutant == "keep2_before_bn":
        dz2 = dz2 * K2 * s
    out["dw2"] = dz2 @ h1.T
    da1 = (c["w2"].T @ dz2) * (a1 > 0)
    out["dbe1"], out["dg1"], dz1 = bn_backward(da1, zh1, c["g1"], r1)
    out["dw1"] = dz1 @ (X * s if mutant == "dw1_unmasked_x" else xt).T
    dx = (c["w1"].T @ dz1) * K1 * sb
    for i, k in enumerate(INPUTS):
        out["d" + k] = _unflat(dx[64 * i:64 * i + 64], b, n)
    return out


def metric(got, ref, key):
    """max|got - ref| / max|ref| of one result; a bias gradient on the scale of its weight's gradient."""
    scale = np.abs(ref[SCALE_OF.get(key, key)]).max()
    return float(np.abs(np.asarray(got[key], dtype=np.float64).reshape(ref[key].shape) - ref[key]).max() / max(scale, 1e-300))


def build_modules(c, dtype, device="cpu"):
    """(CatFusion((64, 64, 64), 64), PredBranch(64, 3)) holding the case's parameters and buffers."""
    import torch
    from streammos_amd.refapi.networks.backbone import CatFusion, PredBranch
    fusion, pred = CatFusion((64, 64, 64), 64), PredBranch(64, 3)
    m = fusion.merge_layer
    with torch.no_grad():
        for conv, k in ((m[0], "w1"), (m[3], "w2"), (pred.pred_layer[0], "w3")):
            conv.weight.copy_(torch.from_numpy(c[k]).reshape(conv.weight.shape))
        pred.pred_layer[0].bias.copy_(torch.from_numpy(c["b3"]))
        for bn, i in ((m[1], "1"), (m[4], "2")):
            bn.weight.copy_(torch.from_numpy(c["g" + i]))
            bn.bias.copy_(torch.from_numpy(c["be" + i]))
            bn.running_mean.copy_(torch.from_numpy(c["rm" + i]))
            bn.running_var.copy_(torch.from_numpy(c["rv" + i]))
    return fusion.to(device=device, dtype=dtype), pred.to(device=device, dtype=dtype)


def module_tensors(fusion, pred):
    m, head = fusion.merge_layer, pred.pred_layer[0]
    params = {"w1": m[0].weight, "g1": m[1].weight, "be1": m[1].bias, "w2": m[3].weight, "g2": m[4].weight, "be2": m[4].bias,
              "w3": head.weight, "b3": head.bias}
    buffers = {"rm1": m[1].running_mean, "rv1": m[1].running_var, "rm2": m[4].running_mean, "rv2": m[4].running_var}
    return params, buffers


def case_tensors(c, dtype, device, grad=True):
    import torch
    xs = [torch.from_numpy(c[k]).to(device=device, dtype=dtype).requires_grad_(grad) for k in INPUTS]
    g = torch.from_numpy(c["g"]).to(device=device, dtype=dtype)
    keep = (torch.from_numpy(c["keep1"]).to(device), torch.from_numpy(c["keep2"]).to(device))
    return xs, g, keep


def collect(logits, xs, fusion, pred, c):
    """the results of one forward + backward as float64 numpy (None for a gradient that was not computed)"""
    params, buffers = module_tensors(fusion, pred)
    out = {"logits": logits.detach().double().cpu().numpy()}
    for k, x in zip(INPUTS, xs):
        out["d" + k] = None if x.grad is None else x.grad.detach().double().cpu().numpy()
    for k, p in params.items():
        out["d" + k] = None if p.grad is None else p.grad.detach().double().cpu().numpy().reshape(c[k].shape)
    for k, buf in buffers.items():
        out[k] = buf.detach().double().cpu().numpy()
    return out


def run_modules(c, training, dtype, device="cpu", modules=None, keep=None):
    """forward + backward through the real CatFusion / PredBranch modules with the masks applied by multiplication
    (``x * keep * 1.25`` in place of F.dropout): the module path with the op's masks -> (results, (fusion, pred))."""
    import torch
    fusion, pred = build_modules(c, dtype, device) if modules is None else modules
    fusion.train(training)
    pred.train(training)
    xs, g, own = case_tensors(c, dtype, device)
    k1, k2 = own if keep is None else keep
    x = torch.cat(xs, dim=1)
    if training:
        x = x * k1[..., None].to(dtype) * SCALE
    y = fusion.merge_layer(x)
    if training:
        y = y * k2[..., None].to(dtype) * SCALE
    logits = pred.pred_layer(y)
    logits.backward(g)
    return collect(logits, xs, fusion, pred, c), (fusion, pred)

"""Dev: the bf16 convolution kernel (csrc/conv_bf16.hip, the engine's conv_precision="bf16") against the fp32 kernel the engine
picks today (Winograd / 1-D Winograd / row-staging / implicit GEMM, as InferenceEngine._conv routes), for every layer of
tools/ubench_conv.py LAYERS at B = 4.  Prints ms, TFLOP/s and GB/s (fp32 activations in and out, weights) for both, the
bf16 / fp32 time ratio, and the bf16 kernel's error against float64 on the bf16-rounded operands (max |err| over max |ref|).

    python tools/ubench_conv_bf16.py [name-filter]
"""
import ast, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F
from streammos_amd import ops

dev = "cuda:0"
B = 4


def _layers():
    """LAYERS of tools/ubench_conv.py (read, not imported: that script runs its benchmark at import)"""
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ubench_conv.py")).read())
    node = next(n for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "LAYERS")
    return ast.literal_eval(node.value)


LAYERS = _layers()


def timeit(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def fp32_engine_conv(x, w, bias, cout, kh, kw, stride, b, ho, wo):
    """the launch InferenceEngine._conv issues in fp32 mode for this layer (default switches)"""
    cin = w.shape[1]
    if kh == 3 and kw == 3 and stride == 1:
        mb = ops.conv_wino_mb(cout)
        wp = ops.conv_wino_prepare(w, mb)
        return "wino", lambda: ops.conv_wino_cl(x, wp, bias, 1, cout, mb=mb)
    if ops.conv_wino1d_ok((kh, kw), stride, cin, cout):
        mb = ops.conv_wino_mb(cout)
        wp = ops.conv_wino1d_prepare(w, mb)
        return "wino1d", lambda: ops.conv_wino1d_cl(x, wp, bias, 1, cout, (kh, kw), mb=mb)
    mt = ops.conv_mt(cout, b * ho * wo)
    if mt <= 1 and ops.conv_rows_ok((kh, kw), stride, cin, cout) and kw >= 3:
        wp = ops.conv_prepare(w, mt, order="rows")
        return "rows", lambda: ops.conv_rows_cl(x, wp, bias, 1, cout, (kh, kw), mt=mt)
    wp = ops.conv_prepare(w, mt)
    return "igemm", lambda: ops.conv_cl(x, wp, bias, 1, cout, (kh, kw), stride=stride, mt=mt)


only = sys.argv[1] if len(sys.argv) > 1 else None
tot32 = tot16 = 0.0
print("%-18s %7s | %-6s %8s %6s %6s | %8s %6s %6s | %5s | %s" % ("layer", "GFLOP", "fp32", "ms", "TF/s", "GB/s", "bf16 ms", "TF/s",
                                                                "GB/s", "ratio", "bf16 err (max |err| / max |ref|)"))
for name, cin, cout, (kh, kw), stride, (h, w) in LAYERS:
    if only and only not in name:
        continue
    torch.manual_seed(0)
    x = torch.randn(B, h, w, cin, device=dev).permute(0, 3, 1, 2)
    wt = torch.randn(cout, cin, kh, kw, device=dev) / (cin * kh * kw) ** 0.5
    bias = torch.randn(cout, device=dev)
    pad = (kh // 2, kw // 2)
    ho, wo = (h + 2 * pad[0] - kh) // stride + 1, (w + 2 * pad[1] - kw) // stride + 1
    gf = 2.0 * B * ho * wo * cin * cout * kh * kw / 1e9
    gb32 = (B * h * w * cin * 4 + B * ho * wo * cout * 4 + wt.numel() * 4) / 1e9
    gb16 = (B * h * w * cin * 4 + B * ho * wo * cout * 4 + wt.numel() * 2) / 1e9
    kind, f32 = fp32_engine_conv(x, wt, bias, cout, kh, kw, stride, B, ho, wo)
    t32 = timeit(f32)
    wp16 = ops.conv_bf16_prepare(wt)
    t16 = timeit(lambda: ops.conv_bf16_cl(x, wp16, bias, 1, cout, (kh, kw), stride=stride))
    y = ops.conv_bf16_cl(x, wp16, bias, 1, cout, (kh, kw), stride=stride)
    ref = F.conv2d(x.to(torch.bfloat16).double(), wt.to(torch.bfloat16).double(), bias.double(), stride, pad).clamp_min(0)
    err = ((y.double() - ref).abs().max() / ref.abs().max()).item()
    tot32 += t32
    tot16 += t16
    print("%-18s %7.2f | %-6s %8.4f %6.1f %6.0f | %8.4f %6.1f %6.0f | %5.2f | %.2e" % (
        name, gf, kind, t32, gf / t32, gb32 / t32 * 1e3, t16, gf / t16, gb16 / t16 * 1e3, t16 / t32, err), flush=True)
print("sum over the layers: fp32 %.3f ms, bf16 %.3f ms (%.2fx)" % (tot32, tot16, tot32 / max(tot16, 1e-9)))

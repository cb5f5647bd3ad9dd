"""CPU side of the opt-in bf16 convolutions: the weight packing of ops.conv_bf16_prepare against an independent numpy
construction of the operand order include/smos.h documents, its rounding on crafted ties, and the precision switches of
the engine, the runners and run_sequence."""
import numpy as np
import pytest
import torch

from streammos_amd import engine, ops, run_sequence, streaming


def _bf16_rne(x32):
    """float32 -> bf16 bit patterns, round to nearest even, in integer arithmetic"""
    u = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_prepare_matches_documented_operand_order():
    rng = np.random.default_rng(0)
    for cout, cin, kh, kw in ((32, 32, 3, 3), (64, 32, 7, 3), (128, 64, 1, 1), (32, 64, 3, 5)):
        w = rng.standard_normal((cout, cin, kh, kw)).astype(np.float32)
        got = _bits(ops.conv_bf16_prepare(torch.from_numpy(w)))
        want = np.zeros(cout * cin * kh * kw, dtype=np.uint16)
        wb = _bf16_rne(w)
        nq = cout // 32
        for cc in range(cin // 32):
            for ky in range(kh):
                for kx in range(kw):
                    stage = (cc * kh + ky) * kw + kx
                    for q in range(nq):
                        for s in range(2):
                            for lane in range(64):
                                base = (((stage * nq + q) * 2 + s) * 64 + lane) * 8
                                m, h = lane & 31, lane >> 5
                                for j in range(8):
                                    want[base + j] = wb[q * 32 + m, cc * 32 + 16 * s + 8 * h + j, ky, kx]
        assert np.array_equal(got, want), (cout, cin, kh, kw)


def test_prepare_rounds_to_nearest_even():
    # 0x3F808000: a tie between 0x3F80 and 0x3F81 -> the even 0x3F80; 0x3F818000: a tie -> the even 0x3F82;
    # one ulp beside the ties (0x7FFF / 0x8001 low bits) rounds down / up; the sign does not change any of it
    pats = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000, 0x3F80FFFF]
    want = [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x3F81, 0x3F82, 0xBF80, 0xBF82, 0x3F81]
    vals = np.array(pats, dtype=np.uint32).view(np.float32)
    w = np.zeros((32, 32, 1, 1), dtype=np.float32)
    w[:len(vals), 0, 0, 0] = vals                     # q = 0, k-step 0, lane h = 0, j = 0: out channel m -> element 8 m
    got = _bits(ops.conv_bf16_prepare(torch.from_numpy(w)))
    assert [int(got[8 * m]) for m in range(len(vals))] == want
    assert np.array_equal(_bf16_rne(vals), np.array(want, dtype=np.uint16))


def test_prepare_refuses_ragged_channels():
    with pytest.raises(RuntimeError):
        ops.conv_bf16_prepare(torch.zeros(48, 32, 3, 3))


def test_support_predicate():
    x = torch.empty((4, 64, 128, 128), device="meta").contiguous(memory_format=torch.channels_last)
    assert ops.conv_bf16_ok(x, 64, (3, 3))
    assert ops.conv_bf16_ok(x, 64, (3, 3), stride=2)
    assert not ops.conv_bf16_ok(x, 48, (3, 3))                                      # Cout not a multiple of 32
    assert not ops.conv_bf16_ok(x, 64, (9, 9))
    big = torch.empty((16, 128, 512, 512), device="meta").contiguous(memory_format=torch.channels_last)
    assert not ops.conv_bf16_ok(big, 128, (3, 3))                                   # 2 GiB and more
    res = torch.empty((4, 64, 128, 128), device="meta").contiguous(memory_format=torch.channels_last)
    assert not ops.conv_bf16_ok(x, 64, (3, 3), residual=res, chan_sums=True)


def test_run_sequence_parser_conv_precision():
    ap = run_sequence.build_parser()
    args = ap.parse_args(["--seq-dir", "s", "--out-dir", "o"])
    assert args.conv_precision == "fp32"
    assert ap.parse_args(["--seq-dir", "s", "--out-dir", "o", "--conv-precision", "bf16"]).conv_precision == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_args(["--seq-dir", "s", "--out-dir", "o", "--conv-precision", "fp16"])


def test_unknown_precision_refused():
    class M:
        engine_conv_precision = "fp32"
    with pytest.raises(ValueError):
        streaming.set_conv_precision(M(), "fp16")
    m = M()
    streaming.set_conv_precision(m, None)
    assert m.engine_conv_precision == "fp32"
    streaming.set_conv_precision(m, "bf16")
    assert m.engine_conv_precision == "bf16"
    with pytest.raises(ValueError):
        engine.InferenceEngine(None, conv_precision="fp16")
    with pytest.raises(ValueError):
        engine.InferenceEngine(None, layout="nchw", conv_precision="bf16")


def test_removed_nchw_layout_refused_before_the_net_is_touched():
    """The NCHW engine is gone: any layout but "cl" is refused at default precision too, and before the constructor
    reads anything from net (None here)."""
    with pytest.raises(ValueError) as err:
        engine.InferenceEngine(None, layout="nchw")
    assert "cl" in str(err.value) and "nchw" in str(err.value)


def test_model_attribute_default():
    from streammos_amd.refapi.config import StreamMOS as cfg
    from streammos_amd.refapi.models import StreamMOS
    assert StreamMOS.AttNet(cfg.get_config()[2]).engine_conv_precision == "fp32"

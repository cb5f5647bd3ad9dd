"""The 3-limb bf16 form of the decoder's tap products (csrc/tap_bf16x3.hip), host side: the weight split and its stream order
(ops.tap_limbs_pack), and a numpy emulation of the kernel's arithmetic against the bound the fp32 form is held to
(tests/util.py::tap_products_bound) -- the derivation's check, independent of any GPU.

The emulation: limbs by round-to-nearest-even; per 16-wide k block the six limb products hh, hm, mh, hl, lh, mm of every term,
each exact, summed exactly (float64 holds them: 16-bit products, 6 x 16 of them); ONE fp32 rounding per accumulated block, eight
blocks chained.  The hardware rounds more often inside a block (48 instructions of 16 terms); the bound's budget for that is
part of the derivation in the kernel's header, not of this emulation.
"""
import numpy as np
import torch

from streammos_amd import ops
from tests import util


def _bf16_representable(t):
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


def _weight_sets():
    rng = np.random.default_rng(util._seed("tap_bf16x3/pack"))
    sets = {
        "random": rng.standard_normal((1152, 128)) * 0.05,
        "exact k/64": rng.integers(-64, 65, (100, 128)) / 64.0,
        "powers of two": np.tile(2.0 ** np.arange(-40, 41), 128)[:81 * 128].reshape(81, 128) * rng.choice([-1.0, 1.0], (81, 128)),
        "all 24 bits set": np.ldexp(float(2 ** 24 - 1), rng.integers(-60, 40, (36, 128))) * rng.choice([-1.0, 1.0], (36, 128)),
        "signed zeros": np.where(rng.random((4, 128)) < 0.5, 0.0, -0.0),
        "one row": rng.standard_normal((1, 128)),
    }
    return {k: torch.tensor(v.astype(np.float32)) for k, v in sets.items()}


def test_tap_limbs_pack_splits_exactly_and_unpacks_to_the_weights():
    for name, w in _weight_sets().items():
        cout = w.shape[0]
        assert torch.equal(w.double().float(), w)
        lo, mid, hi = ops.tap_limbs_split(w)
        for limb in (lo, mid, hi):
            assert limb.dtype == torch.bfloat16 and _bf16_representable(limb), name
        assert torch.equal(hi.double() + mid.double() + lo.double(), w.double()), name          # exact, compared in float64
        stream = ops.tap_limbs_pack(w)
        pad = (cout + 31) // 32 * 32
        assert stream.dtype == torch.bfloat16 and stream.numel() == 3 * pad * 128 and stream.is_contiguous(), name
        ulo, umid, uhi = ops.tap_limbs_unpack(stream, cout)
        assert torch.equal(uhi, hi.float()) and torch.equal(umid, mid.float()) and torch.equal(ulo, lo.float()), name
        got = uhi.double() + umid.double() + ulo.double()
        assert torch.equal(got, w.double()), name
        if name == "signed zeros":
            assert torch.equal(torch.signbit(uhi), torch.signbit(w))
        # the rows past cout are zero, and the stream order is the documented one (include/smos.h)
        s6 = stream.reshape(pad // 32, 8, 3, 64, 8).float()
        for index, limb in enumerate((lo, mid, hi)):                 # every limb by the documented formula, not by the inverse
            full = torch.zeros((pad, 128))
            full[:cout] = limb.float()
            for lane in (0, 5, 31, 32, 44, 63):
                r, h = lane & 31, lane >> 5
                for tile in {0, pad // 32 - 1}:
                    for step in (0, 3, 7):
                        want = full[32 * tile + r, 16 * step + 8 * h:16 * step + 8 * h + 8]
                        assert torch.equal(s6[tile, step, index, lane], want), (name, index, lane)


def test_tap_limbs_pack_refuses_other_shapes():
    import pytest
    with pytest.raises(RuntimeError, match="tap_limbs_pack"):
        ops.tap_limbs_pack(torch.zeros(8, 64))
    with pytest.raises(RuntimeError, match="tap_limbs_pack"):
        ops.tap_limbs_pack(torch.zeros(2052, 128))


def _limbs_np(v):
    lo, mid, hi = ops.tap_limbs_split(torch.tensor(v.astype(np.float32)))
    return tuple(t.double().numpy() for t in (hi, mid, lo))


def _emulate(x, w, products):
    """products: pairs (x limb, w limb) summed per 16-wide k block, one fp32 rounding per accumulated block."""
    xl, wl = _limbs_np(x), _limbs_np(w)
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    for k0 in range(0, x.shape[1], 16):
        block = np.zeros(acc.shape)
        for i, j in products:
            block += xl[i][:, k0:k0 + 16] @ wl[j][:, k0:k0 + 16].T
        acc = (acc.astype(np.float64) + block).astype(np.float32)
    return acc


def test_numpy_emulation_of_the_limb_sum_stays_inside_the_fp32_bound():
    rng = np.random.default_rng(util._seed("tap_bf16x3/emulation"))
    x = (3.0 * np.maximum(rng.standard_normal((256, 128)), 0.0)).astype(np.float32).astype(np.float64)
    w = (0.05 * rng.standard_normal((1152, 128))).astype(np.float32).astype(np.float64)
    xs, ws = _limbs_np(x), _limbs_np(w)
    assert np.array_equal(xs[0] + xs[1] + xs[2], x) and np.array_equal(ws[0] + ws[1] + ws[2], w)
    want, bound = util.tap_products_ref(x, w), util.tap_products_bound(x, w)
    six = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]
    nine = [(i, j) for i in range(3) for j in range(3)]
    worst = {}
    for name, products in (("6 limb products", six), ("9 limb products", nine)):
        ok, ratio = util.msda_worst_ratio(_emulate(x, w, products), want, bound)
        worst[name] = ratio
        print("tap-bf16x3-ratio emulation %-18s %.4f" % (name, ratio))
        assert ok, "%s: worst error / bound = %g" % (name, ratio)
    # the three dropped products are below one fp32 rounding per term: the six-product sum is as good as the nine-product one
    assert worst["6 limb products"] <= worst["9 limb products"] + 2.0 / 128

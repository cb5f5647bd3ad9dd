"""Every kernel path of csrc/msda.hip against a float64 reference, element by element, inside derived bounds.

Kernels and what reaches them here:
  msda_fwd_d32            float32, D == 32, L*P <= 8          the d32_* forward cases and border_d32 in float32
  msda_fwd_heads<float>   every other float32 forward          d32_lp9_generic, g_*, border_d5 in float32
  msda_fwd_heads<double>  float64 forward                      every forward case in float64
  msda_fwd_qp_d32         the inference engine's sampler       qp_*
  msda_bwd<T, 32>         D <= 32                              bwd_d1, bwd_d5_odd_heads, bwd_d32, bwd_d32_second_sweep
  msda_bwd<T, 64>         D > 32                               bwd_d33 .. bwd_d130, bwd_d33_second_sweep

References (tests/util.py, checked on the host by tests/test_host_msda_reference.py): oracle.ops_np.msda_forward in float64
for the forward, float64 CPU autograd through ms_deform_attn_core_pytorch for the backward.  All coordinates are dyadic,
so both precisions sample the same points and the only error left is the rounding of the accumulation.  With eps = 2^-24
(float32) or 2^-53 (float64), per element:
  forward     (4 L P + 2) eps A                      A = the oracle on |value|, |attn|
  qp forward  (4 P + 2 + 32 + 2 max|logit|) eps A    + 8 eps max(H, W) max|value| where H or W is no power of two
  grad_value  4 Lq L P eps G                         G = reference grad_value for |grad_out|, |attn|
  grad_attn   5 D eps R                              R = reference grad_attn for |grad_out|, |value|
  grad_loc    (4 D + 8) eps size_l |attn| 4 max|value| sum_c |grad_out_c|
The float64 runs pin the logic (a wrong corner, a dropped sample chunk or a lost lane is many orders above the bound), the
float32 runs the dispatch and the float-only kernels.  Every test prints its worst error / bound (pytest -s); the figures
of the MI355X run are kept in profiles/msda_error_ratios.txt.
"""
import numpy as np
import pytest
import torch

from streammos_amd import ops
from streammos_amd.refapi.deformattn.functions import MSDeformAttnFunction
from tests import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = ["float32", "float64"]
_FWD = sorted(util.MSDA_FWD_CASES) + sorted(util.MSDA_BORDER_CASES)


def _t(a, dtype="float64"):
    a = np.asarray(a)
    return torch.tensor(a if a.dtype == np.int64 else a.astype(dtype), device=DEV)


def _problem(c, dtype):
    return _t(c.value, dtype), _t(c.shapes), _t(c.lsi), _t(c.loc, dtype), _t(c.attn, dtype)


def _binding(kind):
    """The extension module under the reference's name: the ctypes-backed one or the compiled pybind11 twin."""
    if kind == "pybind":
        from streammos_amd.refapi import compiled
        return compiled.load("MultiScaleDeformableAttention")
    from streammos_amd.refapi import MultiScaleDeformableAttention
    return MultiScaleDeformableAttention


def _check(label, got, want, bound):
    assert tuple(got.shape) == tuple(want.shape), (label, got.shape, want.shape)
    ok, ratio = util.msda_worst_ratio(got.cpu().numpy(), want, bound)
    print("msda-ratio %-58s %.4f" % (label, ratio))
    assert ok, "%s: worst error / bound = %g" % (label, ratio)


# ------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _FWD)
def test_msda_forward_against_float64_oracle(name, dtype):
    c = util.msda_any_fwd_case(name)
    got = ops.msda_fwd(*_problem(c, dtype))
    assert got.dtype == getattr(torch, dtype)
    _check("fwd %s %s" % (name, dtype), got, c.want, util.msda_forward_bound(c, dtype))


def test_msda_d32_and_generic_kernel_give_the_same_answer_across_the_dispatch_bound():
    """The L*P = 8 problem of msda_fwd_d32 with a fifth point of weight 0 per level is an L*P = 10 problem of
    msda_fwd_heads<float> with the same answer: the extra term is an exact 0, so the L*P = 8 bound still holds."""
    c = util.msda_fwd_case("d32_lp8_two_levels")
    value, shapes, lsi, loc, attn = _problem(c, "float32")
    loc10 = torch.cat((loc, torch.full_like(loc[..., :1, :], 0.5)), -2).contiguous()
    attn10 = torch.cat((attn, torch.zeros_like(attn[..., :1])), -1).contiguous()
    assert loc10.shape[3] * loc10.shape[4] == 10 and value.shape[3] == 32
    fast, slow = ops.msda_fwd(value, shapes, lsi, loc, attn), ops.msda_fwd(value, shapes, lsi, loc10, attn10)
    bound = util.msda_forward_bound(c, "float32")
    _check("fwd d32_lp8_two_levels float32 d32 kernel", fast, c.want, bound)
    _check("fwd d32_lp8_two_levels float32 padded to L*P = 10", slow, c.want, bound)


@pytest.mark.parametrize("binding", ["function", "ctypes", "pybind"])
@pytest.mark.parametrize("name", ["d32_lp8_two_levels", "g_d33_lp9"])
def test_msda_forward_through_the_bindings(name, binding):
    c = util.msda_fwd_case(name)
    args = _problem(c, "float32")
    if binding == "function":
        got = MSDeformAttnFunction.apply(*args, 2)
    else:
        got = _binding(binding).ms_deform_attn_forward(*args, 2)
    _check("fwd %s float32 via %s" % (name, binding), got, c.want, util.msda_forward_bound(c, "float32"))


@pytest.mark.parametrize("name", sorted(util.MSDA_QP_CASES))
def test_msda_fwd_qp_against_float64_oracle(name):
    """softmax, off / (W, H) and the cell-centre reference points in float64, then the oracle.  (This entry point builds its
    weights itself, so it has no signed-weights case; qp_8x8_m3_p4_logits30 drives the softmax to its ends instead.)"""
    c = util.msda_qp_case(name)
    got = ops.msda_fwd_qp(_t(c.value, "float32"), _t(c.qp, "float32"), c.h, c.w, c.p)
    _check("qp %s" % name, got, c.want, util.msda_qp_bound(c))


# ------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------
def _check_grads(label, c, dtype, grads):
    wants = (c.want_value, c.want_loc, c.want_attn)
    for what, got, want, bound in zip(("grad_value", "grad_loc", "grad_attn"), grads, wants, util.msda_backward_bounds(c, dtype)):
        _check("%s %s" % (label, what), got, want, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(util.MSDA_BWD_CASES))
def test_msda_backward_against_float64_autograd(name, dtype):
    c = util.msda_bwd_case(name)
    grads = ops.msda_bwd(*_problem(c, dtype), _t(c.grad_out, dtype))
    assert all(g.dtype == getattr(torch, dtype) for g in grads)
    _check_grads("bwd %s %s" % (name, dtype), c, dtype, grads)


@pytest.mark.parametrize("binding", ["function", "ctypes", "pybind"])
@pytest.mark.parametrize("name", ["bwd_d32", "bwd_d71"])
def test_msda_backward_through_the_bindings(name, binding):
    c = util.msda_bwd_case(name)
    value, shapes, lsi, loc, attn = _problem(c, "float32")
    grad_out = _t(c.grad_out, "float32")
    if binding == "function":
        value, loc, attn = (t.requires_grad_(True) for t in (value, loc, attn))
        MSDeformAttnFunction.apply(value, shapes, lsi, loc, attn, 2).backward(grad_out)
        grads = (value.grad, loc.grad, attn.grad)
    else:
        grads = _binding(binding).ms_deform_attn_backward(value, shapes, lsi, loc, attn, grad_out, 2)
        assert len(grads) == 3
    _check_grads("bwd %s float32 via %s" % (name, binding), c, "float32", grads)


@pytest.mark.parametrize("binding", ["ctypes", "pybind"])
def test_msda_backward_does_not_accumulate_across_calls(binding):
    """grad_value is built with atomic adds into a buffer the call itself has to clear: a second call gives the same three
    gradients (each inside its bound; grad_loc and grad_attn, which no atomic touches, bit for bit), not twice them."""
    c = util.msda_bwd_case("bwd_d33")
    args = _problem(c, "float32") + (_t(c.grad_out, "float32"),)
    if binding == "pybind":
        MSDA = _binding(binding)
        call = lambda: MSDA.ms_deform_attn_backward(*args, 2)
    else:
        call = lambda: ops.msda_bwd(*args)
    first = [g.clone() for g in call()]
    second = call()
    _check_grads("bwd bwd_d33 float32 %s first call" % binding, c, "float32", first)
    _check_grads("bwd bwd_d33 float32 %s second call" % binding, c, "float32", second)
    assert torch.equal(first[1], second[1]) and torch.equal(first[2], second[2])

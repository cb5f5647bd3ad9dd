"""tests/tfusion_cases.py without a GPU: the float64 reference against torch.nn.functional in float64, the exact twins of the
projection cases, the instrument (the RMS comparison per row group) measured between the two float32 restatements, the mutants
of the reference against both bars on the groups built for them, and the restated weight stream / parameter block against
ops.TfusionLayer and ops.tfusion_pack_linear on CPU tensors.  Run with -s for the margin figures and the mutant table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tfusion_cases as cases

LAYER = sorted(cases.LAYER_SPECS)
ALN = sorted(cases.ALN_SPECS)


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("name", LAYER)
def test_layer_reference_equals_torch_float64(name):
    c = cases.layer_case(name)
    q1 = F.layer_norm(_t(c.query) + F.linear(_t(c.sampled), _t(c.wo), _t(c.bo)), (128,), _t(c.g1), _t(c.be1), c.eps[0])
    hid = F.relu(F.linear(q1, _t(c.w1), _t(c.b1)))
    want = F.layer_norm(q1 + F.linear(hid, _t(c.w2), _t(c.b2)), (128,), _t(c.g2), _t(c.be2), c.eps[1])
    assert c.ref.shape == (c.tokens, 128)
    assert np.abs(c.ref - want.numpy()).max() <= 1e-10 * np.abs(want.numpy()).max()
    if c.nq:
        want_q = F.linear(want, _t(c.wq), _t(c.bq)).numpy()
        assert c.ref_next.shape == (c.tokens, c.nq) and np.abs(c.ref_next - want_q).max() <= 1e-10 * np.abs(want_q).max()
    else:
        assert c.ref_next is None
    if c.hot is not None:
        # item 4: only hidden tile j* is alive in the reference
        q1n = cases.layer_norm_ref(c.query + c.sampled @ c.wo.T + c.bo, c.g1, c.be1, c.eps[0])
        h = cases.hidden_ref(c, q1n)
        live = np.zeros(c.ffn, dtype=bool)
        live[16 * c.hot:16 * c.hot + 16] = True
        assert not h[:, ~live].any() and (h[:, live] > 0).mean() > 0.25
    if "const" in c.rows:
        rows = c.ref[c.rows["const"]]
        assert np.abs(rows - rows[0]).max() <= 1e-11          # (a float64 BLAS may round the rows of one product differently; norm2 magnifies that ~1e3 times)


@pytest.mark.parametrize("name", ALN)
def test_add_layer_norm_reference_equals_torch_float64(name):
    c = cases.aln_case(name)
    x = _t(c.x) if c.res is None else _t(c.x) + _t(c.res)
    want = F.layer_norm(x, (c.ch,), _t(c.g), _t(c.b), c.eps).numpy()
    assert np.abs(c.ref - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("name", cases.PROJECT_NAMES)
def test_project_reference_and_exact_twins(name):
    """The reference equals F.linear in float64; on the exact twins both float32 restatements equal float32(reference) bit for
    bit; on the random ones the kernel-order restatement is inside the derived bound."""
    for j in cases.project_case(name):
        want = F.linear(_t(j.x), _t(j.w), None if j.b is None else _t(j.b)).numpy()
        assert np.abs(j.ref - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
        a, b = cases.project_f32(j.x, j.w, j.b), cases.project_f32_plain(j.x, j.w, j.b)
        if j.exact:
            assert np.array_equal(a, j.ref.astype(np.float32)) and np.array_equal(b, j.ref.astype(np.float32))
        else:
            assert (np.abs(a.astype(np.float64) - j.ref) <= cases.project_bound(j)).all()
            assert (np.abs(b.astype(np.float64) - j.ref) <= cases.project_bound(j)).all()


def _layer_margins(name):
    """-> [(group, which, rms ratio, max ratio)] of the second restatement against the kernel-order one"""
    c = cases.layer_case(name)
    out, nxt = cases.layer_restatement(name)
    out2, nxt2 = cases.layer_f32_plain(c)
    res = []
    for g, rows in c.rows.items():
        res.append((g, "out") + cases.figures(out2, c.ref, out, rows))
        if c.nq:
            res.append((g, "qp_next") + cases.figures(nxt2, c.ref_next, nxt, rows))
    return res


def _aln_margins(name):
    c = cases.aln_case(name)
    a, b = cases.aln_f32(c), cases.aln_f32_plain(c)
    return [(g, "out") + cases.figures(b, c.ref, a, rows) for g, rows in c.rows.items()]


def test_the_instrument_between_the_two_restatements():
    """RMS(second restatement - ref) / RMS(kernel-order restatement - ref) <= RMS_FACTOR on every case and row group, and
    MAX_FACTOR = the worst max|second restatement - ref| / RMS(kernel-order restatement - ref), doubled, rounded up to a power of
    two.  Measured between two references, never against a kernel."""
    worst_rms, worst_max = (0.0, None), (0.0, None)
    for kind, names, fn in (("layer", LAYER, _layer_margins), ("aln", ALN, _aln_margins)):
        for name in names:
            for g, which, r, m in fn(name):
                print("tfusion-margin %-5s %-16s %-14s %-8s rms %.3f  max %.2f" % (kind, name, g, which, r, m))
                assert r <= cases.RMS_FACTOR, (kind, name, g, which, r)
                worst_rms = max(worst_rms, (r, (kind, name, g, which)))
                worst_max = max(worst_max, (m, (kind, name, g, which)))
    print("tfusion-margin worst rms ratio %.3f %s; worst max ratio %.2f %s" % (worst_rms + worst_max))
    want = 2.0 ** np.ceil(np.log2(2.0 * worst_max[0]))
    assert cases.MAX_FACTOR == want, (cases.MAX_FACTOR, want, worst_max)


STEERED = [n for n in LAYER if cases.LAYER_SPECS[n]["groups"] == cases.GROUPS and cases.LAYER_SPECS[n]["eps"] == cases.EPS_STEERED]
HOT = [n for n in LAYER if cases.LAYER_SPECS[n]["hot"] is not None]


def _mutant_out(c, mutant):
    if mutant == "one_pass":
        return cases.layer_f32_plain(c, one_pass=True)
    return cases.layer_ref(c, mutant=mutant)


@pytest.mark.parametrize("mutant", sorted(cases.LAYER_MUTANTS))
def test_every_layer_mutant_exceeds_both_bars_on_its_group(mutant):
    """Items 1, 2 and 4: a swapped eps, one eps for both norms, eps = 1e-5 whatever was passed, a one-pass float32 variance, b1
    read one hidden tile late and a hidden tile meeting a neighbour's W2 k-tile each exceed RMS_FACTOR and MAX_FACTOR on the
    group built for them by a factor of at least MUTANT_MARGIN, on every steered case (the tile mutants: also on every one-hot
    case).  The groups on which a mutant stays inside both bars are printed: that is why the groups are judged separately."""
    target = cases.LAYER_MUTANTS[mutant]
    names = STEERED + (HOT if mutant in ("b1_late", "w2_shift_up", "w2_shift_down") else [])
    for name in names:
        c = cases.layer_case(name)
        rest, _ = cases.layer_restatement(name)
        got, _ = _mutant_out(c, mutant)
        for g, rows in c.rows.items():
            r, m = cases.figures(got, c.ref, rest, rows)
            seen = r > cases.RMS_FACTOR or m > cases.MAX_FACTOR
            print("tfusion-mutant %-14s %-16s %-14s rms %.3g  max %.3g%s" % (mutant, name, g, r, m, "" if seen else "   INVISIBLE"))
            if g == target:
                assert r >= cases.MUTANT_MARGIN * cases.RMS_FACTOR and m >= cases.MUTANT_MARGIN * cases.MAX_FACTOR, (mutant, name, g, r, m)


def test_model_eps_case_cannot_tell_the_eps_apart():
    """Item 1, the other way round: with both eps at the model's 1e-5 the eps mutants return the reference itself."""
    c = cases.layer_case("f512_model_eps")
    for mutant in ("eps_swapped", "eps_one", "eps_1e5"):
        assert np.array_equal(cases.layer_ref(c, mutant=mutant)[0], c.ref)


@pytest.mark.parametrize("mutant", sorted(cases.ALN_MUTANTS))
def test_every_add_layer_norm_mutant_exceeds_both_bars_on_its_group(mutant):
    target = cases.ALN_MUTANTS[mutant]
    for name in ALN:
        c = cases.aln_case(name)
        if target not in c.rows:
            continue
        rest = cases.aln_f32(c)
        got = cases.aln_f32_plain(c, one_pass=True) if mutant == "one_pass" else cases.aln_ref(c, mutant)
        for g, rows in c.rows.items():
            r, m = cases.figures(got, c.ref, rest, rows)
            seen = r > cases.RMS_FACTOR or m > cases.MAX_FACTOR
            print("tfusion-mutant aln/%-10s %-16s %-14s rms %.3g  max %.3g%s" % (mutant, name, g, r, m, "" if seen else "   INVISIBLE"))
            if g == target:
                assert r >= cases.MUTANT_MARGIN * cases.RMS_FACTOR and m >= cases.MUTANT_MARGIN * cases.MAX_FACTOR, (mutant, name, g, r, m)


def test_restated_stream_and_parameter_block_equal_ops_on_cpu_tensors():
    """The order of the weight stream and of the parameter block restated from the header of csrc/tfusion.hip equals
    ops.TfusionLayer(...).stream / .params and ops.tfusion_pack_linear bit for bit (CPU tensors; the shared library is only asked
    for the two sizes).  The mutant `rows of Wq / bq beyond nq not zero` changes no stored output -- the store guard of qp_next
    cuts those channels -- so this comparison is what holds the zero padding."""
    from streammos_amd import ops
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    for name in ("f32", "f64", "f96", "f512", "f1248", "hot_f96_j4", "t17"):
        c = cases.layer_case(name)
        prep = ops.TfusionLayer((f(c.wo), f(c.bo)), (f(c.g1), f(c.be1), c.eps[0]), (f(c.w1), f(c.b1)), (f(c.w2), f(c.b2)),
                                (f(c.g2), f(c.be2), c.eps[1]), next_qproj=(f(c.wq), f(c.bq)) if c.nq else None)
        stream, params = cases.layer_stream(c), cases.layer_params(c)
        assert stream.size == cases.stream_slot_count(c.ffn, c.nq) * 8 * 64 * 4 and params.size == 6 * 128 + c.ffn + 64
        assert np.array_equal(prep.stream.numpy().view(np.uint32), stream.view(np.uint32))
        assert np.array_equal(prep.params.numpy().view(np.uint32), params.view(np.uint32))
        assert (prep.eps1, prep.eps2, prep.ffn, prep.nq) == (c.eps[0], c.eps[1], c.ffn, c.nq)
        if 0 < c.nq < 64:
            assert not np.array_equal(cases.layer_stream(c, wq_tail=1.0), stream)
            assert not np.array_equal(cases.layer_params(c, bq_tail=1.0), params)
    for j in cases.project_case("cout6"):
        assert np.array_equal(ops.tfusion_pack_linear(f(j.w)).numpy().view(np.uint32), cases.project_stream(j.w).view(np.uint32))


def test_case_tables_cover_what_they_are_named_for():
    """Items 3 - 7 as data: the parameter rounds (2048 floats each) change over between ffn 1216 / 1248 and 3264 / 3296; ffn 32
    has two hidden tiles and 96 six; every token count and every cout of the issue occurs."""
    rounds = {f: -(-(6 * 128 + f + 64) // 2048) for f in (32, 512, 1216, 1248, 3264, 3296, 4096)}
    assert rounds == {32: 1, 512: 1, 1216: 1, 1248: 2, 3264: 2, 3296: 3, 4096: 3}
    assert all("f%d" % f in cases.LAYER_SPECS for f in (32, 64, 96, 512, 1216, 1248, 3264, 3296, 4096))
    assert {cases.layer_case("t%d" % t).tokens for t in cases.TOKEN_COUNTS} == set(cases.TOKEN_COUNTS)
    assert {cases.LAYER_SPECS[n]["nq"] for n in cases.LAYER_SPECS} >= {0, 4, 20, 48, 64}
    assert any(s["qpitch"] and s["opitch"] for s in cases.LAYER_SPECS.values())
    jobs = [j for n in cases.PROJECT_SPECS for j in cases.PROJECT_SPECS[n]]
    assert {j["cout"] for j in jobs} >= {4, 20, 48, 100, 128, 2048} and {j["tokens"] for j in jobs} >= set(cases.TOKEN_COUNTS)
    assert len(cases.PROJECT_SPECS["tok8"]) == 8 and {j["bias"] for j in cases.PROJECT_SPECS["tok8"]} == {True, False}
    assert {cases.aln_case(n).n for n in cases.ALN_SPECS} >= {1, 3, 4, 5, 1000}


def test_chain_reference_is_well_posed():
    """The float32 chain of the five launches stays close to the float64 one (item: the contracts between the kernels)."""
    a, b = cases.chain_run(np.float64), cases.chain_run(np.float32)
    assert a.shape == (84, 128) and np.isfinite(a).all()
    print("tfusion-chain float32 chain against float64: rms %.3g of rms %.3g" % (cases.rms(b - a), cases.rms(a)))
    assert cases.rms(b - a) <= 1e-4 * cases.rms(a)

"""Host restatement of the copy-paste augmentation (streammos_amd.preprocess.copy_paste_sample) against the reference's own run
(tests/golden/copy_paste.npz, written by tests/golden/make_copy_paste_golden.py)."""
import numpy as np
import pytest

from streammos_amd import kitti, preprocess

from . import copy_paste_cases as cc
from . import train_prep_cases as tc

SPEC = preprocess.VoxelSpec()


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden("copy_paste")
    return cc.fixture_sample(g), g


def test_twin_matches_reference(fixture):
    s, g = fixture
    bad, ratios = cc.compare_with_reference(s["out_scans"], s["out_words"], s["status"], s, g)
    print(bad, dict((i, float(r.max())) for i, r in ratios.items()))
    assert all(v == 0 for v in bad.values()), bad
    assert tuple(g["status"]) == cc.EXPECTED
    assert sorted(ratios) == [i for i, st in enumerate(cc.EXPECTED) if st >= 0]
    # per element: |dz| <= lifts * ((ceil(log2 12) + 2) 2^-24 max|z_road| + 2^-22), cc.z_bound
    for i, r in ratios.items():
        assert float(r.max()) <= 1.0, (i, float(r.max()))


def test_stage_two_labels(fixture):
    """copy_paste_seg.py appends label 2 to the second label list for every pasted point."""
    s, g = fixture
    for k in range(5):
        assert g["tail_bf_%d" % k].shape == g["tail_label_%d" % k].shape and (g["tail_bf_%d" % k] == 2).all()
    assert set(np.concatenate([g["tail_label_%d" % k] for k in range(5)]).tolist()) == {0, 1, 2}


@pytest.mark.parametrize("variant", preprocess.PASTE_VARIANTS)
def test_mutants_of_the_twin_change_the_comparison(fixture, variant):
    s, g = fixture
    scans, words, status = preprocess.copy_paste_sample(s["aligned"], s["words"], s["road"], s["bank"], s["draws"], cc.LABEL_BASE,
                                                        variant=variant)
    bad, _ = cc.compare_with_reference(scans, words, status, s, g)
    print(variant, bad)
    assert any(v != 0 for v in bad.values())


def test_fixed_length_layout_feeds_the_sample_builder(fixture):
    """The padding rows drop out in the builder's range filter: the sample built from the fixed-length layout equals the sample
    built from the arrays the reference leaves behind."""
    s, g = fixture
    maps, base = preprocess.paste_label_maps(tc.label_maps(two=True), {"pcds_target": (0, 1, 2), "pcds_bf_target": (2, 2, 2)})
    assert base == cc.LABEL_BASE
    draws = tc.explicit_draws(tc.FIXTURE_N, 515)
    ref_scans, ref_words = cc.reference_arrays(s, g)
    got = preprocess.build_train_sample(s["out_scans"], s["out_words"], s["poses"], tc.FIXTURE_N, SPEC, preprocess.AugParam(), draws,
                                        label_maps=maps, aligned=True)
    want = preprocess.build_train_sample(ref_scans, ref_words, s["poses"], tc.FIXTURE_N, SPEC, preprocess.AugParam(), draws,
                                         label_maps=maps, aligned=True)
    assert sorted(got) == sorted(want)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    # pasted points reach the targets: the plain maps would have sent their words to 0
    plain = preprocess.build_train_sample(s["out_scans"], s["out_words"], s["poses"], tc.FIXTURE_N, SPEC, preprocess.AugParam(),
                                          draws, label_maps=tc.label_maps(two=True), aligned=True)
    assert any(not np.array_equal(plain["pcds_bf_target_%d" % w], got["pcds_bf_target_%d" % w]) for w in range(3))


def test_paste_label_maps():
    maps, base = preprocess.paste_label_maps({"a": np.arange(5), "b": np.arange(3)}, {"a": (0, 1, 2), "b": (2, 2, 2)})
    assert base == 5 and maps["a"].tolist() == [0, 1, 2, 3, 4, 0, 1, 2] and maps["b"].tolist() == [0, 1, 2, 0, 0, 2, 2, 2]
    with pytest.raises(ValueError):
        preprocess.paste_label_maps({"a": np.arange(5)}, {"b": (0, 1, 2)})


def test_seeded_scalars_are_draws():
    cats = [[0], [], [1, 2], [], [], [3], [], []]
    seen = set()
    for index in range(40):
        idx, vel, order = preprocess.seeded_paste_scalars(11, index, cats)
        assert len(idx) == len(vel) == order.shape[0] <= preprocess.PASTE_MAX_OBJECTS
        seen.add(len(idx))
        for i, v, o in zip(idx, vel, order):
            assert i in (0, 1, 2, 3) and sorted(o.tolist()) == list(range(20))
            lo, hi = preprocess.PASTE_VELOCITY[preprocess.PASTE_CATEGORIES[[c for c in range(8) if i in cats[c]][0]]]
            assert lo <= v <= hi
    assert len(seen) > 5
    a, b = preprocess.seeded_paste_scalars(11, 3, cats), preprocess.seeded_paste_scalars(11, 3, cats)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    noise = preprocess.seeded_paste_noise(11, 3, 2, 500)
    assert noise.shape == (5, 500, 3) and abs(noise.std() - preprocess.PASTE_NOISE_STD) < 1e-4

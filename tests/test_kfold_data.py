"""CPU checks of the K-fold sweep's test cases (tests/kfold.py): every case
holds queries whose label the reference's order among equal distances decides
(the sweep tie scan queues them: KNN_FLAG_TIE_REF), and queries whose nearest
rows lie in their own fold -- without those, holding the fold out would change
nothing and a build that ignored the folds would pass.  No GPU."""
import numpy as np
import pytest

import kfold


@pytest.mark.parametrize("name", kfold.CASES)
def test_case_shape(name):
    s = kfold.case(name)
    sizes = np.bincount(s["folds"], minlength=s["F"])
    assert sizes.min() >= 1 and sizes.max() == s["fold_max"] and len(sizes) == s["F"]
    assert max(s["ks"]) <= s["n"] - s["fold_max"]


@pytest.mark.parametrize("name", kfold.CASES)
def test_ties_and_own_fold_neighbours(name):
    w = kfold.expected(name)
    nv = w["naive"]
    assert nv["queued"].any(), "no query the reference's tie order is consulted for"
    assert nv["tied"].sum() > nv["queued"].sum(), "\"ties\" = 2 re-orders more rows than 1"
    assert kfold.nearest_in_own_fold(name).any(), "no query whose nearest row is in its fold"


def test_the_order_decides_labels_somewhere():
    """On the large cases the (dist, index) order and the reference's order
    give different labels for some row: "ties" = 0 and 1 are told apart."""
    assert any(kfold.expected(n)["sensitive"].any() for n in ("inter_l2", "inter_l1", "unequal"))


def test_small_case_has_padded_lists():
    s = kfold.case("small")
    assert np.bincount(s["folds"]).min() < max(s["ks"]) + 1


def test_dups_case_keeps_distance_zero_neighbours():
    w = kfold.expected("dups")
    s = kfold.case("dups")
    assert (w["dist"][:, 0] == 0.0).all()
    assert (s["folds"][w["idx"][:, 0]] != s["folds"]).all()

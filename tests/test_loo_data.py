"""CPU checks of the leave-one-out test data (tests/loo.py): the data sets
hold enough rows whose label only the reference's std::sort order over the
n - 1 REMAINING records gives, and enough rows in drop case two, that a GPU
pass of test_gpu_loo.py cannot be vacuous.  The floors are about half the
counts measured with the oracle (A: 694 order-sensitive rows, 14 rows with an
exact duplicate, none in case two; A1: 1090; B: 440 and 153 in case two).
No GPU calls are made."""
import numpy as np
import pytest

import loo


@pytest.mark.parametrize("name,floor,case2_floor", [("A", 350, 0), ("A1", 500, 0), ("B", 200, 75)])
def test_order_sensitive_rows(name, floor, case2_floor):
    w = loo.expected_loo(name)
    sens = int(w["sensitive"].sum())
    case2 = int(w["naive"]["case2"].sum())
    print("%s: %d order-sensitive rows, %d in drop case two" % (name, sens, case2))
    assert sens >= floor
    assert case2 >= case2_floor


def test_set_a_has_duplicates_but_no_case_two():
    tr, _ = loo.data("A")
    assert loo.duplicates(tr).sum() >= 2
    assert not loo.expected_loo("A")["naive"]["case2"].any()


@pytest.mark.parametrize("name", ["A", "A1", "B"])
def test_expected_values_are_consistent(name):
    """No row is its own neighbour; the oracle's and the (dist, index) rows
    hold the same distances; every order-sensitive row is one the "ties" = 1
    rule hands to the reference-order pass."""
    w = loo.expected_loo(name)
    n = loo.SETS[name]["n"]
    assert not (w["idx"] == np.arange(n)[:, None]).any()
    assert not (w["naive"]["idx"] == np.arange(n)[:, None]).any()
    assert w["idx"].min() >= 0 and w["idx"].max() < n
    np.testing.assert_array_equal(w["dist"], w["naive"]["dist"])
    assert not (w["sensitive"] & ~w["naive"]["queued"]).any()
    assert (w["correct"] == (w["labels"] == loo.data(name)[1]).sum(axis=1)).all()

"""CPU checks that the leave-group-out data sets (tests/lgo.py) exercise what
the GPU tests rely on, by the oracle alone: rows whose label needs the
reference's std::sort order over the remaining records, both cases of the drop
kernel's boundary bit, and zero-distance duplicates that stay (another group)
and that go (the query's own group).
No GPU calls are made."""
import numpy as np
import pytest

import lgo


@pytest.mark.parametrize("name", sorted(lgo.SETS))
def test_sets_exercise_the_cases(name):
    s = lgo.SETS[name]
    tr, lab, groups = lgo.data(name)
    assert tr.shape == (1500, 6) and tr.min() >= 0 and tr.max() <= 7
    assert lab.max() == s["classes"] - 1
    sizes = np.bincount(groups)
    gmax = lgo.group_max(groups)
    assert gmax == lgo.GMAX and set(sizes) == set(range(1, gmax + 1))
    w = lgo.expected_lgo(name)
    nv = w["naive"]
    # the removed rows are gone, every index is a row of another group
    assert (groups[w["idx"]] != groups[:, None]).all()
    assert (groups[nv["idx"]] != groups[:, None]).all()
    sensitive = int(w["sensitive"].sum())
    whole = nv["c"] == gmax
    part = (nv["c"] > 0) & (nv["c"] < gmax)
    differ = nv["bnd_in"] != nv["bnd_out"]
    # zero-distance duplicates of a row in its own group (they go) and in
    # another group (they stay: the nearest kept neighbour is at distance 0)
    _, inv = np.unique(tr, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    own = np.zeros(s["n"], bool)
    other = np.zeros(s["n"], bool)
    for i in range(s["n"]):
        same = np.flatnonzero(inv == inv[i])
        same = same[same != i]
        own[i] = (groups[same] == groups[i]).any()
        other[i] = (groups[same] != groups[i]).any()
    print("%s: %d order-sensitive rows, %d queued, %d with the whole group in the top k1, "
          "%d with 0 < c < gmax, %d rows whose boundary formulas differ, %d / %d rows with a "
          "duplicate in another / their own group"
          % (name, sensitive, nv["queued"].sum(), whole.sum(), part.sum(), differ.sum(),
             other.sum(), own.sum()))
    assert sensitive >= 20
    assert whole.sum() >= 20 and part.sum() >= 20
    assert differ.sum() >= 5
    assert other.sum() >= 10 and own.sum() >= 10
    # the boundary bit is each case's own formula
    bit = (nv["flags"] & 2) != 0
    np.testing.assert_array_equal(bit[~whole], nv["bnd_in"][~whole])
    # (whole group inside: the full order's bit for k1, and the last kept
    # distance must be the row's last -- it is not when the row ends with
    # dropped entries at a larger distance)
    np.testing.assert_array_equal(
        bit[whole], (nv["bnd_out"] & (nv["dist"][:, -1] == last_dist(name)))[whole])
    # a duplicate in another group stays as the nearest neighbour; the row's
    # own group never shows
    assert (w["dist"][other, 0] == 0).all()


def last_dist(name):
    """dist[k1 - 1] of the full (dist, index) order for every row."""
    import oracle
    s = lgo.SETS[name]
    tr, _, groups = lgo.data(name)
    k1 = max(s["ks"]) + lgo.group_max(groups)
    out = np.empty(s["n"])
    for i in range(s["n"]):
        out[i] = np.sort(oracle.row_distances(tr[i], tr, s["metric"] == 0))[k1 - 1]
    return out


def test_removing_nothing_is_the_plain_sweep():
    """A group id no row carries (-1, n_groups) removes nothing."""
    import oracle
    s = lgo.SETS["G"]
    tr, lab, groups = lgo.data("G")
    Q = np.array(tr[:8])
    for gq in (-1, int(groups.max()) + 1):
        w = lgo.expected_gexcl(tr, lab, groups, Q, np.full(8, gq), [1, 5], True, s["classes"])
        plain = oracle.knn(tr, lab, Q, 5, True, s["classes"], n_out=5)
        np.testing.assert_array_equal(w["labels"][1], plain[0])
        np.testing.assert_array_equal(w["idx"], plain[1])

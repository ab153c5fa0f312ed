"""CPU checks of the weighted-vote oracle (tests/wvote.py) and of its data sets:
the one-pass oracle equals a literal per-K restatement of the rule, with
constant distances it gives the reference's uniform label (oracle.sort_vote),
and the sets contain what test_gpu_wvote.py needs them for: (query, K) pairs
where the weighted label differs from the uniform one, rows with exact matches
(z >= 1) and rows whose top class sums tie exactly.  No GPU."""
import numpy as np
import pytest

import oracle
import wvote


def literal_label(lrow, drow, K):
    """The rule as knn_amd.h states it, for one K, nothing shared with wvote."""
    K = int(K)
    z = sum(1 for t in range(K) if drow[t] == 0.0)
    S = {}
    best, label = -np.inf, -1
    for t in range(K):
        if lrow[t] < 0:
            continue  # an empty slot counts nothing
        if z >= 1:
            if t >= z:
                continue
            w = np.float64(1.0)
        else:
            with np.errstate(divide="ignore"):
                w = np.float64(1.0) / np.float64(drow[t])
        c = int(lrow[t])
        S[c] = S.get(c, np.float64(0.0)) + w
        if S[c] > best:
            best, label = S[c], c
    return label, S


@pytest.mark.parametrize("kmax", [1, 7, 64, 130])
def test_oracle_equals_the_literal_rule(kmax):
    C, n_lab = 3, 50
    lab = np.random.default_rng(5).integers(0, C, n_lab).astype(np.int32)
    idx, dist = wvote.synthetic_rows(40, kmax, n_lab, C, seed=100 + kmax)
    lrows = wvote.lab_rows(lab, idx)
    ks = sorted(set([0, 1, kmax, kmax // 2, max(kmax - 1, 0)]))
    got = wvote.labels(lrows, dist, ks)
    for q in range(40):
        for j, K in enumerate(ks):
            want, S = literal_label(lrows[q], dist[q], K)
            assert got[j, q] == want, (q, K)
            s = wvote.sums(lrows[q:q + 1], dist[q:q + 1], K, C)[0]
            np.testing.assert_array_equal(s, [S.get(c, 0.0) for c in range(C)])
    # the special rows are what they claim to be
    assert got[:, 3].tolist() == [-1] * len(ks)  # no neighbours
    if kmax >= 7:
        k_last = ks.index(kmax)
        assert got[k_last, 7] == lrows[7, 0]  # every weight 0: the first entry records
        assert got[k_last, 2] == wvote.labels(lrows[2:3], np.full((1, kmax), 2.0), [kmax])[0, 0]


@pytest.mark.parametrize("const", [0.0, 2.0, 3.0])
def test_constant_distances_give_the_uniform_label(const):
    """Unit weights (or any one weight for every entry): the scan is the
    reference's first-to-strictly-exceed vote."""
    rng = np.random.default_rng(11)
    C, kmax = 4, 40
    for q in range(60):
        lrow = rng.integers(0, C, kmax).astype(np.int32)
        drow = np.full(kmax, const)
        win = wvote.prefix_winners(lrow, drow)
        for K in (1, 2, 5, 17, kmax):
            # records in fill order with increasing distances: the sort keeps them
            want, _ = oracle.sort_vote(np.arange(kmax, dtype=np.float64), lrow, K, C)
            assert win[K] == want, (q, K)


def _stats(name, metric):
    e = wvote.expected(name, metric)
    d = wvote.dataset(name, metric)
    differ = int((e["weighted"] != e["uniform"]).sum())
    zpairs = sum(int((e["dist"][:, 0] == 0.0).sum()) for K in wvote.KS if K > 0)
    ties = sum(int(wvote.top_sum_ties(e["lrows"], e["dist"], K, d["classes"]).sum())
               for K in wvote.KS if K > 0)
    pairs = e["weighted"].size
    print("set %s metric %d: %d of %d (query, K) pairs differ, %d with z >= 1, %d with tied "
          "top class sums" % (name, metric, differ, pairs, zpairs, ties))
    return differ, zpairs, ties, pairs


@pytest.mark.parametrize("metric", [0, 1])
def test_grid4_has_exact_matches_and_sum_ties(metric):
    differ, zpairs, ties, pairs = _stats("a", metric)
    assert pairs == 900
    assert differ >= 90 and zpairs >= 450 and ties >= 15


@pytest.mark.parametrize("metric", [0, 1])
def test_grid8_has_differing_labels_and_sum_ties(metric):
    # (the set is evalcases.tie_data's, fixed: the conditions ask for a few per
    # cent of the 900 pairs differing and at least ten exact sum ties)
    differ, _, ties, pairs = _stats("b", metric)
    assert pairs == 900
    assert differ >= 30 and ties >= 10


@pytest.mark.parametrize("metric", [0, 1])
def test_clusters_differ_on_one_percent(metric):
    differ, zpairs, _, pairs = _stats("c", metric)
    assert pairs == 1800 and zpairs == 0
    assert differ >= pairs // 100


def test_k0_and_duplicates_in_the_list():
    e = wvote.expected("a", 0)
    ks = wvote.KS
    assert (e["weighted"][ks.index(0)] == -1).all()
    np.testing.assert_array_equal(e["weighted"][0], e["weighted"][4])  # K = 5 twice

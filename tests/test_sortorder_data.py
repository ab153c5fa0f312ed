"""The inputs of test_gpu_sortorder.py, checked on the CPU: conditions on the
data (the port of sortorder.py, the oracle's real std::sort), not on the
library.

1. std_sort_port is pinned to the oracle: on every sequence the GPU tests use
   and on 20 seeded few-valued ones, at every n where the emulation's
   geometry changes, its full order equals the oracle's neighbour order.
2. Every killer case sends a range [f, l) with l - f > 16 and f < k into the
   heap-sort fallback; the extra k at or below f leave it beyond the top k.
3. Every killer case can tell a wrong fallback from a right one: the
   reference order of positions [0, k) differs from the (distance, index)
   order and from the order a stable sort of the heap range would leave, and
   the vote under either wrong order gives another label.
4. A random permutation of the same keys takes no heap range: why the random
   tie data of the older tests never got there.
These are conditions, not measurements: a case that misses one is replaced.
"""
import numpy as np
import pytest

import oracle
import sortorder as so

PIN_N = [16, 17, 33, 300, 1024, 1025, 2049]


def oracle_order(keys, metric=0, d=1):
    """The oracle's neighbour order of all n rows for the query at 0, and its
    distances."""
    train, queries = so.as_train(keys, d)
    n = train.shape[0]
    _, idx, dist = oracle.knn(train, np.zeros(n, np.int32), queries, 1, metric == 0, 1, n_out=n)
    return idx[0], dist[0]


def heap_ranges(keys):
    return so.std_sort_port(keys)[1].heap


@pytest.mark.parametrize("n", PIN_N)
def test_port_matches_oracle(n):
    seqs = {name: f(n) for name, f in so.SEQUENCES.items()}
    for s in range(20):
        seqs["few_values_%d" % s] = so.few_values(s, n, 2 + s % 5)
    seqs["killer"] = so.killer(n)
    seqs["killer_ties2"] = so.with_ties(seqs["killer"], 2)
    fell_back = []
    for name, keys in seqs.items():
        order, trace = so.std_sort_port(keys)
        widx, wdist = oracle_order(keys)
        np.testing.assert_array_equal(order, widx, err_msg="%s n=%d" % (name, n))
        assert (wdist == np.sort(keys)).all()
        if trace.heap:
            fell_back.append(name)
    print("n = %d: heap fallback taken by %s" % (n, fell_back))


@pytest.mark.parametrize("name", sorted(so.KILLERS))
def test_killer_cases_match_oracle(name):
    keys, lab, k = so.killer_case(name)
    order, _ = so.std_sort_port(keys)
    for metric, d in ((0, 1), (1, 3)):
        widx, wdist = oracle_order(keys, metric, d)
        np.testing.assert_array_equal(order, widx)
        assert (wdist == np.sort(keys)).all()
    train, queries = so.as_train(keys, 1, m=2)
    want, widx, _ = oracle.knn(train, lab, queries, k, True, so.CLASSES, n_out=k)
    assert (want == so.vote(lab[order[:k]])).all()
    np.testing.assert_array_equal(widx, np.stack([order[:k]] * 2))


def test_killer_is_a_permutation():
    for n in (17, 300):
        keys = so.killer(n)
        np.testing.assert_array_equal(np.sort(keys), np.arange(n))
        np.testing.assert_array_equal(keys, so.killer(n))
    np.testing.assert_array_equal(so.with_ties([0, 1, 2, 3, 4], 2), [0, 0, 1, 1, 2])


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [1, 3])
def test_as_train_distances_exact(d, metric):
    keys = so.with_ties(so.killer(300), 2)
    train, queries = so.as_train(keys, d, m=5)
    assert train.shape == (300, d) and queries.shape == (5, d)
    for c in range(5):
        dist = oracle.row_distances(queries[c], train, metric == 0)
        assert (dist == keys + c).all()


@pytest.mark.parametrize("name", sorted(so.KILLERS))
def test_killer_fires_fallback_inside_top_k(name):
    keys, _, k = so.killer_case(name)
    n = keys.shape[0]
    _, trace = so.std_sort_port(keys)
    print("case %s: n %d k %d heap ranges %s depth %d" % (name, n, k, trace.heap, trace.depth))
    assert trace.depth == 2 * (n.bit_length() - 1)
    assert any(f < k and l - f > 16 for f, l in trace.heap)
    assert k <= 1000 or name in ("n2049", "n2000_large_k")


@pytest.mark.parametrize("name", sorted(so.EXTRA_K))
def test_heap_range_beyond_small_k(name):
    """k at or below the heap range's start: the range cannot reach the top k
    (so the emulation may skip it) -- whatever sorts it, positions [0, k) come
    out the same; k just above the start and k = n stay inside it."""
    keys, _, _ = so.killer_case(name)
    n = keys.shape[0]
    order, trace = so.std_sort_port(keys)
    stable, _ = so.std_sort_port(keys, fallback="stable")
    (f, l), = trace.heap
    ks = so.EXTRA_K[name]
    assert f in ks and n in ks
    for k in ks:
        if k <= f:
            np.testing.assert_array_equal(order[:k], stable[:k])
        else:
            assert f < k and l - f > 16
    if name == "n2000":
        assert f == 40 and 10 in ks and min(so.SWEEP_KS) < f and f in so.SWEEP_KS and max(so.SWEEP_KS) > f + 1


@pytest.mark.parametrize("name", sorted(so.KILLERS))
def test_cases_tell_wrong_from_right(name):
    keys, lab, k = so.killer_case(name)
    assert k % 2 == 0 and so.KILLERS[name]["classes"] in (2, 3)
    order, _ = so.std_sort_port(keys)
    wrong = {"(distance, index) order": so.index_order(keys),
             "stable sort of the heap range": so.std_sort_port(keys, fallback="stable")[0]}
    want = so.vote(lab[order[:k]])
    for what, w in wrong.items():
        np.testing.assert_array_equal(keys[w], keys[order])  # sorted all the same
        differs = int((w[:k] != order[:k]).sum())
        got = so.vote(lab[w[:k]])
        print("case %s, %s: %d of the first %d positions differ, label %d (reference %d)"
              % (name, what, differs, k, got, want))
        assert differs > 0
        assert got != want


@pytest.mark.parametrize("name", sorted(so.KILLERS))
def test_random_permutation_takes_no_heap_range(name):
    keys, _, _ = so.killer_case(name)
    perm = np.random.default_rng(1).permutation(keys)
    order, trace = so.std_sort_port(perm)
    np.testing.assert_array_equal(order, oracle_order(perm)[0])
    assert trace.heap == []
    assert trace.depth < 2 * (keys.shape[0].bit_length() - 1)


def test_edge_sequences_shape():
    for name, f in so.SEQUENCES.items():
        for n in so.EDGE_N:
            keys = f(n)
            assert keys.shape == (n,) and keys.dtype == np.int64 and keys.min() >= 0, name
            np.testing.assert_array_equal(keys, f(n))
    assert so.EDGE_K(17) == [1, 2, 16, 17] and so.EDGE_K(1025) == [1, 2, 16, 17, 1024, 1025]
    assert len(set(so.SEQUENCES["random4"](1024))) == 4
    assert heap_ranges(so.SEQUENCES["organ_pipe"](1024))  # a fallback off the killer's path too

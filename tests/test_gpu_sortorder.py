"""GPU parity of the reference-tie-order passes (knn_select.hip:
ref_sort_prefix in tie_order_kernel and tie_resolve_kernel) on row orders
that steer the reference's std::sort where random tie data never takes it.

The inputs (tests/sortorder.py; shown on the CPU to do so by
test_sortorder_data.py) dictate the distance sequence the sort sees:
  * killer cases: a median-of-3 killer order with tied pairs.  Introsort
    runs out of depth and heap-sorts a range that reaches into the top k
    (ref_heap_sort / ref_adjust_heap), and the (distance, index) order -- or
    any fallback that merely sorts -- gives another label;
  * edge orders (all equal, two values, ascending, descending, organ pipe,
    sawtooth, ...) at the n where the parallel partition's geometry changes
    (the 16 / 17 threshold, seg = ceil(len / 1024) at 1024 / 1025 / 2049).
Every case compares against oracle.knn: labels equal, fp64 distances
bit-identical, under "ties" = 2 the neighbour indices equal index for index
and KNN_FLAG_TIE_REF on exactly the queries with a tie in (or across the end
of) their top k.  All queries of a call see the same order (query c's
distances are the keys + c); there are 16 of them, one per workgroup of the
tie kernels.
"""
import numpy as np
import pytest

import oracle
import sortorder as so
from test_gpu_parity import knn  # noqa: F401
from test_gpu_sharded import GROUPS, _resolve_pending, _sharded_blocks

pytestmark = pytest.mark.gpu

TIE_BITS = 14  # KNN_FLAG_TIE_BOUNDARY | KNN_FLAG_TIE_VOTE | KNN_FLAG_TIE_ORDER
M = 16
SHAPES = [(1, 0), (1, 1), (3, 0), (3, 1)]  # (d, metric)


def expected(train, lab, queries, k, metric):
    """The oracle's (labels, idx [m, k], dist [m, k], tied [m]): tied = equal
    distances among the k nearest or across the k-th place."""
    w = min(k + 1, train.shape[0])
    want, widx, wdist = oracle.knn(train, lab, queries, k, metric == 0, so.CLASSES, n_out=w)
    tied = (np.diff(wdist, axis=1) == 0).any(axis=1)
    return want, widx[:, :k], wdist[:, :k], tied


def compare(knn, out, exp, ties):
    """Returns the mask of the queries re-ordered as the reference."""
    got, idx, dist, flags = out
    want, widx, wdist, tied = exp
    assert (dist.view(np.int64) == wdist.view(np.int64)).all()
    np.testing.assert_array_equal(got, want)
    assert not (flags & knn.FLAG_TIE_PENDING).any()
    ref = (flags & knn.FLAG_TIE_REF) != 0
    assert not (ref & ~tied).any(), "untied query re-ordered"
    np.testing.assert_array_equal(idx[~tied], widx[~tied])
    np.testing.assert_array_equal(idx[ref], widx[ref])
    if ties == 2:
        np.testing.assert_array_equal(ref, tied)
        np.testing.assert_array_equal(idx, widx)
    return ref


def case_ks(name):
    return [so.KILLERS[name]["k"]] + so.EXTRA_K.get(name, [])


@pytest.mark.parametrize("ties", [2, 1])
@pytest.mark.parametrize("d,metric", SHAPES)
@pytest.mark.parametrize("name", sorted(so.KILLERS))
def test_heap_fallback(knn, name, d, metric, ties):
    """The killer cases through the single-context path at their own k (the
    heap range reaches into the top k and decides the label; n2049 and
    n2000_large_k at k > 1000, the exact large-k path) and at k at and below
    the heap range's start (the range is skipped), just above it and k = n.
    "ties" = 1 re-orders only where the label depends on it: at the case's
    own k it does, for every query."""
    keys, lab, k0 = so.killer_case(name)
    train, queries = so.as_train(keys, d, M)
    c = knn.Classifier(0)
    c.set_tuning("ties", ties)
    c.set_train(train, lab, so.CLASSES)
    for k in case_ks(name):
        exp = expected(train, lab, queries, k, metric)
        assert exp[3].all()
        out = c.classify(queries, k, metric, return_neighbors=True)
        assert (((out[3] & TIE_BITS) != 0) == exp[3]).all()
        ref = compare(knn, out, exp, ties)
        if k == k0:
            assert ref.all(), "label-deciding tie not re-ordered"
    c.close()


def _sharded_group(knn, name, devs, rccl):
    """knn_group mode 1: the group does the exchange itself."""
    keys, lab, k0 = so.killer_case(name)
    train, queries = so.as_train(keys, 1, M)
    g = knn.Group(devs, 1, rccl=rccl)
    g.set_train(train, lab, so.CLASSES)
    for metric in (0, 1):
        exp = expected(train, lab, queries, k0, metric)
        ref = compare(knn, g.classify(queries, k0, metric, return_neighbors=True), exp, 1)
        assert ref.all(), "label-deciding tie not resolved"
        assert g.last_tie_count() == ref.sum() > 0
    g.set_tuning("ties", 2)
    for metric in (0, 1):
        for k in case_ks(name):
            exp = expected(train, lab, queries, k, metric)
            ref = compare(knn, g.classify(queries, k, metric, return_neighbors=True), exp, 2)
            assert g.last_tie_count() == ref.sum() > 0
    g.close()


def _sharded_abi(knn, name):
    """The ABI building blocks on 3 ragged shards: search_partial, merge_vote
    (flags the queries), shard distances, tie_resolve."""
    import torch
    dev = torch.device("cuda", 0)
    keys, lab, k0 = so.killer_case(name)
    train, queries = so.as_train(keys, 1, M)
    n = train.shape[0]
    shards = [(0, n // 3), (n // 3, 2 * n // 3 + 1), (2 * n // 3 + 1, n)]
    Q = torch.from_numpy(queries).to(dev)
    lab_all = torch.from_numpy(lab.copy()).to(dev)
    for metric, ties, ks in ((0, 2, case_ks(name)), (1, 2, case_ks(name)), (0, 1, [k0]),
                             (1, 1, [k0])):
        for k in ks:
            w = min(k + 1, n)
            ctxs, gd, gi, gl = _sharded_blocks(knn, train, lab, Q, shards, w, metric, dev)
            exp = expected(train, lab, queries, k, metric)
            ctxs[0].set_tuning("ties", ties)
            out = (torch.empty(M, dtype=torch.int32, device=dev),
                   torch.empty((M, k), dtype=torch.int64, device=dev),
                   torch.empty((M, k), dtype=torch.float64, device=dev),
                   torch.empty(M, dtype=torch.int32, device=dev))
            ctxs[0].merge_vote_device(gd.data_ptr(), gi.data_ptr(), gl.data_ptr(), 3, M, w, k,
                                      out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                      out[3].data_ptr())
            ctxs[0].sync()
            pending = (out[3].cpu().numpy() & knn.FLAG_TIE_PENDING) != 0
            if ties == 2:
                np.testing.assert_array_equal(pending, exp[3])
            resolved = _resolve_pending(knn, ctxs, shards, Q, lab_all, k, metric, out, dev)
            assert resolved == pending.sum()
            ref = compare(knn, tuple(t.cpu().numpy() for t in out), exp, ties)
            np.testing.assert_array_equal(ref, pending)
            if k == k0:
                assert ref.all(), "label-deciding tie not resolved"
            for c in ctxs:
                c.close()


ROUTES = {"loopback3": ([0, 0, 0], False), "rccl1": ([0], True)}
assert all(g in GROUPS for g in ROUTES.values())  # the transports test_gpu_sharded.py offers


@pytest.mark.parametrize("route", sorted(ROUTES) + ["abi"])
@pytest.mark.parametrize("name", sorted(so.KILLERS))
def test_heap_fallback_sharded(knn, name, route):
    """The killer cases through the train-sharded routes (tie_resolve_kernel
    over distances assembled from every shard): knn_group mode 1 on three
    loopback ranks and on one rank over RCCL, and the ABI building blocks on 3
    ragged shards.  The oracle's labels and tie-ordered indices, no query
    left pending, the exchange ran (at the case's own k for every query)."""
    if route == "abi":
        _sharded_abi(knn, name)
    else:
        _sharded_group(knn, name, *ROUTES[route])


@pytest.mark.parametrize("metric", [0, 1])
def test_heap_fallback_sweep(knn, metric):
    """classify_sweep over ks on both sides of the heap range's start (f = 40
    on the n = 2000 killer): the oracle's label at every K, and with "ties" =
    2 its neighbour order at kmax."""
    keys, lab, _ = so.killer_case("n2000")
    train, queries = so.as_train(keys, 1, M)
    want = np.stack([oracle.knn(train, lab, queries, k, metric == 0, so.CLASSES)[0]
                     for k in so.SWEEP_KS])
    kmax = max(so.SWEEP_KS)
    exp = expected(train, lab, queries, kmax, metric)
    c = knn.Classifier(0)
    c.set_train(train, lab, so.CLASSES)
    for ties in (1, 2):
        c.set_tuning("ties", ties)
        labels, idx, dist, flags = c.classify_sweep(queries, so.SWEEP_KS, metric,
                                                    return_neighbors=True)
        np.testing.assert_array_equal(labels, want)
        ref = compare(knn, (labels[so.SWEEP_KS.index(kmax)], idx, dist, flags), exp, ties)
        assert ref.all()
    c.close()


@pytest.mark.parametrize("n", so.EDGE_N)
@pytest.mark.parametrize("seq", sorted(so.SEQUENCES))
def test_edge_orders(knn, seq, n):
    """Every named sequence at the n where ref_partition's geometry changes,
    k in {1, 2, 16, 17, n - 1, n}, both metrics, "ties" = 2: every tied query
    re-ordered, every index the oracle's."""
    keys = so.SEQUENCES[seq](n)
    lab = so.labels(n, n, so.CLASSES)
    train, queries = so.as_train(keys, 1, M)
    c = knn.Classifier(0)
    c.set_tuning("ties", 2)
    c.set_train(train, lab, so.CLASSES)
    for metric in (0, 1):
        for k in so.EDGE_K(n):
            exp = expected(train, lab, queries, k, metric)
            out = c.classify(queries, k, metric, return_neighbors=True)
            assert (((out[3] & TIE_BITS) != 0) == exp[3]).all(), (metric, k)
            compare(knn, out, exp, 2)
    c.close()

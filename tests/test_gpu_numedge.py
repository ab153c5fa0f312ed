"""GPU parity at the numeric edges of operand preparation and of AUTO's path
choice: the code that looks at the VALUES of the data to decide how to run
(knn_prep.hip; build_train, detect_i8, use_fp16 / use_i8, auto_check in
knn_api.cpp).

The inputs (tests/numedge.py; shown on the CPU to sit where they should by
test_numedge_data.py) are degenerate, extremely scaled, anisotropic or
overflowing train sets and queries, integer-coded sets on either side of each
limit of the int8 grid detection, and batches that keep or retire AUTO's
reduced-precision passes.  The oracle is the reference throughout, under
run_case's rules: labels equal, distances bit-identical, indices equal
outside exact ties, the reference's order on KNN_FLAG_TIE_REF rows.  A
mistake in any of this code does not crash: it shows as a wrong neighbour, or
as the wrong kernel silently taking over, on data no other test produces.
"""
import numpy as np
import pytest

import numedge
from test_gpu_parity import assert_neighbors_match, clf, knn, run_case  # noqa: F401

pytestmark = pytest.mark.gpu

TIE_FLAGS = 14  # KNN_FLAG_TIE_BOUNDARY | KNN_FLAG_TIE_VOTE | KNN_FLAG_TIE_ORDER
I8_PATHS = (5, 6)


def run_named(c, knn, name, k, metric):
    tr, lab, te = numedge.case(name)[:3]
    return run_case(c, knn, tr, lab, te, k, metric, numedge.classes(name))


def run_distinct(c, knn, name, k, metric):
    """run_case where the oracle's k+1 distances are pairwise distinct: the
    oracle's neighbours index for index, no tie flag, nothing re-ordered."""
    got, want, flags = run_named(c, knn, name, k, metric)
    assert ((flags & TIE_FLAGS) == 0).all(), "distinct distances flagged as a tie: queries %s" % (
        np.nonzero(flags & TIE_FLAGS)[0][:10],)
    assert ((flags & knn.FLAG_TIE_REF) == 0).all(), "untied queries re-ordered"
    np.testing.assert_array_equal(got, want)
    return flags


def compare(knn, out, ref):
    """run_case's bar on one call's outputs against a cached oracle result
    (the calls of a sequence on one trained context: run_case would set the
    train set again and with it reset what the sequence is about)."""
    got, idx, dist, flags = out
    want, widx, wdist = ref
    tie_vote = (flags & knn.FLAG_TIE_VOTE) != 0
    assert (got[~tie_vote] == want[~tie_vote]).all(), "labels differ on untied queries"
    ref_order = (flags & knn.FLAG_TIE_REF) != 0
    assert not (ref_order & ((flags & TIE_FLAGS) == 0)).any(), "untied query re-ordered"
    np.testing.assert_array_equal(idx[ref_order], widx[ref_order])
    assert_neighbors_match(idx, dist, widx, wdist, flags)
    differs = int((got[tie_vote] != want[tie_vote]).sum())
    assert differs == 0, "%d exact-tie votes differ from the reference order" % differs
    return flags


# ------------------------------------------------------------ 1. operand scale
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", numedge.DEGENERATE)
def test_degenerate_spread(name, metric, clf, knn):
    """max |x - mu| = 0 (one row; 300 identical rows: jx at its 2^450 cap,
    the frexp skipped) or 36 * 2^-30 (rows that differ in one dimension);
    mixed labels, k = 1, 7 and n: whole-row-set exact ties."""
    for k in numedge.degenerate_ks(name):
        run_named(clf, knn, name, k, metric)


@pytest.mark.parametrize("e", numedge.LADDER_EXACT)
def test_ladder_exact(e, clf, knn):
    """Train and queries scaled by 2^e with nothing under- or overflowing:
    the oracle's answer, and the unscaled run's indices with distances
    ldexp(dist, e) bit for bit."""
    k = numedge.LADDER_K
    tr, lab, te = numedge.case("ladder0")
    clf.set_train(tr, lab, numedge.CLASSES)
    _, idx0, dist0, flags0 = clf.classify(te, k, knn.L2, return_neighbors=True)
    assert ((flags0 & TIE_FLAGS) == 0).all()
    run_distinct(clf, knn, "ladder%d" % e, k, 0)
    _, idx, dist, _ = clf.classify(numedge.case("ladder%d" % e)[2], k, knn.L2,
                                   return_neighbors=True)
    np.testing.assert_array_equal(idx, idx0)
    assert (dist.view(np.int64) == np.ldexp(dist0, e).view(np.int64)).all()


@pytest.mark.parametrize("e", numedge.LADDER_LOSSY)
def test_ladder_lossy(e, clf, knn):
    """2^-520 (squares denormal), 2^-600 (squares flush to 0: every distance
    0) and 2^-1060 (the inputs themselves denormal): the operands vanish and
    the bound's absolute terms, the rescan and the tie rules carry the
    answer."""
    run_named(clf, knn, "ladder%d" % e, numedge.LADDER_K, 0)


def test_range_accepted(clf, knn):
    """max |x - mean| = 2^400 (1 - 2^-20): accepted and exact."""
    run_named(clf, knn, "range_below", 7, 0)
    run_named(clf, knn, "range_below", 7, 1)


def test_range_refused(knn):
    """max |x - mean| = 2^400 (1 + 2^-20): set_train and set_train_device
    raise, classify on that context then raises (no train set), and a good
    set_train makes it work again."""
    import torch
    tr, lab, te = numedge.case("range_above")
    good = numedge.case("range_below")
    c = knn.Classifier(0)
    run_named(c, knn, "range_below", 7, 0)
    with pytest.raises(knn.KnnError, match="out of range"):
        c.set_train(tr, lab, numedge.CLASSES)
    with pytest.raises(knn.KnnError, match="before set_train"):
        c.classify(te, 7)
    dev = torch.device("cuda", 0)
    Xd, Ld = torch.from_numpy(tr.copy()).to(dev), torch.from_numpy(lab.copy()).to(dev)
    with pytest.raises(knn.KnnError, match="out of range"):
        c.set_train_device(Xd.data_ptr(), Ld.data_ptr(), tr.shape[0], tr.shape[1],
                           numedge.CLASSES, keep=(Xd, Ld))
    with pytest.raises(knn.KnnError, match="before set_train"):
        c.classify(good[2], 7)
    run_named(c, knn, "range_below", 7, 0)
    c.close()


@pytest.mark.parametrize("name", sorted(numedge.ANISO))
def test_anisotropic(name, clf, knn):
    """Feature scales from 1 down to 2^-40 (d = 16 and 300); clusters of 40
    and 600 rows and their queries equal in the large dimensions and apart
    only in those scaled by <= 2^-36, which vanish from the fp16 operands and
    drown in the fp32 ones' rounding: index-for-index parity, no tie flag."""
    run_distinct(clf, knn, name, numedge.ANISO_K, 0)


@pytest.mark.parametrize("k", [7, 1200])
@pytest.mark.parametrize("metric", [0, 1])
def test_overflowing_queries(metric, k, clf, knn):
    """Finite queries whose reference distance to every row is +inf (a
    coordinate of 1e160 under L2; two of +-1.5e308 under L1) among ordinary
    ones: the reference still orders and votes them (every row ties), +inf is
    also the pad value of empty list slots.  Distances +inf bit for bit, real
    row indices, no KNN_FLAG_NONFINITE, the other queries unaffected; k = 7
    and the large-k path."""
    name = "overflow_l2" if metric == 0 else "overflow_l1"
    tr, lab, te = numedge.case(name)
    got, want, flags = run_named(clf, knn, name, k, metric)
    _, idx, dist, flags = clf.classify(te, k, metric, return_neighbors=True)
    bad = list(numedge.OVERFLOW_Q[metric])
    assert np.isposinf(dist[bad]).all()
    assert (idx[bad] >= 0).all() and (idx[bad] < tr.shape[0]).all()
    assert not (flags & knn.FLAG_NONFINITE).any()
    np.testing.assert_array_equal(got[bad], want[bad])
    ok = np.setdiff1d(np.arange(te.shape[0]), bad)
    assert np.isfinite(dist[ok]).all()


# ------------------------------------------------------ 2. int8 grid detection
@pytest.mark.parametrize("i8w", [0, 1])
@pytest.mark.parametrize("name", sorted(numedge.GRID_CASES))
def test_grid_detection(name, i8w, knn):
    """The int8 pass forced ("i8" = 1) on train sets on either side of each
    limit of detect_i8: it runs (path 5 / 6) exactly where the rule accepts
    the set, another path answers where it refuses (never an error), and the
    answer is the oracle's either way."""
    c = knn.Classifier(0)
    c.set_tuning("i8", 1)
    c.set_tuning("i8w", i8w)
    run_named(c, knn, name, numedge.GRID_K, 0)
    path = c.last_candidate_path()
    if numedge.GRID_CASES[name]:
        assert path in I8_PATHS, "grid data not taken by the int8 pass (path %d)" % path
    else:
        assert path not in I8_PATHS, "int8 pass on data off its grid (path %d)" % path
    c.close()


@pytest.mark.parametrize("i8w", [0, 1])
def test_grid_query_edges(i8w, knn):
    """Queries at the edge of the code range of a dimension spanning all 255
    codes: on codes -128 and 127 (exact), one code outside (saturated), 1000
    codes outside, and 2^-31 off a grid point.  Exact answers; the queries on
    the end codes are certified no less often than interior ones."""
    c = knn.Classifier(0)
    c.set_tuning("i8", 1)
    c.set_tuning("i8w", i8w)
    got, want, flags = run_named(c, knn, "grid_edges", numedge.GRID_K, 0)
    assert c.last_candidate_path() in I8_PATHS
    resc = (flags & knn.FLAG_EXACT_RESCAN) != 0
    B = numedge.EDGE_BLOCK
    inner = resc[numedge.EDGE_OFFGRID[1]:]
    for b in (0, 1):
        edge = resc[b * B:(b + 1) * B]
        print("code %d: %d of %d rescanned; interior %d of %d"
              % (numedge.EDGE_CODES[b], edge.sum(), edge.size, inner.sum(), inner.size))
        assert edge.mean() <= inner.mean(), "queries on code %d rescanned more often" % (
            numedge.EDGE_CODES[b],)
    c.close()


def test_grid_offsets_all_paths(clf, knn):
    """The offset case on every configuration: the fp16 / bf16x3 / fp32
    passes centre on a mean near +-2^49 (launch_round_mu, the x - mu
    subtraction)."""
    run_named(clf, knn, "grid_offsets", numedge.GRID_K, 0)


# ------------------------------------------- 3. large offset, continuous data
def test_large_offset_continuous(clf, knn):
    run_named(clf, knn, "offset40", 10, 0)


# ------------------------------------------------ 4. AUTO choice, retirement
K4 = numedge.AUTO_K


def _auto_classifier(knn, name):
    c = knn.Classifier(0)   # AUTO precision, no path tuning
    tr, lab, _ = numedge.case(name)
    c.set_train(tr, lab, numedge.AUTO_CLASSES)
    return c


def _batch(c, knn, name, m=None):
    """One classify of the named batch (its first m queries) against the
    cached oracle; returns the candidate path."""
    te = numedge.case(name)[2]
    ref = numedge.oracle_knn(name, K4, 0)
    if m is not None:
        te, ref = te[:m], [r[:m] for r in ref]
    compare(knn, c.classify(te, K4, knn.L2, return_neighbors=True), ref)
    return c.last_candidate_path()


@pytest.mark.parametrize("name,big", [("auto_grid", I8_PATHS), ("auto_cont", (4,))])
def test_auto_limit(name, big, knn):
    """4095 queries: bf16x3 on 32x32x16 (path 2); 4096: int8 on grid data,
    fp16 on continuous data."""
    c = _auto_classifier(knn, name)
    assert _batch(c, knn, name, 4095) == 2
    c.sync()
    assert _batch(c, knn, name, 4096) in big
    c.close()


# after a retirement a batch of >= 4096 queries takes bf16x3 on the 16x16x32
# layout (path 3: tuning "mfma16" auto is on from 4096 queries, knn_amd.h)
@pytest.mark.parametrize("name,first,then", [("auto_grid", I8_PATHS, (4,)),
                                             ("auto_cont", (4,), (3,))])
def test_auto_retirement(name, first, then, knn):
    """Batch A (4096 benign queries) keeps the reduced-precision pass; batch
    B (400 of them far outside the operand range) leaves more than 1/16 of
    its queries to the rescan, which retires the pass for this train set once
    the call has completed: A then runs on the next path (int8 -> fp16 ->
    bf16x3).  A forced request overrides the retirement, clearing it does not
    undo it, a new set_train does."""
    m = numedge.AUTO_M
    tr, lab, _ = numedge.case(name)
    c = _auto_classifier(knn, name)
    for _ in range(2):
        assert _batch(c, knn, name) in first
        assert c.last_rescan_count() * 16 <= m, "premise: batch A keeps the pass"
        c.sync()
    assert _batch(c, knn, name + "_b") in first
    assert c.last_rescan_count() * 16 > m, "premise: batch B retires the pass"
    c.sync()
    assert _batch(c, knn, name) in then
    c.sync()
    if name == "auto_grid":
        c.set_tuning("i8", 1)
        assert _batch(c, knn, name) in first
        c.sync()
        c.set_tuning("i8", -1)
        assert _batch(c, knn, name) not in first
    else:
        c.set_precision(knn.PRECISION_FP16)
        assert _batch(c, knn, name) == 4
        c.sync()
        c.set_precision(knn.PRECISION_AUTO)
        assert _batch(c, knn, name) in then
    c.sync()
    c.set_train(tr, lab, numedge.AUTO_CLASSES)
    assert _batch(c, knn, name) in first
    c.close()


@pytest.mark.parametrize("name,first", [("auto_grid", I8_PATHS), ("auto_cont", (4,))])
def test_auto_pending_decision_dropped(name, first, knn):
    """The decision is taken from the LAST call's count, once that call has
    completed, by the next call (or sync / a count read-back): "armed by an
    fp16 call and dropped by any other".  Batch B and an L1 call enqueued
    behind it (device API: neither waits) while B cannot have completed --
    the context's stream is held behind a large product on the device's
    default stream -- so the L1 call finds B pending and takes over the
    counters: B's count is never read, batch A stays on the reduced-precision
    path.  Through the host API, which returns after its call has completed,
    the next call of any kind takes the decision."""
    import torch
    dev = torch.device("cuda", 0)
    m = numedge.AUTO_M
    c = _auto_classifier(knn, name)
    B = torch.from_numpy(numedge.case(name + "_b")[2].copy()).to(dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    big = torch.ones((8192, 8192), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    held = torch.mm(big, big)   # ~1.1 TFLOP of fp64 ahead of the context's stream
    c.classify_device(B.data_ptr(), m, K4, knn.L2, out.data_ptr())
    assert c.last_candidate_path() in first
    c.classify_device(B.data_ptr(), 64, K4, knn.L1, out.data_ptr())
    c.sync()
    torch.cuda.synchronize()
    del held
    assert _batch(c, knn, name) in first, "a dropped decision retired the pass"
    c.sync()
    # the host API: B has completed when the L1 call starts, which decides
    assert _batch(c, knn, name + "_b") in first
    c.classify(numedge.case(name)[2][:64], K4, knn.L1)
    assert _batch(c, knn, name) not in first
    c.close()

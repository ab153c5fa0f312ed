"""GPU parity of candidate path 8 above 256 dims: the wide L1 pass on 16-bit
fixed-point codes (v_sad_u16, csrc/knn_cand_fix16_wide.hip; tuning key
"u16l1w") against the CPU oracle -- labels, neighbour indices, fp64 distance
bit patterns and tie flags, as test_gpu_l1fix.py compares them.  Every case
sets "u16l1w" = 1 unless it is about the plan's own choice, and asserts that
path 8 served the call with the wide kernel.  The data sets and the CPU model
of the pass are in tests/l1fixwide.py; test_l1fixwide_data.py checks the error
bound, rounding term included, on them."""
import numpy as np
import pytest

import l1fixwide
import loo
import oracle
import wvote
from l1codes import assert_neighbors_match

pytestmark = pytest.mark.gpu

WIDE = "cand_fix16_wide_kernel<"


@pytest.fixture(scope="module")
def knn():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(root, "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.lib().knn_device_count() < 1:
        pytest.fail("no HIP device visible: the KNN path has no CPU fallback")
    return mod


def _clf(knn, **tuning):
    c = knn.Classifier(0)
    c.set_tuning("u16l1w", 1)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    return c


def _check(knn, c, tr, lab, te, k, classes, kernel=WIDE):
    """One classify against the oracle; returns (labels, idx, dist, flags)."""
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8
    assert c.last_kernel_name().startswith(kernel)
    want, widx, wdist = oracle.knn(tr, lab, te, k, False, classes, n_out=k)
    assert (idx < tr.shape[0]).all() and (idx >= 0).all()
    tie_vote = (flags & knn.FLAG_TIE_VOTE) != 0
    np.testing.assert_array_equal(got[~tie_vote], want[~tie_vote])
    ref = (flags & knn.FLAG_TIE_REF) != 0
    np.testing.assert_array_equal(idx[ref], widx[ref])
    np.testing.assert_array_equal(got, want)
    assert_neighbors_match(idx, dist, widx, wdist, flags)
    return got, idx, dist, flags


# ------------------------------------------------------------ 1. shape edges
@pytest.mark.parametrize("d", l1fixwide.SHAPE_D)
@pytest.mark.parametrize("n", l1fixwide.SHAPE_N)
def test_shape_edges(knn, n, d):
    """Uniform normalised data.  d: the first above the narrow pass (257, 15
    pad dims), no pad dims (272), both sides of the slab boundary (512: one
    slab, 513: two), the reference's 784, the largest (1024).  n: one ragged
    64-row unit (70), several units and a pad row (300), several tiles per
    split (2000).  m = 1, 33, 130: no multiple of the 32-query group.  k = 1,
    10, 50."""
    tr, lab, te = l1fixwide.uniform_norm(n, d)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for m in l1fixwide.SHAPE_M:
        for k in l1fixwide.K_EDGES:
            got, idx, dist, flags = _check(knn, c, tr, lab, te[:m], k, 4)
            assert (flags & 14).sum() == 0  # continuous data: no equal distances
    c.close()


@pytest.mark.parametrize("nw", [4, 8])
@pytest.mark.parametrize("R", [8, 16])
def test_every_instantiation(knn, R, nw):
    tr, lab, te = l1fixwide.uniform_norm(2000, 784)
    c = _clf(knn, R=R, nw=nw)
    c.set_train(tr, lab, 4)
    _check(knn, c, tr, lab, te, 10, 4, kernel="cand_fix16_wide_kernel<%d,%d>" % (R, nw))
    c.close()


def test_k_300_takes_the_long_lists(knn):
    """W = 301: R = 16 lists and the large-k merge."""
    tr, lab, te = l1fixwide.uniform_norm(2000, 513)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    _check(knn, c, tr, lab, te[:33], l1fixwide.BIG_K, 4, kernel="cand_fix16_wide_kernel<16,")
    c.close()


# ----------------------------------------- 2. the pass does the work itself
def test_rescans_on_the_784_dim_set(knn):
    """test_l1fixwide_data.py: every query's gap exceeds 2 E on this set, so
    at most m / 16 queries may reach the rescan."""
    tr, lab, te = l1fixwide.uniform_norm(2000, 784)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in l1fixwide.K_EDGES:
        _check(knn, c, tr, lab, te, k, 4)
        assert c.last_rescan_count() <= te.shape[0] // 16
    c.close()


# ------------------------------------------- 3. sums in the rounding binades
def test_displaced_queries(knn):
    """Every sum at or above 2^24, nine in ten at or above 2^25: the floats
    the lists hold differ from the integer sums by up to 2 code units."""
    tr, lab, te = l1fixwide.displaced()
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in (1, 10, 50):
        _check(knn, c, tr, lab, te, k, 4)
    c.close()


# ------------------------------------ 4. unequal dims and degenerate sets
@pytest.mark.parametrize("kind", ["unequal", "constant"])
def test_odd_sets(knn, kind):
    tr, lab, te = l1fixwide.odd_set(kind)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in (1, 6):
        _check(knn, c, tr, lab, te, k, 4)
    c.close()


def test_query_with_a_nan(knn):
    tr, lab, te, nan = l1fixwide.with_nan()
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    k = 7
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8 and c.last_kernel_name().startswith(WIDE)
    assert (got[nan] == -1).all() and (flags[nan] & knn.FLAG_NONFINITE).all()
    ok = np.setdiff1d(np.arange(te.shape[0]), nan)
    want, widx, wdist = oracle.knn(tr, lab, te[ok], k, False, 4, n_out=k)
    np.testing.assert_array_equal(got[ok], want)
    assert_neighbors_match(idx[ok], dist[ok], widx, wdist, flags[ok])
    c.close()


# ------------------------------------------------------------------ 5. the plan
def test_plan_choices(knn):
    rng = np.random.default_rng(26)
    wide, wide_q = rng.random((2000, 300)), rng.random((64, 300))
    lab = l1fixwide.labels_for(2000, 4, 27)
    big = np.tile(wide_q, (64, 1))  # 4096 queries
    narrow, narrow_q = rng.random((2000, 128)), rng.random((64, 128))
    ints, _, int_q = l1fixwide.int_sets(2000, 64, 300)

    def path(train, q, metric=None, **tuning):
        c = knn.Classifier(0)
        for key, value in tuning.items():
            c.set_tuning(key, value)
        c.set_train(train, lab, 4)
        c.classify(q, 5, knn.L1 if metric is None else metric)
        p, name = c.last_candidate_path(), c.last_kernel_name()
        c.close()
        return p, name

    # key 0 or absent: path 1 at both sizes
    for q in (wide_q, big):
        assert path(wide, q)[0] == 1
        assert path(wide, q, u16l1w=0)[0] == 1
    # key 1: path 8, 4 waves for the small batch, 8 for the large
    assert path(wide, wide_q, u16l1w=1) == (8, "cand_fix16_wide_kernel<8,4>")
    assert path(wide, big, u16l1w=1) == (8, "cand_fix16_wide_kernel<8,8>")
    # the narrow pass's key moves no call at d = 300
    assert path(wide, wide_q, u16l1=1) == path(wide, wide_q)
    assert path(wide, wide_q, u16l1=1)[0] == 1
    # an integer train set: the exact byte-code pass wins where "i8l1" = 2
    # selects it; without it path 8 serves the set too
    assert path(ints, int_q, i8l1=2, u16l1w=1)[0] == 7
    assert path(ints, int_q, u16l1w=1)[0] == 8
    assert path(ints, int_q, i8l1=1, u16l1w=1)[0] == 8
    # L2 and d = 128 calls are unmoved
    for q in (wide_q, big):
        assert path(wide, q, metric=knn.L2, u16l1w=1) == path(wide, q, metric=knn.L2)
        assert path(wide, q, metric=knn.L2, u16l1w=1)[0] != 8
    assert path(narrow, narrow_q, u16l1w=1) == path(narrow, narrow_q)
    assert path(narrow, narrow_q, u16l1w=1)[0] == 1
    assert path(narrow, narrow_q, u16l1=1, u16l1w=1) == (8, "cand_fix16_kernel<128,8,4>")
    # a bad value is refused
    c = knn.Classifier(0)
    for bad in (-1, 2):
        with pytest.raises(knn.KnnError, match="u16l1w"):
            c.set_tuning("u16l1w", bad)
    g = knn.Group([0], mode=0)
    with pytest.raises(knn.KnnError, match="u16l1w"):
        g.set_tuning("u16l1w", 2)
    g.close()
    c.close()


# ------------------------------------------------------------------- 6. callers
def test_classify_sweep_equals_per_k_calls(knn):
    tr, lab, te = l1fixwide.uniform_norm(2000, 272)
    ks = [1, 3, 10]
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    labels, idx, dist, flags = c.classify_sweep(te, ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8 and c.last_kernel_name().startswith(WIDE)
    for j, k in enumerate(ks):
        got, kidx, kdist, kflags = c.classify(te, k, knn.L1, return_neighbors=True)
        assert c.last_candidate_path() == 8
        np.testing.assert_array_equal(labels[j], got)
        want = oracle.knn(tr, lab, te, k, False, 4)[0]
        np.testing.assert_array_equal(labels[j], want)
    np.testing.assert_array_equal(dist.view(np.int64), kdist.view(np.int64))
    c.close()


def test_loo_sweep_on_300_rows(knn):
    tr, lab, te = l1fixwide.uniform_norm(300, 257)
    ks = [1, 3, 10]
    want = loo.expected_excl(tr, lab, tr, np.arange(300), ks, False, 4)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    labels, correct, idx, dist, flags = c.loo_sweep(ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8 and c.last_kernel_name().startswith(WIDE)
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(correct, (want["labels"] == lab).sum(axis=1))
    np.testing.assert_array_equal(dist.view(np.int64), want["dist"].view(np.int64))
    c.close()


def test_distance_weighted_vote(knn):
    """VOTE_DISTANCE over the rows the pass reports: the search is the uniform
    call's, the labels are the rule's over those rows."""
    tr, lab, te = l1fixwide.uniform_norm(2000, 272)
    k = 10
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    l0, i0, d0, f0 = _check(knn, c, tr, lab, te, k, 4)
    c.set_vote(knn.VOTE_DISTANCE)
    l1, i1, d1, f1 = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8 and c.last_kernel_name().startswith(WIDE)
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(d1.view(np.int64), d0.view(np.int64))
    np.testing.assert_array_equal(l1, wvote.labels(wvote.lab_rows(lab, i1), d1, [k])[0])
    c.close()


def test_group_mode_1_equals_the_single_classifier(knn):
    tr, lab, te = l1fixwide.uniform_norm(2000, 784)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, 7, 4)
    c.close()
    g = knn.Group([0, 0, 0], mode=1)
    g.set_tuning("u16l1w", 1)
    g.set_train(tr, lab, 4)
    ggot, gidx, gdist, gflags = g.classify(te, 7, knn.L1, return_neighbors=True)
    np.testing.assert_array_equal(ggot, got)
    np.testing.assert_array_equal(gdist.view(np.int64), dist.view(np.int64))
    assert_neighbors_match(gidx, gdist, idx, dist, gflags | flags)
    g.close()

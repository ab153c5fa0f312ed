"""CPU checks of the 16-bit fixed-point L1 pass's coding and error bound
(tests/l1fix.py, Model; candidate path 8): on every data set of
test_gpu_l1fix.py and for every (query, row) pair, the unscaled integer proxy
is within the certification bound E of the oracle's fp64 L1 distance.  So that
the check cannot pass through a slack E, every query that is not clamped must
have E <= d 2^-e (1 + 2^-20) + the reference-rounding term, and the largest
proxy must stay an exact float (< 2^24)."""
import numpy as np
import pytest

import l1fix
import oracle


def check_bound(tr, te, finite=None):
    """The bound for every pair; returns the model."""
    m = l1fix.Model(tr, te)
    rows = np.arange(te.shape[0]) if finite is None else finite
    top = 0
    for q in rows:
        prox = m.proxies(q)
        top = max(top, int(prox.max()))
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        err = np.abs(np.ldexp(prox.astype(np.float64), -m.e) - ref)
        assert (err <= m.E[q]).all(), "query %d: error %g beyond E %g" % (q, err.max(), m.E[q])
    assert top < 1 << 24 and int(np.float32(top)) == top
    free = rows[~m.clamped[rows]]
    cap = np.ldexp(m.d * (1.0 + 2.0 ** -20), -m.e) + m.round_term[free]
    assert (m.E[free] <= cap).all(), "E of an unclamped query exceeds d code steps"
    # the train rows take at most a little over half the code range
    assert m.ct.min() >= l1fix.BIAS - 16400 and m.ct.max() <= l1fix.BIAS + 16400
    assert m.Dx <= 0.5 * m.d
    return m


@pytest.mark.parametrize("d", l1fix.SHAPE_D)
@pytest.mark.parametrize("n", l1fix.SHAPE_N)
@pytest.mark.parametrize("kind", l1fix.SHAPE_KINDS)
def test_bound_on_shape_sets(kind, n, d):
    tr, lab, te = l1fix.shape_set(kind, n, d)
    assert 40 <= te.shape[0] <= 199
    m = check_bound(tr, te)
    # queries drawn like the train rows: (nearly) none outside the headroom
    assert m.clamped.mean() <= 1.0 / 16.0


@pytest.mark.parametrize("d", [256, 255])
def test_bound_and_code_range_on_code_ends(d):
    tr, lab, te = l1fix.code_ends(d)
    assert (tr.min(0) == 0.0).all() and (tr.max(0) == 1.0).all()
    m = check_bound(tr, te)
    # the far queries take codes 0 and 65535 in every dim, nothing else clamps
    assert (m.cq[2] == 0).all() and (m.cq[3] == 65535).all()
    assert list(np.nonzero(m.clamped)[0]) == [2, 3]
    assert not np.isfinite(m.E[2:4]).all() or (m.E[2:4] > 90.0 * d).all()
    # the farthest row of the query on one end is the row on the other end
    assert int(np.argmax(m.proxies(0))) == 1 and int(np.argmax(m.proxies(1))) == 0
    assert int(max(m.proxies(2).max(), m.proxies(3).max())) > 40000 * d


@pytest.mark.parametrize("name", ["f3_l1", "f10_l1_int", "f4_normedge"])
def test_bound_on_the_reference_configuration(name):
    fx, tr, trl, te, va, val_ = l1fix.fixture_sets(name)
    assert fx.spec["Normalize"]
    check_bound(tr, te)
    check_bound(tr, va)
    if name != "f4_normedge":
        # transductive normalisation: test rows in [0, 1] next to the train
        # rows, inside the code headroom though not inside the train hull
        assert te.min() >= 0.0 and te.max() <= 1.0
        assert not l1fix.Model(tr, te).clamped.any()


def test_near_ties_sit_far_below_one_code_step():
    tr, lab, te, info, k, metric = l1fix.near_ties()
    assert metric == 1
    m = check_bound(tr, te)
    want, widx, wdist = oracle.knn(tr, lab, te, k + 1, False, 5, n_out=k + 1)
    step = 2.0 ** -m.e
    gap = wdist[:, k] - wdist[:, k - 1]
    assert (gap > 0).all()
    tight = np.array([i for i, ct in enumerate(info) if ct is not None and ct[1] <= -16])
    assert tight.size >= 8
    assert (gap[tight] < step / 16.0).all(), "k-th and (k+1)-th differ by %g code steps" % (
        gap[tight].max() / step)
    # ... between rows of different labels, for most of them
    assert (lab[widx[tight, k - 1]] != lab[widx[tight, k]]).mean() > 0.5


def test_duplicates_tie_across_the_kth_place():
    tr, lab, te = l1fix.duplicates()
    check_bound(tr, te)
    k = l1fix.DUP_K
    want, widx, wdist = oracle.knn(tr, lab, te, k + 1, False, 3, n_out=k + 1)
    assert (wdist[:, k - 1] == wdist[:, k]).all()
    assert (lab[widx[:, k - 1]] != lab[widx[:, k]]).all()


def test_handover_gaps_exceed_twice_the_bound():
    tr, lab, te, near, far, nan = l1fix.handover()
    assert (len(near) + len(far) + len(nan)) * 16 <= te.shape[0]
    ok = np.setdiff1d(np.arange(te.shape[0]), nan)
    m = check_bound(tr, te, finite=ok)
    assert list(np.nonzero(m.clamped[ok])[0]) == list(far)
    assert not m.clamped[near].any() and (te[near].max(1) > tr.max()).all()
    served = np.setdiff1d(ok, far)
    k, C = l1fix.HANDOVER_K, l1fix.HANDOVER_C
    want, widx, wdist = oracle.knn(tr, lab, te[served], C, False, 4, n_out=C)
    gap = wdist[:, C - 1] - wdist[:, k]  # (the W-th = (k + 1)-th to the C-th)
    assert (gap > 2.0 * m.E[served]).all(), "smallest gap / 2E = %g" % (gap / (2.0 * m.E[served])).min()
    # a clamped query's E is far beyond every gap: it cannot certify
    assert (m.E[far] > 10.0).all()


@pytest.mark.parametrize("kind", ["unequal", "constant", "far"])
def test_bound_on_odd_sets(kind):
    tr, lab, te = l1fix.odd_set(kind)
    m = check_bound(tr, te)
    if kind == "unequal":
        # the wide dim sets the scale: a dim spanning 1 takes a fraction of a step
        assert np.ldexp(1.0, m.e) < 0.05
    if kind == "constant":
        # extent 0: the scale is the cap's (max |x - mu| = 0 counts as < 2^0)
        assert (tr == tr[0]).all() and m.e == 14 and (m.ct == m.ct[0]).all()
        assert (te[:8] == tr[0]).all() and (m.Dq[:8] == m.Dx).all()
    if kind == "far":
        assert not m.clamped.any() and tr.min() >= 1e9


def test_padding_rule():
    assert [l1fix.pad_dim(d) for d in (1, 32, 33, 100, 128, 129, 161, 193, 256, 257)] == \
        [32, 32, 64, 128, 128, 160, 192, 256, 256, -1]

"""CPU checks of the wide 16-bit fixed-point L1 pass's bound (tests/l1fixwide.py,
Model; candidate path 8 at 256 < d <= 1024): on the data sets of
test_gpu_l1fixwide.py and for every (query, row) pair, the unscaled proxy as
the kernel hands it on -- the integer sum of code differences rounded once to
float -- is within the certification bound E of the oracle's fp64 L1 distance,
E carrying the rounding term r(DP).

The displaced set exercises the rounding.  No set can put EVERY sum of a
query at or above 2^25: the codes are centred on the train mean, so over the
train rows a query's sums average SUM_c |code_q,c - 32768| <= 1024 * 32768 =
2^25, with equality only for a query clamped to code 0 in every dim.  What the
set gives, and the test asserts: every sum is at or above 2^24 (every pair in
a rounding binade), the sums of every query against the low nine tenths of the
train rows are at or above 2^25 (the r = 2 binade) with no query clamped, and
in each binade some pair's float differs from its integer sum."""
import numpy as np
import pytest

import l1fixwide
import oracle


def check_bound(tr, te, finite=None):
    """The bound for every pair; returns (model, every integer proxy [rows, n])."""
    m = l1fixwide.Model(tr, te)
    rows = np.arange(te.shape[0]) if finite is None else finite
    allp = np.empty((len(rows), tr.shape[0]), np.int64)
    for i, q in enumerate(rows):
        prox = m.proxies(q)
        allp[i] = prox
        p32 = m.proxies32(q)
        assert (np.abs(p32 - prox) <= m.r).all()
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        err = np.abs(np.ldexp(p32, -m.e) - ref)
        assert (err <= m.E[q]).all(), "query %d: error %g beyond E %g" % (q, err.max(), m.E[q])
    assert int(allp.max()) < 1 << 26
    # so that the check cannot pass through a slack E: an unclamped query's E
    # is at most d + r code steps and the reference-rounding term
    free = rows[~m.clamped[rows]]
    cap = np.ldexp((m.d + m.r) * (1.0 + 2.0 ** -20), -m.e) + m.round_term[free]
    assert (m.E[free] <= cap).all(), "E of an unclamped query exceeds d + r code steps"
    assert m.ct.min() >= 32768 - 16400 and m.ct.max() <= 32768 + 16400
    assert m.Dx <= 0.5 * m.d
    return m, allp


def test_rounding_term_by_width():
    assert [l1fixwide.r_of(dp) for dp in (256, 272, 512, 528, 1024)] == [0, 1, 1, 2, 2]
    # half an ulp of the binade the largest sum of DP differences falls into
    for dp in (256, 512, 1024):
        top = 65535 * dp
        assert top < 1 << (24 + l1fixwide.r_of(dp))
        p = np.arange(top - 4096, top + 1, dtype=np.int64)
        assert np.abs(l1fixwide.fl32(p) - p).max() <= l1fixwide.r_of(dp)
    # ... and the bound is attained: r is not slack
    assert abs(float(l1fixwide.fl32([(1 << 24) + 1])[0]) - ((1 << 24) + 1)) == 1
    assert abs(float(l1fixwide.fl32([(1 << 25) + 2])[0]) - ((1 << 25) + 2)) == 2


def test_padding_rule():
    assert [l1fixwide.pad_dim(d) for d in (256, 257, 272, 273, 512, 513, 784, 1024, 1025)] == \
        [-1, 272, 272, 288, 512, 528, 784, 1024, -1]


@pytest.mark.parametrize("d", l1fixwide.SHAPE_D)
def test_bound_on_uniform_normalised_sets(d):
    tr, lab, te = l1fixwide.uniform_norm(300, d)
    assert tr.min() >= 0.0 and tr.max() <= 1.0
    m, allp = check_bound(tr, te[:33])
    assert not m.clamped.any()


def test_bound_and_gaps_on_the_784_dim_set():
    """The set of the GPU rescan-count check: every query's gap between its
    W-th and C-th distance exceeds 2 E, so the pass itself certifies it."""
    tr, lab, te = l1fixwide.uniform_norm(2000, 784)
    m, allp = check_bound(tr, te)
    assert not m.clamped.any()
    for k in l1fixwide.K_EDGES:
        C = max(2 * (k + 1), k + 1 + 16)
        want, widx, wdist = oracle.knn(tr, lab, te, C, False, 4, n_out=C)
        gap = wdist[:, C - 1] - wdist[:, k]  # (the W-th = (k + 1)-th to the C-th)
        assert (gap > 2.0 * m.E).all(), "k = %d: smallest gap / 2E = %g" % (
            k, (gap / (2.0 * m.E)).min())


def test_displaced_queries_exercise_the_rounding():
    tr, lab, te = l1fixwide.displaced()
    assert tr.shape[1] == 1024 and (te.min(1) > tr.max()).all()
    m, allp = check_bound(tr, te)
    assert m.r == 2 and not m.clamped.any()
    assert (allp >= 1 << 24).all()
    low = np.arange(tr.shape[0]) % 10 != 3
    assert (allp[:, low] >= 1 << 25).all() and (allp[:, ~low] < 1 << 25).all()
    f = l1fixwide.fl32(allp)
    assert (f[:, low] != allp[:, low]).any() and (f[:, ~low] != allp[:, ~low]).any()
    assert np.abs(f - allp).max() == 2


@pytest.mark.parametrize("kind", ["unequal", "constant"])
def test_bound_on_odd_sets(kind):
    tr, lab, te = l1fixwide.odd_set(kind)
    m, allp = check_bound(tr, te)
    if kind == "unequal":
        # the wide dim sets the scale: a dim spanning 1 takes 32 code steps
        assert np.ldexp(1.0, m.e) == 32.0
    else:
        assert (tr == tr[0]).all() and (m.ct == m.ct[0]).all()
        assert (te[:8] == tr[0]).all() and (m.Dq[:8] == m.Dx).all()


def test_bound_beside_a_nan_query():
    tr, lab, te, nan = l1fixwide.with_nan()
    ok = np.setdiff1d(np.arange(te.shape[0]), nan)
    check_bound(tr, te, finite=ok)

"""Numpy / plain-Python oracle of the distance-weighted vote (KNN_VOTE_DISTANCE,
include/knn_amd.h) and the data sets of its tests.

The rule, for one query with the ascending row dist[t] and l_t = the label of
entry t (-1: an empty slot, which counts nothing), at prefix length K:
    z = #{t < K : dist[t] == 0}
    z >= 1: entries t < z weigh 1.0, entries t >= z do not vote
    else:   w_t = 1.0 / dist[t]       (fp64; 1 / inf = 0)
    S[c] = 0; best = -inf; label = -1
    for t < K in row order (voting entries): S[l_t] += w_t
                                             if S[l_t] > best: best, label = S[l_t], l_t
Everything here is sequential fp64 (Python floats are IEEE doubles), so the
library's results can be compared with == / assert_array_equal.

Expected values never come from the library.
"""
import functools

import numpy as np

import evalcases
import oracle

KS = evalcases.KS_TIES  # [5, 1, 0, 37, 5, 10]: duplicates and a 0, unsorted
INF = float("inf")


def lab_rows(lab, idx, base=0):
    """Labels of neighbour rows idx [m, kmax] (global indices, -1 = empty)."""
    idx = np.asarray(idx, np.int64)
    lab = np.asarray(lab)
    out = np.full(idx.shape, -1, np.int32)
    ok = idx >= base
    out[ok] = lab[idx[ok] - base]
    return out


def _weights(lrow, drow):
    """Per entry (votes, weight) of one ascending row, for EVERY prefix at once:
    on an ascending row the zeros are the first entries, so "t < z" at prefix K
    is "dist[t] == 0" whenever the row starts with a zero."""
    d = [float(v) for v in drow]
    fin = [v for v in d if v == v]
    assert all(a <= b for a, b in zip(fin, fin[1:])), "rows must be ascending"
    zmode = len(d) > 0 and d[0] == 0.0
    out = []
    for lt, dt in zip(lrow, d):
        if lt < 0 or (zmode and dt != 0.0):
            out.append((False, 0.0))
        elif zmode:
            out.append((True, 1.0))
        else:
            out.append((True, 0.0 if dt == INF else 1.0 / dt))
    return out


def prefix_winners(lrow, drow):
    """win[K] = the rule's label at prefix length K, K = 0 .. len(row)."""
    S = {}
    best, label = -INF, -1
    win = [-1]
    for lt, (votes, w) in zip(lrow, _weights(lrow, drow)):
        if votes:
            lt = int(lt)
            s = S.get(lt, 0.0) + w
            S[lt] = s
            if s > best:
                best, label = s, lt
        win.append(label)
    return win


def labels(lab_rows_, dist_rows, ks):
    """labels int32[nk, m] of the rule over rows lab_rows_ / dist_rows [m, kmax]."""
    lab_rows_ = np.asarray(lab_rows_)
    m = lab_rows_.shape[0]
    out = np.empty((len(ks), m), np.int32)
    for q in range(m):
        win = prefix_winners(lab_rows_[q], dist_rows[q])
        for j, K in enumerate(ks):
            out[j, q] = win[int(K)]
    return out


def sums(lab_rows_, dist_rows, k, C):
    """Class sums float64[m, C] after the first k entries, each class added up
    in row order; labels outside [0, C) count nothing."""
    lab_rows_ = np.asarray(lab_rows_)
    m = lab_rows_.shape[0]
    out = np.zeros((m, C), np.float64)
    for q in range(m):
        lrow, drow = lab_rows_[q][:k], dist_rows[q][:k]
        S = [0.0] * C
        for lt, (votes, w) in zip(lrow, _weights(lrow, drow)):
            if votes and 0 <= lt < C:
                S[lt] = S[lt] + w
        out[q] = S
    return out


# ------------------------------------------------------------------ data sets
def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def grid4():
    """(a) integers 0..3 in 5 dims (1024 grid points, 2000 rows): nearly every
    query has exact matches (z >= 1) and class sums tie exactly."""
    rng = np.random.default_rng(7101)
    tr = rng.integers(0, 4, (2000, 5)).astype(np.float64)
    q = rng.integers(0, 4, (150, 5)).astype(np.float64)
    lab = rng.integers(0, 3, 2000).astype(np.int32)
    return _freeze(dict(tr=tr, q=q, lab=lab, classes=3))


def grid8(metric):
    """(b) the 8-level, 6-dim grid of evalcases.tie_data."""
    t = evalcases.tie_data(metric)
    return dict(tr=t["tr"], q=t["q"], lab=t["lab"], classes=3)


@functools.lru_cache(maxsize=None)
def clusters():
    """(c) real-valued clusters, 2000 x 300 at d = 8, 4 classes whose centres
    lie close together: the weighted and the uniform label differ on more than
    1 % of the (query, K) pairs."""
    rng = np.random.default_rng(7103)
    n, m, d, classes = 2000, 300, 8, 4
    centres = rng.uniform(-0.35, 0.35, (classes, d))
    lab = rng.integers(0, classes, n + m).astype(np.int32)
    X = centres[lab] + rng.standard_normal((n + m, d))
    return _freeze(dict(tr=X[:n].copy(), q=X[n:].copy(), lab=lab[:n].copy(), classes=classes))


def dataset(name, metric):
    return grid4() if name == "a" else grid8(metric) if name == "b" else clusters()


@functools.lru_cache(maxsize=None)
def expected(name, metric):
    """The CPU oracle's own rows (the reference's std::sort order) at kmax =
    max(KS), the rule's labels over them and the uniform labels at KS."""
    d = dataset(name, metric)
    kmax = max(KS)
    _, idx, dist = oracle.knn(d["tr"], d["lab"], d["q"], kmax, metric == 0, d["classes"],
                              n_out=kmax)
    lrows = lab_rows(d["lab"], idx)
    out = dict(idx=idx, dist=dist, lrows=lrows, weighted=labels(lrows, dist, KS),
               uniform=evalcases.oracle_labels(d["tr"], d["lab"], d["q"], KS, metric == 0,
                                               d["classes"]))
    return _freeze(out)


def top_sum_ties(lrows, dist, k, C):
    """Queries whose two largest class sums after k entries are exactly equal."""
    s = np.sort(sums(lrows, dist, k, C), axis=1)
    return (s[:, -1] == s[:, -2]) & (s[:, -1] > 0)


# --------------------------------------------------- synthetic rows (no search)
def synthetic_rows(m, kmax, n_lab, C, seed):
    """Ordered rows for the building blocks: ascending distances from a coarse
    grid (so classes tie on exactly equal sums), with
      row 0: z = 0            row 1: z = 1          row 2: z = kmax
      row 3: starts with -1 (no neighbours: idx -1, dist +inf throughout)
      row 4: -1 slots with +inf distances at the end
      row 5: an inf distance under a valid index, then empty slots
      row 6: every distance equal (equal class sums wherever counts are equal)
      row 7: valid indices at distance +inf (every weight 0: the label is l_0)
    wherever m is large enough; the rest random, a third starting with zeros."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_lab, (m, kmax)).astype(np.int64)
    dist = np.sort(rng.integers(1, 9, (m, kmax)).astype(np.float64) / 4.0, axis=1)
    nz = np.where(rng.random(m) < 0.33, rng.integers(1, kmax + 1, m), 0)
    for q in range(m):
        dist[q, :nz[q]] = 0.0
    tail = np.where(rng.random(m) < 0.3, rng.integers(0, kmax + 1, m), 0)  # empty slots
    for q in range(m):
        if tail[q]:
            idx[q, kmax - tail[q]:] = -1
            dist[q, kmax - tail[q]:] = INF

    def put(q, d_row, i_row=None):
        if q < m:
            dist[q] = d_row
            if i_row is not None:
                idx[q] = i_row
            else:
                idx[q] = np.where(idx[q] < 0, 0, idx[q])

    asc = np.sort(rng.integers(1, 9, kmax).astype(np.float64) / 4.0)
    put(0, asc)
    z1 = asc.copy()
    z1[0] = 0.0
    put(1, z1)
    put(2, np.zeros(kmax))
    put(3, np.full(kmax, INF), np.full(kmax, -1, np.int64))
    if kmax >= 3:
        r4, i4 = asc.copy(), np.where(idx[min(4, m - 1)] < 0, 1, idx[min(4, m - 1)])
        r4[kmax - kmax // 3:] = INF
        i4[kmax - kmax // 3:] = -1
        put(4, r4, i4)
        r5, i5 = asc.copy(), np.where(idx[min(5, m - 1)] < 0, 2, idx[min(5, m - 1)])
        cut = kmax - kmax // 3
        r5[cut - 1:] = INF  # entry cut - 1 keeps its index: weight 1 / inf = 0
        i5[cut:] = -1
        put(5, r5, i5)
    put(6, np.full(kmax, 0.5))
    put(7, np.full(kmax, INF))  # valid indices, every weight 0: the label is l_0
    return idx, dist

"""Data sets and expected values of the leave-one-out K sweep tests.

The expected values come from the CPU oracle alone.  One rule defines them:
for a query with excluded train row e the result is the K sweep's on the train
set WITH ROW e REMOVED (np.delete on rows and labels), indices >= e mapped
back by j -> j + (j >= e).  `expected_loo` is the special case where the
queries are train rows and each excludes itself.

`naive` is the answer of a build that drops the row but keeps the plain
(dist, index) order: the (dist, index)-ordered top (kmax + 1) of the full set
minus the excluded row, prefix-voted.  It is the library's answer at "ties" =
0, and where it differs from the oracle at some K the row is ORDER-SENSITIVE:
only the reference's std::sort order over the n - 1 remaining records gives
its label.  A row is in DROP CASE TWO when the excluded row is not inside the
top (kmax + 1) of the full set (more than kmax rows at distance 0 and of lower
index, for a leave-one-out query).
"""
import functools

import numpy as np

import oracle

KS_A = [1, 2, 3, 4, 5, 7, 10, 11, 20, 37]
# name: grid levels, dims, seed, rows, classes, metric (0 L2, 1 L1), ks
SETS = {
    "A": dict(levels=8, dims=6, seed=101, n=1500, classes=3, metric=0, ks=KS_A),
    "A1": dict(levels=8, dims=6, seed=102, n=1500, classes=3, metric=1, ks=KS_A),
    "B": dict(levels=3, dims=4, seed=103, n=600, classes=3, metric=0, ks=[1, 2, 3, 5]),
}
FLAG_MASK = 2 | 4 | 8 | 32  # TIE_BOUNDARY | TIE_VOTE | TIE_ORDER | TIE_REF


def grid(levels, dims, seed, n, classes):
    """Integer grid rows, then labels, from one default_rng(seed)."""
    rng = np.random.default_rng(seed)
    tr = rng.integers(0, levels, (n, dims)).astype(np.float64)
    lab = rng.integers(0, classes, n).astype(np.int32)
    return tr, lab


@functools.lru_cache(maxsize=None)
def data(name):
    s = SETS[name]
    tr, lab = grid(s["levels"], s["dims"], s["seed"], s["n"], s["classes"])
    tr.setflags(write=False)
    lab.setflags(write=False)
    return tr, lab


def vote(labels):
    """cpp:324-337: the first label whose count strictly exceeds the running max."""
    cnt, best, win = {}, 0, -1
    for l in labels:
        c = cnt.get(int(l), 0) + 1
        cnt[int(l)] = c
        if c > best:
            best, win = c, int(l)
    return win


def expected_excl(tr, lab, Q, excl, ks, euclid, classes):
    """The oracle on the row-removed sets: labels [nk, m], idx [m, kmax] (full
    train set indices), dist [m, kmax].  excl[i] = -1 removes nothing."""
    ks = [int(k) for k in ks]
    kmax = max(ks)
    m = Q.shape[0]
    labels = np.empty((len(ks), m), np.int32)
    idx = np.empty((m, kmax), np.int64)
    dist = np.empty((m, kmax), np.float64)
    for i in range(m):
        e = int(excl[i])
        t, l = (np.delete(tr, e, 0), np.delete(lab, e)) if e >= 0 else (tr, lab)
        cache = {}
        for k in sorted(set(ks)):
            n_out = kmax if k == kmax else 0
            got = oracle.knn(t, l, Q[i:i + 1], k, euclid, classes, n_out=n_out, nthreads=1)
            cache[k] = got[0][0]
            if n_out:
                j = got[1][0]
                idx[i] = j + (j >= e) if e >= 0 else j
                dist[i] = got[2][0]
        labels[:, i] = [cache[k] for k in ks]
    return dict(labels=labels, idx=idx, dist=dist)


def naive(tr, lab, Q, excl, ks, euclid):
    """The (dist, index) order minus the excluded row: labels [nk, m], idx /
    dist [m, kmax], the flag bits a kmax search on the reduced set reports
    (TIE_BOUNDARY 2, TIE_VOTE 4, TIE_ORDER 8), `queued` [m] (the rows whose
    label at some K of the list the order among equal distances could change:
    the "ties" = 1 rule of the sweep, TIE_REF), `tied` [m] (any tie in the top
    kmax or across its boundary: "ties" = 2) and `case2` [m]."""
    ks = [int(k) for k in ks]
    kmax = max(ks)
    m, n = Q.shape[0], tr.shape[0]
    ar = np.arange(n)
    labels = np.empty((len(ks), m), np.int32)
    idx = np.empty((m, kmax), np.int64)
    dist = np.empty((m, kmax), np.float64)
    flags = np.zeros(m, np.int32)
    queued = np.zeros(m, bool)
    case2 = np.zeros(m, bool)
    for i in range(m):
        e = int(excl[i])
        D = oracle.row_distances(Q[i], tr, euclid)
        order = np.lexsort((ar, D))
        case2[i] = e not in order[:kmax + 1]
        order = order[order != e][:kmax + 1]  # the reduced top kmax and its successor
        d, l = D[order], lab[order]
        idx[i], dist[i] = order[:kmax], d[:kmax]
        eq = d[1:] == d[:-1]  # eq[t]: entries t and t + 1 at one distance
        inside = eq[:kmax - 1]
        if len(order) > kmax and eq[kmax - 1]:
            flags[i] |= 2
        if (inside & (l[1:kmax] != l[:kmax - 1])).any():
            flags[i] |= 4
        if (inside & (l[1:kmax] == l[:kmax - 1])).any():
            flags[i] |= 8
        for j, k in enumerate(ks):
            w = vote(l[:k])
            labels[j, i] = w
            if k == 0:
                continue
            cnt = np.bincount(l[:k], minlength=int(lab.max()) + 1)
            M = cnt[w]
            cnt[w] = 0
            m2 = cnt.max()
            bnd = k < len(order) and d[k - 1] == d[k]
            gin = int((d[:k] == d[k - 1]).sum())  # (sorted: the run ending at k - 1)
            tie4 = (eq[:k - 1] & (l[1:k] != l[:k - 1])).any()
            if (bnd and M - m2 <= 2 * gin) or (tie4 and m2 == M):
                queued[i] = True
    return dict(labels=labels, idx=idx, dist=dist, flags=flags, queued=queued,
                tied=(flags & 14) != 0, case2=case2)


@functools.lru_cache(maxsize=None)
def expected_loo(name):
    """Leave-one-out over every row of data set `name`: the oracle's labels
    [nk, n], correct [nk], idx / dist [n, kmax]; plus the naive answer, the
    order-sensitive rows and, at "ties" = 1, the expected flag bits and
    indices (the oracle's order on the queued rows, (dist, index) elsewhere)."""
    s = SETS[name]
    tr, lab = data(name)
    rows = np.arange(s["n"])
    want = expected_excl(tr, lab, tr, rows, s["ks"], s["metric"] == 0, s["classes"])
    nv = naive(tr, lab, tr, rows, s["ks"], s["metric"] == 0)
    want["correct"] = (want["labels"] == lab).sum(axis=1).astype(np.int64)
    want["naive"] = nv
    want["sensitive"] = (nv["labels"] != want["labels"]).any(axis=0)
    want["flags1"] = nv["flags"] | np.where(nv["queued"], 32, 0).astype(np.int32)
    want["idx1"] = np.where(nv["queued"][:, None], want["idx"], nv["idx"])
    return want


def duplicates(tr):
    """Rows with an exact duplicate elsewhere in the set."""
    _, inv, cnt = np.unique(tr, axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)] > 1

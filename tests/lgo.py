"""Data sets and expected values of the leave-group-out K sweep tests.

The expected values come from the CPU oracle alone, by the set form of
loo.expected_excl: for a query with group gq the result is the K sweep's on the
train set WITH EVERY ROW OF GROUP gq REMOVED (rows and labels), the indices
mapped back to the full set through the kept rows' numbers.

`naive` is the answer of a build that drops the group but keeps the plain
(dist, index) order: the library's answer at "ties" = 0.  It also reports what
the drop kernel's cases look like for each query: `c`, the number of the
group's rows inside the (dist, index)-ordered top k1 = kmax + gmax of the full
set, and the boundary bit by each of the two formulas (`bnd_in`: read inside
the k1-entry row, `bnd_out`: the full order's dist[k1 - 1] == dist[k1]).
"""
import functools

import numpy as np

import loo
import oracle

KS_G = loo.KS_A
# name: seed, metric (0 L2, 1 L1); all: n = 1500, 6 dims, 8 levels, 3 classes
SETS = {
    "G": dict(seed=301, metric=0, n=1500, classes=3, ks=KS_G),
    "G1": dict(seed=302, metric=1, n=1500, classes=3, ks=KS_G),
}
GMAX = 7


def grouped(seed, n, classes, levels=8, dims=6, gmax=GMAX):
    """Rows on the integer grid in groups of 1..gmax near rows (a base point,
    members off it by at most one level in at most two dims: samples of one
    subject), exact duplicates inside a group and across groups, then one
    shuffle of the row order.  Returns (rows, labels, groups)."""
    rng = np.random.default_rng(seed)
    rows, lab, grp = [], [], []
    g = 0
    while len(rows) < n:
        size = int(min(rng.integers(1, gmax + 1), n - len(rows)))
        base = rng.integers(0, levels, dims)
        glab = int(rng.integers(0, classes))
        first = len(rows)
        for j in range(size):
            u = rng.random()
            if j and u < 0.15:  # an exact duplicate inside the group
                x = rows[first + int(rng.integers(0, j))].copy()
            elif first and u > 0.92:  # an exact duplicate of a row of an earlier group
                x = rows[int(rng.integers(0, first))].copy()
            else:
                x = base.copy()
                for dd in rng.choice(dims, 2, replace=False):
                    x[dd] = np.clip(x[dd] + rng.integers(-1, 2), 0, levels - 1)
            rows.append(x)
            lab.append(glab if rng.random() < 0.7 else int(rng.integers(0, classes)))
            grp.append(g)
        g += 1
    perm = rng.permutation(n)
    tr = np.array(rows, np.float64)[perm]
    return tr, np.array(lab, np.int32)[perm], np.array(grp, np.int32)[perm]


@functools.lru_cache(maxsize=None)
def data(name):
    s = SETS[name]
    out = grouped(s["seed"], s["n"], s["classes"])
    for a in out:
        a.setflags(write=False)
    return out


def expected_gexcl(tr, lab, groups, Q, qgroup, ks, euclid, classes):
    """The oracle on the group-removed sets: labels [nk, m], idx [m, kmax]
    (full train set indices), dist [m, kmax].  A qgroup no row carries removes
    nothing."""
    ks = [int(k) for k in ks]
    kmax = max(ks)
    m = Q.shape[0]
    labels = np.empty((len(ks), m), np.int32)
    idx = np.empty((m, kmax), np.int64)
    dist = np.empty((m, kmax), np.float64)
    sets = {}
    for i in range(m):
        gq = int(qgroup[i])
        if gq not in sets:
            keep = np.flatnonzero(groups != gq)
            sets[gq] = (keep, np.ascontiguousarray(tr[keep]), np.ascontiguousarray(lab[keep]))
        keep, t, l = sets[gq]
        cache = {}
        for k in sorted(set(ks)):
            n_out = kmax if k == kmax else 0
            got = oracle.knn(t, l, Q[i:i + 1], k, euclid, classes, n_out=n_out, nthreads=1)
            cache[k] = got[0][0]
            if n_out:
                idx[i] = keep[got[1][0]]
                dist[i] = got[2][0]
        labels[:, i] = [cache[k] for k in ks]
    return dict(labels=labels, idx=idx, dist=dist)


def naive(tr, lab, groups, Q, qgroup, ks, euclid, gmax):
    """The (dist, index) order minus the group, as loo.naive: labels, idx,
    dist, flags (TIE_BOUNDARY 2, TIE_VOTE 4, TIE_ORDER 8 of a kmax search on
    the reduced set), `queued`, `tied`; and per query `c`, `bnd_in`, `bnd_out`,
    `bnd_last` (see the module text; bnd_last: the last kept entry of the k1
    row is its entry k1 - 1)."""
    ks = [int(k) for k in ks]
    kmax = max(ks)
    k1 = kmax + gmax
    m, n = Q.shape[0], tr.shape[0]
    ar = np.arange(n)
    labels = np.empty((len(ks), m), np.int32)
    idx = np.empty((m, kmax), np.int64)
    dist = np.empty((m, kmax), np.float64)
    flags = np.zeros(m, np.int32)
    queued = np.zeros(m, bool)
    c = np.zeros(m, np.int64)
    bnd_in = np.zeros(m, bool)
    bnd_out = np.zeros(m, bool)
    bnd_last = np.zeros(m, bool)
    for i in range(m):
        gq = int(qgroup[i])
        D = oracle.row_distances(Q[i], tr, euclid)
        full = np.lexsort((ar, D))
        row = full[:k1]
        kept = row[groups[row] != gq]
        c[i] = k1 - len(kept)
        bnd_in[i] = len(kept) > kmax and D[kept[kmax - 1]] == D[kept[kmax]]
        bnd_out[i] = k1 < n and D[full[k1 - 1]] == D[full[k1]]
        bnd_last[i] = groups[row[-1]] != gq
        order = full[groups[full] != gq][:kmax + 1]  # the reduced top kmax and its successor
        d, l = D[order], lab[order]
        idx[i], dist[i] = order[:kmax], d[:kmax]
        eq = d[1:] == d[:-1]
        inside = eq[:kmax - 1]
        if len(order) > kmax and eq[kmax - 1]:
            flags[i] |= 2
        if (inside & (l[1:kmax] != l[:kmax - 1])).any():
            flags[i] |= 4
        if (inside & (l[1:kmax] == l[:kmax - 1])).any():
            flags[i] |= 8
        for j, k in enumerate(ks):
            w = loo.vote(l[:k])
            labels[j, i] = w
            if k == 0:
                continue
            cnt = np.bincount(l[:k], minlength=int(lab.max()) + 1)
            M = cnt[w]
            cnt[w] = 0
            m2 = cnt.max()
            bnd = k < len(order) and d[k - 1] == d[k]
            gin = int((d[:k] == d[k - 1]).sum())
            tie4 = (eq[:k - 1] & (l[1:k] != l[:k - 1])).any()
            if (bnd and M - m2 <= 2 * gin) or (tie4 and m2 == M):
                queued[i] = True
    return dict(labels=labels, idx=idx, dist=dist, flags=flags, queued=queued,
                tied=(flags & 14) != 0, c=c, bnd_in=bnd_in, bnd_out=bnd_out, bnd_last=bnd_last)


def expected(tr, lab, groups, Q, qgroup, ks, euclid, classes, gmax):
    """Oracle + naive answers and, at "ties" = 1, the expected flag bits and
    indices (the oracle's order on the queued rows, (dist, index) elsewhere)."""
    want = expected_gexcl(tr, lab, groups, Q, qgroup, ks, euclid, classes)
    nv = naive(tr, lab, groups, Q, qgroup, ks, euclid, gmax)
    want["naive"] = nv
    want["sensitive"] = (nv["labels"] != want["labels"]).any(axis=0)
    want["flags1"] = nv["flags"] | np.where(nv["queued"], 32, 0).astype(np.int32)
    want["idx1"] = np.where(nv["queued"][:, None], want["idx"], nv["idx"])
    return want


def group_max(groups):
    return int(np.bincount(groups).max())


@functools.lru_cache(maxsize=None)
def expected_lgo(name):
    """Leave-group-out over every row of data set `name`."""
    s = SETS[name]
    tr, lab, groups = data(name)
    want = expected(tr, lab, groups, tr, groups, s["ks"], s["metric"] == 0, s["classes"],
                    group_max(groups))
    want["correct"] = (want["labels"] == lab).sum(axis=1).astype(np.int64)
    return want

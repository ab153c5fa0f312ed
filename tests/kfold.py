"""Cases and expected values of the K-fold sweep tests (knn_set_folds,
knn_kfold_sweep*).

The rule is knn_lgo_sweep's with groups = folds, so the expected values are
tests/lgo.py's, unchanged: lgo.expected runs the CPU oracle on the FOLD-REMOVED
train sets (rows and labels of the query's fold taken out, indices mapped back)
and lgo.naive gives the (dist, index) order minus the fold, the flag bits and
the rows the sweep tie scan queues.  Data: lgo.grouped -- small-integer grids
with near rows and exact duplicates, so exact distance ties are common.
"""
import functools

import numpy as np

import lgo
import oracle

KS = [1, 2, 3, 5, 8, 20]


def _contiguous(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)


def _dups():
    """Rows 100..199 are exact copies of rows 0..99 and lie in the other fold:
    every row has a distance-0 neighbour that must stay."""
    tr, lab, _ = lgo.grouped(415, 100, 3)
    return np.concatenate([tr, tr]), np.concatenate([lab, lab]), _contiguous([100, 100])


# name: data (rows, labels, folds), n_folds, metric (0 L2, 1 L1), classes, ks
def _case(name):
    if name in ("inter_l2", "inter_l1"):  # interleaved folds, row % 4
        tr, lab, _ = lgo.grouped(411, 600, 3)
        return tr, lab, (np.arange(600) % 4).astype(np.int32), 4, int(name == "inter_l1"), 3, KS
    if name == "unequal":  # contiguous folds, one the largest by far
        tr, lab, _ = lgo.grouped(412, 600, 3)
        return tr, lab, _contiguous([97, 150, 203, 150]), 4, 0, 3, KS
    if name == "two":
        tr, lab, _ = lgo.grouped(413, 301, 3)
        return tr, lab, (np.arange(301) % 2).astype(np.int32), 2, 0, 3, KS
    if name == "small":  # folds below kmax + 1 = 13 rows: padded partial lists
        tr, lab, _ = lgo.grouped(414, 40, 3)
        return tr, lab, _contiguous([6, 10, 12, 12]), 4, 0, 3, [1, 3, 12]
    if name == "dups":
        tr, lab, folds = _dups()
        return tr, lab, folds, 2, 0, 3, [1, 2, 3, 5, 8]
    raise KeyError(name)


CASES = ("inter_l2", "inter_l1", "unequal", "two", "small", "dups")


@functools.lru_cache(maxsize=None)
def case(name):
    tr, lab, folds, F, metric, classes, ks = _case(name)
    for a in (tr, lab, folds):
        a.setflags(write=False)
    return dict(tr=tr, lab=lab, folds=folds, F=F, metric=metric, classes=classes, ks=list(ks),
                n=tr.shape[0], fold_max=int(np.bincount(folds).max()))


@functools.lru_cache(maxsize=None)
def expected(name):
    """lgo.expected over every row with groups = folds, plus `correct`."""
    s = case(name)
    w = lgo.expected(s["tr"], s["lab"], s["folds"], s["tr"], s["folds"], s["ks"],
                     s["metric"] == 0, s["classes"], s["fold_max"])
    w["correct"] = (w["labels"] == s["lab"]).sum(axis=1).astype(np.int64)
    return w


def nearest_in_own_fold(name):
    """Rows whose nearest other row (by (dist, index)) lies in their own fold:
    for them holding the fold out changes the neighbour list."""
    s = case(name)
    tr, folds, n = s["tr"], s["folds"], s["n"]
    ar = np.arange(n)
    out = np.zeros(n, bool)
    for i in range(n):
        D = oracle.row_distances(tr[i], tr, s["metric"] == 0)
        order = np.lexsort((ar, D))
        first = order[order != i][0]
        out[i] = folds[first] == folds[i]
    return out


def confusion(labels, truth, C):
    """conf int64[nk, C, C] (row = truth), unl int64[nk] of labels [nk, m]."""
    nk = labels.shape[0]
    conf = np.zeros((nk, C, C), np.int64)
    unl = np.zeros(nk, np.int64)
    for j in range(nk):
        ok = (labels[j] >= 0) & (labels[j] < C)
        np.add.at(conf[j], (truth[ok], labels[j][ok]), 1)
        unl[j] = (~ok).sum()
    return conf, unl

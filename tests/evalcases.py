"""Data sets and expected values of the per-class evaluation tests.

Expected values never come from the library: confusion matrices are numpy
(np.add.at) over the CPU oracle's labels at each K, vote counts np.bincount
over the oracle's neighbour indices.
"""
import functools

import numpy as np

import oracle

# the LDS regimes of eval_confusion_kernel: per-wave copies up to
# SMALL_C classes, one histogram per workgroup up to LDS_C, global atomics
# beyond; eval_vote_counts_kernel keeps LDS counters up to COUNTS_LDS_C classes
SMALL_C, LDS_C, COUNTS_LDS_C = 16, 96, 1024
KS_TIES = [5, 1, 0, 37, 5, 10]  # duplicates and a 0, unsorted


def regime(C):
    return 0 if C <= SMALL_C else 1 if C <= LDS_C else 2


def confusion(labels, truth, C):
    """conf int64[nk, C, C] (row = truth, column = label) and unl int64[nk]
    of labels [nk, m] against truth [m]; a pair with either value outside
    [0, C) is unlabelled."""
    labels = np.asarray(labels, np.int64)
    truth = np.asarray(truth, np.int64)
    nk = labels.shape[0]
    conf = np.zeros((nk, C, C), np.int64)
    unl = np.zeros(nk, np.int64)
    tok = (truth >= 0) & (truth < C)
    for i in range(nk):
        ok = tok & (labels[i] >= 0) & (labels[i] < C)
        np.add.at(conf[i], (truth[ok], labels[i][ok]), 1)
        unl[i] = (~ok).sum()
    return conf, unl


def oracle_labels(tr, lab, q, ks, euclid, classes):
    """labels[nk, m] of the oracle, one run per distinct K (K = 0: -1)."""
    cache = {}
    for k in sorted(set(int(k) for k in ks)):
        cache[k] = (np.full(q.shape[0], -1, np.int32) if k == 0
                    else oracle.knn(tr, lab, q, k, euclid, classes)[0])
    return np.stack([cache[int(k)] for k in ks])


@functools.lru_cache(maxsize=None)
def tie_data(metric):
    """The tie-heavy construction of test_gpu_sweep.py: an 8-level integer grid
    in 6 dims, 3 classes; the oracle's labels at KS_TIES and a random truth."""
    rng = np.random.default_rng(301 + metric)
    tr = rng.integers(0, 8, (2000, 6)).astype(np.float64)
    q = rng.integers(0, 8, (150, 6)).astype(np.float64)
    lab = rng.integers(0, 3, 2000).astype(np.int32)
    truth = np.random.default_rng(17 + metric).integers(0, 3, 150).astype(np.int32)
    want = oracle_labels(tr, lab, q, KS_TIES, metric == 0, 3)
    for a in (tr, q, lab, truth, want):
        a.setflags(write=False)
    return dict(tr=tr, q=q, lab=lab, truth=truth, want=want, classes=3, ks=KS_TIES)


KS_CODES = [1, 3, 10]


@functools.lru_cache(maxsize=None)
def codes_data():
    """10 classes of byte codes / 256 at d = 16: 4096 queries, the batch size
    at which AUTO takes the int8 candidate passes (L2 path 5 / 6, L1 path 7).
    Truth = the generating class."""
    rng = np.random.default_rng(411)
    n, m, d, classes = 3000, 4096, 16, 10
    centres = rng.uniform(105, 150, (classes, d))  # overlapping: off-diagonal counts
    lab = rng.integers(0, classes, n + m).astype(np.int32)
    X = np.clip(np.rint(centres[lab] + 25 * rng.standard_normal((n + m, d))), 0, 255) / 256.0
    tr, q = X[:n].copy(), X[n:].copy()
    out = dict(tr=tr, q=q, lab=lab[:n].copy(), truth=lab[n:].copy(), classes=classes, ks=KS_CODES)
    for metric in (0, 1):
        out["want%d" % metric] = oracle_labels(tr, out["lab"], q, KS_CODES,
                                               metric == 0, classes)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def vote_counts(lab, idx, k, C):
    """counts int32[m, C] of the labels among the first k entries of idx [m,
    >= k] (-1 = an empty slot)."""
    out = np.zeros((idx.shape[0], C), np.int32)
    for i in range(idx.shape[0]):
        row = idx[i, :k]
        out[i] = np.bincount(lab[row[row >= 0]], minlength=C)
    return out


@functools.lru_cache(maxsize=None)
def loo_big():
    """n = 16384 + 37 rows at d = 8 (crosses the leave-one-out batch boundary),
    4 classes, real-valued so that exact ties do not occur."""
    rng = np.random.default_rng(523)
    n, d, classes = 16384 + 37, 8, 4
    centres = rng.uniform(-2, 2, (classes, d))
    lab = rng.integers(0, classes, n).astype(np.int32)
    tr = centres[lab] + rng.standard_normal((n, d))
    tr.setflags(write=False)
    lab.setflags(write=False)
    return tr, lab, classes

"""Data sets and comparison helpers of the L1-on-int8-codes tests (candidate
path 7, csrc/knn_cand_sad.hip).

Every train set here is integer-coded: each value is (cent_i + c) / 2^s with a
code c in [-128, 127] per dimension, so the library's detect_i8 accepts it and
the L1 pass may run on the codes.  `proxy_model` is a numpy restatement of
what the kernel computes (the integer sum of absolute code differences); the
CPU tests check it against the oracle's fp64 L1 distance, which is the
exactness claim independent of any kernel.
"""
import functools

import numpy as np

import datagen


def int_sets(n, m, d, classes=4, seed=None):
    """datagen "int": train [n, d], labels [n], queries [m, d]."""
    seed = n * 31 + d if seed is None else seed
    tr, lab, te, _, _, _ = datagen.make_sets("int", seed, n, m, 0, d, classes)
    return tr, lab, te


# case 1: (n, d) shape edges; every k of K_EDGES that is < n, and k = n - 1 at n = 31
SHAPE_N = (31, 257, 6000)
SHAPE_D = (1, 6, 13, 32, 100, 128, 256)
K_EDGES = (1, 7, 30)


def shape_m(n, d):
    return 40 + (n * 7 + d * 3) % 160  # 40 .. 199, ragged


@functools.lru_cache(maxsize=None)
def byte_ends(d):
    """Case 2: codes at both ends of the byte in every dim.  Row 0 all 0, row 1
    all 255, rows 2..5 half / alternating ends, the rest mixed; queries 0 / 1
    sit on the two ends.  Returns (train, labels, queries)."""
    rng = np.random.default_rng(700 + d)
    n = 48
    tr = rng.integers(0, 256, (n, d)).astype(np.float64)
    tr[0] = 0.0
    tr[1] = 255.0
    tr[2, : d // 2], tr[2, d // 2:] = 0.0, 255.0
    tr[3, : d // 2], tr[3, d // 2:] = 255.0, 0.0
    tr[4, 0::2], tr[4, 1::2] = 0.0, 255.0
    tr[5, 0::2], tr[5, 1::2] = 255.0, 0.0
    # rows between the ends in every dim: a ramp, and values next to each end
    tr[6] = np.arange(d) % 256
    tr[7] = 1.0
    tr[8] = 254.0
    tr[9] = 127.0
    tr[10] = 128.0
    lab = (np.arange(n) % 3).astype(np.int32)
    te = rng.integers(0, 256, (40, d)).astype(np.float64)
    te[0] = 0.0
    te[1] = 255.0
    te[2] = tr[2]
    te[3] = tr[5]
    return tr, lab, te


def byte_ends_max(d):
    """The largest integer proxy of byte_ends(d) over all (query, row) pairs."""
    tr, _, te = byte_ends(d)
    return int(np.abs(te[:, None, :] - tr[None, :, :]).sum(2).max())


@functools.lru_cache(maxsize=None)
def offset_grid(kind):
    """Case 3: "offset" = values 1000000 + c (centre far from 0, s = 0),
    "eighths" = values c / 8 (s = 3); c in 0..255.  Dim 0 is constant, dim 1
    spans exactly 255 codes.  Returns (train, labels, queries, s)."""
    rng = np.random.default_rng(41 if kind == "offset" else 43)
    n, m, d = 3000, 60, 10
    c = rng.integers(0, 256, (n + m, d))
    c[:, 0] = 77
    c[:n, 1] = rng.integers(0, 256, n)
    c[0, 1], c[1, 1] = 0, 255
    c[:, 2] = rng.integers(100, 110, n + m)  # a narrow dim
    c[2, 3:], c[3, 3:] = 0, 255              # the other dims span the byte too
    x = c.astype(np.float64)
    x, s = (1000000.0 + x, 0) if kind == "offset" else (x / 8.0, 3)
    lab = rng.integers(0, 4, n).astype(np.int32)
    return x[:n].copy(), lab, x[n:].copy(), s


def proxy_model(tr, te, s):
    """What path 7 computes: per dim the centre the library derives
    (floor((lo + hi + 1) / 2) of the scaled train range), signed codes, the
    top bit of every byte flipped, and the integer sum of absolute
    differences of the unsigned bytes.  Returns int64 [m, n]; raises if a
    value is off the grid or a code leaves the byte."""
    T, Q = np.ldexp(tr, s), np.ldexp(te, s)
    lo, hi = T.min(0), T.max(0)
    cent = np.floor((lo + hi + 1.0) / 2.0)
    ct, cq = T - cent, Q - cent
    assert (ct == np.rint(ct)).all() and (cq == np.rint(cq)).all(), "off the grid"
    assert ct.min() >= -128 and ct.max() <= 127 and cq.min() >= -128 and cq.max() <= 127
    ut = (ct.astype(np.int64) & 0xFF) ^ 0x80
    uq = (cq.astype(np.int64) & 0xFF) ^ 0x80
    return np.abs(uq[:, None, :] - ut[None, :, :]).sum(2)


TIE_K = 30  # the place at which tie_grid's typical query has dozens of equal rows


@functools.lru_cache(maxsize=None)
def tie_grid():
    """Case 4: a 0..3 grid at d = 6, n = 600: dozens of rows share the
    distance at the TIE_K-th place.  Returns (train, labels, queries)."""
    rng = np.random.default_rng(404)
    tr = rng.integers(0, 4, (600, 6)).astype(np.float64)
    lab = rng.integers(0, 3, 600).astype(np.int32)
    te = rng.integers(0, 4, (64, 6)).astype(np.float64)
    return tr, lab, te


@functools.lru_cache(maxsize=None)
def handover():
    """Case 5: 160 queries against a 0..255 train set (both ends present in
    every dim): rows 0..3 half a step off the grid, 4..7 at 300 in one dim
    (beyond the codes), 8 holds a NaN, the rest on the grid.  Returns (train,
    labels, queries, off, beyond, nan) with the index arrays of the three kinds."""
    tr, lab, te = int_sets(3000, 160, 24, seed=515)
    tr[0], tr[1] = 0.0, 255.0
    te = te.copy()
    off, beyond, nan = np.arange(0, 4), np.arange(4, 8), np.array([8])
    te[off, 3] += 0.5
    te[beyond, 5] = 300.0
    te[nan, 7] = np.nan
    return tr, lab, te, off, beyond, nan


def handover_share():
    """Queries of `handover` the pass cannot serve from its codes / all queries."""
    _, _, te, off, beyond, nan = handover()
    return (len(off) + len(beyond) + len(nan)) / te.shape[0]


def assert_neighbors_match(idx, dist, widx, wdist, flags):
    """Distances bit for bit; indices equal except inside runs of equal
    distances, and then only on queries flagged as tied (flags & 14)."""
    assert idx.shape == widx.shape
    bad = np.nonzero((dist.view(np.int64) != wdist.view(np.int64)).any(1))[0]
    assert bad.size == 0, "distance mismatch at queries %s" % bad[:10]
    k = idx.shape[1]
    for q in np.nonzero((idx != widx).any(1))[0]:
        d = dist[q]
        boundary = bool(flags[q] & 2)
        for t in np.nonzero(idx[q] != widx[q])[0]:
            run = np.nonzero(d == d[t])[0]
            at_edge = run[-1] == k - 1 and boundary
            assert len(run) > 1 or at_edge, "query %d pos %d: index differs without a tie" % (q, t)
            if not at_edge:
                assert set(idx[q][run]) == set(widx[q][run]), "query %d tie group differs" % q
        assert flags[q] & 14, "query %d differs but is not flagged as a tie" % q

"""Data sets of the wide L1-on-int8-codes tests (candidate path 7 at 256 < d <=
1024, csrc/knn_cand_sad_wide.hip, tuning key "i8l1" = 2).

Every train set here is integer-coded as tests/l1codes.py describes; the sets
put their structure where the wide kernel can go wrong: at the ends of its
256-dim stretches and 64-dim chunks, in a partial last chunk, in the pad
dims, and at the top of the accumulator's range (255 * 1024).
"""
import functools

import numpy as np

import l1codes

# case 1: one dim into the second stretch, a partial granule, pad dims, every
# count of 64-dim chunks modulo 4 and of 256-dim stretches
SHAPE_D = (257, 272, 300, 512, 784, 1000, 1024)
SHAPE_N = (31, 257, 3000)
K_EDGES = (1, 7, 30)
WIDE_MAX = 255 * 1024  # the largest sum the pass can produce


def pad_dim(d):
    """The library's pad_dim_i8l1w: 16-dim granule on (256, 1024], else -1."""
    return (d + 15) // 16 * 16 if 256 < d <= 1024 else -1


# case 2: the dims of a d = 784 row that carry information; every other dim
# is constant.  Both sides of every 256-dim boundary, the row's ends.
BOUNDARY_D = 784
BOUNDARY_DIMS = (0, 255, 256, 257, 511, 512, 767, 768, 783)
BOUNDARY_K = 5


@functools.lru_cache(maxsize=None)
def chunk_boundaries():
    """Returns (train [600, 784], labels, queries [48, 784])."""
    rng = np.random.default_rng(2784)
    n, m, d = 600, 48, BOUNDARY_D
    x = np.full((n + m, d), 9.0)
    x[:, 1::2] = 200.0  # (two constants: a mis-offset read of a constant dim shows too)
    dims = list(BOUNDARY_DIMS)
    x[:, dims] = rng.integers(0, 256, (n + m, len(dims)))
    x[0, dims], x[1, dims] = 0.0, 255.0  # the full byte in every marked dim
    lab = rng.integers(0, 4, n).astype(np.int32)
    return x[:n].copy(), lab, x[n:].copy()


@functools.lru_cache(maxsize=None)
def offset_grid(kind):
    """Case 4 at d = 300: "offset" = values 1000000 + c (s = 0), "eighths" =
    c / 8 (s = 3); c in 0..255, dim 0 constant, dim 1 and dim 299 spanning
    exactly 255 codes.  Returns (train, labels, queries, s)."""
    rng = np.random.default_rng(341 if kind == "offset" else 343)
    n, m, d = 3000, 60, 300
    c = rng.integers(0, 256, (n + m, d))
    c[:, 0] = 77
    c[0, 1], c[1, 1] = 0, 255
    c[0, 299], c[1, 299] = 0, 255
    c[:, 2] = rng.integers(100, 110, n + m)  # a narrow dim
    x = c.astype(np.float64)
    x, s = (1000000.0 + x, 0) if kind == "offset" else (x / 8.0, 3)
    lab = rng.integers(0, 4, n).astype(np.int32)
    return x[:n].copy(), lab, x[n:].copy(), s


# case 5: the 0..3 grid on six dims spread over a d = 784 row
TIE_D = 784
TIE_DIMS = (0, 255, 256, 300, 600, 783)
TIE_K = 30


@functools.lru_cache(maxsize=None)
def tie_grid():
    """Returns (train [600, 784], labels, queries [64, 784])."""
    rng = np.random.default_rng(1404)
    tr = np.full((600, TIE_D), 5.0)
    te = np.full((64, TIE_D), 5.0)
    tr[:, list(TIE_DIMS)] = rng.integers(0, 4, (600, 6))
    lab = rng.integers(0, 3, 600).astype(np.int32)
    te[:, list(TIE_DIMS)] = rng.integers(0, 4, (64, 6))
    return tr, lab, te


# case 6: the queries the pass hands over, their marks beyond dim 256
HANDOVER_OFF_DIM, HANDOVER_BEYOND_DIM, HANDOVER_NAN_DIM = 260, 290, 299


@functools.lru_cache(maxsize=None)
def handover():
    """160 queries against a 0..255 train set at d = 300: rows 0..3 half a
    step off the grid, 4..7 at 300 in one dim, 8 holds a NaN.  Returns (train,
    labels, queries, off, beyond, nan)."""
    tr, lab, te = l1codes.int_sets(3000, 160, 300, seed=1515)
    tr, te = tr.copy(), te.copy()
    tr[0], tr[1] = 0.0, 255.0
    off, beyond, nan = np.arange(0, 4), np.arange(4, 8), np.array([8])
    te[off, HANDOVER_OFF_DIM] += 0.5
    te[beyond, HANDOVER_BEYOND_DIM] = 300.0
    te[nan, HANDOVER_NAN_DIM] = np.nan
    return tr, lab, te, off, beyond, nan


def handover_share():
    _, _, te, off, beyond, nan = handover()
    return (len(off) + len(beyond) + len(nan)) / te.shape[0]


def widen(x, d, value=7.0):
    """x with constant dims appended up to d: every L1 distance unchanged."""
    return np.concatenate([x, np.full((x.shape[0], d - x.shape[1]), value)], axis=1)

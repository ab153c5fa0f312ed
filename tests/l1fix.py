"""Data sets and a numpy model of the 16-bit fixed-point L1 pass (candidate
path 8, csrc/knn_cand_fix16.hip; tuning key "u16l1").

The pass codes every value as
    code_c = clamp(rint(2^e (v_c - mu_c)), -32768, 32767) + 32768
with one power-of-two scale for all dims and the train centre as the per-dim
offset, ranks rows by the integer sum of absolute code differences (the
proxy), and certifies with the bound
    |2^-e proxy - SUM|q - x|| <= 2^-e (Dq + Dx) + f (||q - mu||_1 + max||x - mu||_1)
where D is a vector's summed coding error in code units.
`Model` restates that in numpy: the scale choice of the library (max |x - mu|
2^(e - 5) in [2^8, 2^9), so train codes stay within 32768 +- 2^14), the codes,
the proxies, Dq, Dx and E.  The CPU tests check it against the oracle's fp64
distances for every (query, row) pair of every data set below -- the bound
itself, independent of any kernel.
"""
import functools
import math

import numpy as np

import datagen
import golden_io
import neartie

BIAS = 32768
WIDTHS = (32, 64, 96, 128, 160, 192, 256)  # pad_dim_u16l1


def pad_dim(d):
    return next((p for p in WIDTHS if p >= d), -1)


def f_err(dp):
    """err_factor(8, DP): fp64 rounding of v - mu on both sides and of the
    reference's own loop, relative to ||q - mu||_1 + max||x - mu||_1."""
    return 2.0 * (dp + 4) * 2.0 ** -53


class Model:
    """The pass on (train, queries): mu, e, codes ct / cq, Dx, Dq, E, clamped."""

    def __init__(self, tr, te):
        mu0 = tr.mean(0)
        xamax = float(np.abs(tr - mu0).max())
        ex = math.frexp(xamax)[1] if xamax > 0.0 else 0  # xamax < 2^ex
        jx = min(9 - ex, 450)
        with np.errstate(over="ignore"):
            y = np.ldexp(mu0, jx + 2)  # the centre sits on the 2^-(jx + 2) grid
            self.mu = np.where(np.abs(y) < 2.0 ** 52, np.ldexp(np.rint(y), -(jx + 2)), mu0)
        self.e = jx + 5
        self.d = tr.shape[1]
        self.ct, dx, _ = self.encode(tr)
        self.cq, self.Dq, self.clamped = self.encode(te)
        self.Dx = float(dx.max())
        self.x1max = float(np.abs(tr - self.mu).sum(1).max())
        with np.errstate(invalid="ignore"):
            q1 = np.abs(te - self.mu).sum(1)
        self.round_term = f_err(pad_dim(self.d)) * (q1 + self.x1max) * (1.0 + 1e-12)
        with np.errstate(over="ignore"):
            self.E = np.ldexp((self.Dq + self.Dx) * (1.0 + 1e-12), -self.e) + self.round_term + 1e-300

    def encode(self, v):
        """codes [rows, d] (int64), summed coding error per row, clamped per row"""
        with np.errstate(over="ignore", invalid="ignore"):
            y = np.ldexp(v - self.mu, self.e)
            r0 = np.rint(y)
            r = np.clip(r0, -32768.0, 32767.0)
            err = np.abs(y - r).sum(1)
        r = np.where(np.isnan(r), 0.0, r)
        return r.astype(np.int64) + BIAS, err, (r0 != r).any(1)

    def proxies(self, q):
        """integer proxies of query q against every train row"""
        return np.abs(self.ct - self.cq[q]).sum(1)


def labels_for(n, classes, seed):
    return np.random.default_rng(seed).integers(0, classes, n).astype(np.int32)


# case 1: shape edges on continuous data
SHAPE_KINDS = ("uniform", "gauss")
SHAPE_N = (31, 257, 6000)
SHAPE_D = (1, 7, 13, 32, 100, 128, 129, 256)
K_EDGES = (1, 7, 30)


def shape_m(n, d):
    return 40 + (n * 7 + d * 3) % 160  # 40 .. 199, ragged


@functools.lru_cache(maxsize=None)
def shape_set(kind, n, d):
    """Continuous train [n, d] / queries, 4 random classes."""
    rng = np.random.default_rng(n * 131 + d * 7 + (kind == "gauss"))
    m = shape_m(n, d)
    x = rng.random((n + m, d)) if kind == "uniform" else rng.standard_normal((n + m, d))
    return _frozen(x[:n].copy(), labels_for(n, 4, n + d), x[n:].copy())


def shape_ks(n):
    return sorted(set(k for k in K_EDGES + ((n - 1,) if n == 31 else ()) if k < n))


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# case 2: both ends of the train range in every dim, and of the code range
@functools.lru_cache(maxsize=None)
def code_ends(d):
    """48 rows in [0, 1]^d: row 0 all 0, row 1 all 1 (every dim as wide as the
    widest), rows 2..5 half / alternating ends; queries 0 / 1 sit on the two
    ends, queries 2 / 3 far outside in every dim (codes 0 and 65535: the
    largest sums the accumulator sees).  Returns (train, labels, queries)."""
    rng = np.random.default_rng(800 + d)
    n = 48
    tr = rng.random((n, d))
    tr[0], tr[1] = 0.0, 1.0
    tr[2, : d // 2], tr[2, d // 2:] = 0.0, 1.0
    tr[3, : d // 2], tr[3, d // 2:] = 1.0, 0.0
    tr[4, 0::2], tr[4, 1::2] = 0.0, 1.0
    tr[5, 0::2], tr[5, 1::2] = 1.0, 0.0
    te = rng.random((40, d))
    te[0], te[1] = 0.0, 1.0
    te[2], te[3] = -100.0, 100.0
    return _frozen(tr, (np.arange(n) % 3).astype(np.int32), te)


# case 3: the reference's own configuration
def fixture_sets(name):
    """(fixture, train, labels, test, validation, validation labels), normalised
    as the reference ran it."""
    fx = golden_io.Fixture(name)
    tr, trl, te, tel, va, val_ = fx.normalized()
    return fx, tr, trl, te, va, val_


# case 4: near ties far below one code step, and exact duplicates
def near_ties():
    """neartie case E (L1, d = 40): clusters of 40 / 1500 rows at radii 2^-8 ..
    2^-24 of their distance from the train mean, uniform labels."""
    return neartie.case("E")


@functools.lru_cache(maxsize=None)
def duplicates():
    """600 rows at d = 12, rows 300.. copies of rows 0..299 under another
    label: every distance occurs twice, and at an odd k the k-th place falls
    between the two copies.  Returns (train, labels, queries)."""
    rng = np.random.default_rng(909)
    half = rng.standard_normal((300, 12))
    lab = rng.integers(0, 3, 300).astype(np.int32)
    tr = np.concatenate([half, half])
    return _frozen(tr, np.concatenate([lab, (lab + 1) % 3]).astype(np.int32),
                   rng.standard_normal((64, 12)))


DUP_K = 5

# case 5: queries the pass hands over
HANDOVER_K = 7
HANDOVER_C = 24  # max(2 W, W + 16) re-rank candidates at W = k + 1


@functools.lru_cache(maxsize=None)
def handover():
    """160 queries against 3000 uniform rows in [0, 1]^24: queries 0..3 outside
    the train hull in one dim but inside the codes' headroom (1.3), 4..7 far
    outside (100.0: clamped), 8 holds a NaN.  Returns (train, labels, queries,
    near, far, nan)."""
    rng = np.random.default_rng(515)
    tr = rng.random((3000, 24))
    te = rng.random((160, 24))
    near, far, nan = np.arange(0, 4), np.arange(4, 8), np.array([8])
    te[near, 3] = 1.3
    te[far, 5] = 100.0
    te[nan, 7] = np.nan
    return _frozen(tr, labels_for(3000, 4, 516), te) + (near, far, nan)


# case 6: unequal dims and degenerate sets
@functools.lru_cache(maxsize=None)
def odd_set(kind):
    """"unequal": dim 0 spans 1e6 beside dims spanning 1; "constant": every
    train row the same vector; "far": values 1e9 + U[0, 1]."""
    rng = np.random.default_rng({"unequal": 61, "constant": 62, "far": 63}[kind])
    if kind == "unequal":
        n, m, d = 2000, 64, 8
        x = rng.random((n + m, d))
        x[:, 0] *= 1e6
    elif kind == "constant":
        n, m, d = 300, 48, 5
        x = np.tile(np.array([3.25, -1.5, 0.0, 1024.0, 0.125]), (n + m, 1))  # (exact column means)
        x[n + 8:] += rng.standard_normal((m - 8, d))  # queries 0..7 equal the rows
    else:
        n, m, d = 2000, 64, 16
        x = 1e9 + rng.random((n + m, d))
    return _frozen(x[:n].copy(), labels_for(n, 4, n + d), x[n:].copy())


def int_sets(n, m, d, seed=None):
    """datagen "int" (byte-valued: the library's detect_i8 accepts it)."""
    seed = n * 31 + d if seed is None else seed
    tr, lab, te, _, _, _ = datagen.make_sets("int", seed, n, m, 0, d, 4)
    return tr, lab, te

"""Data sets and a numpy model of the 16-bit fixed-point L1 pass above 256
dims (candidate path 8's wide form, csrc/knn_cand_fix16_wide.hip; tuning key
"u16l1w").

Codes, scale and coding errors are those of the narrow pass (tests/l1fix.py,
Model).  What the wide form adds: the integer sum of absolute code
differences P reaches 65535 * 1024 < 2^26, exact in the kernel's uint32
accumulators but not as a float.  The kernel converts it once, round to
nearest (fl32), so |fl32(P) - P| <= r(DP) code units,
    r = 0 for DP <= 256, 1 for DP <= 512, 2 for DP <= 1024
(half an ulp of [2^24, 2^25) and of [2^25, 2^26)), and the certification bound
becomes
    E = 2^-e (Dq + Dx + r)(1 + 1e-12) + f (||q - mu||_1 + max||x - mu||_1)
with f = err_factor(8, DP).  `Model` restates that; the CPU
tests check |2^-e fl32(P) - oracle distance| <= E for every pair of every set
below.
"""
import functools

import numpy as np

import l1fix
import oracle
from l1fix import _frozen, labels_for


def pad_dim(d):
    """pad_dim_u16l1w: d rounded up to 16 in (256, 1024], else -1."""
    return (d + 15) // 16 * 16 if 256 < d <= 1024 else -1


def r_of(dp):
    """fix16_wide_round: the sums' rounding to float at most, in code units."""
    return 0 if dp <= 256 else 1 if dp <= 512 else 2


def fl32(p):
    """v_cvt_f32_u32 of integer sums (round to nearest even), as float64."""
    return np.asarray(p, np.uint32).astype(np.float32).astype(np.float64)


class Model(l1fix.Model):
    """The pass on (train, queries) at 256 < d <= 1024: l1fix.Model's mu, e,
    codes ct / cq, Dx, Dq, clamped, with the wide form's DP, r and E."""

    def __init__(self, tr, te):
        super().__init__(tr, te)
        self.dp = pad_dim(self.d)
        assert self.dp > 0
        self.r = r_of(self.dp)
        with np.errstate(invalid="ignore"):
            q1 = np.abs(te - self.mu).sum(1)
        self.round_term = l1fix.f_err(self.dp) * (q1 + self.x1max) * (1.0 + 1e-12)
        with np.errstate(over="ignore"):
            self.E = np.ldexp((self.Dq + self.Dx + self.r) * (1.0 + 1e-12), -self.e) + \
                self.round_term + 1e-300

    def proxies32(self, q):
        """what the kernel hands the lists: fl32 of the integer proxies"""
        return fl32(self.proxies(q))


# ---------------------------------------------------------------- the shapes
SHAPE_D = (257, 272, 512, 513, 784, 1024)
SHAPE_N = (70, 300, 2000)
SHAPE_M = (1, 33, 130)
K_EDGES = (1, 10, 50)
BIG_K = 300


@functools.lru_cache(maxsize=None)
def uniform_norm(n, d, m=130):
    """Uniform rows, min-max normalised as the reference's Normalize = true
    does: values in [0, 1] (queries nearly) on no binary grid.
    Returns (train, labels, queries)."""
    rng = np.random.default_rng(n * 131 + d * 7 + 5)
    x = rng.random((n + m, d))
    tr, te = x[:n].copy(), x[n:].copy()
    oracle.normalize(tr, te, None)
    return _frozen(tr, labels_for(n, 4, n + d), te)


DISPLACED_D = 1024


@functools.lru_cache(maxsize=None)
def displaced():
    """d = 1024, every query displaced outside the train hull in every dim,
    inside the codes' headroom: 9 of 10 train rows uniform in [0, 0.2], the
    rest in [0.8, 1] (mu near 0.18, max |x - mu| near 0.82: e = 14, the codes
    reach mu +- 2), queries at 2.13 +- 0.02 per dim.  A query's sums against
    the low rows exceed 2^25, against the high rows 2^24.  Returns (train,
    labels, queries)."""
    rng = np.random.default_rng(1024)
    n, m, d = 2000, 33, DISPLACED_D
    tr = rng.random((n, d)) * 0.2
    high = np.arange(n) % 10 == 3
    tr[high] += 0.8
    te = 2.13 + (rng.random((m, d)) - 0.5) * 0.04
    return _frozen(tr, labels_for(n, 4, 1025), te)


@functools.lru_cache(maxsize=None)
def odd_set(kind):
    """"unequal": dim 0 spans 1e3 beside dims spanning 1 (coarse codes: a dim
    spanning 1 takes 32 code steps, and rescans appear); "constant": every
    train row the same vector.  Returns (train, labels, queries)."""
    rng = np.random.default_rng({"unequal": 71, "constant": 72}[kind])
    if kind == "unequal":
        n, m, d = 2000, 64, 300
        x = rng.random((n + m, d))
        x[:, 0] *= 1e3
    else:
        n, m, d = 300, 48, 272
        row = np.tile(np.array([3.25, -1.5, 0.0, 1024.0, 0.125, 7.0, -0.5, 2.0]), d // 8)
        x = np.tile(row, (n + m, 1))  # (exact column means)
        x[n + 8:] += rng.standard_normal((m - 8, d))  # queries 0..7 equal the rows
    return _frozen(x[:n].copy(), labels_for(n, 4, n + d), x[n:].copy())


@functools.lru_cache(maxsize=None)
def with_nan():
    """uniform_norm(300, 513)'s sets with a NaN in query 5 (its last dim).
    Returns (train, labels, queries, nan rows)."""
    tr, lab, te = uniform_norm(300, 513)
    te = te[:40].copy()
    te[5, 512] = np.nan
    return _frozen(tr, lab, te) + (np.array([5]),)


def int_sets(n, m, d):
    return l1fix.int_sets(n, m, d)

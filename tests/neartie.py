"""Near-tie inputs for the certification bound, and a reduced-precision proxy
emulation that shows they bite.  Plain numpy, deterministic from a seed.

The candidate passes rank rows by a reduced-precision proxy of the distance
and trust the result only where the per-path error bound E (DESIGN.md §2,
"Certified candidates") separates the k-th place from every row left out.
On well-spread data the proxy order and the exact order agree, so E is never
put to the test.  The generators here build data where they disagree:

  clusters      tight clusters far from the train mean: the centred operands
                are large, the distances inside a cluster far below the
                operands' rounding, so inside a cluster the proxy order is
                noise while the exact fp64 distances stay well separated;
  grid_offgrid  integer codes with queries a hair off a grid point: the int8
                proxies tie exactly over whole shells of rows and only the
                queries' sub-grid offsets decide the exact order.

proxy_misses() emulates the proxies (fp16 or fp32 operands, fp32 arithmetic)
and counts how much of the exact top k the proxy top k lacks.  It is a
stand-in for the kernels' arithmetic, not a model of it: its only job is to
show that an input is not vacuous.
"""
import numpy as np


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _sphere(rng, rows, d):
    u = rng.standard_normal((rows, d))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def clusters(seed, d, nbulk, spec, qper, off=3.0, shift=0.0, mbulk=60, classes=5):
    """Bulk of `nbulk` standard-normal rows plus, per (size, t) of `spec`, a
    cluster of `size` train rows and `qper` queries: centre c in a random
    direction at norm off*sqrt(d), points c + u*r*(0.5 + U[0,1)) with u uniform
    on the sphere and r = ||c|| * 2^t.  `mbulk` bulk-like queries are appended
    (ragged m, benign queries among the others); the train rows are permuted
    (a cluster's rows spread over tiles, splits and lane lists); labels are
    uniform and independent of position (a wrong neighbour usually flips the
    vote); `shift` is added to every coordinate of train and queries.

    Returns (train, labels, queries, info): info[i] is query i's (size, t),
    or None for a bulk query."""
    rng = _rng(seed)
    train = [rng.standard_normal((nbulk, d))]
    queries, info = [], []
    for size, t in spec:
        c = _sphere(rng, 1, d)[0] * (off * np.sqrt(d))
        r = np.linalg.norm(c) * 2.0 ** t
        pts = c + _sphere(rng, size + qper, d) * (r * (0.5 + rng.random((size + qper, 1))))
        train.append(pts[:size])
        queries.append(pts[size:])
        info += [(size, t)] * qper
    queries.append(rng.standard_normal((mbulk, d)))
    info += [None] * mbulk
    train = np.concatenate(train)
    train = train[rng.permutation(train.shape[0])]
    labels = rng.integers(0, classes, train.shape[0]).astype(np.int32)
    train = np.ascontiguousarray(train + shift)
    queries = np.ascontiguousarray(np.concatenate(queries) + shift)
    return train, labels, queries, info


def grid_offgrid(seed, n, m, d, levels=16, eps=2.0 ** -12, classes=5):
    """Integer codes 0..levels-1 at scale 1 around per-class centres (the
    shape of SIFT-like byte data, shrunk to `levels` values so that many rows
    share a squared code distance); each query is a random train row's grid
    point plus U(-eps, eps) per coordinate.  Labels are independent of the
    centres.  Returns (train, labels, queries)."""
    rng = _rng(seed)
    centres = rng.uniform(levels / 4.0, levels - 1 - levels / 4.0, (classes, d))
    grp = rng.integers(0, classes, n)
    train = np.clip(np.rint(centres[grp] + 0.1 * levels * rng.standard_normal((n, d))),
                    0, levels - 1)
    labels = rng.integers(0, classes, n).astype(np.int32)
    src = rng.integers(0, n, m)
    queries = train[src] + rng.uniform(-eps, eps, (m, d))
    return np.ascontiguousarray(train), labels, np.ascontiguousarray(queries)


def _operands(train, queries, prec):
    """Centred operands (train column means) rounded to `prec`, as fp32; fp16
    operands are first scaled by the power of two that brings the largest
    magnitude just below 65504."""
    mu = train.mean(axis=0)
    x, q = train - mu, queries - mu
    if prec == "fp16":
        top = max(np.abs(x).max(), np.abs(q).max())
        s = 2.0 ** np.floor(np.log2(65504.0 / top))
        return (x * s).astype(np.float16).astype(np.float32), \
               (q * s).astype(np.float16).astype(np.float32)
    if prec == "fp32":
        return x.astype(np.float32), q.astype(np.float32)
    raise ValueError(prec)


def exact_topk(train, queries, k, metric):
    """Indices [m, k] of the k nearest rows in fp64 (plain differences)."""
    out = np.empty((queries.shape[0], k), np.int64)
    for i, q in enumerate(queries):
        df = train - q
        dist = (df * df).sum(axis=1) if metric == 0 else np.abs(df).sum(axis=1)
        out[i] = np.argsort(dist, kind="stable")[:k]
    return out


def proxy_topk(train, queries, k, metric, prec):
    """Indices [m, k] of the k smallest emulated proxies: L2 (metric 0)
    fl32(||x'||^2) - 2 q'.x', L1 (metric 1) an fp32 running sum of |q' - x'|,
    on operands rounded to `prec`."""
    x, q = _operands(train, queries, prec)
    out = np.empty((queries.shape[0], k), np.int64)
    if metric == 0:
        x2 = (x * x).sum(axis=1, dtype=np.float32)
        for i in range(q.shape[0]):
            v = x2 - np.float32(2.0) * (x @ q[i])
            out[i] = np.argsort(v, kind="stable")[:k]
    else:
        for i in range(q.shape[0]):
            a = np.abs(x - q[i])
            v = np.zeros(x.shape[0], np.float32)
            for c in range(a.shape[1]):
                v += a[:, c]
            out[i] = np.argsort(v, kind="stable")[:k]
    return out


def proxy_misses(train, queries, k, metric, prec, exact=None):
    """Per query: how many of the exact top k the emulated proxy top k lacks.
    `exact`: the exact top-k indices [m, k] if already known (the oracle's)."""
    if exact is None:
        exact = exact_topk(train, queries, k, metric)
    got = proxy_topk(train, queries, k, metric, prec)
    return np.array([k - np.intersect1d(e[:k], g).size for e, g in zip(exact, got)])


def shell_sizes(train, queries, kth_rows):
    """Per query: how many train rows share the rounded-code squared distance
    of the query's k-th neighbour (train row kth_rows[i])."""
    codes = np.rint(queries)
    out = np.empty(queries.shape[0], np.int64)
    for i, c in enumerate(codes):
        r = ((train - c) ** 2).sum(axis=1)
        out[i] = int((r == r[kth_rows[i]]).sum())
    return out


def shell_crossings(train, queries, topk):
    """Per query: whether the exact top k (train rows topk[i]) crosses the
    shells of the rounded codes -- some row outside it has a smaller
    rounded-code squared distance than some row inside it, so no cut of the
    int8 proxy order gives the exact top k."""
    codes = np.rint(queries)
    out = np.empty(queries.shape[0], bool)
    for i, c in enumerate(codes):
        r = ((train - c) ** 2).sum(axis=1)
        inside = r[topk[i]].max()
        r[topk[i]] = np.inf
        out[i] = r.min() < inside
    return out


# The cases of test_gpu_neartie.py (and of test_neartie_data.py, which checks
# on the CPU that each of them bites).  `seed` is chosen so that the k+1
# oracle distances of every query are pairwise distinct.
_SPEC_A = [(40, -6), (40, -10), (40, -14), (40, -20), (40, -26), (600, -10), (600, -20),
           (1500, -12), (1500, -24)]
CASES = {
    # name: metric, k, clusters() arguments
    "A": dict(metric=0, k=10, seed=1, d=64, nbulk=6000, mbulk=100, spec=_SPEC_A, qper=4),
    "B": dict(metric=0, k=50, seed=1, d=64, nbulk=6000, mbulk=100, spec=_SPEC_A, qper=4),
    "C": dict(metric=0, k=12, seed=3, d=300, nbulk=3000, mbulk=60,
              spec=[(40, -8), (40, -16), (40, -24), (1500, -12), (1500, -24)], qper=4),
    "D": dict(metric=0, k=5, seed=4, d=13, nbulk=3000, mbulk=60,
              spec=[(40, -10), (40, -20), (1500, -22)], qper=4),
    "E": dict(metric=1, k=7, seed=14, d=40, nbulk=4000, mbulk=60,
              spec=[(40, -8), (40, -16), (40, -24), (1500, -22)], qper=4),
    "F": dict(metric=0, k=10, seed=6, d=64, nbulk=6000, mbulk=100, spec=_SPEC_A, qper=4,
              shift=1000.0),
}
CLASSES = 5
GRID = dict(seed=7, n=8000, m=200, d=16, k=10)
# H: G's shape with queries up to a quarter code off the grid.  At G's 2^-12
# the offsets move a squared distance by 2 |delta . (x - q)| < 0.03 code
# units, inside the one unit the int8 bound always allows, so G passes even
# with the measured coding-error term of E scaled by 2^-12; at 2^-2 they move
# it by several units, the exact order crosses the codes' shells, and only
# that term keeps the window and the certification sound.
GRID_H = dict(seed=8, n=8000, m=200, d=16, k=10, eps=0.25)

_cache = {}


def case(name):
    """(train, labels, queries, info, k, metric) of a named case; built once
    per process and shared (callers must not modify the arrays)."""
    if name not in _cache:
        if name in ("G", "H"):
            g = dict(GRID if name == "G" else GRID_H)
            k = g.pop("k")
            tr, lab, te = grid_offgrid(classes=CLASSES, **g)
            _cache[name] = (tr, lab, te, [None] * te.shape[0], k, 0)
        else:
            c = dict(CASES[name])
            metric, k = c.pop("metric"), c.pop("k")
            tr, lab, te, info = clusters(classes=CLASSES, **c)
            _cache[name] = (tr, lab, te, info, k, metric)
        for a in _cache[name][:3]:
            a.setflags(write=False)
    return _cache[name]

"""The near-tie inputs of test_gpu_neartie.py, checked on the CPU: conditions
on the data (oracle + numpy proxy emulation), not on the kernels.

1. every query's k+1 oracle distances are pairwise distinct -- which is what
   lets the GPU test demand index-for-index equality and no tie flag;
2. for every query of a cluster with t <= -14 the emulated reduced-precision
   proxy top k (fp16 and fp32 operands) lacks at least 3 of the exact top k:
   the proxy order is wrong there, only the certification bound stands
   between the candidate pass and a wrong neighbour;
3. for the off-grid integer case, at least half the queries have >= 2 train
   rows sharing the rounded-code squared distance of their k-th neighbour.
The floors prove that a case bites; they are not tolerances on the kernels.
"""
import numpy as np
import pytest

import neartie
import oracle

MISS_FLOOR = 3


def _floor(metric, prec):
    """(largest t, fewest misses) the proxy emulation must show per query.

    L2, and L1 on fp16 operands: at least 3 misses in every cluster with
    t <= -14.  Two limits follow from the arithmetic, not from any seed:
      * a cluster of no more than k rows (case B's 40-row clusters at k = 50)
        lies wholly inside both top-k sets, whatever the proxy error, and the
        rest of the top k comes from the well-separated bulk: only clusters
        of more than k rows are held to the floor;
      * the L1 proxy on fp32 operands has no cancellation: q' - x' of two
        nearby fp32 values is exact, so its only error is the operands' own
        rounding, about sqrt(d) 2^-25 |x'| = 4e-7 at d = 40, |x'| = 3.  The
        gaps between successive neighbours of a 40-row cluster are about 1 %
        of an L1 distance of 5 ||c|| 2^t: 4e-6 at t = -16 (no miss in any of
        20 seeds), 6e-8 and less from t = -22 down.  There the emulation is
        asked for a proxy top k that differs from the exact one (>= 1 miss;
        measured 2-3), which is all this path can show; the kernels' bound
        f_err (||q'||_1 + max ||x'||_1) is about 1e-3 there, far above the
        cluster's diameter, so they must re-rank the whole cluster exactly
        or hand the query to the rescan (test_gpu_neartie.py)."""
    if metric == 1 and prec == "fp32":
        return -22, 1
    return -14, MISS_FLOOR


_ORACLE = {}


def _data(name):
    """The case and its oracle top k+1 (computed once, shared, left unchanged)."""
    tr, lab, te, info, k, metric = neartie.case(name)
    if name not in _ORACLE:
        _ORACLE[name] = oracle.knn(tr, lab, te, k, metric == 0, neartie.CLASSES, n_out=k + 1)[1:]
    return (name, tr, te, info, k, metric) + _ORACLE[name]


def test_generators_are_deterministic():
    a = neartie.clusters(5, 8, 50, [(10, -12)], 2, mbulk=3, shift=2.0)
    b = neartie.clusters(5, 8, 50, [(10, -12)], 2, mbulk=3, shift=2.0)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[0].shape == (60, 8) and a[2].shape == (5, 8)
    assert a[3] == [(10, -12)] * 2 + [None] * 3
    g, h = neartie.grid_offgrid(9, 100, 7, 4), neartie.grid_offgrid(9, 100, 7, 4)
    for x, y in zip(g, h):
        assert x.tobytes() == y.tobytes()
    assert (g[0] == np.rint(g[0])).all() and g[0].min() >= 0 and g[0].max() <= 15
    off = np.abs(g[2] - np.rint(g[2]))
    assert off.max() < 2.0 ** -12 and (off > 0).any()


def test_cluster_geometry():
    """Radius r = ||c|| 2^t around a centre at off * sqrt(d) from the origin."""
    d, t = 32, -9
    tr, _, te, info = neartie.clusters(2, d, 0, [(200, t)], 8, mbulk=0)
    pts = np.concatenate([tr, te])
    c = pts.mean(axis=0)
    assert abs(np.linalg.norm(c) / (3.0 * np.sqrt(d)) - 1.0) < 1e-3
    r = np.linalg.norm(pts - c, axis=1) / (3.0 * np.sqrt(d) * 2.0 ** t)
    assert 0.45 < r.min() and r.max() < 1.55
    assert info == [(200, t)] * 8


@pytest.mark.parametrize("case", sorted(neartie.CASES) + ["G", "H"])
def test_distances_distinct(case):
    name, tr, te, info, k, metric, widx, wdist = _data(case)
    gaps = np.diff(wdist, axis=1)
    print("case %s: smallest gap among the k+1 oracle distances %.3g (relative %.3g)"
          % (name, gaps.min(), (gaps / wdist[:, 1:]).min()))
    assert (gaps > 0).all(), "queries %s have tied oracle distances: change the seed" % (
        np.nonzero((gaps <= 0).any(axis=1))[0][:10],)


@pytest.mark.parametrize("case", sorted(neartie.CASES))
def test_proxy_order_breaks_in_tight_clusters(case):
    name, tr, te, info, k, metric, widx, wdist = _data(case)
    for prec in ("fp16", "fp32"):
        t_max, floor = _floor(metric, prec)
        tight = [i for i, c in enumerate(info) if c is not None and c[0] > k and c[1] <= t_max]
        assert tight
        mis = neartie.proxy_misses(tr, te[tight], k, metric, prec, exact=widx[tight, :k])
        per = {}
        for i, v in zip(tight, mis):
            per.setdefault(info[i], []).append(int(v))
        print("case %s %s: proxy_misses min %d over the %d queries of clusters with t <= %d; "
              "per (size, t) (min, max): %s"
              % (name, prec, mis.min(), len(tight), t_max,
                 {c: (min(v), max(v)) for c, v in sorted(per.items())}))
        assert mis.min() >= floor, (name, prec, per)


def test_offgrid_shells():
    _, tr, te, _, k, _, widx, _ = _data("G")
    sh = neartie.shell_sizes(tr, te, widx[:, k - 1])
    print("case G: %d of %d queries share their k-th neighbour's code distance with another "
          "row (median shell %d)" % ((sh >= 2).sum(), len(sh), np.median(sh)))
    assert 2 * (sh >= 2).sum() >= len(sh)


def test_offgrid_shell_crossings():
    """H (offsets up to a quarter code): for at least half the queries the
    exact top k crosses the codes' shells, which no cut of the int8 proxy
    order reproduces; at G's 2^-12 the offsets move a squared distance by
    less than 0.03 code units and no query's does."""
    _, tr, te, _, k, _, widx, _ = _data("H")
    cross = neartie.shell_crossings(tr, te, widx[:, :k])
    print("case H: the exact top %d crosses the code shells for %d of %d queries"
          % (k, cross.sum(), len(cross)))
    assert 2 * cross.sum() >= len(cross)
    _, tr, te, _, k, _, widx, _ = _data("G")
    assert not neartie.shell_crossings(tr, te, widx[:, :k]).any()

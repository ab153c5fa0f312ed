"""The inputs of test_gpu_kcap.py, checked on the CPU: conditions on the data
(oracle + numpy), not on the kernels.

1. the builders are deterministic;
2. for every continuous case the oracle's first W distances of every query
   (W the largest the GPU tests ask of the case, in each metric they use) are
   strictly increasing -- which is what lets the GPU tests demand
   index-for-index equality and no tie flag.  The grid (int8) cases are
   exempt: ties are inherent there;
3. the rescan constructions have the stated number of rows at exactly equal
   (a, c) or pairwise distinct (b) distance from the queries sitting on them,
   and their other queries are as in 2 (exact copies tie for them too, and
   only those).
"""
import numpy as np
import pytest

import kcap

# metrics the GPU tests run a continuous case in (default: L2 only)
METRICS = {"ladder48": (0, 1), "ladder300": (0, 1), "wide24": (0, 1), "part32": (0, 1),
           "sweep40": (0, 1)}
CONTINUOUS = sorted(n for n in kcap.CASES if not kcap.is_grid(n))


def test_builders_are_deterministic():
    for name in ("edge257", "gedge300"):
        a = kcap.case(name)
        kcap._data.pop(name)
        b = kcap.case(name)
        assert a[0] is not b[0]
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        kind, _, n, m, d, _ = kcap.CASES[name]
        assert a[0].shape == (n, d) and a[1].shape == (n,) and a[2].shape == (m, d)
        assert not a[0].flags.writeable
    a = kcap.rescan_case(32, "b")
    kcap._data.pop(("rescan", 32, "b"))
    b = kcap.rescan_case(32, "b")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # the int8 paths' data are codes / 256 over the whole byte range's grid
    g = kcap.case("gedge300")[0] * 256.0
    assert (g == np.rint(g)).all() and g.min() >= 0 and g.max() <= 255


def test_rerank_count():
    assert [kcap.rerank_count(W, 20000) for W in (102, 512, 513, 1001)] == [204, 1024, 1024, 1024]
    assert kcap.rerank_count(5, 20000) == 21 and kcap.rerank_count(1000, 1000) == 1000


@pytest.mark.parametrize("name", CONTINUOUS)
def test_distances_strictly_increasing(name):
    W = kcap.CASES[name][5]
    for metric in METRICS.get(name, (0,)):
        _, widx, wdist = kcap.oracle_knn(name, W - 1, metric, n_out=W)
        gaps = np.diff(wdist, axis=1)
        print("case %s metric %d: smallest gap among the first %d oracle distances %.3g"
              % (name, metric, W, gaps.min()))
        assert (gaps > 0).all(), "queries %s have tied oracle distances: change the seed" % (
            np.nonzero((gaps <= 0).any(axis=1))[0][:10],)


@pytest.mark.parametrize("d", sorted(kcap.RESCAN_SEED))
@pytest.mark.parametrize("variant", sorted(kcap.RESCAN))
def test_rescan_constructions(d, variant):
    copies, noise, ks = kcap.RESCAN[variant]
    tr, lab, te = kcap.rescan_case(d, variant)
    sit = kcap.RESCAN_SITTING
    assert (te[:sit] == tr[kcap.RESCAN_ROW]).all()
    W = max(ks) + 1
    _, widx, wdist = kcap.oracle_knn(("rescan", d, variant), W - 1, 0, n_out=max(W, copies + 2))
    # the other queries: strictly increasing as every continuous case, except
    # that exact copies (a, c) are equidistant from every query
    gaps = np.diff(wdist[sit:, :W], axis=1)
    dup = (widx == kcap.RESCAN_ROW) | ((widx >= kcap.RESCAN_AT) & (widx < kcap.RESCAN_AT + copies))
    both = dup[sit:, :W - 1] & dup[sit:, 1:W]
    assert (gaps >= 0).all() and ((gaps > 0) | both).all()
    assert noise == 0.0 or (gaps > 0).all()
    on = wdist[:sit]
    if noise:
        # row 5 itself at distance 0, then the perturbed copies, all distinct
        # and all closer than any other row
        assert (on[:, 0] == 0).all() and (np.diff(on[:, :copies + 2], axis=1) > 0).all()
        rows = np.sort(widx[:sit, :copies + 1], axis=1)
        want = np.sort(np.r_[kcap.RESCAN_ROW, np.arange(kcap.RESCAN_AT, kcap.RESCAN_AT + copies)])
        assert (rows == want).all()
        assert (on[:, copies] < 1e-6).all() and (on[:, copies + 1] > 1e-6).all()
    else:
        # exactly copies + 1 rows (the copies and row 5) at distance 0, the
        # rest strictly increasing
        assert (on[:, :copies + 1] == 0).all() and (on[:, copies + 1] > 0).all()
        assert (np.diff(on[:, copies:], axis=1) > 0).all()
    print("rescan %s d %d: %d rows at %s distance from the %d sitting queries, W up to %d"
          % (variant, d, copies + 1, "distinct" if noise else "equal", sit, W))

"""The numeric-edge inputs of test_gpu_numedge.py, checked on the CPU:
conditions on the data (oracle + numpy), not on the kernels.

1. degenerate train sets have max |x - mean| = 0 (or 36 * 2^-30) and every
   query of the identical-row sets ties over all rows;
2. each rung of the power-of-two ladder is in the regime the GPU test
   assumes: exact scalings keep every k+1 oracle distances distinct and equal
   to ldexp(unscaled, e) bit for bit; with flushed squares or denormal inputs
   every query ties; with denormal squares (e = -520) the distances stay
   distinct but are no longer the scaled bits of the unscaled ones;
3. the range cases sit on either side of 2^400;
4. anisotropic cases: the k+1 oracle distances of every query are pairwise
   distinct, the cluster queries' neighbours differ from them in the small
   dimensions only, and the emulated fp16 and fp32 proxies (neartie.py) miss
   part of the exact top k there;
5. overflowing queries: every oracle distance +inf, the others finite;
6. each grid case's fractional bits, code span and magnitude fall on the
   intended side of detect_i8's limits, recomputed in numpy from the rule in
   knn_amd.h; the edge queries sit on the codes the GPU test names;
7. the retirement batches differ from batch A in the first 400 queries only.
"""
import numpy as np
import pytest

import neartie
import numedge


def _dist(name, k, metric, n_out=None):
    return numedge.oracle_knn(name, k, metric, n_out)


def test_generators_are_deterministic():
    for name in ("deg_onedim", "aniso16", "grid_offsets", "grid_edges"):
        a = numedge.case(name)
        numedge._data.pop(name)
        b = numedge.case(name)
        for x, y in zip(a[:3], b[:3]):
            assert x.tobytes() == y.tobytes()
        assert not a[0].flags.writeable


@pytest.mark.parametrize("name", numedge.DEGENERATE)
def test_degenerate_spread(name):
    tr, lab, te = numedge.case(name)
    spread = np.abs(tr - tr.mean(axis=0)).max()
    n = tr.shape[0]
    assert len(set(lab.tolist())) > 1 or n == 1, "labels must be mixed"
    if name == "deg_onedim":
        assert (tr[:, np.arange(16) != 3] == tr[0, np.arange(16) != 3]).all()
        assert 0 < spread <= 36 * 2.0 ** -30
    else:
        assert spread == 0.0
    assert numedge.degenerate_ks(name) == ([1] if n == 1 else [1, 7, 300])
    if name == "deg_same":
        for metric in (0, 1):
            _, _, wd = _dist(name, n, metric)
            assert (wd == wd[:, :1]).all(), "identical rows: every distance of a query ties"


@pytest.mark.parametrize("e", numedge.LADDER_EXACT + numedge.LADDER_LOSSY)
def test_ladder_regime(e):
    k = numedge.LADDER_K
    _, bidx, bdist = _dist("ladder0", k, 0, k + 1)
    assert (np.diff(bdist, axis=1) > 0).all(), "the unscaled base must be free of ties"
    _, widx, wdist = _dist("ladder%d" % e, k, 0, k + 1)
    tied = (np.diff(wdist, axis=1) == 0).any(axis=1)
    print("ladder e = %d: %d of %d queries have a tie among their k+1 oracle distances; "
          "%d distinct values in all" % (e, tied.sum(), len(tied), np.unique(wdist).size))
    if e in numedge.LADDER_EXACT:
        assert not tied.any()
        np.testing.assert_array_equal(widx, bidx)
        assert (wdist.view(np.int64) == np.ldexp(bdist, e).view(np.int64)).all()
    elif e == -520:
        # squares denormal: they keep about 30 bits here, enough for distinct
        # distances, but no longer the unscaled ones' bits
        assert not tied.any()
        assert (wdist.view(np.int64) != np.ldexp(bdist, e).view(np.int64)).any()
    else:
        assert 2 * tied.sum() > len(tied), "expected most queries to tie"


def test_ladder_inputs():
    tr = numedge.case("ladder0")[0]
    tiny = np.finfo(np.float64).tiny
    assert np.abs(numedge.case("ladder-1060")[0]).max() < tiny        # inputs denormal
    lo = numedge.case("ladder-600")[0]
    assert np.abs(lo).max() > tiny and (lo * lo == 0).all()           # squares flush to 0
    mid = numedge.case("ladder-520")[0]
    assert 0 < (mid * mid).max() < tiny                               # squares denormal
    for e in numedge.LADDER_EXACT:
        x = numedge.case("ladder%d" % e)[0]
        assert (np.ldexp(x, -e) == tr).all() and np.isfinite(x * x * 24).all()
        nz = x[x != 0]
        assert (nz * nz).min() * 2.0 ** -60 > tiny


def test_range_sides():
    for name, above in (("range_below", False), ("range_above", True)):
        tr = numedge.case(name)[0]
        a = np.abs(tr - tr.mean(axis=0)).max()
        r = a / 2.0 ** numedge.RANGE_LIMIT
        assert (1 < r < 1 + 2.0 ** -19) if above else (1 - 2.0 ** -19 < r < 1)
        assert np.isfinite(tr).all()
    _, _, wd = _dist("range_below", 7, 0)
    assert np.isfinite(wd).all()


@pytest.mark.parametrize("name", sorted(numedge.ANISO))
def test_aniso(name, metric=0):
    tr, lab, te, info = numedge.case(name)
    d = tr.shape[1]
    k = numedge.ANISO_K
    sc = numedge.aniso_scales(d)
    assert sc.max() == 1.0 and sc.min() <= 2.0 ** -40
    small = sc <= 2.0 ** -numedge.ANISO_SMALL
    assert small.any() and not small.all()
    # below fp16's denormal floor 2^-24 after the 2^9 operand scale
    assert sc[small].max() * 2.0 ** 9 < 2.0 ** -24
    _, widx, wdist = _dist(name, k, metric, k + 1)
    gaps = np.diff(wdist, axis=1)
    assert (gaps > 0).all(), "tied oracle distances at queries %s" % (
        np.nonzero((gaps <= 0).any(axis=1))[0][:10],)
    cl = [i for i, s in enumerate(info) if s]
    assert len(cl) == 8 and sorted(set(info)) == [0, 40, 600]
    for i in cl:   # the k+1 neighbours: identical in the large dimensions
        assert (tr[widx[i]][:, ~small] == te[i, ~small]).all()
    for prec in ("fp16", "fp32"):
        mis = neartie.proxy_misses(tr, te[cl], k, metric, prec, exact=widx[cl, :k])
        print("%s metric %d %s: proxy misses per cluster query %s" % (name, metric, prec, mis))
        assert (mis > 0).all(), (name, prec, mis)


@pytest.mark.parametrize("metric", [0, 1])
def test_overflow_distances(metric):
    name = "overflow_l2" if metric == 0 else "overflow_l1"
    tr, lab, te = numedge.case(name)
    assert np.isfinite(te).all()
    bad = list(numedge.OVERFLOW_Q[metric])
    ok = np.setdiff1d(np.arange(te.shape[0]), bad)
    for k in (7, 1200):
        _, widx, wdist = _dist(name, k, metric)
        assert np.isposinf(wdist[bad]).all() and np.isfinite(wdist[ok]).all()
        assert (widx >= 0).all() and (widx < tr.shape[0]).all()


@pytest.mark.parametrize("name", sorted(numedge.GRID_CASES))
def test_grid_rule(name):
    tr, lab, te = numedge.case(name)
    ok, s, span, top = numedge.grid_rule(tr)
    print("%s: d %d, s %d, largest span %g, largest |code| %g -> %s"
          % (name, tr.shape[1], s, span, top, "accept" if ok else "refuse"))
    assert ok == numedge.GRID_CASES[name]
    assert tr.shape == (numedge.GRID_N, tr.shape[1]) and te.shape[0] == numedge.GRID_M
    want = {"grid_span255": (8, 255), "grid_span256": (8, 256), "grid_half254": (1, 254),
            "grid_half257": (1, 257), "grid_frac30": (30, 255), "grid_frac31": (31, 510),
            "grid_offsets": (0, 255), "grid_big": (0, 255), "grid_d257": (8, 255)}
    if name in want:
        assert (s, span) == want[name]
    if name == "grid_offsets":
        off = tr.min(axis=0)
        assert (off > 0).any() and (off < 0).any() and 2.0 ** 49 <= top < 2.0 ** 50
    if name == "grid_big":
        assert top >= 2.0 ** 50
        assert (np.abs(tr[:, np.arange(48) != 7]).max() < 2.0 ** 50)
    if name.startswith("grid_const"):
        spans = np.ptp(tr, axis=0)
        assert tr.shape[1] == 1 or (spans == 0).sum() >= tr.shape[1] // 3
        assert (spans > 0).any()
    if name == "grid_d257":
        assert numedge.grid_rule(tr[:, :256])[0], "only the width refuses this set"


def test_grid_edge_queries():
    tr, lab, te = numedge.case("grid_edges")
    assert numedge.grid_rule(tr)[:2] == (True, 8)
    codes0 = np.ldexp(tr[:, 0], 8)
    assert codes0.min() == 0 and codes0.max() == 255
    centre = np.floor((codes0.min() + codes0.max() + 1) / 2)   # detect_i8's centre
    assert centre == 128
    q0 = np.ldexp(te[:, 0], 8) - centre
    B = numedge.EDGE_BLOCK
    for b, code in enumerate(numedge.EDGE_CODES):
        assert (q0[b * B:(b + 1) * B] == code).all()
    lo, hi = numedge.EDGE_OFFGRID
    off = q0[lo:hi] - np.rint(q0[lo:hi])
    assert (off == 2.0 ** -23).all()                           # 2^-31 in value units
    rest = q0[hi:]
    assert len(rest) >= 60 and (rest == np.rint(rest)).all()
    assert (rest >= -128).all() and (rest <= 127).all()
    # every other dimension of every query is an on-grid code in range
    c = np.ldexp(te[:, 1:], 8)
    assert (c == np.rint(c)).all() and c.min() >= 0 and c.max() <= 200


def test_offset40():
    tr, lab, te = numedge.case("offset40")
    mu = np.abs(tr.mean(axis=0))
    assert (mu >= 2.0 ** 40).all() and (mu < 2.0 ** 41 + 1).all()
    assert (tr.mean(axis=0) > 0).any() and (tr.mean(axis=0) < 0).any()
    assert np.abs(tr - tr.mean(axis=0)).max() < 1.0
    assert not numedge.grid_rule(tr)[0], "continuous data: not an int8 grid"


def test_auto_batches():
    for base, ongrid in (("auto_grid", True), ("auto_cont", False)):
        tr, lab, a = numedge.case(base)
        _, _, b = numedge.case(base + "_b")
        nbad = numedge.AUTO_BAD
        assert a.shape == (4096, numedge.AUTO_D) and tr.shape[0] == numedge.AUTO_N
        assert (a[nbad:] == b[nbad:]).all() and (a[:nbad] != b[:nbad]).any(axis=1).all()
        assert nbad * 16 > a.shape[0]
        assert numedge.grid_rule(tr)[0] == ongrid
        if ongrid:
            assert numedge.grid_rule(np.concatenate([tr, a]))[0], "batch A is on the grid"
            assert (np.ldexp(b[:nbad, 0], 8) == 255 + 1000).all()
        else:
            # beyond the fp16 operand range: 2^jx |q - mu| with 2^jx max|x - mu| in [2^8, 2^9)
            mu = tr.mean(axis=0)
            top = np.abs(tr - mu).max()
            assert (np.abs(b[:nbad] - mu).max(axis=1) / top * 2.0 ** 8 > 65504).all()

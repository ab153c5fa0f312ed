"""The inputs of test_gpu_l1kcap.py, checked on the CPU: conditions on the data
(oracle + numpy models of the passes), not on the kernels.

1. the builders are deterministic;
2. every continuous case has strictly increasing L1 oracle distances over its
   first W entries (W the largest asked of it) -- the licence for comparing
   every index and allowing no tie flag;
3. every grid case is integer-coded as detect_i8 requires (l1codes' model: one
   power-of-two scale, codes within a byte) and its integer proxies times 2^-s
   are the oracle's L1 distances bit for bit;
4. every path 8 case keeps the certification bound |2^-e P - dist| <= E of
   l1fix.Model for every (query, row) pair, all proxies below 2^24 and no
   query clamped;
5. the window condition, the premise of the GPU tests' rescan cap: on the
   ladder cases, at every ladder k with W <= 512, at least 3/4 of the queries
   have no more rows inside the selection window (proxy <= P_(W) + 2 E 2^e,
   E = 0 on the grid: the rows tied with the W-th) than the merge re-ranks;
6. the rescan constructions hold what their names say under L1.
"""
import numpy as np
import pytest

import kcap
import l1codes
import l1kcap
import oracle

ALL = sorted(l1kcap.CASES) + sorted(l1kcap.KCAP_CASES)
CONTINUOUS = [n for n in ALL if not l1kcap.is_grid(n)]
GRID = [n for n in ALL if l1kcap.is_grid(n)]
GRID_RESCANS = [("grescan", d, v) for d in sorted(l1kcap.GRID_RESCAN_SEED)
                for v in sorted(l1kcap.GRID_RESCAN)]
FIX16_RESCANS = [("rescan", 32, v) for v in sorted(kcap.RESCAN)]


def _id(name):
    return "-".join(str(x) for x in name) if isinstance(name, tuple) else name


def test_case_tables():
    assert not set(l1kcap.CASES) & set(kcap.CASES)
    assert set(l1kcap.KCAP_CASES) <= set(kcap.CASES)
    for tag, name in l1kcap.LADDER + l1kcap.FORMS + l1kcap.SMALL + l1kcap.SWEEP + l1kcap.LOO:
        kind, _, n, m, d, W = l1kcap.spec(name)
        assert (kind == "mix") == (tag == "fix16")
        assert (d > 256) == (tag == "wide")
    # one ladder width on each side of every kernel's tile-row switch
    rows = sorted((tag, l1kcap.tile_rows(tag, l1kcap.spec(name)[4])) for tag, name in l1kcap.LADDER)
    assert rows == [("fix16", 64), ("fix16", 128), ("sad", 64), ("sad", 128), ("wide", 64)]
    # section 3: fewer than 32 tiles of the kernel that runs, so 2 S 16 < 1001
    for tag, name in l1kcap.SMALL:
        n, d = l1kcap.spec(name)[2], l1kcap.spec(name)[4]
        tiles = (n + 255) // 256 * 256 // l1kcap.tile_rows(tag, d)
        assert tiles < 32 and 32 * tiles < 1001
    # fix16's last width with an 8-wave form, and the first without
    assert l1kcap.pad_dim("fix16", 128) == 128 and l1kcap.pad_dim("fix16", 130) == 160
    assert l1kcap.kernel_name("wide", 300, 16, 8) == "cand_sad_wide_kernel<16,8>"
    assert l1kcap.kernel_name("sad", 200, 8, 4) == "cand_sad_kernel<256,8,4>"


def test_builders_are_deterministic():
    for name in ("wedge257", "small130"):
        a = l1kcap.case(name)
        l1kcap._data.pop(name)
        b = l1kcap.case(name)
        assert a[0] is not b[0]
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        kind, _, n, m, d, _ = l1kcap.CASES[name]
        assert a[0].shape == (n, d) and a[1].shape == (n,) and a[2].shape == (m, d)
        assert not a[0].flags.writeable
    a = l1kcap.grid_rescan_case(32, "c")
    l1kcap._data.pop(("grescan", 32, "c"))
    b = l1kcap.grid_rescan_case(32, "c")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # a kcap name is kcap's own case: the same arrays, the same oracle cache
    assert l1kcap.case("grid48")[0] is kcap.case("grid48")[0]
    assert l1kcap.oracle_knn("edge257", 256)[2] is kcap.oracle_knn("edge257", 256, 1)[2]


@pytest.mark.parametrize("name", CONTINUOUS)
def test_distances_strictly_increasing(name):
    W = l1kcap.spec(name)[5]
    _, widx, wdist = l1kcap.oracle_knn(name, W - 1, n_out=W)
    gaps = np.diff(wdist, axis=1)
    print("case %s: smallest gap among the first %d L1 oracle distances %.3g"
          % (name, W, gaps.min()))
    assert (gaps > 0).all(), "queries %s have tied oracle distances: change the seed" % (
        np.nonzero((gaps <= 0).any(axis=1))[0][:10],)


def _check_grid(tr, te, s):
    """Integer-coded, and proxy 2^-s == the oracle's distance for every pair;
    the compact model agrees with l1codes.proxy_model."""
    ut, uq = l1kcap.grid_codes(tr, te, s)
    m = te.shape[0]
    for q in sorted({0, m // 2, m - 1}):
        want = l1codes.proxy_model(tr, te[q:q + 1], s)[0]
        assert (l1kcap.grid_proxies(ut, uq, q) == want).all()
    top = 0
    for q in range(m):
        prox = l1kcap.grid_proxies(ut, uq, q)
        top = max(top, int(prox.max()))
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        got = np.ldexp(prox.astype(np.float64), -s)
        assert (got.view(np.int64) == ref.view(np.int64)).all(), "query %d" % q
    assert top <= 255 * tr.shape[1] and top < 1 << 24


@pytest.mark.parametrize("name", GRID + GRID_RESCANS + ["ties"], ids=_id)
def test_grid_cases_are_integer_coded(name):
    tr, lab, te = l1kcap.arrays(name)
    _check_grid(tr, te, 0 if name == "ties" else l1kcap.GRID_S)


def _check_fix16(name):
    """The bound for every pair; returns the model."""
    tr, lab, te = l1kcap.arrays(name)
    m = l1kcap.fix16_model(name)
    top = 0
    for q in range(te.shape[0]):
        prox = m.proxies(q)
        top = max(top, int(prox.max()))
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        err = np.abs(np.ldexp(prox.astype(np.float64), -m.e) - ref)
        assert (err <= m.E[q]).all(), "query %d: error %g beyond E %g" % (q, err.max(), m.E[q])
    assert top < 1 << 24 and int(np.float32(top)) == top
    assert not m.clamped.any(), "queries %s are clamped" % np.nonzero(m.clamped)[0][:10]
    # (E is no slack bound: at most d code steps and the reference-rounding term)
    assert (m.E <= np.ldexp(m.d * (1.0 + 2.0 ** -20), -m.e) + m.round_term).all()
    return m


@pytest.mark.parametrize("name", CONTINUOUS + FIX16_RESCANS, ids=_id)
def test_fix16_bound_holds_for_every_pair(name):
    _check_fix16(name)


def test_fix16_codes_integer_data_exactly():
    """Section 7 runs path 8 on the integer tie data: every value sits on the
    code grid, so tied rows have equal proxies and no coding error."""
    tr, lab, te = l1kcap.tie_order_sets()
    m = _check_fix16("ties")
    assert m.Dx == 0.0 and (m.Dq == 0.0).all() and m.e >= 0
    for q in range(0, te.shape[0], 17):
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        assert (m.proxies(q) == np.ldexp(ref, m.e)).all()
    # full of ties: most queries tie inside their top 150
    want, widx, wdist = l1kcap.oracle_knn("ties", 150)
    assert ((np.diff(wdist, axis=1) == 0).any(1)).sum() > 50


@pytest.mark.parametrize("tag,name", [c for c in l1kcap.LADDER if c[0] == "fix16"])
def test_window_condition_fix16(tag, name):
    """The selection window vw + 2 E cannot overflow C by the model's numbers."""
    tr, lab, te = l1kcap.case(name)
    n, mq = tr.shape[0], te.shape[0]
    m = l1kcap.fix16_model(name)
    ks = [k for k in l1kcap.LADDER_KS if k + 1 <= 512]
    over = {k: 0 for k in ks}
    for q in range(mq):
        prox = np.sort(m.proxies(q))
        slack = int(np.ceil(np.ldexp(2.0 * m.E[q], m.e)))
        for k in ks:
            W = k + 1
            over[k] += l1kcap.window_counts(prox, W, slack) > kcap.rerank_count(W, n)
    print("case %s: 2 E = %d code steps at most; queries whose window exceeds C, per k: %s"
          % (name, int(np.ceil(np.ldexp(2.0 * m.E.max(), m.e))), over))
    for k in ks:
        assert over[k] * 4 <= mq, "k = %d: %d of %d windows overflow C" % (k, over[k], mq)


@pytest.mark.parametrize("tag,name", [c for c in l1kcap.LADDER if c[0] != "fix16"])
def test_window_condition_grid(tag, name):
    """E = 0: the window holds the rows tied with the W-th proxy."""
    tr, lab, te = l1kcap.case(name)
    n, mq = tr.shape[0], te.shape[0]
    ut, uq = l1kcap.grid_codes(tr, te)
    ks = [k for k in (l1kcap.WIDE_LADDER_KS if tag == "wide" else l1kcap.LADDER_KS) if k + 1 <= 512]
    over = {k: 0 for k in ks}
    tied = 0
    for q in range(mq):
        prox = np.sort(l1kcap.grid_proxies(ut, uq, q))
        for k in ks:
            W = k + 1
            cnt = l1kcap.window_counts(prox, W, 0)
            tied = max(tied, cnt - W)
            over[k] += cnt > kcap.rerank_count(W, n)
    print("case %s: up to %d rows tied beyond the W-th; windows exceeding C, per k: %s"
          % (name, tied, over))
    for k in ks:
        assert over[k] * 4 <= mq, "k = %d: %d of %d windows overflow C" % (k, over[k], mq)


@pytest.mark.parametrize("variant", sorted(kcap.RESCAN))
def test_fix16_rescan_constructions_under_l1(variant):
    """kcap.rescan_case(32, v) in the L1 metric: the stated number of rows at
    equal (a, c) or pairwise distinct (b) distance from the sitting queries;
    in (b) the copies are far below one code step apart (equal proxies)."""
    copies, noise, ks = kcap.RESCAN[variant]
    name = ("rescan", 32, variant)
    tr, lab, te = kcap.rescan_case(32, variant)
    sit = kcap.RESCAN_SITTING
    W = max(ks) + 1
    _, widx, wdist = l1kcap.oracle_knn(name, W - 1, n_out=max(W, copies + 2))
    gaps = np.diff(wdist[sit:, :W], axis=1)
    dup = (widx == kcap.RESCAN_ROW) | ((widx >= kcap.RESCAN_AT) & (widx < kcap.RESCAN_AT + copies))
    both = dup[sit:, :W - 1] & dup[sit:, 1:W]
    assert (gaps >= 0).all() and ((gaps > 0) | both).all()
    assert noise == 0.0 or (gaps > 0).all()
    on = wdist[:sit]
    m = l1kcap.fix16_model(name)
    rows = np.r_[kcap.RESCAN_ROW, np.arange(kcap.RESCAN_AT, kcap.RESCAN_AT + copies)]
    if noise:
        assert (on[:, 0] == 0).all() and (np.diff(on[:, :copies + 2], axis=1) > 0).all()
        assert (np.sort(widx[:sit, :copies + 1], axis=1) == np.sort(rows)).all()
        assert on[:, copies].max() < np.ldexp(1.0, -m.e) / 64 < on[:, copies + 1].min()
    else:
        assert (on[:, :copies + 1] == 0).all() and (on[:, copies + 1] > 0).all()
        assert (np.diff(on[:, copies:], axis=1) > 0).all()
    # equal integer proxies for the sitting queries on all the copies; with
    # noise a coordinate next to a rounding boundary may take the next code
    # (at most one step per dim), which leaves nearly all proxies at 0
    prox = m.proxies(0)
    if noise:
        assert prox[rows].max() <= tr.shape[1] and (prox[rows] == 0).mean() > 0.99
        assert np.sort(prox)[copies + 1] > 64
    else:
        assert (m.ct[rows] == m.ct[kcap.RESCAN_ROW]).all()
        assert (prox[rows] == 0).all() and (prox == 0).sum() == copies + 1


@pytest.mark.parametrize("name", GRID_RESCANS, ids=_id)
def test_grid_rescan_constructions(name):
    """copies + 1 rows (the copies and row 5) at distance 0 from the 16 sitting
    queries, every other row farther."""
    _, d, variant = name
    copies, ks = l1kcap.GRID_RESCAN[variant]
    tr, lab, te = l1kcap.grid_rescan_case(d, variant)
    sit = kcap.RESCAN_SITTING
    assert (te[:sit] == tr[kcap.RESCAN_ROW]).all()
    assert (tr[kcap.RESCAN_AT:kcap.RESCAN_AT + copies] == tr[kcap.RESCAN_ROW]).all()
    _, widx, wdist = l1kcap.oracle_knn(name, max(ks), n_out=copies + 2)
    on = wdist[:sit]
    assert (on[:, :copies + 1] == 0).all() and (on[:, copies + 1] > 0).all()
    assert len(set(lab[kcap.RESCAN_AT:kcap.RESCAN_AT + copies].tolist())) == l1kcap.CLASSES
    print("grid rescan %s d %d: %d rows at distance 0 from the %d sitting queries, k %s"
          % (variant, d, copies + 1, sit, ks))

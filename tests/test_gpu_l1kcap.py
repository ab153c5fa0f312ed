"""GPU parity at k = 101 .. 1000 on the three L1 code passes.

test_gpu_kcap.py pushes the candidate pipeline to its capacity limits on the
paths that existed when it was written; this file does the same for candidate
path 7 on byte codes (cand_sad_kernel, "i8l1" = 1), its wide form at 256 < d
<= 1024 (cand_sad_wide_kernel, "i8l1" = 2) and path 8 on 16-bit fixed-point
codes (cand_fix16_kernel, "u16l1" = 1): R = 16 lists (W >= 103) with 4 and 8
waves, the merge's 512- and 1024-entry forms and its window-overflow branch
(path 8's window is vw + 2 E with the measured coding error in E; path 7's E
is 0 and grid data tie at the cut), lists that cannot hold W, the fast and
the full rescan on a thousand equal proxies, partial lists and the sharded
merge at w = 1001, the reference tie order over hundreds of entries, the
sweeps at kmax = 1000 and non-finite queries at k = 1000.

Every comparison is against the CPU oracle (fp64): labels equal, distance bit
patterns identical; on continuous data (path 8) every index identical and no
tie flag, on grid data (path 7) the parity suite's tie rules.  Path, kernel
name and geometry are asserted from last_candidate_path / last_kernel_name /
last_geometry after every call.  Rescan shares are printed; they are asserted
where the construction derives them, and capped at 1/4 of the queries in
sections 1 and 2 at W <= 512 so that no ladder passes on the rescan alone
(test_l1kcap_data.py shows that the data do not force more).
"""
import numpy as np
import pytest

import kcap
import l1kcap
import loo
from test_gpu_kcap import TIE_BITS, _all_rescanned_if_short, _compare, _report
from test_gpu_parity import assert_neighbors_match

pytestmark = pytest.mark.gpu

CLASSES = l1kcap.CLASSES
L1 = 1


@pytest.fixture(scope="module")
def knn():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(root, "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.lib().knn_device_count() < 1:
        pytest.fail("no HIP device visible: the KNN path has no CPU fallback")
    return mod


def _clf(knn, tag, **tuning):
    c = knn.Classifier(0)
    for key, value in dict(l1kcap.PASSES[tag][0], **tuning).items():
        c.set_tuning(key, value)
    return c


def _served(c, tag, d, nw, R=None):
    """The last call ran the pass's kernel, in the form named; returns the
    geometry."""
    g = c.last_geometry()
    assert c.last_candidate_path() == l1kcap.PASSES[tag][1]
    assert R is None or g["lists"] == R
    assert c.last_kernel_name() == l1kcap.kernel_name(tag, d, g["lists"], nw), c.last_kernel_name()
    return g


def _check(c, knn, name, k, te=None):
    """One classify call on a trained context against the cached oracle;
    returns the flags.  Rescan flags and count must agree."""
    te = l1kcap.arrays(name)[2] if te is None else te
    out = c.classify(te, k, L1, return_neighbors=True)
    _compare(knn, out, l1kcap.oracle_knn(name, k), not l1kcap.is_grid(name))
    flags = out[3]
    assert int(((flags & knn.FLAG_EXACT_RESCAN) != 0).sum()) == c.last_rescan_count()
    return flags


def _capped(c, W, m):
    """Sections 1 and 2: at W <= 512 at most 1/4 of the queries may be finished
    by the rescan.  Returns the violation, to be asserted once the test's
    other calls have been compared too."""
    if W <= 512 and 4 * c.last_rescan_count() > m:
        return ["%d of %d queries rescanned at W = %d" % (c.last_rescan_count(), m, W)]
    return []


# ---------------------------------------------------------------- 1. k ladder
@pytest.mark.parametrize("tag,name", l1kcap.LADDER)
def test_k_ladder(knn, tag, name):
    """W = k + 1 on both sides of the R = 8 -> 16 switch, of the merge's 256 ->
    512 -> 1024 forms, of 2W reaching the 1024 cap, and the last k of the
    candidate path; one width on each side of every kernel's tile-row switch.

    The rescan cap found a plan fault at [sad-grid48], k = 511: the int8 image
    is in norm blocks at n > 16384, whose spread puts a band of near-norm rows
    on tiles of one parity, so an even split count sent a query's top W to
    half of the lists and 63 of 96 queries were rescanned (S = 44; 5 in train
    order).  choose_geometry now takes the largest odd S for R = 16 on such
    an image: 7 of 96 (profiles/ab_log.md, "l1kcap")."""
    tr, lab, te = l1kcap.case(name)
    (n, d), m = tr.shape, te.shape[0]
    c = _clf(knn, tag)
    c.set_train(tr, lab, CLASSES)
    over = []
    for k in (l1kcap.WIDE_LADDER_KS if tag == "wide" else l1kcap.LADDER_KS):
        W = k + 1
        _check(c, knn, name, k)
        _report("ladder", "%s d=%d" % (tag, d), k, c, m)
        # two lists per split: R = 8 while a share of 0.8 per list fits 64
        # splits ((5W + 7) / 8 <= 64, W <= 102), then R = 16
        g = _served(c, tag, d, 4, R=16 if W >= 103 else 8)
        assert g["rerank"] == kcap.rerank_count(W, n)
        assert 2 * g["splits"] * g["lists"] >= g["rerank"]
        over += _capped(c, W, m)
    c.close()
    assert not over, over


# --------------------------------------------------- 2. every (R, NW) form
@pytest.mark.parametrize("tag,name", l1kcap.FORMS)
def test_every_list_and_wave_form(knn, tag, name):
    """m = 300 (a 256-query tile and a padded one at 8 waves, three tiles at
    4), "nw" = 4 and 8, k = 30 (R = 8) and 150 (R = 16); then the plan's own
    choice for a batch of 4096 queries -- 64 queries tiled 64 times -- which
    must be <..., 16, 8> and give every copy of a query the same row."""
    tr, lab, te = l1kcap.case(name)
    (n, d), m = tr.shape, te.shape[0]
    over = []
    for nw in (4, 8):
        c = _clf(knn, tag, nw=nw)
        c.set_train(tr, lab, CLASSES)
        for k in l1kcap.FORMS_KS:
            W = k + 1
            _check(c, knn, name, k)
            _report("forms", "%s d=%d" % (tag, d), k, c, m)
            g = _served(c, tag, d, nw, R=8 if k == 30 else 16)
            assert g["rerank"] == kcap.rerank_count(W, n)
            assert g["workgroups"] == g["splits"] * ((m + 32 * nw - 1) // (32 * nw))
            over += _capped(c, W, m)
        c.close()
    k, blk, reps = 150, l1kcap.FORMS_BLOCK, l1kcap.FORMS_TILES
    big = np.tile(te[:blk], (reps, 1))
    want, widx, wdist = l1kcap.oracle_knn(name, k)
    ref = (np.tile(want[:blk], reps), np.tile(widx[:blk], (reps, 1)), np.tile(wdist[:blk], (reps, 1)))
    c = _clf(knn, tag)
    c.set_train(tr, lab, CLASSES)
    got, idx, dist, flags = c.classify(big, k, L1, return_neighbors=True)
    _report("forms m=4096", "%s d=%d" % (tag, d), k, c, big.shape[0])
    g = _served(c, tag, d, 8, R=16)
    assert g["rerank"] == kcap.rerank_count(k + 1, n)
    assert g["workgroups"] == g["splits"] * (big.shape[0] // 256)
    _compare(knn, (got, idx, dist, flags), ref, not l1kcap.is_grid(name))
    assert int(((flags & knn.FLAG_EXACT_RESCAN) != 0).sum()) == c.last_rescan_count()
    over += _capped(c, k + 1, big.shape[0])
    # the same results row for row (only the rescan flag may differ)
    keep = ~np.int32(knn.FLAG_EXACT_RESCAN)
    for r in range(1, reps):
        rows = slice(r * blk, (r + 1) * blk)
        np.testing.assert_array_equal(got[rows], got[:blk])
        np.testing.assert_array_equal(idx[rows], idx[:blk])
        np.testing.assert_array_equal(dist[rows].view(np.int64), dist[:blk].view(np.int64))
        np.testing.assert_array_equal(flags[rows] & keep, flags[:blk] & keep)
    c.close()
    assert not over, over


# ------------------------------------------------ 3. lists that cannot hold W
@pytest.mark.parametrize("tag,name", l1kcap.SMALL)
def test_lists_smaller_than_W(knn, tag, name):
    """Fewer than 32 tiles of the kernel that runs: two lists of R = 16 per
    split hold 32 * tiles < 1001 entries, no query can be certified at k =
    1000 and every one must be finished by the rescan, exactly.  At k = 400
    the lists hold W."""
    tr, lab, te = l1kcap.case(name)
    (n, d), m = tr.shape, te.shape[0]
    tiles = (n + 255) // 256 * 256 // l1kcap.tile_rows(tag, d)  # (rows are padded to 256)
    assert tiles < 32
    c = _clf(knn, tag)
    c.set_train(tr, lab, CLASSES)
    for k in (1000, 400):
        W = k + 1
        flags = _check(c, knn, name, k)
        _report("small_n", "%s d=%d" % (tag, d), k, c, m)
        g = _served(c, tag, d, 4, R=16)
        if k == 1000:
            assert g["splits"] == tiles
            assert g["rerank"] == 32 * tiles < W
            assert c.last_rescan_count() == m
            assert ((flags & knn.FLAG_EXACT_RESCAN) != 0).all()
        else:
            assert g["rerank"] >= W
    c.close()


# ---------------------------------------------------------- 4. small-n edges
@pytest.mark.parametrize("tag", sorted(l1kcap.PASSES))
@pytest.mark.parametrize("n,k", kcap.EDGES)
def test_small_n_edges(knn, n, k, tag):
    """W = n, k = n and train sets of one row more or less than the 1024-entry
    union, the 1000-row k cap and a 256-row boundary (d = 16; wide: 272)."""
    name = l1kcap.edge_case(tag, n)
    tr, lab, te = l1kcap.case(name)
    d, m = tr.shape[1], te.shape[0]
    assert tr.shape[0] == n
    c = _clf(knn, tag)
    c.set_train(tr, lab, CLASSES)
    flags = _check(c, knn, name, k)
    _report("edge n=%d" % n, "%s d=%d" % (tag, d), k, c, m)
    _served(c, tag, d, 4)
    _all_rescanned_if_short(c, knn, flags, min(k + 1, n), m)
    c.close()


# ------------------------------------------------------ 5. rescan at large W
def _rescan_variant(c, knn, tag, name, d, variant, k):
    tr, lab, te = l1kcap.arrays(name)
    sit = kcap.RESCAN_SITTING
    c.set_train(tr, lab, CLASSES)
    c.rescan_totals(reset=True)
    out = c.classify(te, k, L1, return_neighbors=True)
    failed, full = c.rescan_totals()
    _report("rescan %s d=%d full=%d" % (variant, d, full), tag, k, c, te.shape[0])
    _served(c, tag, d, 4)
    # (exact copies tie for every query: the tie rules, whatever the data)
    _compare(knn, out, l1kcap.oracle_knn(name, k), False)
    flags = out[3]
    assert failed == c.last_rescan_count()
    assert int(((flags & knn.FLAG_EXACT_RESCAN) != 0).sum()) == failed
    if variant == "a":
        assert full >= sit
        assert ((flags[:sit] & knn.FLAG_EXACT_RESCAN) != 0).all()
    return out


def test_rescan_large_w_fix16(knn):
    """(a) 1500 exact copies of one row under 16 queries at k = 600: 1501 equal
    proxies, more than the fast rescan keeps, so the full scan keeps the top
    601 by (dist, idx); (b) the copies 1e-9 apart, far below one code step:
    (nearly all) equal proxies over distinct distances, k = 600 and 1000, no
    tie flag and every index the oracle's; (c) 700 copies at k = 1000, which
    the fast path can finish."""
    c = _clf(knn, "fix16")
    for variant in sorted(kcap.RESCAN):
        name = ("rescan", 32, variant)
        for k in kcap.RESCAN[variant][2]:
            got, idx, dist, flags = _rescan_variant(c, knn, "fix16", name, 32, variant, k)
            if variant == "b":
                assert not (flags & TIE_BITS).any()
                np.testing.assert_array_equal(idx, l1kcap.oracle_knn(name, k)[1])
    c.close()


@pytest.mark.parametrize("tag,d", [("sad", 32), ("wide", 300)])
def test_rescan_large_w_grid(knn, tag, d):
    """The grid analogues of (a) and (c): the copied rows are exact copies of
    a grid row and the queries sit on it, 1501 / 701 integer proxies of 0.  A
    variant (b) cannot exist on a grid: the smallest move of a row is one
    whole code, which the proxies resolve exactly."""
    c = _clf(knn, tag)
    for variant in sorted(l1kcap.GRID_RESCAN):
        for k in l1kcap.GRID_RESCAN[variant][1]:
            _rescan_variant(c, knn, tag, ("grescan", d, variant), d, variant, k)
    c.close()


# ------------------------------------------------ 6. partial lists and merge
@pytest.mark.parametrize("tag,name", [("sad", "gpart32"), ("fix16", "part32")])
def test_partial_and_merge_large_w(knn, tag, name):
    """search_partial_device at w = 513 and 1001 with the tuning key set, then
    the train set in 2 and in 5 shards (idx_offset, per-shard images and, on
    path 8, per-shard mu, e and Dx) at w = 1001 merged at k = 1000."""
    import torch
    tr, lab, te = l1kcap.case(name)
    n, d = tr.shape
    m = te.shape[0]
    grid = l1kcap.is_grid(name)
    dev = torch.device("cuda", 0)
    Q = torch.from_numpy(te.copy()).to(dev)
    X = torch.from_numpy(tr.copy()).to(dev)
    L = torch.from_numpy(lab.copy()).to(dev)
    c = _clf(knn, tag)
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, CLASSES, keep=(X, L))
    for w in (513, 1001):
        pd = torch.empty((m, w), dtype=torch.float64, device=dev)
        pi = torch.empty((m, w), dtype=torch.int64, device=dev)
        pl = torch.empty((m, w), dtype=torch.int32, device=dev)
        c.search_partial_device(Q.data_ptr(), m, w, L1, pd.data_ptr(), pi.data_ptr(), pl.data_ptr())
        c.sync()
        _report("partial w=%d" % w, tag, w - 1, c, m)
        _served(c, tag, d, 4, R=16)
        _, widx, wdist = l1kcap.oracle_knn(name, w - 1, n_out=w)
        gi, gd = pi.cpu().numpy(), pd.cpu().numpy()
        assert (gd.view(np.int64) == wdist.view(np.int64)).all()
        if grid:  # (indices may differ inside runs of equal distances only)
            assert_neighbors_match(gi, gd, widx, wdist)
        else:
            np.testing.assert_array_equal(gi, widx)
        np.testing.assert_array_equal(pl.cpu().numpy(), lab[gi])
    c.close()
    k, w = 1000, 1001
    ref = l1kcap.oracle_knn(name, k)
    lab_all = torch.from_numpy(lab.copy()).to(dev)
    for parts in (2, 5):
        gd = torch.empty((parts, m, w), dtype=torch.float64, device=dev)
        gi = torch.empty((parts, m, w), dtype=torch.int64, device=dev)
        gl = torch.empty((parts, m, w), dtype=torch.int32, device=dev)
        keep = []
        for p in range(parts):
            r0, r1 = n * p // parts, n * (p + 1) // parts
            cs = _clf(knn, tag)
            Xs = torch.from_numpy(tr[r0:r1].copy()).to(dev)
            Ls = torch.from_numpy(lab[r0:r1].copy()).to(dev)
            cs.set_train_device(Xs.data_ptr(), Ls.data_ptr(), r1 - r0, d, CLASSES, idx_offset=r0,
                                keep=(Xs, Ls))
            cs.search_partial_device(Q.data_ptr(), m, w, L1, gd[p].data_ptr(), gi[p].data_ptr(),
                                     gl[p].data_ptr())
            cs.sync()
            _served(cs, tag, d, 4, R=16)
            keep.append(cs)
        _report("shards=%d w=%d" % (parts, w), tag, k, keep[-1], m)
        # every shard's list: sorted, inside its shard, labelled by its rows
        si = gi.cpu().numpy()
        diffs = np.diff(gd.cpu().numpy(), axis=2)
        assert (diffs >= 0).all() if grid else (diffs > 0).all()
        for p in range(parts):
            assert (si[p] >= n * p // parts).all() and (si[p] < n * (p + 1) // parts).all()
        np.testing.assert_array_equal(gl.cpu().numpy(), lab[si])
        ol = torch.empty(m, dtype=torch.int32, device=dev)
        oi = torch.empty((m, k), dtype=torch.int64, device=dev)
        od = torch.empty((m, k), dtype=torch.float64, device=dev)
        of = torch.empty(m, dtype=torch.int32, device=dev)
        keep[0].merge_vote_device(gd.data_ptr(), gi.data_ptr(), gl.data_ptr(), parts, m, w, k,
                                  ol.data_ptr(), oi.data_ptr(), od.data_ptr(), of.data_ptr())
        keep[0].sync()
        pend = torch.nonzero(of & knn.FLAG_TIE_PENDING).flatten().to(torch.int32)
        if grid and pend.numel():
            # flagged queries: the reference's order over the whole train set
            # (every shard's distances, then the owner's resolve)
            rows = [n * (p + 1) // parts - n * p // parts for p in range(parts)]
            blocks = []
            for cs, nr in zip(keep, rows):
                D = torch.empty((pend.numel(), nr), dtype=torch.float64, device=dev)
                cs.shard_distances_device(Q.data_ptr(), pend.data_ptr(), pend.numel(), L1,
                                          D.data_ptr())
                cs.sync()
                blocks.append(D.reshape(-1))
            Dall = torch.cat(blocks)
            keep[0].tie_resolve_device(Dall.data_ptr(), rows, pend.numel(), lab_all.data_ptr(),
                                       pend.data_ptr(), k, ol.data_ptr(), oi.data_ptr(),
                                       od.data_ptr(), of.data_ptr())
            keep[0].sync()
        flags = of.cpu().numpy()
        assert not (flags & knn.FLAG_TIE_PENDING).any()
        _compare(knn, (ol.cpu().numpy(), oi.cpu().numpy(), od.cpu().numpy(), flags), ref, not grid)
        for cs in keep:
            cs.close()


# ------------------------------------------- 7. reference tie order at large k
@pytest.mark.parametrize("tag,tuning", [("sad", {}), ("fix16", {"i8l1": 0})])
def test_tie_order_large_k(knn, tag, tuning):
    """The reference-tie-order pass ("ties" = 2) over top-k rows of 150 and
    600 entries on integer data full of exact ties, from path 7 and from path
    8 (integer data sit on its code grid: tied rows have equal proxies and no
    coding error): labels, indices and distance bits equal the oracle's for
    every query."""
    tr, lab, te = l1kcap.tie_order_sets()
    c = _clf(knn, tag, ties=2, **tuning)
    c.set_train(tr, lab, CLASSES)
    for k in (150, 600):
        want, widx, wdist = l1kcap.oracle_knn("ties", k)
        c.tie_totals(reset=True)
        got, idx, dist, flags = c.classify(te, k, L1, return_neighbors=True)
        _report("ties=2", tag, k, c, te.shape[0])
        g = _served(c, tag, tr.shape[1], 4, R=16)
        assert g["rerank"] == kcap.rerank_count(k + 1, tr.shape[0])
        tied = (flags & TIE_BITS) != 0
        assert tied.sum() > 50, "expected many tied queries"
        assert ((flags & knn.FLAG_TIE_REF) != 0)[tied].all()
        assert ((flags & knn.FLAG_TIE_REF) != 0).sum() == tied.sum()
        assert c.tie_totals() == tied.sum()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(idx, widx)
        assert (dist.view(np.int64) == wdist.view(np.int64)).all()
    c.close()


# ------------------------------------------------------------------ 8. sweeps
@pytest.mark.parametrize("tag,name", l1kcap.SWEEP)
def test_sweep_kmax_1000(knn, tag, name):
    """classify_sweep with kmax = 1000 rides the pass: labels at every K equal
    the single calls' and the oracle's, counts equal numpy's, the kmax row's
    distances are bit-exact."""
    tr, lab, te = l1kcap.case(name)
    d, m = tr.shape[1], te.shape[0]
    ks = l1kcap.SWEEP_KS
    truth = np.random.default_rng(5).integers(0, CLASSES, m).astype(np.int32)
    c = _clf(knn, tag)
    c.set_train(tr, lab, CLASSES)
    labels, correct, idx, dist, flags = c.classify_sweep(te, ks, L1, truth=truth,
                                                         return_neighbors=True)
    _report("sweep", "%s d=%d" % (tag, d), max(ks), c, m)
    g = _served(c, tag, d, 4, R=16)
    assert g["rerank"] == kcap.rerank_count(max(ks) + 1, tr.shape[0])
    np.testing.assert_array_equal(correct, (labels == truth).sum(axis=1))
    want = l1kcap.oracle_knn(name, max(ks))
    assert (dist.view(np.int64) == want[2].view(np.int64)).all()
    if l1kcap.is_grid(name):
        assert_neighbors_match(idx, dist, want[1], want[2], flags)
    else:
        np.testing.assert_array_equal(idx, want[1])
        assert not (flags & TIE_BITS).any()
    for j, k in enumerate(ks):
        np.testing.assert_array_equal(labels[j], l1kcap.oracle_knn(name, k)[0],
                                      err_msg="oracle, K=%d" % k)
        np.testing.assert_array_equal(labels[j], c.classify(te, k, L1), err_msg="K=%d" % k)
        _served(c, tag, d, 4)
    c.close()


@pytest.mark.parametrize("tag,name", l1kcap.LOO)
def test_loo_sweep_near_the_seam(knn, tag, name):
    """loo_sweep at ks = 1, 500, 999 over a 3000-row train set: the search
    runs at k = 1000, the last one the candidate path serves, against the
    oracle on the row-removed sets."""
    tr, lab, _ = l1kcap.case(name)
    n, d = tr.shape
    ks = l1kcap.LOO_KS
    want = loo.expected_excl(tr, lab, tr, np.arange(n), ks, False, CLASSES)
    c = _clf(knn, tag)
    c.set_train(tr, lab, CLASSES)
    labels, correct, idx, dist, flags = c.loo_sweep(ks, L1, return_neighbors=True)
    _report("loo", "%s d=%d" % (tag, d), max(ks) + 1, c, n)
    _served(c, tag, d, 4, R=16)
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(correct, (want["labels"] == lab).sum(axis=1))
    np.testing.assert_array_equal(dist.view(np.int64), want["dist"].view(np.int64))
    # (train rows against train rows: the tie rules on either kind of data)
    assert_neighbors_match(idx, dist, want["idx"], want["dist"], flags)
    c.close()


# ------------------------------------------- 9. non-finite queries at k = 1000
@pytest.mark.parametrize("tag,name", [("sad", "gnonfin32"), ("fix16", "nonfin32")])
def test_nonfinite_query_k1000(knn, tag, name):
    """One NaN and one -inf query in a k = 1000 batch: label -1,
    KNN_FLAG_NONFINITE, no neighbours; the others bit-identical to a call
    without them."""
    tr, lab, te = l1kcap.case(name)
    d, m, k = tr.shape[1], te.shape[0], 1000
    te2 = te.copy()
    te2[3, 0] = np.nan
    te2[40, 31] = -np.inf
    bad = np.array([3, 40])
    ok = np.setdiff1d(np.arange(m), bad)
    c = _clf(knn, tag)
    c.set_train(tr, lab, CLASSES)
    got, idx, dist, flags = c.classify(te2, k, L1, return_neighbors=True)
    _report("nonfinite", "%s d=%d" % (tag, d), k, c, m)
    _served(c, tag, d, 4, R=16)
    assert (got[bad] == -1).all() and ((flags[bad] & knn.FLAG_NONFINITE) != 0).all()
    assert (idx[bad] == -1).all() and np.isnan(dist[bad]).all()
    assert not (flags[ok] & knn.FLAG_NONFINITE).any()
    want, widx, wdist = l1kcap.oracle_knn(name, k)
    _compare(knn, (got[ok], idx[ok], dist[ok], flags[ok]), (want[ok], widx[ok], wdist[ok]),
             not l1kcap.is_grid(name))
    got1, idx1, dist1, flags1 = c.classify(te, k, L1, return_neighbors=True)
    _served(c, tag, d, 4, R=16)
    np.testing.assert_array_equal(got[ok], got1[ok])
    np.testing.assert_array_equal(idx[ok], idx1[ok])
    np.testing.assert_array_equal(dist[ok].view(np.int64), dist1[ok].view(np.int64))
    keep = ~np.int32(knn.FLAG_EXACT_RESCAN)
    np.testing.assert_array_equal(flags[ok] & keep, flags1[ok] & keep)
    c.close()

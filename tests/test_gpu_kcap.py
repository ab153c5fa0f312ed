"""GPU parity at k = 101 .. 1000 on every candidate path.

Any k <= kMaxK = 1000 is served by the candidate pass, the merge
(merge_rerank_kernel) and the rescan; only above it does the exact large-k
kernel take over.  W = k + 1 from 102 to 1001 is where that pipeline reaches
its capacity limits: the re-rank count C = min(n, max(2W, W + 16), 1024, lists)
loses its 2x headroom above W = 512, the merge runs its 512- and 1024-entry
forms and its window-overflow branch, the lists switch from R = 8 to 16, the
fp16 stream kernel leaves its quad form, the quad-list kernels cannot hold W
on train sets of fewer than 64 tiles, and the full-scan rescan keeps a top W
of a thousand rows.

Every comparison is against the CPU oracle (fp64, pinned to the reference's
own outputs): labels equal, fp64 distances bit-identical, indices identical.
The continuous inputs have strictly increasing oracle distances
(test_kcap_data.py), so no tie flag may be set and every index must match;
the grid inputs of the int8 paths tie inherently and follow the parity
suite's tie rules.  Paths, kernel forms and geometries are asserted from
last_candidate_path / last_kernel_name / last_geometry, never assumed.
Rescan shares are printed, not asserted, except where the construction
derives them (every query where the lists hold fewer than W rows).
"""
import numpy as np
import pytest

import kcap
from test_gpu_parity import _i8_kernel, assert_neighbors_match, run_case

pytestmark = pytest.mark.gpu

CLASSES = kcap.CLASSES
TIE_BITS = 14  # KNN_FLAG_TIE_BOUNDARY | TIE_VOTE | TIE_ORDER


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


def _classifier(knn, prec="auto", **tuning):
    c = knn.Classifier(0)
    c.set_precision({"auto": knn.PRECISION_AUTO, "fp32": knn.PRECISION_FP32,
                     "bf16x3": knn.PRECISION_BF16X3, "fp16": knn.PRECISION_FP16}[prec])
    for key, value in tuning.items():
        c.set_tuning(key, value)
    return c


def _compare(knn, out, ref, strict):
    """run_case's bar on one call's outputs; strict (continuous data, distinct
    oracle distances): no tie flag, every index equal."""
    got, idx, dist, flags = out
    want, widx, wdist = ref
    if strict:
        assert not (flags & TIE_BITS).any(), "tie flag on data without ties"
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(idx, widx)
        assert (dist.view(np.int64) == wdist.view(np.int64)).all(), "distances not bit-exact"
        return
    tie_vote = (flags & knn.FLAG_TIE_VOTE) != 0
    assert (got[~tie_vote] == want[~tie_vote]).all(), "labels differ on untied queries"
    ref_order = (flags & knn.FLAG_TIE_REF) != 0
    assert not (ref_order & ((flags & TIE_BITS) == 0)).any(), "untied query re-ordered"
    np.testing.assert_array_equal(idx[ref_order], widx[ref_order])
    assert_neighbors_match(idx, dist, widx, wdist, flags)
    differs = int((got[tie_vote] != want[tie_vote]).sum())
    assert differs == 0, "%d exact-tie votes differ from the reference order" % differs


def _check(c, knn, name, k, metric):
    """One classify call on a trained context against the cached oracle;
    returns the flags.  Rescan flags and count must agree."""
    te = kcap.case(name)[2]
    out = c.classify(te, k, metric, return_neighbors=True)
    _compare(knn, out, kcap.oracle_knn(name, k, metric), not kcap.is_grid(name))
    flags = out[3]
    assert int(((flags & knn.FLAG_EXACT_RESCAN) != 0).sum()) == c.last_rescan_count()
    return flags


def _report(tag, path, k, c, m):
    g = c.last_geometry()
    print("kcap %s path=%s k=%d kernel=%s (workgroups, S, R, C)=(%d, %d, %d, %d) rescans=%d/%d"
          % (tag, path, k, c.last_kernel_name(), g["workgroups"], g["splits"], g["lists"],
             g["rerank"], c.last_rescan_count(), m))
    return g


# ---------------------------------------------------------------- 1. k ladder
LADDER_KS = [101, 102, 103, 127, 128, 255, 256, 511, 512, 999, 1000]
# path: case, metric, precision, tuning, last_candidate_path, lists of R = 8/16
LADDER = {
    "fp32": ("ladder48", 0, "fp32", {}, 0, True),
    "L1": ("ladder48", 1, "auto", {}, 1, True),
    "bf16x3": ("ladder48", 0, "auto", {"mfma16": 0}, 2, True),
    # (the 16x16x32 bf16x3 kernel exists at DP % 32 == 0 only: d = 64)
    "m16": ("ladder64", 0, "bf16x3", {"mfma16": 1}, 3, False),
    "fp16": ("ladder48", 0, "fp16", {}, 4, False),
    "i8": ("grid48", 0, "auto", {"i8": 1, "i8w": 0}, 5, False),
    "i8w": ("grid96", 0, "auto", {"i8": 1, "i8w": 1}, 6, False),
}


@pytest.mark.parametrize("path", sorted(LADDER))
def test_k_ladder(knn, path):
    """W = k + 1 on both sides of the merge's 256 -> 512 -> 1024 forms, of 2W
    reaching the 1024 cap, of the R = 8 -> 16 switch, and the last k before
    the large-k kernel: one train set per path, every k of the ladder."""
    name, metric, prec, tuning, want_path, pair_lists = LADDER[path]
    tr, lab, te = kcap.case(name)
    n, m = tr.shape[0], te.shape[0]
    c = _classifier(knn, prec, **tuning)
    c.set_train(tr, lab, CLASSES)
    for k in LADDER_KS:
        W = k + 1
        _check(c, knn, name, k, metric)
        g = _report("ladder", path, k, c, m)
        assert c.last_candidate_path() == want_path
        assert c.last_kernel_name().startswith("cand_"), c.last_kernel_name()
        # at this n (>= 64 tiles of every kernel) the lists hold the whole C
        assert g["rerank"] == kcap.rerank_count(W, n)
        if pair_lists:
            # two lists per split: R = 8 while a share of 0.8 per list fits 64
            # splits ((5W + 7) / 8 <= 64, W <= 102), then R = 16
            assert g["lists"] == (16 if W >= 103 else 8)
        else:
            assert g["lists"] == 4 and g["splits"] == 64  # quad lists: 4 * 64 * 4 = 1024
        assert 2 * g["splits"] * g["lists"] * (1 if pair_lists else 2) >= g["rerank"]
    c.close()
    if path == "m16":
        # at a width without a 16x16x32 kernel (DP = 48) the request falls
        # back to the 32x32x16 bf16x3 kernel
        tr, lab, te = kcap.case("ladder48")
        c = _classifier(knn, prec, **tuning)
        c.set_train(tr, lab, CLASSES)
        _check(c, knn, "ladder48", 255, 0)
        assert c.last_candidate_path() == 2
        c.close()


# ------------------------------------------------------ 2. the same at d > 256
LARGE_D_KS = [100, 101, 102, 300, 1000]
# path: metric, precision, last_candidate_path, kernel name by R
# (AUTO takes the fp16 pass at d > 256: the bf16x3 S3 kernel is forced)
LARGE_D = {
    "fp32": (0, "fp32", 0, "cand_stream_kernel<32,%d,0>"),
    "L1": (1, "auto", 1, "cand_stream_kernel<32,%d,1>"),
    "bf16x3": (0, "bf16x3", 2, "cand_s3_kernel<%d,false,false>"),
    "fp16": (0, "fp16", 4, None),
}


@pytest.mark.parametrize("path", sorted(LARGE_D))
def test_k_ladder_large_d(knn, path):
    """d = 300: the stream kernels.  fp16 S3 runs its quad form (16x16x32,
    R = 8 quad lists, (5W + 15) / 16 <= 32 splits) up to k = 101 and the
    32x32x16 form with R = 16 from k = 102; the others switch R = 8 -> 16 at
    the same k ((5W + 7) / 8 <= 64 splits holds up to W = 102)."""
    metric, prec, want_path, kname = LARGE_D[path]
    name = "ladder300"
    tr, lab, te = kcap.case(name)
    n, m = tr.shape[0], te.shape[0]
    c = _classifier(knn, prec)
    c.set_train(tr, lab, CLASSES)
    for k in LARGE_D_KS:
        W = k + 1
        _check(c, knn, name, k, metric)
        g = _report("large_d", path, k, c, m)
        assert c.last_candidate_path() == want_path
        assert g["rerank"] == kcap.rerank_count(W, n)
        R = 8 if k <= 101 else 16
        assert g["lists"] == R
        if path == "fp16":
            want = "cand_s3_kernel<8,true,true>" if k <= 101 else "cand_s3_kernel<16,true,false>"
            assert c.last_kernel_name() == want
        else:
            assert c.last_kernel_name() == kname % R
    c.close()
    if path == "fp16":
        # the query-resident kernel in place of the quad form, at its last k
        tr, lab, te = kcap.case("qres320")
        c = _classifier(knn, "fp16", qres=1)
        c.set_train(tr, lab, CLASSES)
        _check(c, knn, "qres320", 101, 0)
        g = _report("large_d", "qres", 101, c, te.shape[0])
        assert c.last_kernel_name() == "cand_qres_kernel<10>"
        assert c.last_candidate_path() == 4 and g["lists"] == 8
        assert g["rerank"] == kcap.rerank_count(102, tr.shape[0])
        c.close()


# ------------------------------------------------------- 3. forced wide union
@pytest.mark.parametrize("metric", [0, 1])
def test_wide_union(knn, metric):
    """S = 64 splits of R = 16 lists: a union of 2048 entries, the merge's
    32-entries-per-lane forms (64 threads at k = 10, 256 at k = 600); S = 33
    (1056, just over the line) and S = 32 (1024, just under)."""
    name = "wide24"
    tr, lab, te = kcap.case(name)
    for S in (64, 33, 32):
        c = _classifier(knn, "fp32", S=S, R=16)
        c.set_train(tr, lab, CLASSES)
        for k in (10, 600):
            _check(c, knn, name, k, metric)
            g = _report("wide", "fp32" if metric == 0 else "L1", k, c, te.shape[0])
            assert c.last_candidate_path() == metric
            assert g["splits"] == S and g["lists"] == 16
            assert g["rerank"] == kcap.rerank_count(k + 1, tr.shape[0])
            assert c.last_kernel_name() == "cand_kernel<24,16,%d,4>" % metric
        c.close()


# ------------------------------------------------ 4. lists that cannot hold W
# forced quad-list path: case, tuning / precision, path, train rows per tile
SMALL = {
    "fp16": ("small48", "fp16", {}, 4, 128),
    "i8": ("gsmall48", "auto", {"i8": 1, "i8w": 0}, 5, 256),
    "i8w": ("gsmall96", "auto", {"i8": 1, "i8w": 1}, 6, 256),
    "auto": ("small48", "auto", {}, 2, 0),
}


def _all_rescanned_if_short(c, knn, flags, W, m):
    g = c.last_geometry()
    if g["rerank"] < W:
        assert c.last_rescan_count() == m
        assert ((flags & knn.FLAG_EXACT_RESCAN) != 0).all()
    return g


@pytest.mark.parametrize("mode", sorted(SMALL))
def test_lists_smaller_than_W(knn, mode):
    """n = 3000: fewer than 64 train tiles, so the quad-list kernels' 4 lists
    of R = 4 per split hold 16 * tiles < W entries; no query can be certified
    and every one must be finished by the rescan, exactly."""
    name, prec, tuning, want_path, trows = SMALL[mode]
    tr, lab, te = kcap.case(name)
    n, m = tr.shape[0], te.shape[0]
    c = _classifier(knn, prec, **tuning)
    c.set_train(tr, lab, CLASSES)
    for k in (1000, 400):
        W = k + 1
        flags = _check(c, knn, name, k, 0)
        g = _report("small_n", mode, k, c, m)
        assert c.last_candidate_path() == want_path
        assert c.last_kernel_name().startswith("cand_")
        if trows:
            tiles = (n + 255) // 256 * 256 // trows  # (rows are padded to 256)
            assert tiles < 64 and g["splits"] == tiles and g["lists"] == 4
            assert g["rerank"] == 16 * tiles < W
        _all_rescanned_if_short(c, knn, flags, W, m)
    c.close()


@pytest.mark.parametrize("mode", ["auto", "fp16", "i8"])
@pytest.mark.parametrize("n,k", kcap.EDGES)
def test_small_n_edges(knn, n, k, mode):
    """W = n, k = n and train sets of one row more or less than the 1024-row
    union, the 1000-row k cap and a 256-row tile."""
    name = ("gedge%d" if mode == "i8" else "edge%d") % n
    tr, lab, te = kcap.case(name)
    c = _classifier(knn, "fp16" if mode == "fp16" else "auto", **({"i8": 1} if mode == "i8" else {}))
    c.set_train(tr, lab, CLASSES)
    flags = _check(c, knn, name, k, 0)
    _report("edge n=%d" % n, mode, k, c, te.shape[0])
    # (int8 at d = 16: 32x32x32 pads to 32 dims where 16x16x64 pads to 64)
    assert c.last_candidate_path() == {"auto": 2, "fp16": 4, "i8": _i8_kernel(16, -1)[0]}[mode]
    assert c.last_kernel_name().startswith("cand_")
    _all_rescanned_if_short(c, knn, flags, min(k + 1, n), te.shape[0])
    c.close()


# ------------------------------------------------------ 5. rescan at large W
@pytest.mark.parametrize("d,prec,path", [(32, "auto", 2), (32, "fp16", 4), (300, "auto", 4),
                                         (300, "fp32", 0)])
def test_rescan_large_w(knn, d, prec, path):
    """(a) 1500 exact copies of one row under 16 queries at k = 600: more rows
    within reach than the fast rescan keeps, so the full scan keeps the top
    601 by (dist, idx); (b) the copies 1e-9 apart, k = 600 and 1000; (c) 700
    copies at k = 1000, which the fast path can finish."""
    sit = kcap.RESCAN_SITTING
    c = _classifier(knn, prec)
    for variant in sorted(kcap.RESCAN):
        tr, lab, te = kcap.rescan_case(d, variant)
        for k in kcap.RESCAN[variant][2]:
            c.rescan_totals(reset=True)
            got, want, flags = run_case(c, knn, tr, lab, te, k, 0, CLASSES)
            failed, full = c.rescan_totals()
            _report("rescan %s d=%d full=%d" % (variant, d, full), prec, k, c, te.shape[0])
            assert c.last_candidate_path() == path
            assert c.last_kernel_name().startswith("cand_")
            assert failed == c.last_rescan_count()
            assert int(((flags & knn.FLAG_EXACT_RESCAN) != 0).sum()) == failed
            if variant == "a":
                assert full >= sit
                assert ((flags[:sit] & knn.FLAG_EXACT_RESCAN) != 0).all()
            if variant == "b":  # (exact copies tie for every query; these do not)
                assert not (flags & TIE_BITS).any()
    c.close()


# ------------------------------------------------ 6. partial lists and merge
@pytest.mark.parametrize("metric", [0, 1])
def test_partial_and_merge_large_w(knn, metric):
    """search_partial_device at w = 513 and 1001 on the candidate path, then
    the train set in 2 and in 5 shards at w = 1001 merged at k = 1000: unions
    of 2002 (LDS merge) and 5005 entries (rank merge through scratch)."""
    import torch
    name = "part32"
    tr, lab, te = kcap.case(name)
    n, d = tr.shape
    m = te.shape[0]
    dev = torch.device("cuda", 0)
    Q = torch.from_numpy(te.copy()).to(dev)
    X = torch.from_numpy(tr.copy()).to(dev)
    L = torch.from_numpy(lab.copy()).to(dev)
    c = knn.Classifier(0)
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, CLASSES, keep=(X, L))
    for w in (513, 1001):
        pd = torch.empty((m, w), dtype=torch.float64, device=dev)
        pi = torch.empty((m, w), dtype=torch.int64, device=dev)
        pl = torch.empty((m, w), dtype=torch.int32, device=dev)
        c.search_partial_device(Q.data_ptr(), m, w, metric, pd.data_ptr(), pi.data_ptr(),
                                pl.data_ptr())
        c.sync()
        _report("partial w=%d" % w, "auto" if metric == 0 else "L1", w - 1, c, m)
        assert c.last_kernel_name().startswith("cand_")
        assert c.last_candidate_path() == (2 if metric == 0 else 1)
        _, widx, wdist = kcap.oracle_knn(name, w - 1, metric, n_out=w)
        np.testing.assert_array_equal(pi.cpu().numpy(), widx)
        assert (pd.cpu().numpy().view(np.int64) == wdist.view(np.int64)).all()
        np.testing.assert_array_equal(pl.cpu().numpy(), lab[widx])
    c.close()
    k, w = 1000, 1001
    ref = kcap.oracle_knn(name, k, metric)
    for parts in (2, 5):
        gd = torch.empty((parts, m, w), dtype=torch.float64, device=dev)
        gi = torch.empty((parts, m, w), dtype=torch.int64, device=dev)
        gl = torch.empty((parts, m, w), dtype=torch.int32, device=dev)
        keep = []
        for p in range(parts):
            r0, r1 = n * p // parts, n * (p + 1) // parts
            cs = knn.Classifier(0)
            Xs = torch.from_numpy(tr[r0:r1].copy()).to(dev)
            Ls = torch.from_numpy(lab[r0:r1].copy()).to(dev)
            cs.set_train_device(Xs.data_ptr(), Ls.data_ptr(), r1 - r0, d, CLASSES, idx_offset=r0,
                                keep=(Xs, Ls))
            cs.search_partial_device(Q.data_ptr(), m, w, metric, gd[p].data_ptr(),
                                     gi[p].data_ptr(), gl[p].data_ptr())
            cs.sync()
            assert cs.last_kernel_name().startswith("cand_")
            keep.append(cs)
        # every shard's list: sorted, inside its shard, labelled by its rows
        si = gi.cpu().numpy()
        assert (np.diff(gd.cpu().numpy(), axis=2) > 0).all()
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
        flags = of.cpu().numpy()
        assert not (flags & knn.FLAG_TIE_PENDING).any()
        _compare(knn, (ol.cpu().numpy(), oi.cpu().numpy(), od.cpu().numpy(), flags), ref, True)
        for cs in keep:
            cs.close()


# ------------------------------------------- 7. tie order and sweep at large k
@pytest.mark.parametrize("metric", [0, 1])
def test_tie_order_large_k(knn, metric):
    """The reference-tie-order pass (tuning "ties" = 2) over top-k rows of 150
    and 600 entries on integer data full of exact ties: labels, indices and
    distance bits equal the oracle's for every query."""
    from test_gpu_parity import oracle
    rng = np.random.default_rng(71 + metric)
    centres = rng.integers(0, 256, (5, 12))
    lab = rng.integers(0, 5, 5300).astype(np.int32)
    X = np.clip(centres[lab] + rng.integers(-5, 6, (5300, 12)), 0, 255).astype(np.float64)
    tr, te, lab = X[:5000].copy(), X[5000:].copy(), lab[:5000].copy()
    c = knn.Classifier(0)
    c.set_tuning("ties", 2)
    c.set_train(tr, lab, 5)
    for k in (150, 600):
        want, widx, wdist = oracle.knn(tr, lab, te, k, metric == 0, 5, n_out=k)
        c.tie_totals(reset=True)
        got, idx, dist, flags = c.classify(te, k, metric, return_neighbors=True)
        assert c.last_kernel_name().startswith("cand_")
        tied = (flags & TIE_BITS) != 0
        assert tied.sum() > 50, "expected many tied queries"
        assert ((flags & knn.FLAG_TIE_REF) != 0).sum() == tied.sum()
        assert c.tie_totals() == tied.sum()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(idx, widx)
        assert (dist.view(np.int64) == wdist.view(np.int64)).all()
    c.close()


SWEEP_KS = [1, 100, 101, 512, 1000]


@pytest.mark.parametrize("mode,metric,path", [("auto", 0, 2), ("auto", 1, 1), ("i8", 0, 5),
                                              ("i8", 1, 1)])
def test_sweep_kmax_1000(knn, mode, metric, path):
    """classify_sweep with kmax = 1000 rides the candidate path: labels at
    every K equal the single calls' and the oracle's, counts equal numpy's."""
    name = "gsweep64" if mode == "i8" else "sweep40"
    tr, lab, te = kcap.case(name)
    m = te.shape[0]
    truth = np.random.default_rng(5).integers(0, CLASSES, m).astype(np.int32)
    c = _classifier(knn, "auto", **({"i8": 1} if mode == "i8" else {}))
    c.set_train(tr, lab, CLASSES)
    labels, correct, idx, dist, flags = c.classify_sweep(te, SWEEP_KS, metric, truth=truth,
                                                         return_neighbors=True)
    _report("sweep", mode, 1000, c, m)
    assert c.last_candidate_path() == path
    assert c.last_kernel_name().startswith("cand_")
    np.testing.assert_array_equal(correct, (labels == truth).sum(axis=1))
    want1000 = kcap.oracle_knn(name, 1000, metric)
    assert (dist.view(np.int64) == want1000[2].view(np.int64)).all()
    if not kcap.is_grid(name):
        np.testing.assert_array_equal(idx, want1000[1])
        assert not (flags & TIE_BITS).any()
    for j, k in enumerate(SWEEP_KS):
        np.testing.assert_array_equal(labels[j], kcap.oracle_knn(name, k, metric)[0],
                                      err_msg="oracle, K=%d" % k)
        np.testing.assert_array_equal(labels[j], c.classify(te, k, metric), err_msg="K=%d" % k)
    c.close()


@pytest.mark.parametrize("prec,path", [("auto", 2), ("fp16", 4)])
def test_nonfinite_query_k1000(knn, prec, path):
    """One NaN and one inf query in a k = 1000 batch on the candidate path:
    label -1, KNN_FLAG_NONFINITE, no neighbours; the others unchanged."""
    name = "nonfin32"
    tr, lab, te = kcap.case(name)
    m, k = te.shape[0], 1000
    te2 = te.copy()
    te2[3, 0] = np.nan
    te2[40, 31] = -np.inf
    bad = np.array([3, 40])
    ok = np.setdiff1d(np.arange(m), bad)
    c = _classifier(knn, prec)
    c.set_train(tr, lab, CLASSES)
    got, idx, dist, flags = c.classify(te2, k, knn.L2, return_neighbors=True)
    assert c.last_candidate_path() == path and c.last_kernel_name().startswith("cand_")
    assert (got[bad] == -1).all() and ((flags[bad] & knn.FLAG_NONFINITE) != 0).all()
    assert (idx[bad] == -1).all() and np.isnan(dist[bad]).all()
    assert not (flags[ok] & knn.FLAG_NONFINITE).any()
    want, widx, wdist = kcap.oracle_knn(name, k, 0)
    _compare(knn, (got[ok], idx[ok], dist[ok], flags[ok]), (want[ok], widx[ok], wdist[ok]), True)
    got1, idx1, dist1, flags1 = c.classify(te, k, knn.L2, return_neighbors=True)
    np.testing.assert_array_equal(got[ok], got1[ok])
    np.testing.assert_array_equal(idx[ok], idx1[ok])
    np.testing.assert_array_equal(flags[ok], flags1[ok])
    c.close()

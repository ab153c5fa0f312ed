"""Leave-one-out K sweep on the GPU (knn_loo_sweep*, knn_classify_sweep_excl_device,
knn_group_loo_sweep, the driver's --loo) against the CPU oracle run on the
ROW-REMOVED train sets (tests/loo.py): for a query with excluded row e the
result is the K sweep's on the train set without row e, indices mapped back.

The order among equal distances that counts is the reference's std::sort over
the n - 1 remaining records -- another introsort run than the one over all n
-- so a build that drops the row but keeps the n-record order fails on the
order-sensitive rows test_loo_data.py counts.
"""
import os

import numpy as np
import pytest

import datagen
import loo
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def knn():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(root, "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.lib().knn_device_count() < 1:
        pytest.fail("no HIP device visible: the KNN path has no CPU fallback")
    return mod


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _trained(knn, name, prec=None, **tuning):
    s = loo.SETS[name]
    tr, lab = loo.data(name)
    c = knn.Classifier(0)
    if prec is not None:
        c.set_precision(prec)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    c.set_train(tr, lab, s["classes"])
    return c, s


def _loo_device(c, row0, rows, ks, metric, want_correct=True):
    """loo_sweep_device into torch buffers -> numpy (labels, correct, idx, dist, flags)."""
    import torch
    dev = torch.device("cuda", 0)
    nk, kmax, r1 = len(ks), max(ks), max(rows, 1)
    L = torch.full((nk, r1), -7, dtype=torch.int32, device=dev)
    C = torch.full((nk,), -7, dtype=torch.int64, device=dev)
    I = torch.full((r1, kmax), -7, dtype=torch.int64, device=dev)
    D = torch.zeros((r1, kmax), dtype=torch.float64, device=dev)
    F = torch.full((r1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    c.loo_sweep_device(row0, rows, ks, metric, L.data_ptr(), C.data_ptr() if want_correct else None,
                       I.data_ptr(), D.data_ptr(), F.data_ptr())
    c.sync()
    return (L.cpu().numpy()[:, :rows], C.cpu().numpy(), I.cpu().numpy()[:rows],
            D.cpu().numpy()[:rows], F.cpu().numpy()[:rows])


# ------------------------------------------------ 1. the data sets, all rows
@pytest.mark.parametrize("name", ["A", "A1", "B"])
def test_data_sets(knn, name):
    w = loo.expected_loo(name)
    nv = w["naive"]
    c, s = _trained(knn, name)
    labels, correct, idx, dist, flags = c.loo_sweep(s["ks"], s["metric"], return_neighbors=True)
    assert labels.shape == (len(s["ks"]), s["n"])
    wrong = (labels != w["labels"]).any(axis=0)
    print("%s: %d rows differ from the oracle (%d order-sensitive, %d in drop case two)"
          % (name, wrong.sum(), w["sensitive"].sum(), nv["case2"].sum()))
    np.testing.assert_array_equal(labels, w["labels"])
    np.testing.assert_array_equal(correct, w["correct"])
    assert correct.dtype == np.int64
    np.testing.assert_array_equal(idx, w["idx1"])
    np.testing.assert_array_equal(_bits(dist), _bits(w["dist"]))
    np.testing.assert_array_equal(flags & loo.FLAG_MASK, w["flags1"])
    # "ties" = 2: every row with a tie in its top kmax in the reference's order
    c.set_tuning("ties", 2)
    labels2, correct2, idx2, dist2, flags2 = c.loo_sweep(s["ks"], s["metric"], return_neighbors=True)
    np.testing.assert_array_equal(labels2, w["labels"])
    np.testing.assert_array_equal(idx2, np.where(nv["tied"][:, None], w["idx"], nv["idx"]))
    np.testing.assert_array_equal(flags2 & loo.FLAG_MASK, nv["flags"] | np.where(nv["tied"], 32, 0))
    # "ties" = 0: the (dist, index) order minus the row, prefix-voted
    c.set_tuning("ties", 0)
    labels0, correct0, idx0, dist0, flags0 = c.loo_sweep(s["ks"], s["metric"], return_neighbors=True)
    np.testing.assert_array_equal(labels0, nv["labels"])
    np.testing.assert_array_equal(idx0, nv["idx"])
    np.testing.assert_array_equal(_bits(dist0), _bits(nv["dist"]))
    np.testing.assert_array_equal(flags0 & loo.FLAG_MASK, nv["flags"])
    np.testing.assert_array_equal(correct0, (nv["labels"] == loo.data(name)[1]).sum(axis=1))
    c.close()


# ------------------------------------------------ 2. every candidate path
PATHS = {
    "i8": (None, {"i8": 1, "i8w": 0}, 5),
    "i8w": (None, {"i8": 1, "i8w": 1}, 6),
    "fp16": (None, {"fp16": 1}, 4),
    "bf16x3": ("BF16X3", {}, 2),
    "fp32": ("FP32", {}, 0),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_candidate_paths(knn, path):
    """Data set A's grid scaled by 1/8 (exact in every operand format; the
    distances scale by a power of two, so labels and indices are A's)."""
    prec, tuning, want_path = PATHS[path]
    w = loo.expected_loo("A")
    s = loo.SETS["A"]
    tr, lab = loo.data("A")
    c = knn.Classifier(0)
    if prec:
        c.set_precision(getattr(knn, "PRECISION_" + prec))
    for key, value in tuning.items():
        c.set_tuning(key, value)
    c.set_train(tr / 8.0, lab, s["classes"])
    labels, correct, idx, dist, flags = c.loo_sweep(s["ks"], s["metric"], return_neighbors=True)
    assert c.last_candidate_path() == want_path
    np.testing.assert_array_equal(labels, w["labels"])
    np.testing.assert_array_equal(correct, w["correct"])
    np.testing.assert_array_equal(idx, w["idx1"])
    np.testing.assert_array_equal(_bits(dist), _bits(w["dist"] / 8.0))
    np.testing.assert_array_equal(flags & loo.FLAG_MASK, w["flags1"])
    c.close()


# ------------------------------------------------ 3. general exclusion
def test_general_exclusion(knn):
    """200 queries off the train set: a third exclude their nearest row, a
    third a far row, a third nothing."""
    s = loo.SETS["A"]
    tr, lab = loo.data("A")
    rng = np.random.default_rng(211)
    Q = rng.integers(0, 8, (200, 6)).astype(np.float64)
    excl = np.full(200, -1, np.int64)
    ar = np.arange(s["n"])
    for i in range(200):
        D = oracle.row_distances(Q[i], tr, True)
        if i % 3 == 0:
            excl[i] = np.lexsort((ar, D))[0]
        elif i % 3 == 1:
            excl[i] = np.argmax(D)
    want = loo.expected_excl(tr, lab, Q, excl, s["ks"], True, s["classes"])
    nv = loo.naive(tr, lab, Q, excl, s["ks"], True)
    truth = np.random.default_rng(5).integers(0, 3, 200).astype(np.int32)
    c, _ = _trained(knn, "A")
    labels, correct, idx, dist, flags = c.classify_sweep(Q, s["ks"], knn.L2, truth=truth,
                                                         return_neighbors=True, exclude=excl)
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(correct, (want["labels"] == truth).sum(axis=1))
    np.testing.assert_array_equal(idx, np.where(nv["queued"][:, None], want["idx"], nv["idx"]))
    np.testing.assert_array_equal(_bits(dist), _bits(want["dist"]))
    np.testing.assert_array_equal(flags & loo.FLAG_MASK,
                                  nv["flags"] | np.where(nv["queued"], 32, 0))
    sel = excl >= 0
    assert not (idx[sel] == excl[sel, None]).any()
    # nothing excluded: today's sweep (KNN_FLAG_EXACT_RESCAN aside: the
    # search ran at kmax + 1, and certification is not part of the contract)
    plain = c.classify_sweep(Q, s["ks"], knn.L2, truth=truth, return_neighbors=True)
    for ex in (None, np.full(200, -1, np.int64), np.full(200, s["n"], np.int64),
               np.full(200, -5, np.int64)):
        got = c.classify_sweep(Q, s["ks"], knn.L2, truth=truth, return_neighbors=True, exclude=ex)
        for a, b in zip(got[:3], plain[:3]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(_bits(got[3]), _bits(plain[3]))
        np.testing.assert_array_equal(got[4] & ~knn.FLAG_EXACT_RESCAN,
                                      plain[4] & ~knn.FLAG_EXACT_RESCAN)
    c.close()


# ------------------------------------------------ 4. the large-k seam
@pytest.fixture(scope="module")
def seam():
    tr, lab = loo.grid(8, 6, 104, 1300, 3)
    return tr, lab


@pytest.mark.parametrize("ks", [[1, 999, 1000], [5, 1200, 1299]])
def test_large_k_seam(knn, seam, ks):
    """kmax = 1000: the search runs at 1001, the first width on the exact
    large-k path; kmax = n - 1: the list holds the whole set and the drop
    kernel walks rows of 1300 entries."""
    tr, lab = seam
    rows = np.arange(40)
    want = loo.expected_excl(tr, lab, tr[:40], rows, ks, True, 3)
    nv = loo.naive(tr, lab, tr[:40], rows, ks, True)
    c = knn.Classifier(0)
    c.set_train(tr, lab, 3)
    labels, correct, idx, dist, flags = _loo_device(c, 0, 40, ks, knn.L2)
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(correct, (want["labels"] == lab[:40]).sum(axis=1))
    np.testing.assert_array_equal(idx, np.where(nv["queued"][:, None], want["idx"], nv["idx"]))
    np.testing.assert_array_equal(_bits(dist), _bits(want["dist"]))
    np.testing.assert_array_equal(flags & loo.FLAG_MASK,
                                  nv["flags"] | np.where(nv["queued"], 32, 0))
    c.close()


def test_k_of_n_train_is_refused(knn, seam):
    tr, lab = seam
    c = knn.Classifier(0)
    c.set_train(tr, lab, 3)
    with pytest.raises(knn.KnnError, match=r"knn error -1: ks\[1\]"):
        c.loo_sweep([3, 1300])
    with pytest.raises(knn.KnnError, match=r"knn error -1: ks\[0\]"):
        _loo_device(c, 0, 40, [1300], knn.L2)
    assert c.classify_sweep(tr[:4], [1300]).shape == (1, 4)  # (the plain sweep takes K = n)
    c.close()


# ------------------------------------------------ 5. ranges and batches
def test_ranges(knn):
    w = loo.expected_loo("A")
    c, s = _trained(knn, "A")
    ks = s["ks"]
    lo = _loo_device(c, 0, 700, ks, knn.L2)
    hi = _loo_device(c, 700, 800, ks, knn.L2)
    np.testing.assert_array_equal(np.concatenate([lo[0], hi[0]], axis=1), w["labels"])
    np.testing.assert_array_equal(lo[1] + hi[1], w["correct"])
    np.testing.assert_array_equal(np.concatenate([lo[2], hi[2]]), w["idx1"])
    np.testing.assert_array_equal(_bits(np.concatenate([lo[3], hi[3]])), _bits(w["dist"]))
    np.testing.assert_array_equal(np.concatenate([lo[4], hi[4]]) & loo.FLAG_MASK, w["flags1"])
    last = _loo_device(c, 1499, 1, ks, knn.L2)
    np.testing.assert_array_equal(last[0], w["labels"][:, 1499:])
    np.testing.assert_array_equal(last[1], (w["labels"][:, 1499] == loo.data("A")[1][1499]))
    np.testing.assert_array_equal(last[2], w["idx1"][1499:])
    # d_correct is nullable
    nocorr = _loo_device(c, 0, 64, ks, knn.L2, want_correct=False)
    np.testing.assert_array_equal(nocorr[0], w["labels"][:, :64])
    assert (nocorr[1] == -7).all()
    # no rows: nothing written but the zeroed counts
    for row0 in (0, 1500):
        none = _loo_device(c, row0, 0, ks, knn.L2)
        assert (none[1] == 0).all()
    for row0, rows in ((-1, 2), (1499, 2), (1501, 0), (0, 1501), (0, -1)):
        with pytest.raises(knn.KnnError, match="knn error -1"):
            _loo_device(c, row0, rows, ks, knn.L2)
    c.close()


def test_idx_offset(knn):
    """The reported indices and the exclusion both carry the train set's offset."""
    import torch
    w = loo.expected_loo("A")
    s = loo.SETS["A"]
    tr, lab = loo.data("A")
    dev = torch.device("cuda", 0)
    dX = torch.from_numpy(np.array(tr)).to(dev)
    dL = torch.from_numpy(np.array(lab)).to(dev)
    torch.cuda.synchronize(dev)
    c = knn.Classifier(0)
    c.set_train_device(dX.data_ptr(), dL.data_ptr(), s["n"], 6, 3, idx_offset=1000, keep=(dX, dL))
    labels, correct, idx, dist, flags = _loo_device(c, 100, 200, s["ks"], knn.L2)
    np.testing.assert_array_equal(labels, w["labels"][:, 100:300])
    np.testing.assert_array_equal(idx, w["idx1"][100:300] + 1000)
    np.testing.assert_array_equal(flags & loo.FLAG_MASK, w["flags1"][100:300])
    # a general exclusion is a GLOBAL index: row 5 is 1005 here, and 5 is no row
    Q = np.array(tr[5:6])
    for e, same in ((1005, True), (5, False)):
        got = c.classify_sweep(Q, [1, 3], knn.L2, return_neighbors=True,
                               exclude=np.array([e], np.int64))
        assert (got[1][0, 0] != 1005) == same
        if same:
            np.testing.assert_array_equal(got[1][0], w["idx1"][5, :3] + 1000)
    c.close()


def test_host_batches(knn):
    """n = 16384 + 300: the host call crosses its batch boundary."""
    n, d, classes, ks = 16384 + 300, 8, 5, [1, 5]
    tr, lab, _, _, _, _ = datagen.make_sets("gauss", 77, n, 0, 0, d, classes)
    c = knn.Classifier(0)
    c.set_train(tr, lab, classes)
    labels, correct, idx, dist, flags = c.loo_sweep(ks, knn.L2, return_neighbors=True)
    assert labels.shape == (2, n) and idx.shape == (n, 5)
    np.testing.assert_array_equal(correct, (labels == lab).sum(axis=1))
    assert not (idx == np.arange(n)[:, None]).any()
    rows = np.concatenate([np.arange(16384 - 16, 16384 + 16), [0, 1, n - 1, n - 2],
                           np.random.default_rng(3).choice(n, 28, replace=False)])
    assert rows.shape == (64,)
    want = loo.expected_excl(tr, lab, tr[rows], rows, ks, True, classes)
    nv = loo.naive(tr, lab, tr[rows], rows, ks, True)
    np.testing.assert_array_equal(labels[:, rows], want["labels"])
    np.testing.assert_array_equal(idx[rows],
                                  np.where(nv["queued"][:, None], want["idx"], nv["idx"]))
    np.testing.assert_array_equal(_bits(dist[rows]), _bits(want["dist"]))
    c.close()


# ------------------------------------------------ 6. group
def test_group_loopback(knn):
    """Three ranks on one GPU take ragged thirds of the train rows."""
    for name in ("A", "A1"):
        w = loo.expected_loo(name)
        s = loo.SETS[name]
        tr, lab = loo.data(name)
        g = knn.Group([0, 0, 0], mode=0)
        g.set_train(tr, lab, s["classes"])
        labels, correct = g.loo_sweep(s["ks"], s["metric"])
        np.testing.assert_array_equal(labels, w["labels"])
        np.testing.assert_array_equal(correct, w["correct"])
        g.close()


def test_group_train_sharded_is_refused(knn):
    s = loo.SETS["A"]
    tr, lab = loo.data("A")
    g = knn.Group([0, 0, 0], mode=1)
    g.set_train(tr, lab, s["classes"])
    with pytest.raises(knn.KnnError, match=r"knn error -1: .*train-sharded"):
        g.loo_sweep(s["ks"], s["metric"])
    g.close()


# ------------------------------------------------ 7. driver
def test_driver_loo(knn, tmp_path, fmt_cout):
    spec = dict(kind="int", seed=23, N_train=600, N_test=40, N_val=10, dim=6, class_cnt=4)
    (tr, trl, te, _, _, _), _ = datagen.write_csvs(str(tmp_path), spec)
    os.remove(tmp_path / "validation.csv")  # --loo needs no validation file
    cfg = knn.KnnConfig(dim=6, K=7, N_train=600, N_test=40, N_val=10, class_cnt=4,
                        train_file_name="train.csv", validation_file_name="validation.csv",
                        test_file_name="test.csv")
    ks = [1, 3, 5]
    out = knn.run_driver(cfg, str(tmp_path), extra=["--loo", "--K_list", "1,3,5"])
    oracle.normalize(tr, te, None)
    want = loo.expected_excl(tr, trl, tr, np.arange(600), ks, True, 4)
    accs = [float((want["labels"][j] == trl).sum()) / 600 for j in range(3)]
    lines = out.splitlines()
    for j, k in enumerate(ks):
        assert lines[j] == "K = %d loo accuracy = %s" % (k, fmt_cout(accs[j]))
    best, sel = -1.0, None
    for k, a in zip(ks, accs):
        if a > best:
            best, sel = a, k
    assert lines[3] == "selected K = %d" % sel
    assert lines[4].startswith("Running time is ")
    got = np.loadtxt(tmp_path / "Test_label.csv", dtype=np.int64, ndmin=1)
    cfg.K, cfg.Validation = sel, False
    knn.run_driver(cfg, str(tmp_path), extra=["--output", "plain.csv"])
    np.testing.assert_array_equal(got, np.loadtxt(tmp_path / "plain.csv", dtype=np.int64, ndmin=1))
    np.testing.assert_array_equal(got, oracle.knn(tr, trl, te, sel, True, 4)[0])


# ------------------------------------------------ 8. untouched behaviour
def test_other_calls_unchanged(knn):
    """classify_sweep and classify give identical arrays before and after a
    leave-one-out sweep on the same context (shared workspace; the
    reference-order pass without an exclusion array)."""
    w = loo.expected_loo("A")
    c, s = _trained(knn, "A")
    Q = np.random.default_rng(9).integers(0, 8, (300, 6)).astype(np.float64)
    before = (c.classify_sweep(Q, s["ks"], knn.L2, return_neighbors=True),
              c.classify(Q, 5, knn.L2, return_neighbors=True))
    c.tie_totals(reset=True)
    labels, correct = c.loo_sweep(s["ks"], knn.L2)
    np.testing.assert_array_equal(labels, w["labels"])
    # the leave-one-out rows that took the reference-order pass
    assert c.tie_totals() == int(w["naive"]["queued"].sum())
    after = (c.classify_sweep(Q, s["ks"], knn.L2, return_neighbors=True),
             c.classify(Q, 5, knn.L2, return_neighbors=True))
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            np.testing.assert_array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                          y.view(np.int64) if y.dtype == np.float64 else y)
    c.close()

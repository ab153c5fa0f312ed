"""K sweep on the GPU: labels (and accuracy counts) for a list of K from one
search (knn_classify_sweep*, knn_vote_sweep_device, knn_group_classify_sweep,
the driver's --K_list) against the CPU oracle run once per K.

The reference's neighbour order does not depend on K, so the label at K is a
prefix vote over one ordered top-kmax row; with exact distance ties the order
that counts is the reference's std::sort order, at EVERY K of the list.
"""
import numpy as np
import pytest

import datagen
import oracle

pytestmark = pytest.mark.gpu

KS_TIES = [1, 2, 3, 4, 5, 7, 10, 11, 20, 37]


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


def _oracle_labels(tr, lab, q, ks, euclid, classes):
    """labels[nk, m] of the oracle, one run per distinct K (K = 0: -1)."""
    cache = {}
    for k in sorted(set(int(k) for k in ks)):
        cache[k] = (np.full(q.shape[0], -1, np.int32) if k == 0
                    else oracle.knn(tr, lab, q, k, euclid, classes)[0])
    return np.stack([cache[int(k)] for k in ks])


def _vote(labels):
    """cpp:324-337: the first label whose count strictly exceeds the running max."""
    cnt, best, win = {}, 0, -1
    for l in labels:
        c = cnt.get(int(l), 0) + 1
        cnt[int(l)] = c
        if c > best:
            best, win = c, int(l)
    return win


@pytest.fixture(scope="module")
def tie_data():
    """8-level integer grid in 6 dims: dense exact ties.  Per metric: train,
    labels, queries, the oracle's labels at every K of KS_TIES, its first 37
    neighbour indices and a random ground truth."""
    out = {}
    for metric in (0, 1):
        rng = np.random.default_rng(101 + metric)
        tr = rng.integers(0, 8, (3000, 6)).astype(np.float64)
        q = rng.integers(0, 8, (200, 6)).astype(np.float64)
        lab = rng.integers(0, 3, 3000).astype(np.int32)
        want = _oracle_labels(tr, lab, q, KS_TIES, metric == 0, 3)
        _, widx, _ = oracle.knn(tr, lab, q, 37, metric == 0, 3, n_out=37)
        truth = np.random.default_rng(7 + metric).integers(0, 3, 200).astype(np.int32)
        out[metric] = dict(tr=tr, q=q, lab=lab, want=want, widx=widx, truth=truth)
    return out


def _mix(rng, n, m, d, classes, spread=2.0, grid=1024.0):
    centres = rng.uniform(-spread, spread, (classes, d))
    lab = rng.integers(0, classes, n + m).astype(np.int32)
    X = centres[lab] + rng.standard_normal((n + m, d))
    if grid:
        X = np.round(X * grid) / grid
    tr, te = X[:n].copy(), X[n:].copy()
    oracle.normalize(tr, te, None)
    return tr, lab[:n].copy(), te


def _grid_codes(rng, n, m, d, classes, lo=0, hi=255, scale=256.0):
    centres = rng.uniform(lo + 40, hi - 40, (classes, d))
    lab = rng.integers(0, classes, n + m).astype(np.int32)
    X = np.clip(np.rint(centres[lab] + 25 * rng.standard_normal((n + m, d))), lo, hi) / scale
    return X[:n].copy(), lab[:n].copy(), X[n:].copy()


@pytest.mark.parametrize("metric", [0, 1])
def test_tie_decided_votes(knn, tie_data, metric):
    """Every K of the list gets the reference's label although the plain
    (dist, index) order would give another one for many queries."""
    t = tie_data[metric]
    # the input is not vacuous: count the queries whose (dist, index)-ordered
    # prefix vote differs from the reference's label at some K of the list
    sensitive = 0
    ar = np.arange(t["tr"].shape[0])
    for i in range(t["q"].shape[0]):
        D = oracle.row_distances(t["q"][i], t["tr"], metric == 0)
        order = np.lexsort((ar, D))[:max(KS_TIES)]
        sensitive += any(_vote(t["lab"][order[:k]]) != t["want"][j, i]
                         for j, k in enumerate(KS_TIES))
    print("order-sensitive queries (metric %d): %d of %d" % (metric, sensitive, t["q"].shape[0]))
    assert sensitive >= 50
    c = knn.Classifier(0)
    c.set_train(t["tr"], t["lab"], 3)
    labels, idx, dist, flags = c.classify_sweep(t["q"], KS_TIES, metric, return_neighbors=True)
    assert labels.shape == (len(KS_TIES), 200)
    np.testing.assert_array_equal(labels, t["want"])
    n_ref = int(((flags & knn.FLAG_TIE_REF) != 0).sum())
    assert n_ref >= 1
    c.set_tuning("ties", 2)
    labels2, idx2, dist2, flags2 = c.classify_sweep(t["q"], KS_TIES, metric, return_neighbors=True)
    np.testing.assert_array_equal(labels2, t["want"])
    n_ref2 = int(((flags2 & knn.FLAG_TIE_REF) != 0).sum())
    print("re-ordered queries: ties=1 %d, ties=2 %d" % (n_ref, n_ref2))
    assert n_ref <= n_ref2
    np.testing.assert_array_equal(idx2, t["widx"])
    c.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_equals_single_calls(knn, metric):
    """Unsorted ks with a duplicate and a zero: each row is classify(Q, k)."""
    tr, lab, te = _mix(np.random.default_rng(31 + metric), 4000, 300, 20, 5)
    ks = [50, 1, 7, 7, 0]
    c = knn.Classifier(0)
    c.set_train(tr, lab, 5)
    labels = c.classify_sweep(te, ks, metric)
    for j, k in enumerate(ks):
        np.testing.assert_array_equal(labels[j], c.classify(te, k, metric), err_msg="k=%d" % k)
    assert (labels[4] == -1).all()
    # nk = 1 is knn_classify's labels for that K
    np.testing.assert_array_equal(c.classify_sweep(te, [7], metric)[0], c.classify(te, 7, metric))
    c.close()


@pytest.mark.parametrize("kind,d,path", [("i8", 96, 6), ("i8", 128, 6), ("fp16", 300, 4)])
def test_candidate_paths(knn, kind, d, path):
    """The sweep rides the search's candidate paths: the int8 pass (AUTO at
    4096 queries of byte data) and the fp16 stream kernel at d > 256."""
    rng = np.random.default_rng(200 + d)
    c = knn.Classifier(0)
    if kind == "i8":
        tr, lab, te = _grid_codes(rng, 20000, 4096, d, 7)
    else:
        tr, lab, te = _mix(rng, 3000, 512, d, 7)
        c.set_precision(knn.PRECISION_FP16)
    ks = [1, 5, 10]
    c.set_train(tr, lab, 7)
    labels = c.classify_sweep(te, ks, knn.L2)
    assert c.last_candidate_path() == path
    sub = np.random.default_rng(1).choice(te.shape[0], 256, replace=False)
    want = _oracle_labels(tr, lab, te[sub], ks, True, 7)
    np.testing.assert_array_equal(labels[:, sub], want)
    c.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_large_k(knn, metric):
    """ks across kMaxK = 1000: the exact large-k search and the chunked row walk."""
    rng = np.random.default_rng(55 + metric)
    tr = rng.integers(0, 12, (1500, 5)).astype(np.float64)
    q = rng.integers(0, 12, (64, 5)).astype(np.float64)
    lab = rng.integers(0, 4, 1500).astype(np.int32)
    ks = [3, 1000, 1001, 1200]
    want = _oracle_labels(tr, lab, q, ks, metric == 0, 4)
    c = knn.Classifier(0)
    c.set_train(tr, lab, 4)
    np.testing.assert_array_equal(c.classify_sweep(q, ks, metric), want)
    # kmax <= kMaxK on the candidate path, same data
    np.testing.assert_array_equal(c.classify_sweep(q, ks[:2], metric), want[:2])
    c.close()


@pytest.mark.parametrize("m", [200, 1, 65])
def test_accuracy_counts(knn, tie_data, m):
    t = tie_data[0]
    c = knn.Classifier(0)
    c.set_train(t["tr"], t["lab"], 3)
    labels, correct = c.classify_sweep(t["q"][:m], KS_TIES, knn.L2, truth=t["truth"][:m])
    np.testing.assert_array_equal(labels, t["want"][:, :m])
    np.testing.assert_array_equal(correct, (labels == t["truth"][:m]).sum(axis=1))
    assert correct.dtype == np.int64
    c.close()


def test_nonfinite_query(knn, tie_data):
    t = tie_data[0]
    q = t["q"][:70].copy()
    q[33, 2] = np.nan
    truth = np.full(70, -1, np.int32)  # even a truth of -1 is never "correct" for no label
    truth[:33] = t["truth"][:33]
    c = knn.Classifier(0)
    c.set_train(t["tr"], t["lab"], 3)
    labels, correct, idx, dist, flags = c.classify_sweep(q, KS_TIES, knn.L2, truth=truth,
                                                         return_neighbors=True)
    assert (labels[:, 33] == -1).all()
    assert flags[33] & knn.FLAG_NONFINITE
    keep = np.arange(70) != 33
    np.testing.assert_array_equal(labels[:, keep], t["want"][:, :70][:, keep])
    np.testing.assert_array_equal(correct, (labels[:, keep] == truth[keep]).sum(axis=1))
    c.close()


@pytest.mark.parametrize("base", [0, 1000])
def test_vote_sweep_device_alone(knn, tie_data, base):
    """The prefix votes over the oracle's own ordered rows."""
    import torch
    t = tie_data[1]
    dev = torch.device("cuda", 0)
    m, kmax = t["widx"].shape
    ks = [37, 1, 4, 4, 0, 20]
    want = _oracle_labels(t["tr"], t["lab"], t["q"], ks, False, 3)
    idx = torch.from_numpy(t["widx"] + base).to(dev)
    lab = torch.from_numpy(t["lab"]).to(dev)
    truth = torch.from_numpy(t["truth"]).to(dev)
    out = torch.full((len(ks), m), -7, dtype=torch.int32, device=dev)
    corr = torch.full((len(ks),), -7, dtype=torch.int64, device=dev)
    c = knn.Classifier(0)
    c.vote_sweep_device(idx.data_ptr(), m, kmax, lab.data_ptr(), ks, out.data_ptr(), idx_base=base,
                        d_truth=truth.data_ptr(), d_correct=corr.data_ptr())
    c.sync()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(corr.cpu().numpy(), (want == t["truth"]).sum(axis=1))
    c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_groups_over_loopback(knn, tie_data, mode):
    """Three ranks on one GPU (ragged thirds of 200 queries; mode 1: three
    train shards, cross-shard reference tie order) equal the single context."""
    ks = [1, 4, 11, 37]
    rows = [KS_TIES.index(k) for k in ks]
    for metric in (0, 1):
        t = tie_data[metric]
        g = knn.Group([0, 0, 0], mode)
        g.set_train(t["tr"], t["lab"], 3)
        labels, correct = g.classify_sweep(t["q"], ks, metric, truth=t["truth"])
        np.testing.assert_array_equal(labels, t["want"][rows])
        np.testing.assert_array_equal(correct, (t["want"][rows] == t["truth"]).sum(axis=1))
        if mode == 1:
            assert g.last_tie_count() > 0
        g.close()


def test_driver_k_list(knn, tmp_path, fmt_cout):
    spec = dict(kind="int", seed=21, N_train=900, N_test=60, N_val=90, dim=6, class_cnt=4)
    (tr, trl, te, _, va, val), _ = datagen.write_csvs(str(tmp_path), spec)
    cfg = knn.KnnConfig(dim=6, K=5, N_train=900, N_test=60, N_val=90, class_cnt=4,
                        train_file_name="train.csv", validation_file_name="validation.csv",
                        test_file_name="test.csv")
    ks = [1, 3, 9]
    out = knn.run_driver(cfg, str(tmp_path), extra=["--K_list", "1,3,9"])
    oracle.normalize(tr, te, va)
    accs = [oracle.acc(val, oracle.knn(tr, trl, va, k, True, 4)[0]) for k in ks]
    lines = out.splitlines()
    for i, k in enumerate(ks):
        assert lines[i] == "K = %d accuracy = %s" % (k, fmt_cout(accs[i]))
    best, sel = -1.0, None
    for k, a in zip(ks, accs):
        if a > best:
            best, sel = a, k
    assert lines[3] == "selected K = %d" % sel
    assert lines[4] == "accuracy = " + fmt_cout(best)
    assert lines[5].startswith("Running time is ")
    got = np.loadtxt(tmp_path / "Test_label.csv", dtype=np.int64, ndmin=1)
    np.testing.assert_array_equal(got, oracle.knn(tr, trl, te, sel, True, 4)[0])


def test_argument_errors(knn, tie_data):
    import ctypes
    t = tie_data[0]
    c = knn.Classifier(0)
    L = knn.lib()
    m = 4
    q = np.ascontiguousarray(t["q"][:m])
    out = np.empty((2, m), np.int32)
    corr = np.zeros(2, np.int64)
    truth = np.zeros(m, np.int32)

    def call(ks, truth_p=None, corr_p=None):
        a = np.asarray(ks, np.int32)
        return L.knn_classify_sweep(c.handle, q.ctypes.data, m, a.ctypes.data if len(a) else None,
                                    len(a), 0, out.ctypes.data, truth_p, corr_p, None, None, None)

    assert call([1, 2]) == -3  # KNN_ERR_STATE before set_train
    c.set_train(t["tr"], t["lab"], 3)
    assert call([]) == -1
    assert call([1, 3001]) == -1
    assert "ks[1]" in L.knn_last_error().decode()
    assert call([-1, 2]) == -1
    assert "ks[0]" in L.knn_last_error().decode()
    assert call([1, 2], truth_p=truth.ctypes.data) == -1
    assert call([1, 2], corr_p=corr.ctypes.data) == -1
    with pytest.raises(knn.KnnError):
        c.classify_sweep(q, [])
    assert call([1, 2], truth.ctypes.data, corr.ctypes.data) == 0
    c.close()

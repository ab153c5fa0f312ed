"""Per-class evaluation on the GPU: the confusion matrix at every K of a sweep
(knn_confusion_device, knn_classify_sweep_eval*, knn_loo_sweep_eval*, the group
calls, the driver's --confusion) and the vote counts (knn_vote_counts_device,
Classifier.classify(return_counts=True)).

Expected values never come from the library: confusion matrices are numpy
(np.add.at, evalcases.confusion) over the CPU oracle's labels at each K, vote
counts np.bincount over the oracle's neighbour indices.  The regimes of the
confusion kernel are fixed by C alone (per-wave LDS copies up to 16
classes, one LDS histogram up to 96, global atomics beyond), so the C of a
case names its regime (evalcases.regime).
"""
import os

import numpy as np
import pytest

import datagen
import evalcases
import loo
import oracle

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
CONF_C = [1, 2, 10, evalcases.SMALL_C, evalcases.SMALL_C + 1, evalcases.LDS_C,
          evalcases.LDS_C + 1]


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


@pytest.fixture(scope="module")
def clf(knn):
    """A context without a train set: the building blocks need none."""
    c = knn.Classifier(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))


def _run_confusion(clf, labels, truth, C, calls=1):
    """knn_confusion_device over host arrays -> (conf [nk, C, C], unl [nk])."""
    import torch
    nk, m = labels.shape
    dL, dT = _dev(labels), _dev(truth)
    dC = torch.zeros((nk, C, C), dtype=torch.int64, device=dL.device)
    dU = torch.zeros(nk, dtype=torch.int64, device=dL.device)
    torch.cuda.synchronize()
    for _ in range(calls):
        clf.confusion_device(dL.data_ptr(), nk, m, dT.data_ptr(), C, dC.data_ptr(), dU.data_ptr())
    clf.sync()
    return dC.cpu().numpy(), dU.cpu().numpy()


def test_regimes_are_covered(knn):
    assert (knn.CONF_SMALL_C, knn.CONF_LDS_C, knn.COUNTS_LDS_C) == (
        evalcases.SMALL_C, evalcases.LDS_C, evalcases.COUNTS_LDS_C)
    assert [evalcases.regime(C) for C in CONF_C] == [0, 0, 0, 0, 1, 1, 2]


@pytest.mark.parametrize("C", CONF_C)
def test_confusion_alone(clf, C):
    """Synthetic label arrays, no search: labels in [-1, C), truth in [0, C)
    with -1, C and 2^31 - 1 mixed in."""
    rng = np.random.default_rng(900 + C)
    shapes = [(m, nk) for m in (1, 63, 65, 1031) for nk in (1, 7)] + [(65, 4096)]
    for m, nk in shapes:
        labels = rng.integers(-1, C, (nk, m)).astype(np.int32)
        truth = rng.integers(0, C, m).astype(np.int32)
        bad = rng.random(m) < 0.2
        truth[bad] = rng.choice(np.array([-1, C, INT32_MAX], np.int32), int(bad.sum()))
        if m == 1031:  # every special value is present
            truth[:3] = [-1, C, INT32_MAX]
            labels[:, 5] = -1
        want, wunl = evalcases.confusion(labels, truth, C)
        conf, unl = _run_confusion(clf, labels, truth, C)
        np.testing.assert_array_equal(conf, want, err_msg="C=%d m=%d nk=%d" % (C, m, nk))
        np.testing.assert_array_equal(unl, wunl, err_msg="C=%d m=%d nk=%d" % (C, m, nk))
        np.testing.assert_array_equal(conf.sum(axis=(1, 2)) + unl, np.full(nk, m))


def test_confusion_without_unl(clf):
    import torch
    labels = np.array([[0, 1, -1, 1]], np.int32)
    truth = np.array([0, 0, 1, 7], np.int32)
    dL, dT = _dev(labels), _dev(truth)
    dC = torch.zeros((1, 2, 2), dtype=torch.int64, device=dL.device)
    torch.cuda.synchronize()
    clf.confusion_device(dL.data_ptr(), 1, 4, dT.data_ptr(), 2, dC.data_ptr(), None)
    clf.sync()
    np.testing.assert_array_equal(dC.cpu().numpy(), [[[1, 1], [0, 0]]])


@pytest.mark.parametrize("C", [10, evalcases.SMALL_C + 1, evalcases.LDS_C + 1])
def test_confusion_max_contention(clf, C):
    """Every query on one (t, p): the bin equals m, so a lost update shows; a
    second call into the same buffers gives the sum."""
    m, t, p = 20000, C - 1, C - 2
    labels = np.full((2, m), p, np.int32)
    labels[1, 7] = -1
    truth = np.full(m, t, np.int32)
    for calls in (1, 2):
        conf, unl = _run_confusion(clf, labels, truth, C, calls=calls)
        want = np.zeros((2, C, C), np.int64)
        want[0, t, p], want[1, t, p] = calls * m, calls * (m - 1)
        np.testing.assert_array_equal(conf, want)
        np.testing.assert_array_equal(unl, [0, calls])


# ------------------------------------------------------------ sweep eval
def _check_eval(labels, correct, conf, unl, want, truth, C):
    m = truth.shape[0]
    wconf, wunl = evalcases.confusion(want, truth, C)
    np.testing.assert_array_equal(labels, want)
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    assert conf.dtype == np.int64 and unl.dtype == np.int64
    np.testing.assert_array_equal(np.trace(conf, axis1=1, axis2=2), correct)
    np.testing.assert_array_equal(conf.sum(axis=(1, 2)) + unl, np.full(len(want), m))


def _eval_device(knn, c, q, ks, metric, truth, with_labels):
    """classify_sweep_eval_device through torch tensors -> (correct, conf, unl)."""
    import torch
    nk, m, C = len(ks), q.shape[0], c.class_cnt
    dQ, dT = _dev(q), _dev(truth)
    dL = torch.empty((nk, m), dtype=torch.int32, device=dQ.device) if with_labels else None
    dC = torch.full((nk,), -7, dtype=torch.int64, device=dQ.device)
    dF = torch.full((nk, C, C), -7, dtype=torch.int64, device=dQ.device)  # the call zeroes them
    dU = torch.full((nk,), -7, dtype=torch.int64, device=dQ.device)
    torch.cuda.synchronize()
    c.classify_sweep_eval_device(dQ.data_ptr(), m, ks, metric, dT.data_ptr(),
                                 d_labels=None if dL is None else dL.data_ptr(),
                                 d_correct=dC.data_ptr(), d_conf=dF.data_ptr(),
                                 d_unl=dU.data_ptr())
    c.sync()
    return dC.cpu().numpy(), dF.cpu().numpy(), dU.cpu().numpy()


@pytest.mark.parametrize("metric", [0, 1])
def test_sweep_eval_ties(knn, metric):
    """The tie-heavy set: 3 classes, ks with duplicates and a 0."""
    t = evalcases.tie_data(metric)
    c = knn.Classifier(0)
    c.set_train(t["tr"], t["lab"], 3)
    labels, correct, conf, unl = c.classify_sweep(t["q"], t["ks"], metric, truth=t["truth"],
                                                  confusion=True)
    _check_eval(labels, correct, conf, unl, t["want"], t["truth"], 3)
    assert unl[t["ks"].index(0)] == t["q"].shape[0]  # K = 0: no query has a label
    # without a label array: the same counts
    for with_labels in (True, False):
        correct2, conf2, unl2 = _eval_device(knn, c, t["q"], t["ks"], metric, t["truth"],
                                             with_labels)
        np.testing.assert_array_equal(correct2, correct)
        np.testing.assert_array_equal(conf2, conf)
        np.testing.assert_array_equal(unl2, unl)
    # a NaN query is unlabelled at every K; a truth out of range too
    q = t["q"].copy()
    q[33, 2] = np.nan
    truth = t["truth"].copy()
    truth[5] = 3
    want = t["want"].copy()
    want[:, 33] = -1
    labels, correct, conf, unl = c.classify_sweep(q, t["ks"], metric, truth=truth, confusion=True)
    wconf, wunl = evalcases.confusion(want, truth, 3)
    np.testing.assert_array_equal(labels, want)
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    assert (wunl >= 2).all()
    np.testing.assert_array_equal(conf.sum(axis=(1, 2)) + unl, np.full(len(want), 150))
    c.close()


@pytest.mark.parametrize("metric,paths", [(0, (5, 6)), (1, (7,))])
def test_sweep_eval_int8_codes(knn, metric, paths):
    """10 classes of byte codes, 4096 queries: the sweep rides the int8
    candidate passes and conf equals numpy over the oracle's labels."""
    d = evalcases.codes_data()
    c = knn.Classifier(0)
    c.set_train(d["tr"], d["lab"], d["classes"])
    labels, correct, conf, unl = c.classify_sweep(d["q"], d["ks"], metric, truth=d["truth"],
                                                  confusion=True)
    assert c.last_candidate_path() in paths
    _check_eval(labels, correct, conf, unl, d["want%d" % metric], d["truth"], d["classes"])
    assert (unl == 0).all()
    correct2, conf2, unl2 = _eval_device(knn, c, d["q"], d["ks"], metric, d["truth"], False)
    np.testing.assert_array_equal(conf2, conf)
    np.testing.assert_array_equal(correct2, correct)
    c.close()


# ------------------------------------------------------------ exclusion / leave-one-out
@pytest.mark.parametrize("name", ["A", "A1", "B"])
def test_loo_eval(knn, name):
    """tests/loo.py's sets: conf equals numpy over the labels of the existing
    loo_sweep (pinned to the oracle by test_gpu_loo.py) -- and, on set B, over
    the oracle's own leave-one-out labels."""
    s = loo.SETS[name]
    tr, lab = loo.data(name)
    C = s["classes"]
    c = knn.Classifier(0)
    c.set_train(tr, lab, C)
    plain, pcorrect = c.loo_sweep(s["ks"], s["metric"])
    labels, correct, conf, unl = c.loo_sweep(s["ks"], s["metric"], confusion=True)
    wconf, wunl = evalcases.confusion(plain, lab, C)
    np.testing.assert_array_equal(labels, plain)
    np.testing.assert_array_equal(correct, pcorrect)
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    np.testing.assert_array_equal(np.trace(conf, axis1=1, axis2=2), correct)
    if name == "B":
        w = loo.expected_loo(name)
        oconf, ounl = evalcases.confusion(w["labels"], lab, C)
        np.testing.assert_array_equal(conf, oconf)
        np.testing.assert_array_equal(unl, ounl)
    correct3, conf3, unl3 = c.loo_sweep(s["ks"], s["metric"], confusion=True, labels=False)
    np.testing.assert_array_equal(correct3, correct)
    np.testing.assert_array_equal(conf3, conf)
    np.testing.assert_array_equal(unl3, unl)
    # the sweep under exclusion through the same call: rows 10..49 exclude themselves
    rows = np.arange(10, 50)
    l4, c4, f4, u4 = c.classify_sweep(tr[rows], s["ks"], s["metric"], truth=lab[rows],
                                      exclude=rows, confusion=True)
    np.testing.assert_array_equal(l4, plain[:, rows])
    w4, wu4 = evalcases.confusion(plain[:, rows], lab[rows], C)
    np.testing.assert_array_equal(f4, w4)
    np.testing.assert_array_equal(u4, wu4)
    np.testing.assert_array_equal(c4, (plain[:, rows] == lab[rows]).sum(axis=1))
    c.close()


def test_loo_eval_batch_boundary(knn):
    """n = 16384 + 37: conf is summed over the two batches on the device."""
    tr, lab, C = evalcases.loo_big()
    ks = [1, 4]
    c = knn.Classifier(0)
    c.set_train(tr, lab, C)
    plain, pcorrect = c.loo_sweep(ks, knn.L2)
    wconf, wunl = evalcases.confusion(plain, lab, C)
    labels, correct, conf, unl = c.loo_sweep(ks, knn.L2, confusion=True)
    np.testing.assert_array_equal(labels, plain)
    np.testing.assert_array_equal(correct, pcorrect)
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    assert conf.sum() == 2 * (16384 + 37)
    correct3, conf3, unl3 = c.loo_sweep(ks, knn.L2, confusion=True, labels=False)
    np.testing.assert_array_equal(correct3, correct)
    np.testing.assert_array_equal(conf3, conf)
    np.testing.assert_array_equal(unl3, unl)
    c.close()


# ------------------------------------------------------------ vote counts
@pytest.mark.parametrize("C", [3, evalcases.COUNTS_LDS_C + 1])
def test_vote_counts(knn, C):
    """"ties" = 2: the reported rows are the reference's top k, so the counts
    equal the bincount over the oracle's idx; under the default ties they are
    the bincount of the rows the call returns."""
    t = evalcases.tie_data(0)
    lab = t["lab"] if C == 3 else (t["lab"] + (C - 3)).astype(np.int32)  # the top 3 of C labels
    kmax = 37
    q = t["q"][:66]
    c = knn.Classifier(0)
    c.set_train(t["tr"], lab, C)
    for k in (0, 1, 7, kmax):
        got1 = c.classify(q, k, knn.L2, return_neighbors=True, return_counts=True)
        assert got1[4].shape == (66, C) and got1[4].dtype == np.int32
        np.testing.assert_array_equal(got1[4], evalcases.vote_counts(lab, got1[1], k, C))
        np.testing.assert_array_equal(got1[4].sum(axis=1), np.full(66, k))
    c.set_tuning("ties", 2)
    for k in (0, 1, 7, kmax):
        labels, counts = c.classify(q, k, knn.L2, return_counts=True)
        if k == 0:
            assert not counts.any()
            continue
        wlab, widx, _ = oracle.knn(t["tr"], lab, q, k, True, C, n_out=k)
        np.testing.assert_array_equal(labels, wlab)
        np.testing.assert_array_equal(counts, evalcases.vote_counts(lab, widx, k, C))
    c.close()


@pytest.mark.parametrize("C", [5, evalcases.COUNTS_LDS_C + 1])
def test_vote_counts_device_alone(clf, C):
    """Hand-made rows with -1 slots, idx_base = 1000, a row without
    neighbours, more rows than one workgroup's waves."""
    import torch
    rng = np.random.default_rng(40 + C)
    m, kmax, n, base = 70, 130, 500, 1000
    lab = rng.integers(0, C, n).astype(np.int32)
    idx = rng.integers(0, n, (m, kmax)).astype(np.int64)
    idx[rng.random((m, kmax)) < 0.15] = -1
    idx[3] = -1  # no neighbours at all
    idx[4, 0] = -1
    dI, dL = _dev(np.where(idx >= 0, idx + base, -1)), _dev(lab)
    for k in (0, 1, 64, 65, kmax):
        dC = torch.full((m, C), -7, dtype=torch.int32, device=dI.device)
        torch.cuda.synchronize()
        clf.vote_counts_device(dI.data_ptr(), m, kmax, dL.data_ptr(), k, C, dC.data_ptr(),
                               idx_base=base)
        clf.sync()
        got = dC.cpu().numpy()
        np.testing.assert_array_equal(got, evalcases.vote_counts(lab, idx, k, C), err_msg="k=%d" % k)
        np.testing.assert_array_equal(got.sum(axis=1), (idx[:, :k] >= 0).sum(axis=1))
        assert not got[3].any()


# ------------------------------------------------------------ groups
@pytest.mark.parametrize("mode", [0, 1])
def test_group_sweep_eval(knn, mode):
    """Three ranks on one GPU (ragged thirds of 150 queries; mode 1: three
    train shards) equal the oracle's matrices, i.e. the single context's."""
    for metric in (0, 1):
        t = evalcases.tie_data(metric)
        g = knn.Group([0, 0, 0], mode)
        g.set_train(t["tr"], t["lab"], 3)
        labels, correct, conf, unl = g.classify_sweep(t["q"], t["ks"], metric, truth=t["truth"],
                                                      confusion=True)
        _check_eval(labels, correct, conf, unl, t["want"], t["truth"], 3)
        g.close()


def test_group_loo_eval(knn):
    s = loo.SETS["B"]
    tr, lab = loo.data("B")
    w = loo.expected_loo("B")
    wconf, wunl = evalcases.confusion(w["labels"], lab, s["classes"])
    g = knn.Group([0, 0, 0], mode=0)
    g.set_train(tr, lab, s["classes"])
    labels, correct, conf, unl = g.loo_sweep(s["ks"], s["metric"], confusion=True)
    np.testing.assert_array_equal(labels, w["labels"])
    np.testing.assert_array_equal(correct, w["correct"])
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    correct2, conf2, unl2 = g.loo_sweep(s["ks"], s["metric"], confusion=True, labels=False)
    np.testing.assert_array_equal(conf2, wconf)
    np.testing.assert_array_equal(correct2, w["correct"])
    g.close()
    g = knn.Group([0, 0, 0], mode=1)
    g.set_train(tr, lab, s["classes"])
    with pytest.raises(knn.KnnError, match=r"knn error -1: .*train-sharded"):
        g.loo_sweep(s["ks"], s["metric"], confusion=True)
    g.close()


# ------------------------------------------------------------ driver
def _matrix(lines, at, C):
    return np.array([[int(v) for v in lines[at + 1 + t].split(" ")] for t in range(C)], np.int64)


def test_driver_confusion(knn, tmp_path, fmt_cout):
    """The spec of test_driver_k_list: with --confusion the matrix of the
    selected K follows the validation lines; without it stdout keeps the
    format test_driver_k_list expects."""
    spec = dict(kind="int", seed=21, N_train=900, N_test=60, N_val=90, dim=6, class_cnt=4)
    (tr, trl, te, _, va, val), _ = datagen.write_csvs(str(tmp_path), spec)
    cfg = knn.KnnConfig(dim=6, K=5, N_train=900, N_test=60, N_val=90, class_cnt=4,
                        train_file_name="train.csv", validation_file_name="validation.csv",
                        test_file_name="test.csv")
    ks = [1, 3, 9]
    out = knn.run_driver(cfg, str(tmp_path), extra=["--K_list", "1,3,9", "--confusion"])
    plain = knn.run_driver(cfg, str(tmp_path), extra=["--K_list", "1,3,9"])
    oracle.normalize(tr, te, va)
    want = evalcases.oracle_labels(tr, trl, va, ks, True, 4)
    accs = [oracle.acc(val, want[i]) for i in range(3)]
    best, sel = -1.0, None
    for i, a in enumerate(accs):
        if a > best:
            best, sel = a, i
    head = ["K = %d accuracy = %s" % (k, fmt_cout(a)) for k, a in zip(ks, accs)]
    head += ["selected K = %d" % ks[sel], "accuracy = " + fmt_cout(best)]
    lines = out.splitlines()
    assert lines[:5] == head
    assert lines[5] == "confusion K = %d" % ks[sel]
    wconf, wunl = evalcases.confusion(want[sel:sel + 1], val, 4)
    np.testing.assert_array_equal(_matrix(lines, 5, 4), wconf[0])
    assert lines[10] == "unlabelled = %d" % wunl[0]
    assert lines[11].startswith("Running time is ") and len(lines) == 12
    # without the flag: exactly the lines of test_driver_k_list
    plines = plain.splitlines()
    assert plines[:5] == head
    assert plines[5].startswith("Running time is ") and len(plines) == 6


def test_driver_confusion_loo(knn, tmp_path, fmt_cout):
    spec = dict(kind="int", seed=23, N_train=600, N_test=40, N_val=10, dim=6, class_cnt=4)
    (tr, trl, te, _, _, _), _ = datagen.write_csvs(str(tmp_path), spec)
    cfg = knn.KnnConfig(dim=6, K=7, N_train=600, N_test=40, N_val=10, class_cnt=4,
                        train_file_name="train.csv", validation_file_name="validation.csv",
                        test_file_name="test.csv")
    ks = [1, 3, 5]
    out = knn.run_driver(cfg, str(tmp_path), extra=["--loo", "--K_list", "1,3,5", "--confusion"])
    oracle.normalize(tr, te, None)
    want = loo.expected_excl(tr, trl, tr, np.arange(600), ks, True, 4)["labels"]
    accs = [float((want[j] == trl).sum()) / 600 for j in range(3)]
    best, sel = -1.0, None
    for i, a in enumerate(accs):
        if a > best:
            best, sel = a, i
    lines = out.splitlines()
    assert lines[:3] == ["K = %d loo accuracy = %s" % (k, fmt_cout(a)) for k, a in zip(ks, accs)]
    assert lines[3] == "selected K = %d" % ks[sel]
    assert lines[4] == "confusion K = %d" % ks[sel]
    wconf, wunl = evalcases.confusion(want[sel:sel + 1], trl, 4)
    np.testing.assert_array_equal(_matrix(lines, 4, 4), wconf[0])
    assert lines[9] == "unlabelled = %d" % wunl[0]
    assert lines[10].startswith("Running time is ") and len(lines) == 11


# ------------------------------------------------------------ argument errors
def test_argument_errors(knn):
    import torch
    t = evalcases.tie_data(0)
    L = knn.lib()
    c = knn.Classifier(0)
    m, C = 4, 3
    dQ, dT = _dev(t["q"][:m]), _dev(t["truth"][:m])
    dF = torch.zeros((2, C, C), dtype=torch.int64, device=dQ.device)
    dI = torch.zeros((m, 5), dtype=torch.int64, device=dQ.device)
    dL = torch.zeros(10, dtype=torch.int32, device=dQ.device)
    dN = torch.zeros((m, C), dtype=torch.int32, device=dQ.device)
    torch.cuda.synchronize()
    err = lambda: L.knn_last_error().decode()  # noqa: E731

    def sweep(ks, truth=dT.data_ptr()):
        a = np.asarray(ks, np.int32)
        return L.knn_classify_sweep_eval_device(c.handle, dQ.data_ptr(), m, None,
                                                a.ctypes.data if len(a) else None, len(a), 0,
                                                None, truth, None, dF.data_ptr(), None, None)

    def host(ks, truth):
        a = np.asarray(ks, np.int32)
        q = np.ascontiguousarray(t["q"][:m])
        conf = np.zeros((len(a), C, C), np.int64)
        return L.knn_classify_sweep_eval(c.handle, q.ctypes.data, m, a.ctypes.data, len(a), 0,
                                         None, truth, None, conf.ctypes.data, None)

    ks2 = np.asarray([1, 2], np.int32)
    assert sweep([1, 2]) == -3  # KNN_ERR_STATE before set_train
    assert L.knn_loo_sweep_eval_device(c.handle, 0, 1, ks2.ctypes.data, 2, 0, None, None,
                                       dF.data_ptr(), None, None) == -3
    assert L.knn_loo_sweep_eval(c.handle, ks2.ctypes.data, 2, 0, None, None, None, None) == -3
    assert host([1, 2], np.zeros(m, np.int32).ctypes.data) == -3
    c.set_train(t["tr"], t["lab"], C)
    assert sweep([1, 2], truth=None) == -1
    assert "d_truth" in err()
    assert host([1, 2], None) == -1
    assert "truth" in err()
    assert sweep([]) == -1
    assert "nk" in err()
    assert sweep([1] * 4097) == -1
    assert "nk = 4097" in err()
    assert sweep([1, 2001]) == -1
    assert "ks[1]" in err()
    assert L.knn_loo_sweep_eval(c.handle, np.asarray([2000], np.int32).ctypes.data, 1, 0, None,
                                None, None, None) == -1  # K <= n_train - 1
    assert "ks[0]" in err()
    # the building blocks
    conf = lambda nk, truth, out: L.knn_confusion_device(  # noqa: E731
        c.handle, dL.data_ptr(), nk, 5, truth, C, out, None, None)
    assert conf(0, dT.data_ptr(), dF.data_ptr()) == -1
    assert "nk" in err()
    assert conf(4097, dT.data_ptr(), dF.data_ptr()) == -1
    assert conf(2, None, dF.data_ptr()) == -1
    assert "d_truth" in err()
    assert conf(2, dT.data_ptr(), None) == -1
    assert "d_conf" in err()
    counts = lambda k, kmax: L.knn_vote_counts_device(  # noqa: E731
        c.handle, dI.data_ptr(), m, kmax, dL.data_ptr(), 0, k, C, dN.data_ptr(), None)
    assert counts(6, 5) == -1
    assert "k = 6 exceeds kmax = 5" in err()
    assert counts(-1, 5) == -1
    assert counts(5, 5) == 0
    assert sweep([1, 2]) == 0
    c.sync()
    with pytest.raises(ValueError):
        c.classify_sweep(t["q"][:m], [1], confusion=True)  # no truth
    c.close()

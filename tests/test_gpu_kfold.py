"""F-fold cross-validated K sweep on the GPU (knn_set_folds, knn_kfold_sweep*,
knn_group_kfold_sweep) against the CPU oracle run on the FOLD-REMOVED train
sets (tests/kfold.py -> tests/lgo.py): for train row r the result is the K
sweep's on the train set without the rows of r's fold, indices mapped back.
Everything is compared exactly: the label at every K, idx and its order, dist
bit for bit, the four tie bits, at "ties" = 1, 2 and 0.
"""
import os

import numpy as np
import pytest

import kfold
import loo
import wvote

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


def _trained(knn, name, folds=True, precision=None, **tuning):
    s = kfold.case(name)
    c = knn.Classifier(0)
    if precision is not None:
        c.set_precision(precision)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    c.set_train(s["tr"], s["lab"], s["classes"])
    if folds:
        c.set_folds(s["folds"], s["F"])
    return c, s


def _check(got, w, ties):
    """(labels, correct, idx, dist, flags) against kfold.expected at "ties"."""
    labels, correct, idx, dist, flags = got
    nv = w["naive"]
    if ties == 0:
        wl, wi, wf = nv["labels"], nv["idx"], nv["flags"]
    elif ties == 1:
        wl, wi, wf = w["labels"], w["idx1"], w["flags1"]
    else:
        wl = w["labels"]
        wi = np.where(nv["tied"][:, None], w["idx"], nv["idx"])
        wf = nv["flags"] | np.where(nv["tied"], 32, 0)
    np.testing.assert_array_equal(labels, wl)
    np.testing.assert_array_equal(idx, wi)
    np.testing.assert_array_equal(_bits(dist), _bits(w["dist"]))
    np.testing.assert_array_equal(flags & loo.FLAG_MASK, wf)
    return wl


# ------------------------------------------------ 1. the cases, every row
@pytest.mark.parametrize("name", kfold.CASES)
def test_cases(knn, name):
    """Interleaved folds under both metrics, contiguous unequal folds, two
    folds, folds smaller than kmax + 1 (padded partial lists) and exact
    duplicates in the other fold, each at "ties" = 1, 2 and 0."""
    w = kfold.expected(name)
    c, s = _trained(knn, name)
    assert c.fold_max() == s["fold_max"]
    for ties in (1, 2, 0):
        c.set_tuning("ties", ties)
        got = c.kfold_sweep(s["ks"], s["metric"], return_neighbors=True)
        assert got[0].shape == (len(s["ks"]), s["n"]) and got[1].dtype == np.int64
        wl = _check(got, w, ties)
        np.testing.assert_array_equal(got[1], (wl == s["lab"]).sum(axis=1))
    c.close()


def test_duplicates_in_the_other_fold_stay(knn):
    c, s = _trained(knn, "dups")
    _, _, idx, dist, _ = c.kfold_sweep(s["ks"], s["metric"], return_neighbors=True)
    assert (dist[:, 0] == 0.0).all()
    assert (s["folds"][idx] != s["folds"][:, None]).all(), "a row of the query's own fold voted"
    c.close()


# ------------------------------------------------ 2. the bound on ks
def test_bound_on_ks(knn):
    c, s = _trained(knn, "small")
    top = s["n"] - s["fold_max"]  # the rows the largest fold's queries have left
    w = kfold.lgo.expected(s["tr"], s["lab"], s["folds"], s["tr"], s["folds"], [top, 2],
                           True, s["classes"], s["fold_max"])
    got = c.kfold_sweep([top, 2], s["metric"], return_neighbors=True)
    _check(got, w, 1)
    with pytest.raises(knn.KnnError, match=r"knn error -1: ks\[1\] = %d" % (top + 1)):
        c.kfold_sweep([1, top + 1], s["metric"])
    labels, correct = c.kfold_sweep([0, 0], s["metric"])
    assert (labels == -1).all() and (correct == 0).all()
    c.close()


def test_argument_errors(knn):
    c, s = _trained(knn, "small", folds=False)
    with pytest.raises(knn.KnnError, match="knn error -3"):
        c.kfold_sweep([1])
    bad = s["folds"].copy()
    bad[17] = 4
    with pytest.raises(knn.KnnError, match="knn error -1: fold id out of .* at row 17"):
        c.set_folds(bad, 4)
    assert c.fold_max() == 0
    with pytest.raises(knn.KnnError, match="knn error -1: fold 4 is empty"):
        c.set_folds(s["folds"], 5)
    for F in (1, 65):
        with pytest.raises(knn.KnnError, match="knn error -1: n_folds"):
            c.set_folds(np.zeros(s["n"], np.int32), F)
    c.set_folds(s["folds"], 4)
    assert c.fold_max() == 12
    c.set_folds(None)
    assert c.fold_max() == 0
    fresh = knn.Classifier(0)
    with pytest.raises(knn.KnnError, match="knn error -3"):
        fresh.set_folds(s["folds"], 4)
    fresh.close()
    c.close()


# ------------------------------------------------ 3. against lgo_sweep
@pytest.mark.parametrize("ties", [1, 2])
def test_equals_lgo_sweep(knn, ties):
    """groups = folds on the unequal case (kmax + gmax = 223 <= 1000): both
    routes give the same labels, counts, rows and tie bits; with folds AND
    groups set, each call keeps its own."""
    c, s = _trained(knn, "unequal", ties=ties)
    c.set_groups(s["folds"], s["F"])
    a = c.kfold_sweep(s["ks"], s["metric"], return_neighbors=True, confusion=True)
    b = c.lgo_sweep(s["ks"], s["metric"], return_neighbors=True, confusion=True)
    for x, y in zip(a[:5], b[:5]):  # labels, correct, conf, unl, idx
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(_bits(a[5]), _bits(b[5]))
    np.testing.assert_array_equal(a[6] & loo.FLAG_MASK, b[6] & loo.FLAG_MASK)
    c.close()


# ------------------------------------------------ 4. tuning reaches the shards
@pytest.mark.parametrize("what, path", [("auto", None), ("fp32", 0), ("fp16", 4), ("i8l1", 7)])
def test_candidate_paths(knn, what, path):
    """The parent's precision and tuning keys select the shards' candidate
    pass: knn_last_candidate_path reports the last shard search.  AUTO is
    compared with what a plain classify of the same batch size selects."""
    name = "inter_l1" if what == "i8l1" else "inter_l2"
    prec = {"fp32": knn.PRECISION_FP32, "fp16": knn.PRECISION_FP16}.get(what)
    tuning = {"i8l1": 1} if what == "i8l1" else {}
    c, s = _trained(knn, name, precision=prec, **tuning)
    if path is None:
        c.classify(s["tr"][:150], 21, s["metric"])
        path = c.last_candidate_path()
    got = c.kfold_sweep(s["ks"], s["metric"], return_neighbors=True)
    assert c.last_candidate_path() == path
    _check(got, kfold.expected(name), 1)
    c.close()


# ------------------------------------------------ 5. weighted votes
def test_weighted_votes(knn):
    c, s = _trained(knn, "inter_l2")
    c.set_vote(knn.VOTE_DISTANCE)
    labels, correct, idx, dist, flags = c.kfold_sweep(s["ks"], s["metric"], return_neighbors=True)
    w = kfold.expected("inter_l2")
    np.testing.assert_array_equal(idx, w["idx1"])  # the rows are the uniform call's
    want = wvote.labels(wvote.lab_rows(s["lab"], idx), dist, s["ks"])
    np.testing.assert_array_equal(labels, want)
    np.testing.assert_array_equal(correct, (want == s["lab"]).sum(axis=1))
    assert (want != w["labels"]).any(), "the weights decide somewhere"
    c.close()


# ------------------------------------------------ 6. evaluation
def test_evaluation(knn):
    c, s = _trained(knn, "unequal")
    w = kfold.expected("unequal")
    correct, conf, unl = c.kfold_sweep(s["ks"] + [0], s["metric"], confusion=True, labels=False)
    wl = np.concatenate([w["labels"], np.full((1, s["n"]), -1, np.int32)])
    wconf, wunl = kfold.confusion(wl, s["lab"], s["classes"])
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    np.testing.assert_array_equal(conf.sum(axis=(1, 2)) + unl, np.full(len(wl), s["n"]))
    np.testing.assert_array_equal(np.trace(conf, axis1=1, axis2=2), correct)
    assert unl[-1] == s["n"]
    c.close()


# ------------------------------------------------ 7. the group
def test_group_loopback(knn):
    s = kfold.case("unequal")
    w = kfold.expected("unequal")
    g = knn.Group([0, 0, 0], mode=0)
    g.set_train(s["tr"], s["lab"], s["classes"])
    g.set_folds(s["folds"], s["F"])
    labels, correct, conf, unl = g.kfold_sweep(s["ks"], s["metric"], confusion=True)
    np.testing.assert_array_equal(labels, w["labels"])
    np.testing.assert_array_equal(correct, w["correct"])
    wconf, wunl = kfold.confusion(w["labels"], s["lab"], s["classes"])
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    g.close()
    g1 = knn.Group([0, 0], mode=1)
    g1.set_train(s["tr"], s["lab"], s["classes"])
    with pytest.raises(knn.KnnError, match="not served in the train-sharded mode"):
        g1.set_folds(s["folds"], s["F"])
    with pytest.raises(knn.KnnError, match="not served in the train-sharded mode"):
        g1.kfold_sweep(s["ks"], s["metric"])
    g1.close()


# ------------------------------------------------ 8. set_train drops the folds
def test_set_train_clears_the_folds(knn):
    c, s = _trained(knn, "two")
    c.kfold_sweep(s["ks"], s["metric"])
    other = kfold.case("unequal")
    c.set_train(other["tr"], other["lab"], other["classes"])
    assert c.fold_max() == 0
    with pytest.raises(knn.KnnError, match="knn error -3"):
        c.kfold_sweep(s["ks"], s["metric"])
    fresh = knn.Classifier(0)
    fresh.set_train(other["tr"], other["lab"], other["classes"])
    Q = other["tr"][:64] + 0.25
    a = c.classify(Q, 7, return_neighbors=True)
    b = fresh.classify(Q, 7, return_neighbors=True)
    for x, y in zip(a[:2], b[:2]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]))
    np.testing.assert_array_equal(a[3] & loo.FLAG_MASK, b[3] & loo.FLAG_MASK)
    fresh.close()
    c.close()


# ------------------------------------------------ 9. the per-fold device call
def _fold_device(c, fold, rows, ks, metric, stream=None):
    import torch
    dev = torch.device("cuda", 0)
    nk, kmax = len(ks), max(ks)
    L = torch.full((nk, rows), -7, dtype=torch.int32, device=dev)
    C = torch.full((nk,), -7, dtype=torch.int64, device=dev)
    I = torch.full((rows, kmax), -7, dtype=torch.int64, device=dev)
    D = torch.zeros((rows, kmax), dtype=torch.float64, device=dev)
    F = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    c.kfold_sweep_device(fold, ks, metric, L.data_ptr(), C.data_ptr(), I.data_ptr(), D.data_ptr(),
                         F.data_ptr(), stream=stream)
    return L, C, I, D, F


def test_fold_device_call(knn):
    """One fold into device buffers: its rows in ascending original order."""
    c, s = _trained(knn, "inter_l2")
    w = kfold.expected("inter_l2")
    rows = np.flatnonzero(s["folds"] == 2)
    got = _fold_device(c, 2, len(rows), s["ks"], s["metric"])
    c.sync()
    L, C, I, D, F = (t.cpu().numpy() for t in got)
    np.testing.assert_array_equal(L, w["labels"][:, rows])
    np.testing.assert_array_equal(C, (w["labels"][:, rows] == s["lab"][rows]).sum(axis=1))
    np.testing.assert_array_equal(I, w["idx1"][rows])
    np.testing.assert_array_equal(_bits(D), _bits(w["dist"][rows]))
    np.testing.assert_array_equal(F & loo.FLAG_MASK, w["flags1"][rows])
    with pytest.raises(knn.KnnError, match="knn error -1: fold = 4"):
        c.kfold_sweep_device(4, s["ks"], s["metric"], got[0].data_ptr())
    c.close()


def test_fold_sweep_held(knn):
    """The per-fold device call on a held caller stream (the protocol of
    test_gpu_streams.py): the shard searches, the index maps, the merge, the
    tie scan, the reference-order pass and the votes all run on S -- sentinel
    outputs that a copy on S reads hold the results, the call does not wait."""
    import torch
    import streams as st
    from test_gpu_streams import finish, held_run
    dev = torch.device("cuda", 0)
    c, s = _trained(knn, "inter_l2", ties=2)
    w = kfold.expected("inter_l2")
    nv = w["naive"]
    rows = np.flatnonzero(s["folds"] == 1)
    m, ks = len(rows), s["ks"]
    nk, kmax = len(ks), max(ks)
    b = st.Poisoned(dev)
    ol = b.out((nk, m), torch.int32)
    oc = b.out((nk,), torch.int64)
    oi = b.out((m, kmax), torch.int64)
    od = b.out((m, kmax), torch.float64)
    of = b.out((m,), torch.int32)

    def call(stream):
        c.kfold_sweep_device(1, list(ks), s["metric"], ol.data_ptr(), oc.data_ptr(), oi.data_ptr(),
                             od.data_ptr(), of.data_ptr(), stream=stream)

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    np.testing.assert_array_equal(b.result(ol), w["labels"][:, rows])
    np.testing.assert_array_equal(b.result(oc), (w["labels"][:, rows] == s["lab"][rows]).sum(axis=1))
    np.testing.assert_array_equal(b.result(oi),
                                  np.where(nv["tied"][:, None], w["idx"], nv["idx"])[rows])
    np.testing.assert_array_equal(_bits(b.result(od)), _bits(w["dist"][rows]))
    finish(dev, [c])

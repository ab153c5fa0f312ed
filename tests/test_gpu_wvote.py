"""Distance-weighted voting on the GPU (KNN_VOTE_DISTANCE): the building blocks
knn_vote_sweep_weighted_device / knn_vote_weights_device over synthetic rows,
and every classify call in distance mode -- classify, classify_sweep (exclusion
and confusion included), loo_sweep, the group calls and the driver's --weights.

Expected values never come from the library: labels and class sums are the
sequential fp64 oracle of tests/wvote.py over ordered neighbour rows, and are
compared with assert_array_equal (the float64 sums bit for bit).  The rows are
the ones the call itself reports and, under "ties" = 2, the CPU oracle's own.
"""
import os

import numpy as np
import pytest

import datagen
import evalcases
import loo
import oracle
import wvote

pytestmark = pytest.mark.gpu

KS = wvote.KS


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


# ------------------------------------------------------------ building blocks
def _ks_of(kmax, nk):
    if nk == 1:
        return [kmax]
    return [kmax, 0, 1, kmax // 2, kmax, min(kmax, 513), max(kmax - 1, 0)]


@pytest.mark.parametrize("kmax", [1, 64, 65, 1000, 1100])
def test_building_blocks(clf, kmax):
    """Synthetic rows, no search (wvote.synthetic_rows: -1 slots with +inf
    distances, a row starting with -1, z = 0 / 1 / kmax, equal class sums, an
    inf distance, all-zero weights); idx_base = 1000.  Rows beyond 512 entries
    cross the kernel's LDS chunk."""
    import torch
    base, n_lab = 1000, 300
    for m in (1, 63, 65, 1031):
        for C in ((3,) if m == 1031 else (3, 70)):
            rng = np.random.default_rng(31 * kmax + m + C)
            lab = rng.integers(0, C, n_lab).astype(np.int32)
            idx, dist = wvote.synthetic_rows(m, kmax, n_lab, C, seed=kmax * 7 + m)
            lrows = wvote.lab_rows(lab, idx)
            truth = rng.integers(0, C, m).astype(np.int32)
            dI, dD, dL, dT = _dev(np.where(idx >= 0, idx + base, -1)), _dev(dist), _dev(lab), _dev(truth)
            win = [wvote.prefix_winners(lrows[q], dist[q]) for q in range(m)]
            for nk in (1, 7):
                ks = _ks_of(kmax, nk)
                want = np.array([[win[q][K] for q in range(m)] for K in ks], np.int32)
                dO = torch.full((nk, m), -7, dtype=torch.int32, device=dI.device)
                dC = torch.full((nk,), -7, dtype=torch.int64, device=dI.device)
                torch.cuda.synchronize()
                clf.vote_sweep_weighted_device(dI.data_ptr(), dD.data_ptr(), m, kmax, dL.data_ptr(),
                                               ks, dO.data_ptr(), idx_base=base,
                                               d_truth=dT.data_ptr(), d_correct=dC.data_ptr())
                clf.sync()
                msg = "kmax=%d m=%d nk=%d" % (kmax, m, nk)
                np.testing.assert_array_equal(dO.cpu().numpy(), want, err_msg=msg)
                np.testing.assert_array_equal(dC.cpu().numpy(), (want == truth).sum(axis=1),
                                              err_msg=msg)
                # without truth: the same labels
                dO2 = torch.full((nk, m), -7, dtype=torch.int32, device=dI.device)
                torch.cuda.synchronize()
                clf.vote_sweep_weighted_device(dI.data_ptr(), dD.data_ptr(), m, kmax, dL.data_ptr(),
                                               ks, dO2.data_ptr(), idx_base=base)
                clf.sync()
                np.testing.assert_array_equal(dO2.cpu().numpy(), want, err_msg=msg)
            if m > 65 and kmax > 65:
                continue  # (the sums of the long rows are checked at m <= 65)
            for k in sorted(set([0, 1, kmax // 2, kmax])):
                dW = torch.full((m, C), -7.0, dtype=torch.float64, device=dI.device)
                torch.cuda.synchronize()
                clf.vote_weights_device(dI.data_ptr(), dD.data_ptr(), m, kmax, dL.data_ptr(), k, C,
                                        dW.data_ptr(), idx_base=base)
                clf.sync()
                got = dW.cpu().numpy()
                np.testing.assert_array_equal(got, wvote.sums(lrows, dist, k, C),
                                              err_msg="kmax=%d m=%d k=%d C=%d" % (kmax, m, k, C))
                if m > 3:
                    assert not got[3].any()  # the row without neighbours


def test_building_block_arguments(knn, clf):
    import torch
    L = knn.lib()
    dI = torch.zeros((4, 5), dtype=torch.int64, device="cuda:0")
    dD = torch.ones((4, 5), dtype=torch.float64, device="cuda:0")
    dL = torch.zeros(10, dtype=torch.int32, device="cuda:0")
    dO = torch.zeros((2, 4), dtype=torch.int32, device="cuda:0")
    dW = torch.zeros((4, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    err = lambda: L.knn_last_error().decode()  # noqa: E731

    def sweep(ks, dist=dD.data_ptr(), truth=None, correct=None, out=dO.data_ptr()):
        a = np.asarray(ks, np.int32)
        return L.knn_vote_sweep_weighted_device(clf.handle, dI.data_ptr(), dist, 4, 5, dL.data_ptr(),
                                                0, a.ctypes.data if len(a) else None, len(a), out,
                                                truth, correct, None)

    assert sweep([1, 6]) == -1 and "ks[1]" in err()
    assert sweep([]) == -1 and "nk" in err()
    assert sweep([1], dist=None) == -1 and "distances" in err()
    assert sweep([1], truth=dL.data_ptr()) == -1 and "go together" in err()
    assert sweep([1], out=None) == -1
    assert sweep([1, 5]) == 0
    sums = lambda k, kmax, C=3, out=dW.data_ptr(): L.knn_vote_weights_device(  # noqa: E731
        clf.handle, dI.data_ptr(), dD.data_ptr(), 4, kmax, dL.data_ptr(), 0, k, C, out, None)
    assert sums(6, 5) == -1 and "k = 6 exceeds kmax = 5" in err()
    assert sums(-1, 5) == -1
    assert sums(1, 5, C=0) == -1
    assert sums(1, 5, out=None) == -1 and "d_wsum" in err()
    assert sums(5, 5) == 0
    clf.sync()


# ------------------------------------------------------------ classify / sweep
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_classify_and_sweep(knn, name, metric):
    d = wvote.dataset(name, metric)
    e = wvote.expected(name, metric)
    tr, lab, q, C = d["tr"], d["lab"], d["q"], d["classes"]
    m = q.shape[0]
    truth = np.random.default_rng(5).integers(0, C, m).astype(np.int32)
    c = knn.Classifier(0)
    c.set_train(tr, lab, C)
    assert c.get_vote() == knn.VOTE_UNIFORM
    for ties in (1, 2):
        c.set_tuning("ties", ties)
        c.set_vote(knn.VOTE_UNIFORM)
        lu, cu, iu, du, fu = c.classify_sweep(q, KS, metric, truth=truth, return_neighbors=True)
        np.testing.assert_array_equal(lu, e["uniform"])
        c.set_vote(knn.VOTE_DISTANCE)
        assert c.get_vote() == knn.VOTE_DISTANCE
        lw, cw, iw, dw, fw = c.classify_sweep(q, KS, metric, truth=truth, return_neighbors=True)
        # the search, the tie passes and the rows are the uniform call's
        np.testing.assert_array_equal(iw, iu)
        np.testing.assert_array_equal(dw, du)
        np.testing.assert_array_equal(fw, fu)
        # the labels are the rule's over the rows the call reports
        np.testing.assert_array_equal(lw, wvote.labels(wvote.lab_rows(lab, iw), dw, KS))
        np.testing.assert_array_equal(cw, (lw == truth).sum(axis=1))
        assert (lw != lu).any()  # (fails without the feature)
        if ties == 2:  # the reference's own rows
            np.testing.assert_array_equal(iw, e["idx"])
            np.testing.assert_array_equal(dw, e["dist"])
            np.testing.assert_array_equal(lw, e["weighted"])
        # plain classify at single K, with the class sums
        for k in (0, 1, 5, 37):
            c.set_vote(knn.VOTE_UNIFORM)
            l0, i0, d0, f0 = c.classify(q, k, metric, return_neighbors=True)
            c.set_vote(knn.VOTE_DISTANCE)
            l1, i1, d1, f1, w1 = c.classify(q, k, metric, return_neighbors=True,
                                            return_weights=True)
            np.testing.assert_array_equal(i1, i0)
            np.testing.assert_array_equal(d1, d0)
            np.testing.assert_array_equal(f1, f0)
            lr = wvote.lab_rows(lab, i1)
            if k == 0:
                assert (l1 == -1).all() and not w1.any()
                continue
            np.testing.assert_array_equal(l1, wvote.labels(lr, d1, [k])[0])
            np.testing.assert_array_equal(w1, wvote.sums(lr, d1, k, C))
            assert w1.dtype == np.float64 and w1.shape == (m, C)
            if ties == 2:
                np.testing.assert_array_equal(l1, wvote.labels(e["lrows"], e["dist"], [k])[0])
            np.testing.assert_array_equal(c.classify(q, k, metric), l1)  # without caller rows
        # the confusion matrices follow from the weighted labels
        l2, c2, conf, unl = c.classify_sweep(q, KS, metric, truth=truth, confusion=True)
        wconf, wunl = evalcases.confusion(lw, truth, C)
        np.testing.assert_array_equal(l2, lw)
        np.testing.assert_array_equal(c2, cw)
        np.testing.assert_array_equal(conf, wconf)
        np.testing.assert_array_equal(unl, wunl)
        np.testing.assert_array_equal(np.trace(conf, axis1=1, axis2=2), c2)
        # back to uniform: the uniform labels again
        c.set_vote(knn.VOTE_UNIFORM)
        np.testing.assert_array_equal(c.classify_sweep(q, KS, metric), lu)
    c.close()


def test_set_vote_refuses_other_values(knn):
    c = knn.Classifier(0)
    c.set_vote(knn.VOTE_DISTANCE)
    for bad in (7, -1, 2):
        with pytest.raises(knn.KnnError, match="knn error -1: .*vote mode"):
            c.set_vote(bad)
        assert c.get_vote() == knn.VOTE_DISTANCE
    c.close()
    g = knn.Group([0, 0], 0)
    with pytest.raises(knn.KnnError, match="knn error -1: .*vote mode"):
        g.set_vote(7)
    g.close()


def test_nonfinite_query(knn):
    d = wvote.dataset("c", 0)
    q = d["q"][:70].copy()
    q[33, 2] = np.nan
    q[64, 0] = np.inf
    c = knn.Classifier(0)
    c.set_train(d["tr"], d["lab"], d["classes"])
    c.set_vote(knn.VOTE_DISTANCE)
    lw, iw, dw, fw = c.classify_sweep(q, KS, knn.L2, return_neighbors=True)
    for bad in (33, 64):
        assert (lw[:, bad] == -1).all() and fw[bad] & knn.FLAG_NONFINITE
        assert (iw[bad] == -1).all()
    ok = np.ones(70, bool)
    ok[[33, 64]] = False
    want = wvote.labels(wvote.lab_rows(d["lab"], iw[ok]), dw[ok], KS)
    np.testing.assert_array_equal(lw[:, ok], want)
    l1, i1, d1, f1, w1 = c.classify(q, 5, knn.L2, return_neighbors=True, return_weights=True)
    assert l1[33] == -1 and l1[64] == -1 and f1[33] & knn.FLAG_NONFINITE
    assert not w1[33].any() and not w1[64].any()
    np.testing.assert_array_equal(l1[ok], want[0])
    c.close()


def test_candidate_path_independence(knn):
    """The labels are a function of the exact rows: the same under the fp32
    candidate pass and under AUTO's."""
    d = wvote.dataset("c", 0)
    got = []
    for prec in (knn.PRECISION_FP32, knn.PRECISION_AUTO):
        c = knn.Classifier(0)
        c.set_precision(prec)
        c.set_train(d["tr"], d["lab"], d["classes"])
        c.set_vote(knn.VOTE_DISTANCE)
        got.append(c.classify_sweep(d["q"], KS, knn.L2))
        c.close()
    np.testing.assert_array_equal(got[0], got[1])
    np.testing.assert_array_equal(got[0], wvote.expected("c", 0)["weighted"])


def test_large_k(knn):
    """k = 1100 > 1000: the exact large-k path, rows of three LDS chunks."""
    rng = np.random.default_rng(77)
    n, m, dim, C, k = 1200, 64, 8, 4, 1100
    centres = rng.uniform(-0.35, 0.35, (C, dim))
    lab = rng.integers(0, C, n + m).astype(np.int32)
    X = centres[lab] + rng.standard_normal((n + m, dim))
    tr, q, lab = X[:n], X[n:], lab[:n]
    _, widx, wdist = oracle.knn(tr, lab, q, k, True, C, n_out=k)
    want = wvote.labels(wvote.lab_rows(lab, widx), wdist, [k, 1001])
    c = knn.Classifier(0)
    c.set_train(tr, lab, C)
    lu = c.classify(q, k, knn.L2)
    c.set_vote(knn.VOTE_DISTANCE)
    l1, i1, d1, _ = c.classify(q, k, knn.L2, return_neighbors=True)
    np.testing.assert_array_equal(i1, widx)
    np.testing.assert_array_equal(d1, wdist)
    np.testing.assert_array_equal(l1, want[0])
    np.testing.assert_array_equal(c.classify_sweep(q, [k, 1001], knn.L2), want)
    print("large k: %d of %d labels differ from the uniform vote" % ((l1 != lu).sum(), m))
    c.close()


# ------------------------------------------------------------ exclusion / leave-one-out
def test_loo_with_duplicated_rows(knn):
    """loo.py's set B (a 3-level grid in 4 dims: every row has duplicates, so z
    >= 1 after the row itself is taken out)."""
    s = loo.SETS["B"]
    tr, lab = loo.data("B")
    w = loo.expected_loo("B")
    ks, C = s["ks"], s["classes"]
    assert (w["dist"][:, 0] == 0.0).sum() > 500  # z >= 1 after exclusion
    c = knn.Classifier(0)
    c.set_train(tr, lab, C)
    for ties in (1, 2):
        c.set_tuning("ties", ties)
        c.set_vote(knn.VOTE_UNIFORM)
        _, _, iu, du, fu = c.loo_sweep(ks, s["metric"], return_neighbors=True)
        c.set_vote(knn.VOTE_DISTANCE)
        lw, cw, iw, dw, fw = c.loo_sweep(ks, s["metric"], return_neighbors=True)
        np.testing.assert_array_equal(iw, iu)
        np.testing.assert_array_equal(dw, du)
        np.testing.assert_array_equal(fw, fu)
        np.testing.assert_array_equal(lw, wvote.labels(wvote.lab_rows(lab, iw), dw, ks))
        np.testing.assert_array_equal(cw, (lw == lab).sum(axis=1))
        if ties == 2:
            np.testing.assert_array_equal(iw, w["idx"])
            np.testing.assert_array_equal(lw, wvote.labels(wvote.lab_rows(lab, w["idx"]),
                                                           w["dist"], ks))
        # the sweep under exclusion: rows 10..49 exclude themselves
        rows = np.arange(10, 50)
        l4, c4 = c.classify_sweep(tr[rows], ks, s["metric"], truth=lab[rows], exclude=rows)
        np.testing.assert_array_equal(l4, lw[:, rows])
        np.testing.assert_array_equal(c4, (lw[:, rows] == lab[rows]).sum(axis=1))
        l5, c5, f5, u5 = c.classify_sweep(tr[rows], ks, s["metric"], truth=lab[rows], exclude=rows,
                                          confusion=True)
        np.testing.assert_array_equal(l5, l4)
        np.testing.assert_array_equal(f5, evalcases.confusion(l4, lab[rows], C)[0])
    c.set_vote(knn.VOTE_UNIFORM)
    c.set_tuning("ties", 1)
    lu, _ = c.loo_sweep(ks, s["metric"])
    np.testing.assert_array_equal(lu, w["labels"])
    c.close()


def test_loo_eval_batch_boundary(knn):
    """n = 16384 + 37 (two leave-one-out batches), no label array anywhere:
    conf equals numpy over the rule's labels on the oracle's rows."""
    tr, lab, C = evalcases.loo_big()
    n = tr.shape[0]
    ks = [1, 4]
    _, idx, dist = oracle.knn(tr, lab, tr, 5, True, C, n_out=5)
    np.testing.assert_array_equal(idx[:, 0], np.arange(n))  # each row finds itself first
    widx, wdist = idx[:, 1:], dist[:, 1:]
    want = wvote.labels(wvote.lab_rows(lab, widx), wdist, ks)
    wconf, wunl = evalcases.confusion(want, lab, C)
    c = knn.Classifier(0)
    c.set_train(tr, lab, C)
    uni = c.loo_sweep(ks, knn.L2, confusion=True, labels=False)
    c.set_vote(knn.VOTE_DISTANCE)
    correct, conf, unl = c.loo_sweep(ks, knn.L2, confusion=True, labels=False)
    np.testing.assert_array_equal(conf, wconf)
    np.testing.assert_array_equal(unl, wunl)
    np.testing.assert_array_equal(correct, (want == lab).sum(axis=1))
    np.testing.assert_array_equal(np.trace(conf, axis1=1, axis2=2), correct)
    assert conf.sum() == 2 * n
    assert (conf != uni[1]).any()
    c.close()


# ------------------------------------------------------------ groups
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["a", "c"])
def test_group(knn, name, mode):
    """Three ranks on one GPU (ragged thirds of the queries; mode 1: three
    train shards) equal the one-context result."""
    for metric in (0, 1):
        d = wvote.dataset(name, metric)
        tr, lab, q, C = d["tr"], d["lab"], d["q"], d["classes"]
        truth = np.random.default_rng(6).integers(0, C, q.shape[0]).astype(np.int32)
        c = knn.Classifier(0)
        c.set_train(tr, lab, C)
        c.set_vote(knn.VOTE_DISTANCE)
        lw, cw = c.classify_sweep(q, KS, metric, truth=truth)
        l5, i5, d5, _ = c.classify(q, 5, metric, return_neighbors=True)
        c.set_vote(knn.VOTE_UNIFORM)
        lu = c.classify_sweep(q, KS, metric)
        c.close()
        g = knn.Group([0, 0, 0], mode)
        g.set_train(tr, lab, C)
        g.set_vote(knn.VOTE_DISTANCE)
        gl, gc = g.classify_sweep(q, KS, metric, truth=truth)
        np.testing.assert_array_equal(gl, lw)
        np.testing.assert_array_equal(gc, cw)
        g5, gi, gd, _ = g.classify(q, 5, metric, return_neighbors=True)
        np.testing.assert_array_equal(gi, i5)
        np.testing.assert_array_equal(gd, d5)
        np.testing.assert_array_equal(g5, l5)
        np.testing.assert_array_equal(g5, wvote.labels(wvote.lab_rows(lab, gi), gd, [5])[0])
        l2, c2, conf, unl = g.classify_sweep(q, KS, metric, truth=truth, confusion=True)
        np.testing.assert_array_equal(l2, lw)
        np.testing.assert_array_equal(conf, evalcases.confusion(lw, truth, C)[0])
        if mode == 1:
            with pytest.raises(knn.KnnError, match=r"knn error -1: .*train-sharded"):
                g.loo_sweep([1, 3], metric)
        g.set_vote(knn.VOTE_UNIFORM)
        np.testing.assert_array_equal(g.classify_sweep(q, KS, metric), lu)
        g.close()


# ------------------------------------------------------------ driver
def test_driver_weights(knn, tmp_path, fmt_cout):
    """--weights distance --K_list 1,3,5: the printed accuracies and the test
    labels are the oracle's ("ties" = 2: the rows are the reference's)."""
    spec = dict(kind="int", seed=29, N_train=900, N_test=60, N_val=90, dim=6, class_cnt=4)
    (tr, trl, te, _, va, val), _ = datagen.write_csvs(str(tmp_path), spec)
    cfg = knn.KnnConfig(dim=6, K=5, N_train=900, N_test=60, N_val=90, class_cnt=4,
                        train_file_name="train.csv", validation_file_name="validation.csv",
                        test_file_name="test.csv")
    ks = [1, 3, 5]
    out = knn.run_driver(cfg, str(tmp_path), extra=["--weights", "distance", "--K_list", "1,3,5",
                                                    "--tune", "ties=2"])
    oracle.normalize(tr, te, va)
    _, vidx, vdist = oracle.knn(tr, trl, va, 5, True, 4, n_out=5)
    want = wvote.labels(wvote.lab_rows(trl, vidx), vdist, ks)
    accs = [oracle.acc(val, want[i]) for i in range(3)]
    best, sel = -1.0, None
    for i, a in enumerate(accs):
        if a > best:
            best, sel = a, i
    head = ["K = %d accuracy = %s" % (k, fmt_cout(a)) for k, a in zip(ks, accs)]
    head += ["selected K = %d" % ks[sel], "accuracy = " + fmt_cout(best)]
    lines = out.splitlines()
    assert lines[:5] == head
    assert lines[5].startswith("Running time is ") and len(lines) == 6
    _, tidx, tdist = oracle.knn(tr, trl, te, ks[sel], True, 4, n_out=ks[sel])
    twant = wvote.labels(wvote.lab_rows(trl, tidx), tdist, [ks[sel]])[0]
    got = np.loadtxt(os.path.join(str(tmp_path), "Test_label.csv"), dtype=np.int32)
    np.testing.assert_array_equal(got, twant)
    # the default is the uniform vote
    plain = knn.run_driver(cfg, str(tmp_path), extra=["--K_list", "1,3,5", "--tune", "ties=2"])
    same = knn.run_driver(cfg, str(tmp_path), extra=["--K_list", "1,3,5", "--tune", "ties=2",
                                                     "--weights", "uniform"])
    assert plain.splitlines()[:5] == same.splitlines()[:5]
    uni = evalcases.oracle_labels(tr, trl, va, ks, True, 4)
    assert plain.splitlines()[:3] == ["K = %d accuracy = %s" % (k, fmt_cout(oracle.acc(val, uni[i])))
                                      for i, k in enumerate(ks)]

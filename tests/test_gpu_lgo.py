"""Leave-group-out K sweep on the GPU (knn_set_groups, knn_lgo_sweep*,
knn_classify_sweep_gexcl_device, knn_group_lgo_sweep, the driver's --groups)
against the CPU oracle run on the GROUP-REMOVED train sets (tests/lgo.py): for
a query with group gq the result is the K sweep's on the train set without the
rows of group gq, indices mapped back.

The order among equal distances that counts is the reference's std::sort over
the n - c remaining records, so a build that drops the group but keeps the
n-record order fails on the order-sensitive rows test_lgo_data.py counts.
The stream-order test of the two device calls is test_group_sweep_held in
test_gpu_lgo_streams.py.
"""
import os

import numpy as np
import pytest

import datagen
import lgo
import loo
import oracle
import wvote
from test_gpu_loo import PATHS, _loo_device

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


def _trained(knn, name, groups=True, **tuning):
    s = lgo.SETS[name]
    tr, lab, grp = lgo.data(name)
    c = knn.Classifier(0)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    c.set_train(tr, lab, s["classes"])
    if groups:
        c.set_groups(grp)
    return c, s


def _device(c, call, rows, ks, *args):
    """A *_sweep_device call into torch buffers -> numpy (labels, correct, idx, dist, flags)."""
    import torch
    dev = torch.device("cuda", 0)
    nk, kmax, r1 = len(ks), max(max(ks), 1), max(rows, 1)
    L = torch.full((nk, r1), -7, dtype=torch.int32, device=dev)
    C = torch.full((nk,), -7, dtype=torch.int64, device=dev)
    I = torch.full((r1, kmax), -7, dtype=torch.int64, device=dev)
    D = torch.zeros((r1, kmax), dtype=torch.float64, device=dev)
    F = torch.full((r1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    call(*args, L.data_ptr(), C.data_ptr(), I.data_ptr(), D.data_ptr(), F.data_ptr())
    c.sync()
    return (L.cpu().numpy()[:, :rows], C.cpu().numpy(), I.cpu().numpy()[:rows],
            D.cpu().numpy()[:rows], F.cpu().numpy()[:rows])


def _lgo_device(c, row0, rows, ks, metric):
    return _device(c, lambda *a: c.lgo_sweep_device(row0, rows, ks, metric, *a), rows, ks)


def _check1(got, w):
    """(labels, correct, idx, dist, flags) at "ties" = 1 against lgo.expected."""
    labels, correct, idx, dist, flags = got
    np.testing.assert_array_equal(labels, w["labels"])
    if "correct" in w:
        np.testing.assert_array_equal(correct, w["correct"])
    np.testing.assert_array_equal(idx, w["idx1"])
    np.testing.assert_array_equal(_bits(dist), _bits(w["dist"]))
    np.testing.assert_array_equal(flags & loo.FLAG_MASK, w["flags1"])


# ------------------------------------------------ 1. the data sets, all rows
@pytest.mark.parametrize("name", sorted(lgo.SETS))
def test_data_sets(knn, name):
    w = lgo.expected_lgo(name)
    nv = w["naive"]
    c, s = _trained(knn, name)
    assert c.group_max() == lgo.GMAX
    got = c.lgo_sweep(s["ks"], s["metric"], return_neighbors=True)
    assert got[0].shape == (len(s["ks"]), s["n"]) and got[1].dtype == np.int64
    print("%s: %d rows differ from the oracle (%d order-sensitive)"
          % (name, (got[0] != w["labels"]).any(axis=0).sum(), w["sensitive"].sum()))
    _check1(got, w)
    # "ties" = 2: every row with a tie in its top kmax in the reference's order
    c.set_tuning("ties", 2)
    labels2, correct2, idx2, dist2, flags2 = c.lgo_sweep(s["ks"], s["metric"],
                                                         return_neighbors=True)
    np.testing.assert_array_equal(labels2, w["labels"])
    np.testing.assert_array_equal(correct2, w["correct"])
    np.testing.assert_array_equal(idx2, np.where(nv["tied"][:, None], w["idx"], nv["idx"]))
    np.testing.assert_array_equal(_bits(dist2), _bits(w["dist"]))
    np.testing.assert_array_equal(flags2 & loo.FLAG_MASK, nv["flags"] | np.where(nv["tied"], 32, 0))
    # "ties" = 0: the (dist, index) order minus the group, prefix-voted
    c.set_tuning("ties", 0)
    labels0, correct0, idx0, dist0, flags0 = c.lgo_sweep(s["ks"], s["metric"],
                                                         return_neighbors=True)
    np.testing.assert_array_equal(labels0, nv["labels"])
    np.testing.assert_array_equal(idx0, nv["idx"])
    np.testing.assert_array_equal(_bits(dist0), _bits(nv["dist"]))
    np.testing.assert_array_equal(flags0 & loo.FLAG_MASK, nv["flags"])
    np.testing.assert_array_equal(correct0, (nv["labels"] == lgo.data(name)[1]).sum(axis=1))
    c.close()


# ------------------------------------------------ 2. groups of one row
def test_singletons_equal_leave_one_out(knn):
    import torch
    s = lgo.SETS["G"]
    tr, lab, _ = lgo.data("G")
    n, ks = s["n"], s["ks"]
    c = knn.Classifier(0)
    c.set_train(tr, lab, s["classes"])
    c.set_groups(np.arange(n, dtype=np.int32))
    assert c.group_max() == 1
    a = _lgo_device(c, 300, 500, ks, knn.L2)
    b = _loo_device(c, 300, 500, ks, knn.L2)
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(_bits(a[3]), _bits(b[3]))
    np.testing.assert_array_equal(a[4] & loo.FLAG_MASK, b[4] & loo.FLAG_MASK)
    # arbitrary queries: train rows excluding themselves, grid points excluding
    # their nearest row, and every third query nothing (-1)
    rng = np.random.default_rng(17)
    m = 240
    Q = rng.integers(0, 8, (m, 6)).astype(np.float64)
    excl = np.full(m, -1, np.int64)
    ar = np.arange(n)
    for i in range(m):
        if i % 3 == 0:
            excl[i] = int(rng.integers(0, n))
            Q[i] = tr[excl[i]]
        elif i % 3 == 1:
            excl[i] = np.lexsort((ar, oracle.row_distances(Q[i], tr, True)))[0]
    dev = torch.device("cuda", 0)
    dQ = torch.from_numpy(Q).to(dev)
    dE = torch.from_numpy(excl).to(dev)
    dG = torch.from_numpy(excl.astype(np.int32)).to(dev)
    torch.cuda.synchronize(dev)
    ge = _device(c, lambda *p: c.classify_sweep_gexcl_device(
        dQ.data_ptr(), m, dG.data_ptr(), ks, knn.L2, p[0], None, None, *p[2:]), m, ks)
    ex = _device(c, lambda *p: c.classify_sweep_device(
        dQ.data_ptr(), m, ks, knn.L2, p[0], None, None, *p[2:], d_excl=dE.data_ptr()), m, ks)
    np.testing.assert_array_equal(ge[0], ex[0])
    np.testing.assert_array_equal(ge[2], ex[2])
    np.testing.assert_array_equal(_bits(ge[3]), _bits(ex[3]))
    np.testing.assert_array_equal(ge[4] & loo.FLAG_MASK, ex[4] & loo.FLAG_MASK)
    c.close()


# ------------------------------------------------ 3. row-length edges
ROWS = 48  # queries of the edge runs: the first train rows of set G


@pytest.mark.parametrize("ks", [[56], [3, 57], [58, 1], [122, 5], [1], [5, 0, 37, 5, 10, 0]],
                         ids=["k1=63", "k1=64", "k1=65", "k1=129", "kmax=1", "zero-and-dups"])
def test_row_length_edges(knn, ks):
    """gmax = 7: the searched rows hold kmax + 7 entries, one short of, at and
    one past the 64-entry chunk of the drop kernel, and past two chunks."""
    s = lgo.SETS["G"]
    tr, lab, grp = lgo.data("G")
    w = lgo.expected(tr, lab, grp, tr[:ROWS], grp[:ROWS], ks, True, s["classes"], lgo.GMAX)
    w["correct"] = (w["labels"] == lab[:ROWS]).sum(axis=1)
    c, _ = _trained(knn, "G")
    _check1(_lgo_device(c, 0, ROWS, ks, knn.L2), w)
    c.set_tuning("ties", 0)
    got = _lgo_device(c, 0, ROWS, ks, knn.L2)
    np.testing.assert_array_equal(got[2], w["naive"]["idx"])
    np.testing.assert_array_equal(got[4] & loo.FLAG_MASK, w["naive"]["flags"])
    c.close()


def test_large_group_takes_the_large_k_path(knn):
    """A 400-row group and kmax = 700: the search runs at 1100 > 1000 entries
    (the exact large-k path) and the drop kernel walks 18 chunks; queries on
    both sides of the group's last row."""
    s = lgo.SETS["G"]
    tr, lab, grp = lgo.data("G")
    big = np.where(np.arange(s["n"]) < 400, 0, grp + 1).astype(np.int32)
    ks = [700, 3]
    rows = np.arange(392, 408)
    w = lgo.expected(tr, lab, big, tr[rows], big[rows], ks, True, s["classes"], 400)
    w["correct"] = (w["labels"] == lab[rows]).sum(axis=1)
    c, _ = _trained(knn, "G", groups=False)
    c.set_groups(big)
    assert c.group_max() == 400
    _check1(_lgo_device(c, 392, 16, ks, knn.L2), w)
    c.close()


def test_k_limit(knn):
    """ks[i] = n - gmax is served (the row holds the whole set); one more is refused."""
    s = lgo.SETS["G"]
    tr, lab, grp = lgo.data("G")
    n = s["n"]
    ks = [2, n - lgo.GMAX]
    w = lgo.expected(tr, lab, grp, tr[:8], grp[:8], ks, True, s["classes"], lgo.GMAX)
    w["correct"] = (w["labels"] == lab[:8]).sum(axis=1)
    c, _ = _trained(knn, "G")
    _check1(_lgo_device(c, 0, 8, ks, knn.L2), w)
    with pytest.raises(knn.KnnError, match=r"knn error -1: ks\[1\] = %d" % (n - lgo.GMAX + 1)):
        _lgo_device(c, 0, 8, [2, n - lgo.GMAX + 1], knn.L2)
    with pytest.raises(knn.KnnError, match=r"knn error -1: ks\[0\]"):
        c.lgo_sweep([n - lgo.GMAX + 1])
    c.close()


def test_group_at_the_end_of_the_searched_row(knn):
    """The whole group lies inside the searched row and the row ENDS with it,
    at a larger distance than the last kept entry, while the full order's
    record k1 ties with entry k1 - 1: the search's boundary bit for k1 is set,
    the reduced set's is not (its kmax-th record is nearer than its
    successor).  One dimension, query at 0, train row j at j + 1; rows 5..11
    are the group, row 12 repeats row 11's value."""
    n, kmax, gmax = 40, 5, 7
    x = np.arange(1, n + 1, dtype=np.float64)
    x[12] = x[11]
    tr = x[:, None].copy()
    lab = (np.arange(n) % 2).astype(np.int32)
    grp = np.arange(n, dtype=np.int32)
    grp[5:12] = 5
    Q = np.zeros((2, 1))
    qg = np.array([5, -1], np.int32)
    w = lgo.expected(tr, lab, grp, Q, qg, [kmax], True, 2, gmax)
    assert w["naive"]["c"][0] == gmax and w["naive"]["bnd_out"][0] and not w["naive"]["flags"][0] & 2
    c = knn.Classifier(0)
    c.set_train(tr, lab, 2)
    c.set_groups(grp)
    labels, idx, dist, flags = c.classify_sweep(Q, [kmax], knn.L2, return_neighbors=True,
                                                exclude_group=qg)
    np.testing.assert_array_equal(labels, w["labels"])
    np.testing.assert_array_equal(idx, w["idx1"])
    np.testing.assert_array_equal(flags & loo.FLAG_MASK, w["flags1"])
    c.close()


# ------------------------------------------------ 4. every candidate path
@pytest.mark.parametrize("path", sorted(PATHS))
def test_candidate_paths(knn, path):
    """Data set G's grid scaled by 1/8 (exact in every operand format; the
    distances scale by a power of two, so labels and indices are G's)."""
    prec, tuning, want_path = PATHS[path]
    w = lgo.expected_lgo("G")
    s = lgo.SETS["G"]
    tr, lab, grp = lgo.data("G")
    c = knn.Classifier(0)
    if prec:
        c.set_precision(getattr(knn, "PRECISION_" + prec))
    for key, value in tuning.items():
        c.set_tuning(key, value)
    c.set_train(tr / 8.0, lab, s["classes"])
    c.set_groups(grp)
    labels, correct, idx, dist, flags = c.lgo_sweep(s["ks"], s["metric"], return_neighbors=True)
    assert c.last_candidate_path() == want_path
    np.testing.assert_array_equal(labels, w["labels"])
    np.testing.assert_array_equal(correct, w["correct"])
    np.testing.assert_array_equal(idx, w["idx1"])
    np.testing.assert_array_equal(_bits(dist), _bits(w["dist"] / 8.0))
    np.testing.assert_array_equal(flags & loo.FLAG_MASK, w["flags1"])
    c.close()


# ------------------------------------------------ 5. arbitrary queries
@pytest.fixture(scope="module")
def offset_queries():
    """200 grid points; query i excludes the group of its nearest row (i % 4
    == 0), of its 20th row (1), nothing through -1 (2) or through an id past
    n_groups (3)."""
    s = lgo.SETS["G"]
    tr, lab, grp = lgo.data("G")
    rng = np.random.default_rng(311)
    m = 200
    Q = rng.integers(0, 8, (m, 6)).astype(np.float64)
    qg = np.full(m, -1, np.int32)
    ar = np.arange(s["n"])
    for i in range(m):
        order = np.lexsort((ar, oracle.row_distances(Q[i], tr, True)))
        if i % 4 == 0:
            qg[i] = grp[order[0]]
        elif i % 4 == 1:
            qg[i] = grp[order[19]]
        elif i % 4 == 3:
            qg[i] = int(grp.max()) + 1 + i
    truth = np.random.default_rng(5).integers(0, 3, m).astype(np.int32)
    w = lgo.expected(tr, lab, grp, Q, qg, s["ks"], True, s["classes"], lgo.GMAX)
    return Q, qg, truth, w


def test_arbitrary_queries(knn, offset_queries):
    Q, qg, truth, w = offset_queries
    c, s = _trained(knn, "G")
    labels, correct, idx, dist, flags = c.classify_sweep(Q, s["ks"], knn.L2, truth=truth,
                                                         return_neighbors=True, exclude_group=qg)
    w = dict(w, correct=(w["labels"] == truth).sum(axis=1))
    _check1((labels, correct, idx, dist, flags), w)
    grp = lgo.data("G")[2]
    sel = (qg >= 0) & (qg <= grp.max())
    assert not (grp[idx[sel]] == qg[sel, None]).any()
    # nothing excluded: the plain sweep (KNN_FLAG_EXACT_RESCAN aside)
    none = ~sel
    plain = c.classify_sweep(Q[none], s["ks"], knn.L2, return_neighbors=True)
    np.testing.assert_array_equal(labels[:, none], plain[0])
    np.testing.assert_array_equal(idx[none], plain[1])
    np.testing.assert_array_equal(_bits(dist[none]), _bits(plain[2]))
    np.testing.assert_array_equal(flags[none] & ~knn.FLAG_EXACT_RESCAN,
                                  plain[3] & ~knn.FLAG_EXACT_RESCAN)
    with pytest.raises(ValueError, match="mutually exclusive"):
        c.classify_sweep(Q, s["ks"], exclude=np.full(200, -1, np.int64), exclude_group=qg)
    c.close()


def test_confusion_and_a_nonfinite_query(knn, offset_queries):
    Q, qg, truth, w = offset_queries
    Q = Q.copy()
    Q[7, 2] = np.nan  # (query 7 excludes nothing: i % 4 == 3)
    c, s = _trained(knn, "G")
    labels, correct, conf, unl = c.classify_sweep(Q, s["ks"], knn.L2, truth=truth, confusion=True,
                                                  exclude_group=qg)
    want = w["labels"].copy()
    want[:, 7] = -1
    np.testing.assert_array_equal(labels, want)
    np.testing.assert_array_equal(correct, (want == truth).sum(axis=1))
    C, m = s["classes"], Q.shape[0]
    for j in range(len(s["ks"])):
        ok = want[j] >= 0
        hist = np.zeros((C, C), np.int64)
        np.add.at(hist, (truth[ok], want[j][ok]), 1)
        np.testing.assert_array_equal(conf[j], hist)
        assert conf[j].sum() + unl[j] == m and unl[j] == 1
    got = c.classify_sweep(Q, s["ks"], knn.L2, return_neighbors=True, exclude_group=qg)
    assert got[3][7] & knn.FLAG_NONFINITE and (got[1][7] == -1).all()
    c.close()


# ------------------------------------------------ 6. distance weights
def test_vote_distance(knn, offset_queries):
    """KNN_VOTE_DISTANCE: the sequential rule of tests/wvote.py over the rows
    the call reports, which are the expected rows."""
    Q, qg, truth, w = offset_queries
    c, s = _trained(knn, "G")
    c.set_vote(knn.VOTE_DISTANCE)
    labels, idx, dist, flags = c.classify_sweep(Q, s["ks"], knn.L2, return_neighbors=True,
                                                exclude_group=qg)
    np.testing.assert_array_equal(idx, w["idx1"])
    np.testing.assert_array_equal(_bits(dist), _bits(w["dist"]))
    lab = lgo.data("G")[1]
    np.testing.assert_array_equal(labels, wvote.labels(wvote.lab_rows(lab, w["idx1"]), w["dist"],
                                                       s["ks"]))
    tr, lab, grp = lgo.data("G")
    wl = lgo.expected_lgo("G")
    got = c.lgo_sweep(s["ks"], knn.L2, return_neighbors=True)
    np.testing.assert_array_equal(got[2], wl["idx1"])
    want = wvote.labels(wvote.lab_rows(lab, wl["idx1"]), wl["dist"], s["ks"])
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], (want == lab).sum(axis=1))
    c.close()


# ------------------------------------------------ 7. state
def test_state(knn):
    import torch
    s = lgo.SETS["G"]
    tr, lab, grp = lgo.data("G")
    c = knn.Classifier(0)
    with pytest.raises(knn.KnnError, match="knn error -3"):
        c.set_groups(grp)
    c.set_train(tr, lab, s["classes"])
    assert c.group_max() == 0
    with pytest.raises(knn.KnnError, match="knn error -3"):
        c.lgo_sweep([1, 3])
    bad = np.array(grp)
    bad[1234] = int(grp.max()) + 1
    bad[1300] = -1
    with pytest.raises(knn.KnnError, match=r"knn error -1: .*row 1234\b"):
        c.set_groups(bad, n_groups=int(grp.max()) + 1)
    assert c.group_max() == 0
    c.set_groups(grp)
    assert c.group_max() == lgo.GMAX
    c.set_train(tr, lab, s["classes"])  # a new train set carries no groups
    assert c.group_max() == 0
    c.set_groups(grp)
    c.set_groups(None)
    assert c.group_max() == 0
    with pytest.raises(knn.KnnError, match="knn error -3"):
        c.classify_sweep(tr[:4], [1, 3], exclude_group=np.zeros(4, np.int32))
    # without a group array the call is the plain sweep, groups or none
    np.testing.assert_array_equal(c.classify_sweep(tr[:4], [1, 3]),
                                  oracle_sweep(tr, lab, tr[:4], [1, 3], s["classes"]))
    # the device variant borrows the caller's array
    dev = torch.device("cuda", 0)
    dG = torch.from_numpy(np.array(grp)).to(dev)
    torch.cuda.synchronize(dev)
    c.set_groups_device(dG.data_ptr(), int(grp.max()) + 1, keep=dG)
    assert c.group_max() == lgo.GMAX
    w = lgo.expected_lgo("G")
    got = _lgo_device(c, 0, 64, s["ks"], knn.L2)
    np.testing.assert_array_equal(got[0], w["labels"][:, :64])
    c.close()


def oracle_sweep(tr, lab, Q, ks, classes):
    return np.stack([oracle.knn(tr, lab, Q, k, True, classes)[0] for k in ks])


# ------------------------------------------------ 9. group
def test_group_loopback(knn):
    """Three ranks on one GPU take ragged thirds of the train rows."""
    for name in sorted(lgo.SETS):
        w = lgo.expected_lgo(name)
        s = lgo.SETS[name]
        tr, lab, grp = lgo.data(name)
        g = knn.Group([0, 0, 0], mode=0)
        g.set_train(tr, lab, s["classes"])
        g.set_groups(grp)
        labels, correct, conf, unl = g.lgo_sweep(s["ks"], s["metric"], confusion=True)
        np.testing.assert_array_equal(labels, w["labels"])
        np.testing.assert_array_equal(correct, w["correct"])
        for j in range(len(s["ks"])):
            hist = np.zeros((s["classes"],) * 2, np.int64)
            np.add.at(hist, (lab, w["labels"][j]), 1)
            np.testing.assert_array_equal(conf[j], hist)
        assert (unl == 0).all()
        g.close()


def test_group_train_sharded_is_refused(knn):
    s = lgo.SETS["G"]
    tr, lab, grp = lgo.data("G")
    g = knn.Group([0, 0, 0], mode=1)
    g.set_train(tr, lab, s["classes"])
    with pytest.raises(knn.KnnError, match=r"knn error -1: .*train-sharded"):
        g.set_groups(grp)
    with pytest.raises(knn.KnnError, match=r"knn error -1: .*leave-group-out.*train-sharded"):
        g.lgo_sweep(s["ks"], s["metric"])
    with pytest.raises(knn.KnnError, match=r"knn error -1: .*leave-one-out.*train-sharded"):
        g.loo_sweep(s["ks"], s["metric"])
    g.close()


# ------------------------------------------------ 10. driver
def test_driver_groups(knn, tmp_path, fmt_cout):
    spec = dict(kind="int", seed=23, N_train=600, N_test=40, N_val=10, dim=6, class_cnt=4)
    (tr, trl, te, _, _, _), _ = datagen.write_csvs(str(tmp_path), spec)
    os.remove(tmp_path / "validation.csv")  # --loo needs no validation file
    grp = (np.random.default_rng(29).permutation(600) // 4).astype(np.int32)
    np.savetxt(tmp_path / "groups.csv", grp, fmt="%d")
    cfg = knn.KnnConfig(dim=6, K=7, N_train=600, N_test=40, N_val=10, class_cnt=4,
                        train_file_name="train.csv", validation_file_name="validation.csv",
                        test_file_name="test.csv")
    ks = [1, 3, 5]
    plain = knn.run_driver(cfg, str(tmp_path), extra=["--loo", "--K_list", "1,3,5"])
    out = knn.run_driver(cfg, str(tmp_path),
                         extra=["--loo", "--K_list", "1,3,5", "--groups", "groups.csv"])
    oracle.normalize(tr, te, None)
    want = lgo.expected_gexcl(tr, trl, grp, tr, grp, ks, True, 4)
    accs = [float((want["labels"][j] == trl).sum()) / 600 for j in range(3)]
    lines = out.splitlines()
    for j, k in enumerate(ks):
        assert lines[j] == "K = %d lgo accuracy = %s" % (k, fmt_cout(accs[j]))
    best, sel = -1.0, None
    for k, a in zip(ks, accs):
        if a > best:
            best, sel = a, k
    assert lines[3] == "selected K = %d" % sel
    assert lines[4].startswith("Running time is ")
    got = np.loadtxt(tmp_path / "Test_label.csv", dtype=np.int64, ndmin=1)
    np.testing.assert_array_equal(got, oracle.knn(tr, trl, te, sel, True, 4)[0])
    # without --groups: the leave-one-out lines, as before
    loo_want = loo.expected_excl(tr, trl, tr, np.arange(600), ks, True, 4)
    pl = plain.splitlines()
    for j, k in enumerate(ks):
        acc = float((loo_want["labels"][j] == trl).sum()) / 600
        assert pl[j] == "K = %d loo accuracy = %s" % (k, fmt_cout(acc))
    assert "lgo" not in plain

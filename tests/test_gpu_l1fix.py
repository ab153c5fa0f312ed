"""GPU parity of candidate path 8: the L1 pass on 16-bit fixed-point codes
(v_sad_u16, csrc/knn_cand_fix16.hip; tuning key "u16l1") against the CPU
oracle -- labels, neighbour indices, fp64 distance bit patterns and tie flags,
as test_gpu_parity.py compares them.  Every case sets "u16l1" = 1 unless it is
about the plan's own choice, and asserts that path 8 served the call.  The
data sets and the CPU model of the pass are in tests/l1fix.py;
test_l1fix_data.py checks the error bound itself on every one of them."""
import numpy as np
import pytest

import l1fix
import loo
import oracle
from l1codes import assert_neighbors_match

pytestmark = pytest.mark.gpu


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


def _clf(knn, **tuning):
    c = knn.Classifier(0)
    c.set_tuning("u16l1", 1)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    return c


def _check(knn, c, tr, lab, te, k, classes, path=8):
    """One classify against the oracle; returns (labels, idx, dist, flags)."""
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == path
    if path == 8:
        assert c.last_kernel_name().startswith("cand_fix16_kernel<%d," % l1fix.pad_dim(tr.shape[1]))
    want, widx, wdist = oracle.knn(tr, lab, te, k, False, classes, n_out=k)
    assert (idx < tr.shape[0]).all() and (idx >= 0).all()
    tie_vote = (flags & knn.FLAG_TIE_VOTE) != 0
    np.testing.assert_array_equal(got[~tie_vote], want[~tie_vote])
    # the tied queries whose label the order could change carry the
    # reference's own order: index for index, hence the same label
    ref = (flags & knn.FLAG_TIE_REF) != 0
    np.testing.assert_array_equal(idx[ref], widx[ref])
    np.testing.assert_array_equal(got, want)
    assert_neighbors_match(idx, dist, widx, wdist, flags)
    return got, idx, dist, flags


# ------------------------------------------------------------ 1. shape edges
@pytest.mark.parametrize("d", l1fix.SHAPE_D)
@pytest.mark.parametrize("n", l1fix.SHAPE_N)
def test_shape_edges(knn, n, d):
    """Continuous data, uniform and Gaussian: a pad row in the last tile (n =
    31, 257, 6000 are no multiple of 64), an odd d (half a dword: 1, 7, 13,
    129), pad dims inside a ds_read_b128 (d = 100), one sub-tile only (n =
    31), every padded width; k = 1, 7, 30 and n - 1."""
    for kind in l1fix.SHAPE_KINDS:
        tr, lab, te = l1fix.shape_set(kind, n, d)
        c = _clf(knn)
        c.set_train(tr, lab, 4)
        for k in l1fix.shape_ks(n):
            got, idx, dist, flags = _check(knn, c, tr, lab, te, k, 4)
            assert (flags & 14).sum() == 0  # continuous data: no equal distances
        c.close()


# ------------------------------- 2. the code ends and the accumulator's range
@pytest.mark.parametrize("d", [256, 255])
def test_code_ends(knn, d):
    tr, lab, te = l1fix.code_ends(d)
    n = tr.shape[0]
    c = _clf(knn)
    c.set_train(tr, lab, 3)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, n - 1, 3)
    # the one row k = n - 1 leaves out is the farthest: for the query of all 0
    # the row of all 1 and the other way round ...
    assert 1 not in idx[0] and 0 not in idx[1]
    # ... and at k = n it comes last, at the largest distance of the set
    got, idx, dist, flags = _check(knn, c, tr, lab, te, n, 3)
    assert dist[0, -1] == float(d) and idx[0, -1] == 1
    assert dist[1, -1] == float(d) and idx[1, -1] == 0
    # (k = n - 1 leaves no row outside the lists to bound: such calls finish in
    # the exact rescan on every path; a small k is certified from the proxies)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, 3, 3)
    # the two queries coded at 0 / 65535 in every dim cannot certify
    assert (flags[2:4] & knn.FLAG_EXACT_RESCAN).all()
    assert ((flags & knn.FLAG_EXACT_RESCAN) != 0).sum() <= 2 + te.shape[0] // 16
    c.close()


# --------------------------------- 3. the reference's own configuration
@pytest.mark.parametrize("name", ["f3_l1", "f10_l1_int"])
def test_golden_l1_fixtures_as_the_reference_ran_them(knn, name, fmt_cout):
    """Normalize = true takes the values off every binary grid: no exact code
    pass can serve these; path 8 gives the golden labels, the golden
    neighbours and the accuracy line."""
    fx, tr, trl, te, va, val_ = l1fix.fixture_sets(name)
    s = fx.spec
    assert not s["Euclidean_distance"] and s["Normalize"]
    K = s["K"]
    c = _clf(knn, i8l1=1)  # (the byte-code pass asked for too: the data refuse it)
    c.set_train(tr, trl, s["class_cnt"])
    got, idx, dist, flags = c.classify(te, K, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8
    np.testing.assert_array_equal(got, fx.test_labels)
    nq = fx.test_nbr_idx.shape[0]
    assert_neighbors_match(idx[:nq], dist[:nq], fx.test_nbr_idx[:nq, :K],
                           fx.test_nbr_dist[:nq, :K], flags[:nq])
    vl, vidx, vdist, vflags = c.classify(va, K, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8
    acc = float((vl == val_).sum()) / len(val_)
    assert "accuracy = " + fmt_cout(acc) == str(fx.accuracy_line)
    nv = fx.val_nbr_idx.shape[0]
    assert_neighbors_match(vidx[:nv], vdist[:nv], fx.val_nbr_idx[:nv, :K],
                           fx.val_nbr_dist[:nv, :K], vflags[:nv])
    c.close()


def test_normedge_fixture_under_l1(knn):
    """f4_normedge's sets (a constant dim, dims the normalisation leaves
    unscaled) under L1 against the oracle."""
    fx, tr, trl, te, va, val_ = l1fix.fixture_sets("f4_normedge")
    s = fx.spec
    c = _clf(knn)
    c.set_train(tr, trl, s["class_cnt"])
    for q in (te, va):
        _check(knn, c, tr, trl, q, s["K"], s["class_cnt"])
    c.close()


# ------------------------------- 4. near ties at the pass's error scale
def test_near_ties_below_one_code_step(knn):
    """neartie case E: the k-th and (k + 1)-th rows differ by far less than a
    code step inside the tight clusters; the fp64 re-rank must order them as
    the oracle does, index for index, with no tie flag."""
    tr, lab, te, info, k, metric = l1fix.near_ties()
    c = _clf(knn)
    c.set_train(tr, lab, 5)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, k, 5)
    want, widx, wdist = oracle.knn(tr, lab, te, k, False, 5, n_out=k)
    np.testing.assert_array_equal(idx, widx)
    assert ((flags & 14) == 0).all() and ((flags & knn.FLAG_TIE_REF) == 0).all()
    c.close()


@pytest.mark.parametrize("ties", [1, 2])
def test_exact_duplicates_with_different_labels(knn, ties):
    tr, lab, te = l1fix.duplicates()
    k = l1fix.DUP_K
    c = _clf(knn, ties=ties)
    c.set_train(tr, lab, 3)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, k, 3)
    # every query: equal distances inside the top k and across the k-th place
    assert (flags & knn.FLAG_TIE_BOUNDARY).all()
    assert ((flags & 14) != 0).all()
    if ties == 2:
        want, widx, wdist = oracle.knn(tr, lab, te, k, False, 3, n_out=k)
        assert ((flags & knn.FLAG_TIE_REF) != 0).all()
        np.testing.assert_array_equal(idx, widx)
    c.close()


# --------------------------------------- 5. queries the pass must hand over
def test_handover_queries(knn):
    tr, lab, te, near, far, nan = l1fix.handover()
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    k = l1fix.HANDOVER_K
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8
    assert (got[nan] == -1).all() and (flags[nan] & knn.FLAG_NONFINITE).all()
    assert (flags[far] & knn.FLAG_EXACT_RESCAN).all()
    ok = np.setdiff1d(np.arange(te.shape[0]), nan)
    want, widx, wdist = oracle.knn(tr, lab, te[ok], k, False, 4, n_out=k)
    np.testing.assert_array_equal(got[ok], want)
    assert_neighbors_match(idx[ok], dist[ok], widx, wdist, flags[ok])
    # inside the code headroom -- the train hull or not: served by the pass
    # itself (test_l1fix_data.py: every such query's gap exceeds 2 E)
    served = np.setdiff1d(ok, far)
    assert ((flags[served] & knn.FLAG_EXACT_RESCAN) != 0).sum() * 16 <= len(served)
    assert ((flags[near] & knn.FLAG_EXACT_RESCAN) == 0).all()
    c.close()


# ------------------------------------ 6. unequal dims and degenerate sets
@pytest.mark.parametrize("kind", ["unequal", "constant", "far"])
def test_odd_sets(knn, kind):
    tr, lab, te = l1fix.odd_set(kind)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in (1, 6):
        _check(knn, c, tr, lab, te, k, 4)
    if kind == "far":
        assert c.last_rescan_count() * 16 <= te.shape[0]
    c.close()


# ------------------------------------------------------------------ 7. the plan
def test_plan_choices(knn):
    rng = np.random.default_rng(6)
    cont = rng.random((2000, 128))
    lab = l1fix.labels_for(2000, 4, 7)
    q64 = rng.random((64, 128))
    big = np.tile(q64, (64, 1))  # 4096 queries
    ints, _, int_q = l1fix.int_sets(2000, 64, 128)
    wide, wide_q = rng.random((2000, 300)), rng.random((64, 300))

    def path(train, q, metric=None, **tuning):
        c = knn.Classifier(0)
        for key, value in tuning.items():
            c.set_tuning(key, value)
        c.set_train(train, lab, 4)
        c.classify(q, 5, knn.L1 if metric is None else metric)
        p, name = c.last_candidate_path(), c.last_kernel_name()
        c.close()
        return p, name

    # key 0 or absent: path 1 at both sizes
    for q in (q64, big):
        assert path(cont, q)[0] == 1
        assert path(cont, q, u16l1=0)[0] == 1
    # key 1: path 8 at both sizes, 4 waves for the small batch, 8 for the large
    assert path(cont, q64, u16l1=1) == (8, "cand_fix16_kernel<128,8,4>")
    assert path(cont, big, u16l1=1) == (8, "cand_fix16_kernel<128,8,8>")
    # an integer train set: the exact byte-code pass wins where "i8l1" selects
    # it; without it path 8 serves the set too
    assert path(ints, int_q, i8l1=1, u16l1=1)[0] == 7
    assert path(ints, np.tile(int_q, (64, 1)), u16l1=1)[0] == 7  # (AUTO's own choice)
    assert path(ints, int_q, u16l1=1)[0] == 8
    assert path(ints, int_q, i8l1=0, u16l1=1)[0] == 8
    # L2 and d = 300 calls are unmoved
    for q in (q64, big):
        assert path(cont, q, metric=knn.L2, u16l1=1) == path(cont, q, metric=knn.L2)
        assert path(cont, q, metric=knn.L2, u16l1=1)[0] != 8
    assert path(wide, wide_q, u16l1=1) == path(wide, wide_q)
    assert path(wide, wide_q, u16l1=1)[0] == 1
    # a bad value is refused
    c = knn.Classifier(0)
    for bad in (-1, 2):
        with pytest.raises(knn.KnnError, match="u16l1"):
            c.set_tuning("u16l1", bad)
    g = knn.Group([0], mode=0)
    with pytest.raises(knn.KnnError, match="u16l1"):
        g.set_tuning("u16l1", 2)
    g.close()
    c.close()


# ------------------------------------------------------------------- 8. callers
def test_classify_sweep_equals_per_k_calls(knn):
    tr, lab, te = l1fix.shape_set("gauss", 6000, 32)
    ks = [1, 3, 10]
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    labels, idx, dist, flags = c.classify_sweep(te, ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8
    for j, k in enumerate(ks):
        got, kidx, kdist, kflags = c.classify(te, k, knn.L1, return_neighbors=True)
        assert c.last_candidate_path() == 8
        np.testing.assert_array_equal(labels[j], got)
        want = oracle.knn(tr, lab, te, k, False, 4)[0]
        np.testing.assert_array_equal(labels[j], want)
    np.testing.assert_array_equal(dist.view(np.int64), kdist.view(np.int64))
    # with exclusions: query i leaves train row i out
    excl = np.arange(te.shape[0], dtype=np.int64)
    want = loo.expected_excl(tr, lab, te, excl, ks, False, 4)
    labels = c.classify_sweep(np.array(te), ks, knn.L1, exclude=excl)
    assert c.last_candidate_path() == 8
    np.testing.assert_array_equal(labels, want["labels"])
    c.close()


def test_loo_sweep_on_600_rows(knn):
    rng = np.random.default_rng(777)
    tr = rng.standard_normal((600, 6))
    lab = l1fix.labels_for(600, 3, 778)
    ks = [1, 3, 10]
    want = loo.expected_excl(tr, lab, tr, np.arange(600), ks, False, 3)
    c = _clf(knn)
    c.set_train(tr, lab, 3)
    labels, correct, idx, dist, flags = c.loo_sweep(ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 8
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(correct, (want["labels"] == lab).sum(axis=1))
    np.testing.assert_array_equal(dist.view(np.int64), want["dist"].view(np.int64))
    c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_group_modes_equal_the_single_classifier(knn, mode):
    tr, lab, te = l1fix.shape_set("gauss", 6000, 32)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, 7, 4)
    c.close()
    g = knn.Group([0, 0, 0], mode=mode)
    g.set_tuning("u16l1", 1)
    g.set_train(tr, lab, 4)
    ggot, gidx, gdist, gflags = g.classify(te, 7, knn.L1, return_neighbors=True)
    np.testing.assert_array_equal(ggot, got)
    np.testing.assert_array_equal(gdist.view(np.int64), dist.view(np.int64))
    assert_neighbors_match(gidx, gdist, idx, dist, gflags | flags)
    g.close()


def test_driver_manhattan_normalized_csvs(tmp_path, knn, fmt_cout):
    """The drop-in driver in the reference's default configuration under
    Manhattan (--Euclidean_distance false --Normalize true) on a 600 x 6 CSV
    set with --tune u16l1=1: the oracle's labels and accuracy line."""
    import datagen
    spec = dict(kind="gauss", seed=67, N_train=600, N_test=90, N_val=80, dim=6, class_cnt=3)
    cfg = knn.KnnConfig(dim=6, K=5, N_train=600, N_test=90, N_val=80, class_cnt=3,
                        Euclidean_distance=False, Normalize=True, Validation=True)
    sets, _ = datagen.write_csvs(str(tmp_path), spec, names=(
        cfg.train_file_name, cfg.validation_file_name, cfg.test_file_name))
    tr, trl, te, tel, va, val_ = [a.copy() for a in sets]
    oracle.normalize(tr, te, va)
    want = oracle.knn(tr, trl, te, 5, False, 3)[0]
    wval = oracle.knn(tr, trl, va, 5, False, 3)[0]
    line = "accuracy = " + fmt_cout(float((wval == val_).sum()) / len(val_))
    out = knn.run_driver(cfg, str(tmp_path), extra=["--tune", "u16l1=1"])
    labels = np.loadtxt(tmp_path / "Test_label.csv", dtype=np.int64, ndmin=1)
    np.testing.assert_array_equal(labels, want)
    assert line in out
    with pytest.raises(knn.KnnError, match="u16l1"):
        knn.run_driver(cfg, str(tmp_path), extra=["--tune", "u16l1=7"])

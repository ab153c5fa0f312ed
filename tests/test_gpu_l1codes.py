"""GPU parity of candidate path 7: the L1 pass on int8 codes (v_sad_u8,
csrc/knn_cand_sad.hip; tuning key "i8l1") against the CPU oracle -- labels,
neighbour indices, fp64 distance bit patterns and tie flags, as
test_gpu_parity.py compares them.  Every case sets "i8l1" = 1 unless it is
about the plan's own choice, and asserts that path 7 served the call."""
import numpy as np
import pytest

import golden_io
import l1codes
import loo
import oracle

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
    c.set_tuning("i8l1", 1)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    return c


def _check(knn, c, tr, lab, te, k, classes, path=7):
    """One classify against the oracle; returns (labels, idx, dist, flags)."""
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == path
    want, widx, wdist = oracle.knn(tr, lab, te, k, False, classes, n_out=k)
    assert (idx < tr.shape[0]).all() and (idx >= 0).all()
    tie_vote = (flags & knn.FLAG_TIE_VOTE) != 0
    np.testing.assert_array_equal(got[~tie_vote], want[~tie_vote])
    # the tied queries whose label the order could change carry the
    # reference's own order: index for index, hence the same label
    ref = (flags & knn.FLAG_TIE_REF) != 0
    np.testing.assert_array_equal(idx[ref], widx[ref])
    np.testing.assert_array_equal(got, want)
    l1codes.assert_neighbors_match(idx, dist, widx, wdist, flags)
    return got, idx, dist, flags


# ------------------------------------------------------------ 1. shape edges
@pytest.mark.parametrize("d", l1codes.SHAPE_D)
@pytest.mark.parametrize("n", l1codes.SHAPE_N)
def test_shape_edges(knn, n, d):
    """A pad row in the last tile (n = 31, 257, 6000 are no multiple of 32),
    pad dims inside a dword (d = 1, 6, 13) and inside the 32-dim pad (d = 100),
    one sub-tile only (n = 31), every padded width; k = 1, 7, 30 and n - 1."""
    tr, lab, te = l1codes.int_sets(n, l1codes.shape_m(n, d), d)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in sorted(set(k for k in l1codes.K_EDGES + ((n - 1,) if n == 31 else ()) if k < n)):
        _check(knn, c, tr, lab, te, k, 4)
        dp = min(p for p in (32, 64, 96, 128, 160, 192, 256) if p >= d)
        assert c.last_kernel_name().startswith("cand_sad_kernel<%d," % dp)
    c.close()


# -------------------------------- 2. the sign flip and the accumulator's range
@pytest.mark.parametrize("d", [256, 255])
def test_byte_ends(knn, d):
    tr, lab, te = l1codes.byte_ends(d)
    c = _clf(knn)
    c.set_train(tr, lab, 3)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, tr.shape[0] - 1, 3)
    # the one row k = n - 1 leaves out is the farthest: for the query of all 0
    # the row of all 255 and the other way round ...
    assert 1 not in idx[0] and 0 not in idx[1]
    # ... and at k = n it comes last, at the largest distance the accumulator holds
    got, idx, dist, flags = _check(knn, c, tr, lab, te, tr.shape[0], 3)
    assert dist[0, -1] == 255.0 * d and idx[0, -1] == 1
    assert dist[1, -1] == 255.0 * d and idx[1, -1] == 0
    # (k = n - 1 leaves no row outside the lists to bound: such calls finish in
    # the exact rescan on every path; a small k is certified from the proxies,
    # the largest of them included in the thresholds' range)
    _check(knn, c, tr, lab, te, 3, 3)
    c.close()


# ------------------------------------------------ 3. offset and scaled grids
@pytest.mark.parametrize("kind", ["offset", "eighths"])
def test_offset_and_scaled_grids(knn, kind):
    tr, lab, te, s = l1codes.offset_grid(kind)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in (1, 9):
        _check(knn, c, tr, lab, te, k, 4)
    assert c.last_rescan_count() * 16 <= te.shape[0]
    c.close()


# --------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("ties", [1, 2])
def test_ties_on_a_coarse_grid(knn, ties):
    tr, lab, te = l1codes.tie_grid()
    k = l1codes.TIE_K
    c = _clf(knn, ties=ties)
    c.set_train(tr, lab, 3)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, k, 3)
    tied = (flags & 14) != 0
    assert tied.sum() > te.shape[0] // 2
    if ties == 2:
        # every tied query in the reference's own std::sort order
        want, widx, wdist = oracle.knn(tr, lab, te, k, False, 3, n_out=k)
        assert ((flags & knn.FLAG_TIE_REF) != 0).sum() == tied.sum()
        np.testing.assert_array_equal(idx, widx)
    c.close()


@pytest.mark.parametrize("name", ["f10_l1_int", "f6_int_ties"])
def test_int_fixtures_raw_sets_on_the_codes(knn, name):
    """The two integer fixtures' own (unnormalised) byte-valued sets under L1
    through path 7, at the fixture's K, against the oracle."""
    fx = golden_io.Fixture(name)
    s = fx.spec
    tr, trl, te, tel, va, val_ = fx.sets()
    c = _clf(knn, ties=2)
    c.set_train(tr, trl, s["class_cnt"])
    for q in (te, va):
        got, idx, dist, flags = _check(knn, c, tr, trl, q, s["K"], s["class_cnt"])
        want, widx, wdist = oracle.knn(tr, trl, q, s["K"], False, s["class_cnt"], n_out=s["K"])
        np.testing.assert_array_equal(idx, widx)
    c.close()


def test_int_fixture_golden_outputs_with_the_key_on(knn, fmt_cout):
    """f10_l1_int as the reference ran it (Normalize = true) with "i8l1" = 1:
    the golden labels, neighbours and accuracy line.  The reference's min-max
    normalisation takes byte values off every binary grid (x / 255), so
    detect_i8 refuses the set and the call is served by path 1 -- the key
    asks for the pass only where the data allow it."""
    fx = golden_io.Fixture("f10_l1_int")
    s = fx.spec
    tr, trl, te, tel, va, val_ = fx.normalized()
    c = _clf(knn)
    c.set_train(tr, trl, s["class_cnt"])
    K = s["K"]
    got, idx, dist, flags = c.classify(te, K, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 1
    np.testing.assert_array_equal(got, fx.test_labels)
    nq = fx.test_nbr_idx.shape[0]
    l1codes.assert_neighbors_match(idx[:nq], dist[:nq], fx.test_nbr_idx[:nq, :K],
                                   fx.test_nbr_dist[:nq, :K], flags[:nq])
    vl = c.classify(va, K, knn.L1)
    acc = float((vl == val_).sum()) / len(val_)
    assert "accuracy = " + fmt_cout(acc) == str(fx.accuracy_line)
    c.close()


# --------------------------------------- 5. queries the pass must hand over
def test_handover_queries(knn):
    tr, lab, te, off, beyond, nan = l1codes.handover()
    assert l1codes.handover_share() <= 1.0 / 16.0
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    k = 7
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 7
    assert (got[nan] == -1).all() and (flags[nan] & knn.FLAG_NONFINITE).all()
    assert (flags[off] & knn.FLAG_EXACT_RESCAN).all()
    assert (flags[beyond] & knn.FLAG_EXACT_RESCAN).all()
    ok = np.setdiff1d(np.arange(te.shape[0]), nan)
    want, widx, wdist = oracle.knn(tr, lab, te[ok], k, False, 4, n_out=k)
    np.testing.assert_array_equal(got[ok], want)
    l1codes.assert_neighbors_match(idx[ok], dist[ok], widx, wdist, flags[ok])
    # on the grid and in range: served by the pass itself, nearly all certified
    grid = np.setdiff1d(ok, np.concatenate([off, beyond]))
    assert ((flags[grid] & knn.FLAG_EXACT_RESCAN) != 0).sum() * 16 <= len(grid)
    c.close()


# ------------------------------------------------------------------ 6. the plan
def test_plan_choices(knn):
    tr, lab, te = l1codes.int_sets(2000, 64, 128)
    rng = np.random.default_rng(6)
    gauss = np.round(rng.standard_normal((2000, 128)) * 1024) / 1024 + 1e-3 / 3
    wide, _, wide_q = l1codes.int_sets(2000, 64, 300)

    def path(train, q, k=5, prec=None, **tuning):
        c = knn.Classifier(0)
        if prec is not None:
            c.set_precision(prec)
        for key, value in tuning.items():
            c.set_tuning(key, value)
        c.set_train(train, lab, 4)
        c.classify(q, k, knn.L1)
        p, name = c.last_candidate_path(), c.last_kernel_name()
        c.close()
        return p, name

    big = np.tile(te, (64, 1))  # 4096 queries
    # the key at -1 (auto): the pass from 4096 queries on, where the data allow
    p, name = path(tr, big)
    assert p == 7 and name == "cand_sad_kernel<128,8,8>"
    assert path(tr, big[:4095])[0] == 1
    assert path(tr, te)[0] == 1
    assert path(tr, big, i8l1=0)[0] == 1
    assert path(gauss, big[:, :128] + 0.0)[0] == 1
    assert path(wide, np.tile(wide_q, (64, 1)))[0] == 1
    assert path(tr, big, prec=knn.PRECISION_FP32)[0] == 1
    assert path(tr, big, k=100)[0] == 1
    # "i8l1" = 1: at every batch size, where the data allow
    p, name = path(tr, te, i8l1=1)
    assert p == 7 and name == "cand_sad_kernel<128,8,4>"
    p, name = path(tr, big, i8l1=1)
    assert p == 7 and name == "cand_sad_kernel<128,8,8>"
    assert path(gauss, te, i8l1=1)[0] == 1
    assert path(wide, wide_q, i8l1=1)[0] == 1
    # "i8" is the L2 pass only: alone it moves no L1 call (a large batch is
    # AUTO's own choice, with or without it)
    assert path(tr, te, i8=1)[0] == 1
    assert path(tr, big[:4095], i8=1)[0] == 1
    assert path(tr, big, i8=1, i8l1=0)[0] == 1


# ------------------------------------------------------------------- 7. callers
def test_classify_sweep_equals_per_k_calls(knn):
    tr, lab, te = l1codes.int_sets(6000, 150, 32)
    ks = [1, 3, 10]
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    labels, idx, dist, flags = c.classify_sweep(te, ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 7
    for j, k in enumerate(ks):
        got, kidx, kdist, kflags = c.classify(te, k, knn.L1, return_neighbors=True)
        assert c.last_candidate_path() == 7
        np.testing.assert_array_equal(labels[j], got)
        want = oracle.knn(tr, lab, te, k, False, 4)[0]
        np.testing.assert_array_equal(labels[j], want)
    np.testing.assert_array_equal(dist.view(np.int64), kdist.view(np.int64))
    c.close()


def test_loo_sweep_on_600_rows(knn):
    tr, lab = loo.grid(4, 6, 777, 600, 3)
    ks = [1, 3, 10]
    want = loo.expected_excl(tr, lab, tr, np.arange(600), ks, False, 3)
    c = _clf(knn)
    c.set_train(tr, lab, 3)
    labels, correct, idx, dist, flags = c.loo_sweep(ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 7
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(correct, (want["labels"] == lab).sum(axis=1))
    np.testing.assert_array_equal(dist.view(np.int64), want["dist"].view(np.int64))
    c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_group_modes_equal_the_single_classifier(knn, mode):
    if knn.lib().knn_device_count() < 1:
        pytest.fail("no HIP device visible")
    tr, lab, te = l1codes.int_sets(6000, 150, 32)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, 7, 4)
    c.close()
    g = knn.Group([0, 0, 0], mode=mode)
    g.set_tuning("i8l1", 1)
    g.set_train(tr, lab, 4)
    ggot, gidx, gdist, gflags = g.classify(te, 7, knn.L1, return_neighbors=True)
    np.testing.assert_array_equal(ggot, got)
    np.testing.assert_array_equal(gdist.view(np.int64), dist.view(np.int64))
    l1codes.assert_neighbors_match(gidx, gdist, idx, dist, gflags | flags)
    g.close()


def test_driver_manhattan_on_int_csvs(tmp_path, knn, fmt_cout):
    """The drop-in driver with --Euclidean_distance false on a 600 x 6 int CSV
    set, the pass switched on by --tune i8l1=1 and left off: the oracle's
    labels and accuracy line either way."""
    spec = dict(kind="int", seed=66, N_train=600, N_test=90, N_val=80, dim=6, class_cnt=3)
    import datagen
    cfg = knn.KnnConfig(dim=6, K=5, N_train=600, N_test=90, N_val=80, class_cnt=3,
                        Euclidean_distance=False, Normalize=False, Validation=True)
    sets, _ = datagen.write_csvs(str(tmp_path), spec, names=(
        cfg.train_file_name, cfg.validation_file_name, cfg.test_file_name))
    tr, trl, te, tel, va, val_ = sets
    want = oracle.knn(tr, trl, te, 5, False, 3)[0]
    wval = oracle.knn(tr, trl, va, 5, False, 3)[0]
    line = "accuracy = " + fmt_cout(float((wval == val_).sum()) / len(val_))
    for extra in (["--tune", "i8l1=1"], []):
        out = knn.run_driver(cfg, str(tmp_path), extra=extra)
        labels = np.loadtxt(tmp_path / "Test_label.csv", dtype=np.int64, ndmin=1)
        np.testing.assert_array_equal(labels, want)
        assert line in out
    with pytest.raises(knn.KnnError, match="i8l1"):
        knn.run_driver(cfg, str(tmp_path), extra=["--tune", "i8l1=7"])

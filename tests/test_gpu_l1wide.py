"""GPU parity of candidate path 7 above 256 dims: the wide L1 pass on int8
codes (csrc/knn_cand_sad_wide.hip; tuning key "i8l1" = 2) against the CPU
oracle -- labels, neighbour indices, fp64 distance bit patterns and tie flags,
as test_gpu_l1codes.py compares them.  Every case sets "i8l1" = 2 and asserts
that path 7 served the call with the wide kernel where the plan says so."""
import numpy as np
import pytest

import l1codes
import l1wide
import loo
import oracle

pytestmark = pytest.mark.gpu

WIDE = "cand_sad_wide_kernel<"


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
    c.set_tuning("i8l1", 2)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    return c


def _check(knn, c, tr, lab, te, k, classes, path=7, kernel=WIDE):
    """One classify against the oracle; returns (labels, idx, dist, flags)."""
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == path
    assert c.last_kernel_name().startswith(kernel)
    want, widx, wdist = oracle.knn(tr, lab, te, k, False, classes, n_out=k)
    assert (idx < tr.shape[0]).all() and (idx >= 0).all()
    tie_vote = (flags & knn.FLAG_TIE_VOTE) != 0
    np.testing.assert_array_equal(got[~tie_vote], want[~tie_vote])
    ref = (flags & knn.FLAG_TIE_REF) != 0
    np.testing.assert_array_equal(idx[ref], widx[ref])
    np.testing.assert_array_equal(got, want)
    l1codes.assert_neighbors_match(idx, dist, widx, wdist, flags)
    return got, idx, dist, flags


# ------------------------------------------------------------ 1. shape edges
@pytest.mark.parametrize("d", l1wide.SHAPE_D)
@pytest.mark.parametrize("n", l1wide.SHAPE_N)
def test_shape_edges(knn, n, d):
    """One dim into the second 256-dim stretch (257), a partial granule (300,
    1000), pad dims, every chunk count; one sub-tile (n = 31), a pad row in
    the last tile (257), several tiles per split (3000); k = 1, 7, 30, n - 1."""
    tr, lab, te = l1codes.int_sets(n, l1codes.shape_m(n, d), d)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in sorted(set(k for k in l1wide.K_EDGES + ((n - 1,) if n == 31 else ()) if k < n)):
        _check(knn, c, tr, lab, te, k, 4)
    c.close()


# ------------------------------------------------------- 2. chunk boundaries
def test_chunk_boundaries(knn):
    """Only the dims on both sides of every 256-dim boundary and at the row's
    ends carry information: a chunk skipped, read twice or mis-offset changes
    the neighbours."""
    tr, lab, te = l1wide.chunk_boundaries()
    c = _clf(knn, ties=2)
    c.set_train(tr, lab, 4)
    for k in (1, l1wide.BOUNDARY_K, 20):
        _check(knn, c, tr, lab, te, k, 4)
    c.close()


# -------------------------------- 3. the sign flip and the accumulator's range
@pytest.mark.parametrize("d", [1024, 1023])
def test_byte_ends(knn, d):
    tr, lab, te = l1codes.byte_ends(d)
    c = _clf(knn)
    c.set_train(tr, lab, 3)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, tr.shape[0] - 1, 3)
    assert 1 not in idx[0] and 0 not in idx[1]
    # at k = n the farthest row comes last, at the largest distance the
    # accumulator holds: 255 d (261120 at d = 1024)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, tr.shape[0], 3)
    assert dist[0, -1] == 255.0 * d and idx[0, -1] == 1
    assert dist[1, -1] == 255.0 * d and idx[1, -1] == 0
    _check(knn, c, tr, lab, te, 3, 3)
    c.close()


# ------------------------------------------------ 4. offset and scaled grids
@pytest.mark.parametrize("kind", ["offset", "eighths"])
def test_offset_and_scaled_grids(knn, kind):
    tr, lab, te, s = l1wide.offset_grid(kind)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    for k in (1, 9):
        _check(knn, c, tr, lab, te, k, 4)
        assert c.last_rescan_count() * 16 <= te.shape[0]
    c.close()


# --------------------------------------------------------------------- 5. ties
@pytest.mark.parametrize("ties", [1, 2])
def test_ties_on_a_coarse_grid(knn, ties):
    tr, lab, te = l1wide.tie_grid()
    k = l1wide.TIE_K
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


# --------------------------------------- 6. queries the pass must hand over
def test_handover_queries(knn):
    tr, lab, te, off, beyond, nan = l1wide.handover()
    assert l1wide.handover_share() <= 1.0 / 16.0
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    k = 7
    got, idx, dist, flags = c.classify(te, k, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 7
    assert c.last_kernel_name().startswith(WIDE)
    assert (got[nan] == -1).all() and (flags[nan] & knn.FLAG_NONFINITE).all()
    assert (flags[off] & knn.FLAG_EXACT_RESCAN).all()
    assert (flags[beyond] & knn.FLAG_EXACT_RESCAN).all()
    ok = np.setdiff1d(np.arange(te.shape[0]), nan)
    want, widx, wdist = oracle.knn(tr, lab, te[ok], k, False, 4, n_out=k)
    np.testing.assert_array_equal(got[ok], want)
    l1codes.assert_neighbors_match(idx[ok], dist[ok], widx, wdist, flags[ok])
    grid = np.setdiff1d(ok, np.concatenate([off, beyond]))
    assert ((flags[grid] & knn.FLAG_EXACT_RESCAN) != 0).sum() * 16 <= len(grid)
    c.close()


# ------------------------------------------------------------------ 7. the plan
def test_plan_choices(knn):
    wide, lab, wide_q = l1codes.int_sets(2000, 64, 300)
    tr, _, te = l1codes.int_sets(2000, 64, 128)
    wider, _, wider_q = l1codes.int_sets(2000, 64, 1025)
    rng = np.random.default_rng(16)
    gauss = np.round(rng.standard_normal((2000, 300)) * 1024) / 1024 + 1e-3 / 3

    def path(train, q, k=5, prec=None, metric=None, **tuning):
        c = knn.Classifier(0)
        if prec is not None:
            c.set_precision(prec)
        for key, value in tuning.items():
            c.set_tuning(key, value)
        c.set_train(train, lab, 4)
        c.classify(q, k, knn.L1 if metric is None else metric)
        p, name = c.last_candidate_path(), c.last_kernel_name()
        c.close()
        return p, name

    big = np.tile(wide_q, (64, 1))  # 4096 queries
    p, name = path(wide, wide_q, i8l1=2)
    assert p == 7 and name == "cand_sad_wide_kernel<8,4>"
    p, name = path(wide, big, i8l1=2)
    assert p == 7 and name == "cand_sad_wide_kernel<8,8>"
    # at d <= 256 the value plans what 1 plans
    assert path(tr, te, i8l1=2) == path(tr, te, i8l1=1) == (7, "cand_sad_kernel<128,8,4>")
    # beyond 1024 dims, off the grid, under L2: what 0 plans
    assert path(wider, wider_q, i8l1=2) == path(wider, wider_q, i8l1=0)
    assert path(wider, wider_q, i8l1=2)[0] == 1
    assert path(gauss, wide_q + 0.0, i8l1=2) == path(gauss, wide_q + 0.0, i8l1=0)
    assert path(gauss, wide_q + 0.0, i8l1=2)[0] == 1
    assert path(wide, wide_q, metric=knn.L2, i8l1=2) == path(wide, wide_q, metric=knn.L2, i8l1=0)
    assert path(wide, wide_q, metric=knn.L2, i8l1=2)[0] != 7
    # an explicit key wins over the precision, as for 1; k = 100 as 1 decides
    p, name = path(wide, wide_q, prec=knn.PRECISION_FP32, i8l1=2)
    assert p == 7 and name.startswith(WIDE)
    p, name = path(wide, wide_q, k=100, i8l1=2)
    assert p == 7 and name.startswith(WIDE)
    # -1, 0 and 1 keep d = 300 on the fp32 stream kernel
    for v in (-1, 0, 1):
        assert path(wide, big, i8l1=v)[0] == 1
    c = knn.Classifier(0)
    with pytest.raises(knn.KnnError, match="i8l1"):
        c.set_tuning("i8l1", 3)
    c.close()


# ------------------------------------------------------------------- 8. callers
def test_classify_sweep_equals_per_k_calls(knn):
    tr, lab, te = l1codes.int_sets(3000, 150, 300)
    ks = [1, 3, 10]
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    labels, idx, dist, flags = c.classify_sweep(te, ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 7 and c.last_kernel_name().startswith(WIDE)
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
    tr = l1wide.widen(tr, 300)
    ks = [1, 3, 10]
    want = loo.expected_excl(tr, lab, tr, np.arange(600), ks, False, 3)
    c = _clf(knn)
    c.set_train(tr, lab, 3)
    labels, correct, idx, dist, flags = c.loo_sweep(ks, knn.L1, return_neighbors=True)
    assert c.last_candidate_path() == 7 and c.last_kernel_name().startswith(WIDE)
    np.testing.assert_array_equal(labels, want["labels"])
    np.testing.assert_array_equal(correct, (want["labels"] == lab).sum(axis=1))
    np.testing.assert_array_equal(dist.view(np.int64), want["dist"].view(np.int64))
    c.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_group_modes_equal_the_single_classifier(knn, mode):
    tr, lab, te = l1codes.int_sets(3000, 150, 300)
    c = _clf(knn)
    c.set_train(tr, lab, 4)
    got, idx, dist, flags = _check(knn, c, tr, lab, te, 7, 4)
    c.close()
    g = knn.Group([0, 0, 0], mode=mode)
    g.set_tuning("i8l1", 2)
    g.set_train(tr, lab, 4)
    ggot, gidx, gdist, gflags = g.classify(te, 7, knn.L1, return_neighbors=True)
    np.testing.assert_array_equal(ggot, got)
    np.testing.assert_array_equal(gdist.view(np.int64), dist.view(np.int64))
    l1codes.assert_neighbors_match(gidx, gdist, idx, dist, gflags | flags)
    g.close()


def test_driver_manhattan_on_wide_int_csvs(tmp_path, knn, fmt_cout):
    """The drop-in driver with --Euclidean_distance false --Normalize false on
    a 600 x 300 int CSV set, with --tune i8l1=2 and without: the oracle's
    labels and accuracy line either way."""
    spec = dict(kind="int", seed=366, N_train=600, N_test=90, N_val=80, dim=300, class_cnt=3)
    import datagen
    cfg = knn.KnnConfig(dim=300, K=5, N_train=600, N_test=90, N_val=80, class_cnt=3,
                        Euclidean_distance=False, Normalize=False, Validation=True)
    sets, _ = datagen.write_csvs(str(tmp_path), spec, names=(
        cfg.train_file_name, cfg.validation_file_name, cfg.test_file_name))
    tr, trl, te, tel, va, val_ = sets
    want = oracle.knn(tr, trl, te, 5, False, 3)[0]
    wval = oracle.knn(tr, trl, va, 5, False, 3)[0]
    line = "accuracy = " + fmt_cout(float((wval == val_).sum()) / len(val_))
    for extra in (["--tune", "i8l1=2"], []):
        out = knn.run_driver(cfg, str(tmp_path), extra=extra)
        labels = np.loadtxt(tmp_path / "Test_label.csv", dtype=np.int64, ndmin=1)
        np.testing.assert_array_equal(labels, want)
        assert line in out

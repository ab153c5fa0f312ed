"""GPU parity on near-ties at each candidate path's error scale: the check of
the certification bound E, of the re-rank window and of the rescan thresholds
("Certified candidates").

The inputs (tests/neartie.py; shown on the CPU to bite by
test_neartie_data.py) put the reduced-precision proxy order and the exact
order at odds around the k-th place while the oracle's k+1 distances stay
pairwise distinct.  Every case therefore demands, on each of the 11
candidate configurations of test_gpu_parity's `clf`, the oracle's neighbours
index for index, bit-exact distances, the oracle's labels and no tie flag.
A bound, window or rescan threshold that is too optimistic shows up as a
wrong neighbour here and nowhere else in the suite.
"""
import numpy as np
import pytest

import neartie
from test_gpu_parity import assert_neighbors_match, clf, knn, run_case  # noqa: F401

pytestmark = pytest.mark.gpu

TIE_FLAGS = 14  # KNN_FLAG_TIE_BOUNDARY | KNN_FLAG_TIE_VOTE | KNN_FLAG_TIE_ORDER


def run_distinct(c, knn, name):
    """run_case on a named near-tie case; distinct distances must match the
    oracle index for index and must not be flagged as ties or re-ordered."""
    tr, lab, te, info, k, metric = neartie.case(name)
    got, want, flags = run_case(c, knn, tr, lab, te, k, metric, neartie.CLASSES)
    assert ((flags & TIE_FLAGS) == 0).all(), "distinct distances flagged as a tie: queries %s" % (
        np.nonzero(flags & TIE_FLAGS)[0][:10],)
    assert ((flags & knn.FLAG_TIE_REF) == 0).all(), "untied queries re-ordered"
    # (no tie flag: assert_neighbors_match has compared every index, and
    # run_case the label of every query)
    np.testing.assert_array_equal(got, want)
    return flags, info


def assert_uncertifiable(c, knn, flags, info, full):
    """Queries of a cluster of >= 1500 rows with t <= -20: E >= f_err * x2max
    exceeds the cluster's squared diameter by more than 2^20 on every path, so
    more than kMaxUnion = 1024 rows lie inside the re-rank window and more than
    kRescanCap = 1024 within the fp32 rescan filter's reach: a sound bound
    cannot certify them and the fast rescan cannot hold their rows."""
    hard = [i for i, ct in enumerate(info) if ct is not None and ct[0] >= 1500 and ct[1] <= -20]
    assert hard
    assert (flags[hard] & knn.FLAG_EXACT_RESCAN).all(), \
        "certified inside a cluster no bound can resolve: queries %s" % (
            [i for i in hard if not flags[i] & knn.FLAG_EXACT_RESCAN],)
    assert full >= len(hard), "full exact scans %d < %d such queries" % (full, len(hard))


@pytest.mark.parametrize("name", ["A", "C", "D", "E"])
def test_clusters(name, clf, knn):
    """A: d = 64, k = 10, clusters of 40 / 600 / 1500 rows at radii 2^-6 ..
    2^-26 of their distance from the train mean.  C: d = 300 (S3, query-
    resident and stream kernels; the rescan filter reading rows in place).
    D: d = 13 (zero padding).  E: L1 (fp32 VALU path, the x1max bound)."""
    clf.rescan_totals(reset=True)
    flags, info = run_distinct(clf, knn, name)
    failed, full = clf.rescan_totals(reset=True)
    print("case %s: %d of %d queries failed certification, %d finished by the full scan"
          % (name, failed, len(info), full))
    assert_uncertifiable(clf, knn, flags, info, full)


def test_k_beyond_small_clusters(clf, knn):
    """B: case A's data at k = 50: the k-th place falls between a 40-row
    cluster and the bulk, and deep inside the larger clusters."""
    run_distinct(clf, knn, "B")


def test_second_train_set_shifted(clf, knn):
    """F: case A, then through the same context a second train set of the
    same shape with every coordinate shifted by 1000 (stale dxmax, x2max or mu
    of the first set would leave the operands out of range or E too small);
    centring on the column means is what keeps the operands in range."""
    run_distinct(clf, knn, "A")
    run_distinct(clf, knn, "F")


@pytest.mark.parametrize("name", ["G", "H"])
def test_offgrid_all_paths(name, clf, knn):
    """G and H on every configuration: integer codes, queries 2^-12 (G) and
    up to a quarter code (H) off a grid point (the int8 configurations code
    them rounded and measure the error)."""
    run_distinct(clf, knn, name)


@pytest.mark.parametrize("nblk", [-1, 1])
@pytest.mark.parametrize("i8w", [0, 1])
@pytest.mark.parametrize("name", ["G", "H"])
def test_offgrid_int8(knn, name, i8w, nblk):
    """G and H with the int8 pass forced, on 16x16x64 (path 5) and 32x32x32
    (path 6), in train order and on norm-blocked images: the codes' proxies tie exactly
    over whole shells of rows and the order inside a shell, and across the
    k-th place, is decided by the queries' sub-grid offsets alone, which the
    int8 pass sees only as its measured coding error.  In H the offsets
    reach a quarter code: the exact order crosses the shells, and the
    measured coding-error term of E is what keeps window and certification
    sound (G, within the one code unit the bound always allows, passes
    without it).  Either outcome is sound: uncertified queries finished by
    the rescan, or every query certified through a window that holds the
    whole shell."""
    c = knn.Classifier(0)
    c.set_tuning("i8", 1)
    c.set_tuning("i8w", i8w)
    c.set_tuning("nblk", nblk)
    flags, info = run_distinct(c, knn, name)
    assert c.last_candidate_path() == (6 if i8w else 5)
    resc = c.last_rescan_count()
    certified = int(((flags & knn.FLAG_EXACT_RESCAN) == 0).sum())
    print("case %s i8w %d nblk %d: path %d, %d of %d queries certified, %d rescanned"
          % (name, i8w, nblk, c.last_candidate_path(), certified, len(info), resc))
    assert resc > 0 or certified == len(info)
    c.close()


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("prec", ["fp16", "auto"])
def test_clusters_few_splits(knn, prec, S):
    """Case A with 2 and 3 train splits (fp16 forced, and AUTO, which cannot
    take the int8 pass on these data): a lane list then often holds R of a
    query's top W, so near-ties go through the per-split mask and the "kept
    rows within tau" handoff to the rescan."""
    c = knn.Classifier(0)
    c.set_precision(knn.PRECISION_FP16 if prec == "fp16" else knn.PRECISION_AUTO)
    c.set_tuning("S", S)
    c.rescan_totals(reset=True)
    flags, info = run_distinct(c, knn, "A")
    assert c.last_geometry()["splits"] == S
    if prec == "fp16":
        assert c.last_candidate_path() == 4
    else:
        assert c.last_candidate_path() not in (5, 6)
    failed, full = c.rescan_totals(reset=True)
    assert_uncertifiable(c, knn, flags, info, full)
    c.close()

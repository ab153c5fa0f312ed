"""CPU checks of the wide L1-on-int8-codes data (tests/l1wide.py) and of the
pass's exactness claim above 256 dims: the integer sum of absolute code
differences is 2^s times the reference's fp64 L1 distance for every pair, and
its largest value, 255 * 1024, is still an exact float."""
import numpy as np
import pytest

import l1codes
import l1wide
import oracle


@pytest.mark.parametrize("d", [257, 784, 1024])
def test_proxy_model_is_the_reference_distance(d):
    tr, lab, te = l1codes.int_sets(200, 40, d)
    prox = l1codes.proxy_model(tr, te, 0)
    for q in range(te.shape[0]):
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        assert (ref == prox[q].astype(np.float64)).all()
        assert (prox[q].astype(np.float64).view(np.int64) == ref.view(np.int64)).all()


def test_proxy_model_on_a_scaled_grid():
    tr, lab, te, s = l1wide.offset_grid("eighths")
    assert s == 3 and (tr[:, 0] == tr[0, 0]).all()
    assert np.ldexp(tr[:, 299].max() - tr[:, 299].min(), s) == 255.0
    prox = l1codes.proxy_model(tr, te[:8], s)
    for q in range(8):
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        assert (np.ldexp(prox[q].astype(np.float64), -s).view(np.int64) == ref.view(np.int64)).all()


def test_byte_ends_reach_the_accumulator_range():
    tr, lab, te = l1codes.byte_ends(1024)
    assert (tr.min(0) == 0.0).all() and (tr.max(0) == 255.0).all()
    assert l1codes.byte_ends_max(1024) == 261120 == l1wide.WIDE_MAX
    assert np.float32(261120) == 261120 and 261120 < 1 << 24
    assert int(np.float32(261120)) == 261120 and int(np.float32(261119)) == 261119
    assert int(l1codes.proxy_model(tr, te, 0).max()) == 261120
    assert l1codes.byte_ends_max(1023) == 255 * 1023


def test_padding_rule():
    assert [l1wide.pad_dim(d) for d in (256, 257, 272, 300, 784, 1000, 1024, 1025)] == \
        [-1, 272, 272, 304, 784, 1008, 1024, -1]
    for n in l1wide.SHAPE_N:
        for d in l1wide.SHAPE_D:
            assert 40 <= l1codes.shape_m(n, d) <= 200


def test_handover_share_stays_under_the_retirement_rule():
    tr, lab, te, off, beyond, nan = l1wide.handover()
    assert te.shape == (160, 300)
    assert l1wide.handover_share() <= 1.0 / 16.0
    assert tr.min(0).max() == 0.0 and tr.max(0).min() == 255.0
    assert (te[off, l1wide.HANDOVER_OFF_DIM] % 1.0 == 0.5).all()
    assert (te[beyond, l1wide.HANDOVER_BEYOND_DIM] == 300.0).all()
    assert np.isnan(te[nan]).sum() == 1
    rest = np.setdiff1d(np.arange(te.shape[0]), np.concatenate([off, beyond, nan]))
    assert (te[rest] == np.rint(te[rest])).all()
    assert te[rest].min() >= 0 and te[rest].max() <= 255


def test_tie_set_is_tied_at_the_kth_place():
    tr, lab, te = l1wide.tie_grid()
    assert tr.shape == (600, 784)
    varying = np.nonzero(tr.min(0) != tr.max(0))[0]
    assert tuple(varying) == l1wide.TIE_DIMS
    k = l1wide.TIE_K
    want, widx, wdist = oracle.knn(tr, lab, te, k + 1, False, 3, n_out=k + 1)
    # more than half of the queries have equal distances across the k-th place
    assert (wdist[:, k - 1] == wdist[:, k]).mean() > 0.5


def test_every_marked_dim_of_the_boundary_set_decides_neighbours():
    tr, lab, te = l1wide.chunk_boundaries()
    assert tr.shape == (600, l1wide.BOUNDARY_D)
    varying = np.nonzero(tr.min(0) != tr.max(0))[0]
    assert tuple(varying) == l1wide.BOUNDARY_DIMS
    assert (tr[:, varying].min(0) == 0).all() and (tr[:, varying].max(0) == 255).all()
    k = l1wide.BOUNDARY_K
    base = oracle.knn(tr, lab, te, k, False, 4, n_out=k)[1]
    for dim in l1wide.BOUNDARY_DIMS:
        t2, q2 = tr.copy(), te.copy()
        t2[:, dim] = 0.0
        q2[:, dim] = 0.0
        idx = oracle.knn(t2, lab, q2, k, False, 4, n_out=k)[1]
        changed = (np.sort(idx, 1) != np.sort(base, 1)).any(1)
        assert changed.mean() > 0.5, "dim %d decides too few queries' neighbours" % dim

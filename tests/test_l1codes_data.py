"""CPU checks of the L1-on-int8-codes data (tests/l1codes.py) and of the
pass's exactness claim: for a train set on a grid and a query on the same
grid, the integer sum of absolute code differences is 2^s times the
reference's fp64 L1 distance -- for every pair, independent of any kernel."""
import numpy as np
import pytest

import l1codes
import oracle


@pytest.mark.parametrize("d,want", [(256, 65280), (255, 65025)])
def test_byte_ends_reach_the_accumulator_range(d, want):
    tr, lab, te = l1codes.byte_ends(d)
    assert tr.min() == 0.0 and tr.max() == 255.0
    # both ends in every dim, and rows strictly between them
    assert (tr.min(0) == 0.0).all() and (tr.max(0) == 255.0).all()
    assert ((tr > 0) & (tr < 255)).any(1).sum() > 10
    assert l1codes.byte_ends_max(d) == want == 255 * d
    assert want < 1 << 24  # exact as a float
    # the model on flipped unsigned bytes gives the same sums
    assert int(l1codes.proxy_model(tr, te, 0).max()) == want


def test_handover_share_stays_under_the_retirement_rule():
    tr, lab, te, off, beyond, nan = l1codes.handover()
    assert l1codes.handover_share() <= 1.0 / 16.0
    assert tr.min(0).max() == 0.0 and tr.max(0).min() == 255.0
    assert (te[off, 3] % 1.0 == 0.5).all()
    assert (te[beyond, 5] == 300.0).all()
    assert np.isnan(te[nan]).sum() == 1
    rest = np.setdiff1d(np.arange(te.shape[0]), np.concatenate([off, beyond, nan]))
    assert (te[rest] == np.rint(te[rest])).all()
    assert te[rest].min() >= 0 and te[rest].max() <= 255


@pytest.mark.parametrize("kind", ["offset", "eighths"])
def test_proxy_model_is_the_reference_distance(kind):
    """proxy = 2^s x the oracle's L1 distance (the reference's sequential fp64
    sum) for every (query, row) pair of case 3, bit for bit."""
    tr, lab, te, s = l1codes.offset_grid(kind)
    assert (tr[:, 0] == tr[0, 0]).all()                                # a constant dim
    assert np.ldexp(tr[:, 1].max() - tr[:, 1].min(), s) == 255.0       # exactly 255 codes
    assert tr.mean() > 1e5 if kind == "offset" else s == 3
    prox = l1codes.proxy_model(tr, te, s)
    for q in range(te.shape[0]):
        ref = oracle.row_distances(te[q], tr, euclidean=False)
        want = np.ldexp(ref, s)
        assert (want == prox[q].astype(np.float64)).all()
        assert (np.ldexp(prox[q].astype(np.float64), -s).view(np.int64) == ref.view(np.int64)).all()


def test_shape_cases_cover_the_edges():
    for n in l1codes.SHAPE_N:
        for d in l1codes.SHAPE_D:
            assert 40 <= l1codes.shape_m(n, d) <= 200
    tr, lab, te = l1codes.tie_grid()
    assert tr.shape == (600, 6) and tr.min() == 0 and tr.max() == 3
    # dozens of rows share the distance at the k-th place (k = TIE_K) of a
    # typical query, and for most queries the tie runs across that place
    D = np.abs(te[:, None, :] - tr[None, :, :]).sum(2)
    S = np.sort(D, 1)
    k = l1codes.TIE_K
    assert np.median((D == S[:, k - 1:k]).sum(1)) >= 24
    assert (S[:, k - 1] == S[:, k]).mean() > 0.5

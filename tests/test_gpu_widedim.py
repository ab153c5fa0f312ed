"""Parity above 1024 dims: every candidate path, the merge and the rescan
against the CPU oracle at the widths where their behaviour changes
(widedim.py; test_widedim_data.py shows on the CPU that each input bites).

Which construction covers which threshold:
  d > 1024 (fast rescan's query read in place)      near, every width
  d > 1024 (wide L1 code passes hand over)          test_wide_l1_code_keys_hand_over
  DP 2016 / 2048 (wide filter's LDS at 64 KiB)      near + dups at 2016, 2048
  d 4096 / 4097 (merge stages the query / in place) every kind at 4096, 4097;
                                                    test_kmax_single_query (C2 = 1024)
  DP 5088 / 5120 (filter's queries per pass 8 / 4)  near + dups at 5088, 5089, 6000
  no filter at all (DP > 40896)                     test_width_beyond_the_filter
  qres = 1 falls back to S3                         config fp16qres
  S3 / stream chunk counts, err_factor, prep        plain, every width and config
  tie_order, large k, shards, sweeps                the further tests below
Every comparison is exact (run_case's bar); the only counts, failed - full >=
1 and full >= 16, are conditions test_widedim_data.py establishes.
"""
import numpy as np
import pytest

import loo
import oracle
import widedim
from test_gpu_parity import assert_neighbors_match, knn, run_case  # noqa: F401

pytestmark = pytest.mark.gpu

CLASSES = widedim.CLASSES
_ORACLE = {}


def _want(key, tr, lab, te, k, metric, n_out=None):
    """The oracle's (labels, idx, dist), computed once per key and shared."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle.knn(tr, lab, te, k, metric == 0, CLASSES, n_out=n_out or k)
    return _ORACLE[key]


def _classifier(knn, config):
    prec, tune = widedim.CONFIGS[config]
    c = knn.Classifier(0)
    c.set_precision(getattr(knn, "PRECISION_" + prec))
    for key, value in tune.items():
        c.set_tuning(key, value)
    return c


@pytest.fixture(scope="module", params=list(widedim.CONFIGS))
def wclf(knn, request):
    """fp32 (stream kernel), bf16x3 S3, AUTO (fp16 S3), fp16 forced on its
    q16 form, on the 32x32x16 form ("s3q" = 0) and with the query-resident
    kernel requested ("qres" = 1: no instantiation above 960 dims, S3 runs)."""
    c = _classifier(knn, request.param)
    yield request.param, c
    c.close()


def _family(knn, config, c, width, metric):
    S = widedim.SPECIAL
    kinds = ("plain",) if width == widedim.BYTES else widedim.KINDS
    for kind in kinds:
        tr, lab, te, k = widedim.case(width, kind)
        want = _want((width, kind, metric), tr, lab, te, k, metric)
        c.rescan_totals(reset=True)
        got, _, flags = run_case(c, knn, tr, lab, te, k, metric, CLASSES, want=want)
        failed, full = c.rescan_totals(reset=True)
        assert c.last_kernel_name() == widedim.kernel_name(config, metric, tr.shape[0], k), kind
        assert "qres" not in c.last_kernel_name()
        rescanned = (flags & knn.FLAG_EXACT_RESCAN) != 0
        assert 0 <= full <= failed and failed >= rescanned.sum()
        if kind == "plain":
            assert not rescanned.all(), "no query took the certified path"
        elif kind == "near":
            assert rescanned[:S].all()
            assert failed - full >= 1, "the fast rescan finished no query"
        else:
            assert rescanned[:S].all()
            assert full >= S, "more than kRescanCap rows within reach: the full scan must run"


@pytest.mark.parametrize("width", widedim.WIDTHS)
def test_wide_l2(knn, wclf, width):
    config, c = wclf
    _family(knn, config, c, width, 0)


@pytest.mark.parametrize("width", widedim.WIDTHS)
def test_wide_l1(knn, width):
    """L1 runs the fp32 L1 stream kernel in every precision mode."""
    c = _classifier(knn, "fp32")
    _family(knn, "fp32", c, width, 1)
    c.close()


def test_kmax_single_query(knn, wclf):
    """k = n - 1 = 600 at d = 2048, one query: every row re-ranked (C2 = 1024,
    the merge's largest LDS footprint beside a staged query row)."""
    config, c = wclf
    s = widedim.KMAX
    tr, lab, te, _ = widedim.sized(s["d"], s["n"], s["m"], 77)
    for metric in ((0, 1) if config == "fp32" else (0,)):
        want = _want(("kmax", metric), tr, lab, te, s["k"], metric)
        run_case(c, knn, tr, lab, te, s["k"], metric, CLASSES, want=want)
        assert c.last_kernel_name() == widedim.kernel_name(config, metric, s["n"], s["k"])


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", widedim.TIE_WIDTHS)
def test_reference_tie_order(knn, d, metric):
    """"ties" = 2 on byte data with duplicated rows under other labels: labels
    and indices equal the oracle's index for index, KNN_FLAG_TIE_REF on
    every tied query."""
    tr, lab, te = widedim.ties(d)
    c = knn.Classifier(0)
    c.set_tuning("ties", 2)
    c.set_train(tr, lab, CLASSES)
    for k in (1, 10):
        want, widx, wdist = oracle.knn(tr, lab, te, k, metric == 0, CLASSES, n_out=k)
        got, idx, dist, flags = c.classify(te, k, metric, return_neighbors=True)
        tied = (flags & 14) != 0
        assert tied[:widedim.TIE_QUERIES].all()
        assert ((flags & knn.FLAG_TIE_REF) != 0).sum() == tied.sum()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(idx, widx)
        assert (dist.view(np.int64) == wdist.view(np.int64)).all()
    c.close()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [1536, 4097])
def test_large_k_and_partial(knn, d, metric):
    """k = 1200 on n = 1500 (the exact large-k path) and a partial list of
    w = k + 1 entries."""
    import torch
    n, m, k = 1500, 20, 1200
    tr, lab, te, _ = widedim.sized(d, n, m, 300 + d)
    c = knn.Classifier(0)
    want = oracle.knn(tr, lab, te, k, metric == 0, CLASSES, n_out=k + 1)
    run_case(c, knn, tr, lab, te, k, metric, CLASSES,
             want=(want[0], want[1][:, :k].copy(), want[2][:, :k].copy()))
    assert c.last_kernel_name() == "large_k_kernel<%d>" % metric
    dev = torch.device("cuda", 0)
    X, L, Q = (torch.from_numpy(a).to(dev) for a in (tr, lab, te))
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, CLASSES, keep=(X, L))
    w = k + 1
    pd = torch.empty((m, w), dtype=torch.float64, device=dev)
    pi = torch.empty((m, w), dtype=torch.int64, device=dev)
    pl = torch.empty((m, w), dtype=torch.int32, device=dev)
    c.search_partial_device(Q.data_ptr(), m, w, metric, pd.data_ptr(), pi.data_ptr(), pl.data_ptr())
    c.sync()
    assert_neighbors_match(pi.cpu().numpy(), pd.cpu().numpy(), want[1], want[2])
    np.testing.assert_array_equal(pl.cpu().numpy(), lab[pi.cpu().numpy()])
    c.close()


@pytest.mark.parametrize("d", [1536, 5089, 6000])
def test_two_shards_merged(knn, d):
    """Two train shards with idx_offset, merged by merge_vote_device."""
    import torch
    n, m, k = 1402, 33, 10
    half, w = n // 2, k + 1
    tr, lab, te, _ = widedim.sized(d, n, m, 400 + d)
    want, widx, wdist = oracle.knn(tr, lab, te, k, True, CLASSES, n_out=k)
    dev = torch.device("cuda", 0)
    Q = torch.from_numpy(te).to(dev)
    gd = torch.empty((2, m, w), dtype=torch.float64, device=dev)
    gi = torch.empty((2, m, w), dtype=torch.int64, device=dev)
    gl = torch.empty((2, m, w), dtype=torch.int32, device=dev)
    cs = [knn.Classifier(0), knn.Classifier(0)]
    for p, c in enumerate(cs):
        Xs = torch.from_numpy(tr[p * half:(p + 1) * half].copy()).to(dev)
        Ls = torch.from_numpy(lab[p * half:(p + 1) * half].copy()).to(dev)
        c.set_train_device(Xs.data_ptr(), Ls.data_ptr(), half, d, CLASSES, idx_offset=p * half,
                           keep=(Xs, Ls))
        c.search_partial_device(Q.data_ptr(), m, w, knn.L2, gd[p].data_ptr(), gi[p].data_ptr(),
                                gl[p].data_ptr())
        c.sync()
    ol = torch.empty(m, dtype=torch.int32, device=dev)
    oi = torch.empty((m, k), dtype=torch.int64, device=dev)
    od = torch.empty((m, k), dtype=torch.float64, device=dev)
    of = torch.empty(m, dtype=torch.int32, device=dev)
    cs[0].merge_vote_device(gd.data_ptr(), gi.data_ptr(), gl.data_ptr(), 2, m, w, k, ol.data_ptr(),
                            oi.data_ptr(), od.data_ptr(), of.data_ptr())
    cs[0].sync()
    np.testing.assert_array_equal(ol.cpu().numpy(), want)
    assert_neighbors_match(oi.cpu().numpy(), od.cpu().numpy(), widx, wdist, of.cpu().numpy())
    for c in cs:
        c.close()


@pytest.mark.parametrize("d", [1536, 4097, 5089, 6000])
def test_sweeps(knn, d):
    """classify_sweep with truth and loo_sweep at K = 1, 3, 10 against one
    oracle run per K (LOO: on the train set with the row removed)."""
    ks = [1, 3, 10]
    n, m = 301, 33
    tr, lab, te, truth = widedim.sized(d, n, m, 500 + d)
    c = knn.Classifier(0)
    c.set_train(tr, lab, CLASSES)
    for metric in (0, 1):
        want = np.stack([oracle.knn(tr, lab, te, k, metric == 0, CLASSES)[0] for k in ks])
        labels, correct = c.classify_sweep(te, ks, metric, truth=truth)
        np.testing.assert_array_equal(labels, want)
        np.testing.assert_array_equal(correct, (want == truth).sum(axis=1))
    exp = loo.expected_excl(tr, lab, tr, np.arange(n), ks, True, CLASSES)
    labels, correct, idx, dist, flags = c.loo_sweep(ks, knn.L2, return_neighbors=True)
    np.testing.assert_array_equal(labels, exp["labels"])
    np.testing.assert_array_equal(correct, (exp["labels"] == lab).sum(axis=1))
    assert_neighbors_match(idx, dist, exp["idx"], exp["dist"], flags)
    c.close()


@pytest.mark.parametrize("key,value", [("i8l1", 2), ("u16l1w", 1)])
def test_wide_l1_code_keys_hand_over(knn, key, value):
    """At d = 1025 the wide L1 code passes no longer apply: path 1 (the fp32
    L1 stream kernel) runs, on byte data too, and the answer is the oracle's."""
    tr, lab, te = widedim.ties(1025, n=1203, m=33)
    c = knn.Classifier(0)
    c.set_tuning(key, value)
    run_case(c, knn, tr, lab, te, 10, 1, CLASSES)
    assert c.last_candidate_path() == 1
    assert c.last_kernel_name() == widedim.kernel_name("auto", 1, 1203, 10)
    # ... and at 1024 dims the key still selects its pass
    run_case(c, knn, np.ascontiguousarray(tr[:, :1024]), lab, np.ascontiguousarray(te[:, :1024]),
             10, 1, CLASSES)
    assert c.last_candidate_path() == (7 if key == "i8l1" else 8)
    c.close()


@pytest.mark.parametrize("config", ["auto", "fp32"])
def test_one_context_across_widths(knn, config):
    """One context through d = 300, 4097, 1025, 300: the grow-only workspaces
    and the lazily built images follow the width (DPs, fr_q among them); each
    step has uncertifiable queries, so the fast rescan's buffers are used."""
    c = _classifier(knn, config)
    for step, d in enumerate((300, 4097, 1025, 300)):
        tr, lab, te, _ = widedim.sized(d, 1003, 40, 600 + step)
        tr[100:500] = tr[5] + np.random.default_rng(step).standard_normal((400, d)) * 1e-9
        te[:4] = tr[5]
        for metric in (0, 1):
            c.rescan_totals(reset=True)
            _, _, flags = run_case(c, knn, tr, lab, te, 9, metric, CLASSES)
            failed, full = c.rescan_totals(reset=True)
            assert (flags[:4] & knn.FLAG_EXACT_RESCAN).all() and failed - full >= 1
    c.close()


def test_normalize_wide(knn):
    """Classifier.normalize at d = 4097 on three ragged sets: the oracle's bytes."""
    d = 4097
    rng = np.random.default_rng(41)
    sets = [rng.uniform(-3, 7, (r, d)) for r in (257, 33, 1)]
    sets[0][:, 17] = 2.5  # a constant column among the train rows
    ref = [a.copy() for a in sets]
    oracle.normalize(ref[0], ref[1], ref[2])
    c = knn.Classifier(0)
    c.normalize(*sets)
    for a, b in zip(sets, ref):
        assert a.tobytes() == b.tobytes()
    c.close()


@pytest.mark.parametrize("config", ["auto", "fp32"])
def test_width_beyond_the_filter(knn, config):
    """d = 41000 (DP 41024): not even one query row of the wide rescan filter
    fits a CU's LDS, so no filter runs and every uncertified query must take
    the full scan -- also one whose re-ranked rows alone would have satisfied
    the fast finish."""
    d, n, m, k = 41000, 301, 5, 3
    assert widedim.rescan_wide_queries(widedim.pad_fp32(d)) == 0
    tr, lab, te, _ = widedim.sized(d, n, m, 700)
    tr[20:60] = tr[5] + np.random.default_rng(3).standard_normal((40, d)) * 1e-9
    te[:3] = tr[5]
    c = _classifier(knn, config)
    for metric in (0, 1):
        c.rescan_totals(reset=True)
        _, _, flags = run_case(c, knn, tr, lab, te, k, metric, CLASSES)
        failed, full = c.rescan_totals(reset=True)
        assert (flags[:3] & knn.FLAG_EXACT_RESCAN).all()
        assert failed >= 3 and full == failed
    c.close()

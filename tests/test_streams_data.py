"""The properties of tests/streams.py's data sets that test_gpu_streams.py leans
on, checked with the CPU oracle alone (no GPU)."""
import json
import os
import re

import numpy as np
import pytest

import oracle
import streams as st

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _differs(want, poison):
    """Fraction of the entries of `want` that differ from the poison result
    (NaN differs from everything, another NaN included: a NaN poison result is
    compared with finite expected values only)."""
    want = np.asarray(want)
    assert not (want.dtype.kind == "f" and np.isnan(want).any())
    return float(np.mean(want != poison))


def _rows_differ(want, poison_row):
    """Per-class histograms (vote counts, class sums, confusion matrices): a
    class absent from a prefix is a legitimate zero, so the unit is the row /
    the matrix, which differs from the poison result if any cell does."""
    want = np.asarray(want)
    return float(np.mean((want.reshape(want.shape[0], -1) != poison_row).any(axis=1)))


def _kpos(ks):
    """Rows of a K list with K > 0.  K = 0 gives -1 / zero counts by definition
    for every input, poisoned or not: those rows are guarded by the output
    sentinels alone."""
    return [i for i, k in enumerate(ks) if k > 0]


@pytest.mark.parametrize("metric", [0, 1])
def test_tie_set_ties_across_k_boundaries(metric):
    s = st.tie_set(metric)
    kmax = max(st.KS_SWEEP)
    _, idx, dist = oracle.knn(s["tr"], s["lab"], s["q"], kmax, metric == 0, s["classes"],
                              n_out=kmax + 1)
    lrow = s["lab"][idx]
    for k in sorted(set(k for k in st.KS_SWEEP if k > 0)):
        across = (dist[:, k - 1] == dist[:, k]) & (lrow[:, k - 1] != lrow[:, k])
        assert across.sum() > 20, "K = %d: %d queries with a tie across the boundary" % (
            k, across.sum())
    inside = ((dist[:, 1:kmax] == dist[:, :kmax - 1]) & (lrow[:, 1:kmax] != lrow[:, :kmax - 1]))
    assert inside.any(axis=1).mean() > 0.9


@pytest.mark.parametrize("name", ["dup_gauss", "dup_int"])
def test_duplicate_sets_force_the_rescan(name):
    s = st.dataset(name)
    same = (s["tr"] == s["q"][0]).all(axis=1).sum()
    assert same > st.DUP_ROWS > st.DUP_K  # more identical nearest rows than any list holds
    assert (s["q"][:st.DUP_QUERIES] == s["q"][0]).all()
    _, _, dist = st.expected_knn(name, st.L2, st.DUP_K)
    assert (dist[:st.DUP_QUERIES] == 0).all()


@pytest.mark.parametrize("name", sorted(st.SETS))
def test_grid_criterion(name):
    s = st.dataset(name)
    on = st.on_byte_grid(np.concatenate([s["tr"], s["q"]]))
    assert on == (s["kind"] == "int"), name
    n, m = s["tr"].shape[0], s["q"].shape[0]
    assert n <= 4100 and m <= 512 and n % 32 and m % 16  # small and ragged


def test_tie_set_is_small_and_ragged():
    s = st.tie_set(0)
    assert s["tr"].shape[0] == st.TIE_N <= 4100 and s["q"].shape[0] == st.TIE_M <= 512
    assert st.TIE_SHARDS[0][0] == 0 and st.TIE_SHARDS[-1][1] == st.TIE_N
    assert st.SYN_M <= 512 and st.SYN_M % 64


def test_k_lists():
    assert len(st.KS_A) == 3 and len(st.KS_B) == 5
    assert all(a != b for a, b in zip(st.KS_A, st.KS_B)), "the lists differ in every position"
    assert max(st.KS_B) > max(st.KS_A)
    for ks in (st.KS_SWEEP,) + tuple(st.SYN_KS.values()):  # a 0, a duplicate and kmax
        assert 0 in ks and len(set(ks)) < len(ks)
    assert 0 in st.KS_SWEEP and st.KS_SWEEP.count(5) == 2
    assert max(st.SYN_KS[600]) == 600 > 512  # crosses wvote_sweep_kernel's LDS chunk


# ---- poison: a NaN query gives label -1, idx -1, dist NaN, no flags but
# KNN_FLAG_NONFINITE; idx -1 rows never vote (label -1, zero counts / sums);
# truth -1 is never correct and always unlabelled
@pytest.mark.parametrize("name,metric,k", [("gauss128", 0, 10), ("noisy8", 0, 10),
                                           ("noisy8", 1, 3), ("noisy8", 0, 7),
                                           ("largek", 0, 1100)] +
                         [(v[0], v[1], st.PATH_K) for v in st.PATHS.values()] +
                         [(v[0], v[1], st.DUP_K) for v in st.RESCANS.values()])
def test_poison_differs_classify(name, metric, k):
    lab, idx, dist = st.expected_knn(name, metric, k)
    assert _differs(lab, -1) >= 0.99 and _differs(idx, -1) >= 0.99
    assert np.isfinite(dist).all()  # (the poison result is NaN)
    if name == "noisy8" and metric == 0:
        wtd = st.expected_weighted(name, metric, k)
        assert _differs(wtd, -1) >= 0.99
        assert (wtd != lab).any(), "the weighted and the uniform vote are told apart"
        # no exact ties: the rows the call reports are the oracle's in every tie mode
        assert (dist[:, 1:] > dist[:, :-1]).all()


def _check_scored(want, ks, m):
    kp = _kpos(ks)
    assert _differs(want["labels"][kp], -1) >= 0.99
    assert _differs(want["correct"][kp], 0) >= 0.99
    assert _differs(want["unl"][kp], m) >= 0.99
    assert _rows_differ(want["conf"][kp], 0) >= 0.99
    assert _differs(want["idx"], -1) >= 0.99 and np.isfinite(want["dist"]).all()


@pytest.mark.parametrize("metric", [0, 1])
def test_poison_differs_sweeps(metric):
    name = "ties%d" % metric
    _check_scored(st.expected_sweep(name, metric, st.KS_SWEEP), st.KS_SWEEP, st.TIE_M)
    _check_scored(st.expected_excl(metric, st.KS_SWEEP), st.KS_SWEEP, st.TIE_M)
    r0, r1 = st.LOO_ROWS
    _check_scored(st.expected_loo(name, metric, st.KS_SWEEP, r0, r1), st.KS_SWEEP, r1 - r0)
    # the exclusions matter: they change the label of some query at some K
    plain = st.expected_sweep(name, metric, st.KS_SWEEP)["labels"]
    assert (plain != st.expected_excl(metric, st.KS_SWEEP)["labels"]).any()


def test_poison_differs_sequence():
    m = st.dataset("noisy8")["q"].shape[0]
    for ks in (st.KS_A, st.KS_B):
        _check_scored(st.expected_sweep("noisy8", 0, ks), ks, m)
    _check_scored(st.expected_loo("noisy8", 0, st.KS_A, 10, 50), st.KS_A, 40)
    # the two lists give different label arrays position by position
    a = st.expected_sweep("noisy8", 0, st.KS_A)["labels"]
    b = st.expected_sweep("noisy8", 0, st.KS_B)["labels"]
    assert all((a[i] != b[i]).any() for i in range(3))
    # and the sequence's classify calls differ from one another
    l7, l3 = st.expected_knn("noisy8", 0, 7)[0], st.expected_knn("noisy8", 1, 3)[0]
    assert (l7 != l3).any() and (l7 != st.expected_weighted("noisy8", 0, 7)).any()


@pytest.mark.parametrize("kmax", sorted(st.SYN_KS))
def test_poison_differs_synthetic(kmax):
    s = st.synthetic(kmax)
    kp = _kpos(s["ks"])
    for key in ("uniform", "weighted"):
        assert _differs(s[key][kp], -1) >= 0.99
        assert _differs(s[key + "_correct"][kp], 0) >= 0.99
    assert _rows_differ(s["counts"], 0) >= 0.99 and _rows_differ(s["sums"], 0.0) >= 0.99
    assert (s["uniform"] != s["weighted"]).mean() > 0.01  # the two votes are told apart
    for C in st.COUNTS_CS:
        c = st.synthetic(65, C)
        assert _rows_differ(c["counts"], 0) >= 0.99
        assert C == 3 or c["lab"].max() > C - 16  # labels over the whole class range


@pytest.mark.parametrize("C", st.CONFUSION_CS)
def test_poison_differs_confusion(C):
    c = st.confusion_case(C)
    assert _rows_differ(c["conf"], 0) >= 0.99 and _differs(c["unl"], st.SYN_M) >= 0.99
    assert (c["unl"] > 0).all() and c["conf"].sum() + c["unl"].sum() == 3 * st.SYN_M


def test_poison_differs_normalize():
    n = st.normalize_case()
    # NaN rows lose every compare: the bounds stay at -1 / 999999
    assert _differs(n["mx"], -1.0) >= 0.99 and _differs(n["mn"], 999999.0) >= 0.99
    assert np.isfinite(n["want1"]).all()
    # bounds of 0.0 leave the rows untouched (max - min == 0)
    assert _differs(n["want1"], n["x1"]) >= 0.99  # (one constant dimension of 137)
    assert (n["want1"][:, 0] == 2.5).all()


def test_paths_name_every_parent_family():
    """Part B's patterns name every cand_* kernel family of plan_parent.json."""
    with open(os.path.join(HERE, "plan_parent.json")) as f:
        parent = json.load(f)
    fams = {st.kernel_family(c["kernel"]) for c in parent["cases"].values()}
    assert fams and fams <= set(st.KERNEL_FAMILIES)
    named = {st.kernel_family(v[5]) for v in list(st.PATHS.values()) + list(st.RESCANS.values())}
    assert fams <= named and named == set(st.KERNEL_FAMILIES)


def test_entry_point_table_is_complete():
    """Every function of knn_amd.h with a `void* stream` parameter is in the
    entry point -> test table of test_gpu_streams.py, with a test that exists."""
    with open(os.path.join(ROOT, "include", "knn_amd.h")) as f:
        names = st.stream_entry_points(f.read())
    assert len(names) == 17 and all(n.endswith("_device") for n in names)
    with open(os.path.join(HERE, "test_gpu_streams.py")) as f:
        text = f.read()
    doc = text.split('"""')[1]
    tests = set(re.findall(r"^def (test_\w+)", text, flags=re.M))
    for n in names:
        m = re.search(r"^\s*%s\s+(test_\w+)" % re.escape(n), doc, flags=re.M)
        assert m, "%s is missing from the table" % n
        assert m.group(1) in tests, "%s -> %s: no such test" % (n, m.group(1))
    assert "xfail" not in text.split('"""', 2)[2] and "skip" not in text.split('"""', 2)[2]

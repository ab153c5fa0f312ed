"""The edges the three device forms of the K sweep share: knn_classify_sweep_device
(plain), knn_classify_sweep_excl_device (d_excl) and knn_classify_sweep_gexcl_device
(d_qgroup) check their arguments in the same order, leave through the same
early exits and, on the same rows, return what classify_sweep, loo_sweep and
lgo_sweep return.

n = 200 train rows at d = 8 in 3 classes, groups of 4 consecutive rows (gmax =
4); the m = 5 queries are train rows 6..10 (two groups), each excluding itself
(d_excl) or its own group (d_qgroup).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, CLASSES, M, GMAX, ROW0 = 200, 8, 3, 5, 4, 6
FORMS = ["plain", "excl", "gexcl"]
BOUND = {"plain": N, "excl": N - 1, "gexcl": N - GMAX}


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


def _data():
    rng = np.random.default_rng(2024)
    lab = rng.integers(0, CLASSES, N).astype(np.int32)
    tr = rng.uniform(-1, 1, (CLASSES, D))[lab] + 0.5 * rng.standard_normal((N, D))
    return np.ascontiguousarray(tr), lab, (np.arange(N) // GMAX).astype(np.int32)


@pytest.fixture(scope="module")
def env(knn):
    """The trained context with groups and the queries' device arrays."""
    import torch
    tr, lab, grp = _data()
    c = knn.Classifier(0)
    c.set_train(tr, lab, CLASSES)
    c.set_groups(grp)
    dev = torch.device("cuda", 0)
    rows = np.arange(ROW0, ROW0 + M)
    e = {"c": c, "tr": tr, "lab": lab, "grp": grp, "dev": dev,
         "Q": torch.from_numpy(tr[rows]).to(dev),
         "T": torch.from_numpy(lab[rows]).to(dev),
         "E": torch.from_numpy(rows.astype(np.int64)).to(dev),
         "G": torch.from_numpy(grp[rows]).to(dev)}
    torch.cuda.synchronize(dev)
    yield e
    c.close()


def _call(knn, e, form, ks, m=M, labels=True, truth=False, correct=False, c=None, excl=True):
    """One device call of `form` into fresh torch buffers prefilled with -7 ->
    (rc, last error, labels, correct, idx, dist, flags).  excl=False passes a
    null d_excl / d_qgroup."""
    import torch
    L = knn.lib()
    c = c or e["c"]
    ks = np.ascontiguousarray(ks, dtype=np.int32)
    nk, kmax = len(ks), max(int(ks.max()), 1)
    dev = e["dev"]
    dL = torch.full((nk, M), -7, dtype=torch.int32, device=dev)
    dC = torch.full((nk,), -7, dtype=torch.int64, device=dev)
    dI = torch.full((M, kmax), -7, dtype=torch.int64, device=dev)
    dD = torch.zeros((M, kmax), dtype=torch.float64, device=dev)
    dF = torch.full((M,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # the context's stream is not torch's
    head = (c.handle, e["Q"].data_ptr(), m)
    tail = (ks.ctypes.data, nk, knn.L2, dL.data_ptr() if labels else None,
            e["T"].data_ptr() if truth else None, dC.data_ptr() if correct else None,
            dI.data_ptr(), dD.data_ptr(), dF.data_ptr(), None)
    if form == "plain":
        rc = L.knn_classify_sweep_device(*head, *tail)
    elif form == "excl":
        rc = L.knn_classify_sweep_excl_device(*head, e["E"].data_ptr() if excl else None, *tail)
    else:
        rc = L.knn_classify_sweep_gexcl_device(*head, e["G"].data_ptr() if excl else None, *tail)
    err = L.knn_last_error().decode()
    c.sync()
    return (rc, err, dL.cpu().numpy(), dC.cpu().numpy(), dI.cpu().numpy(), dD.cpu().numpy(),
            dF.cpu().numpy())


@pytest.mark.parametrize("form", FORMS)
def test_empty_batch(knn, env, form):
    """m == 0 is served, and the correct counts are zeroed all the same."""
    rc, _, labels, correct, *_ = _call(knn, env, form, [3, 1], m=0, truth=True, correct=True)
    assert rc == 0
    np.testing.assert_array_equal(correct, 0)
    np.testing.assert_array_equal(labels, -7)


@pytest.mark.parametrize("form", FORMS)
def test_all_zero_ks(knn, env, form):
    rc, _, labels, _, _, _, flags = _call(knn, env, form, [0, 0])
    assert rc == 0
    np.testing.assert_array_equal(labels, -1)
    np.testing.assert_array_equal(flags, 0)


@pytest.mark.parametrize("form", FORMS)
def test_null_labels(knn, env, form):
    rc, err, *_ = _call(knn, env, form, [3, 1], labels=False)
    assert rc == -1 and "null labels output" in err


@pytest.mark.parametrize("form", FORMS)
def test_truth_without_correct(knn, env, form):
    rc, err, *_ = _call(knn, env, form, [3, 1], truth=True)
    assert rc == -1 and "go together" in err


@pytest.mark.parametrize("form", FORMS)
def test_ks_bound(knn, env, form):
    """K up to the rows left to vote over (n, n - 1, n - gmax); one more is
    refused naming the entry."""
    b = BOUND[form]
    rc, err, *_ = _call(knn, env, form, [1, b + 1])
    assert rc == -1 and "ks[1] = %d" % (b + 1) in err
    rc, err, labels, *_ = _call(knn, env, form, [1, b])
    assert rc == 0, err
    assert ((labels >= 0) & (labels < CLASSES)).all()


def test_grouped_needs_groups(knn, env):
    """Before knn_set_groups the grouped form is a state error; a null d_qgroup
    is the plain sweep and asks for no groups."""
    c = knn.Classifier(0)
    c.set_train(env["tr"], env["lab"], CLASSES)
    rc, err, *_ = _call(knn, env, "gexcl", [3, 1], c=c)
    assert rc == -3 and "knn_set_groups" in err
    want = _call(knn, env, "plain", [3, 1], c=c)[2]
    for form in ("excl", "gexcl"):
        rc, err, labels, *_ = _call(knn, env, form, [3, 1], c=c, excl=False)
        assert rc == 0, err
        np.testing.assert_array_equal(labels, want)
    c.close()


@pytest.mark.parametrize("form", FORMS)
def test_same_as_python_api(knn, env, form):
    """Labels, correct counts, idx and dist of the device form on rows 6..10
    against classify_sweep / loo_sweep / lgo_sweep on the same rows."""
    c, ks = env["c"], [3, 1, 7]
    r = slice(ROW0, ROW0 + M)
    if form == "plain":
        wl, wi, wd, _ = c.classify_sweep(env["tr"][r], ks, knn.L2, return_neighbors=True)
    elif form == "excl":
        wl, _, wi, wd, _ = c.loo_sweep(ks, knn.L2, return_neighbors=True)
        wl, wi, wd = wl[:, r], wi[r], wd[r]
    else:
        wl, _, wi, wd, _ = c.lgo_sweep(ks, knn.L2, return_neighbors=True)
        wl, wi, wd = wl[:, r], wi[r], wd[r]
    rc, err, labels, correct, idx, dist, _ = _call(knn, env, form, ks, truth=True, correct=True)
    assert rc == 0, err
    np.testing.assert_array_equal(labels, wl)
    np.testing.assert_array_equal(correct, (wl == env["lab"][r]).sum(axis=1))
    np.testing.assert_array_equal(idx, wi)
    np.testing.assert_array_equal(dist.view(np.int64), np.ascontiguousarray(wd).view(np.int64))
    if form == "excl":
        assert (idx != np.arange(ROW0, ROW0 + M)[:, None]).all()
    if form == "gexcl":
        assert (env["grp"][idx] != env["grp"][r][:, None]).all()

"""Stream order of the two device calls of the sweep under group exclusion,
by the protocol of test_gpu_streams.py (its held_run: a held caller stream S,
poisoned inputs that a copy on S replaces, sentinel outputs that a copy on S
reads, a canary on the context's own and the default stream).  Results are
complete only after S is synchronised, and nothing of a call may run on
another stream or wait for the device.  Expected values are the CPU oracle's
on the group-removed train sets (tests/lgo.py).

Entry point -> test (the stream-taking functions of knn_amd.h that the table of
test_gpu_streams.py does not hold; test_lgo_abi.py checks that the two tables
together hold every one):

    knn_classify_sweep_gexcl_device test_group_sweep_held
    knn_lgo_sweep_device            test_group_sweep_held
"""
import numpy as np
import pytest

import lgo
import streams as st
from test_gpu_streams import _check_rows, _classifier, finish, held_run

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


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


@pytest.mark.parametrize("entry", ["gexcl", "lgo"])
def test_group_sweep_held(knn, dev, entry):
    """The sweeps under group exclusion on the tie set, train rows in groups
    of three (row // 3): the K list's upload, the leave-group-out batch's
    group ids, the search at kmax + gmax, the drop kernel, the sweep tie scan,
    the reference-order pass over the remaining records and the prefix votes,
    all on S.  At "ties" = 2 the indices are the oracle's."""
    import torch
    metric = 0
    s = st.tie_set(metric)
    ks = st.KS_SWEEP
    nk, kmax = len(ks), max(ks)
    groups = (np.arange(st.TIE_N) // 3).astype(np.int32)
    r0, r1 = st.LOO_ROWS
    if entry == "lgo":
        Qh, qg, truth = s["tr"][r0:r1], groups[r0:r1], s["lab"][r0:r1]
    else:  # the group of one of the query's nearest rows (every fifth: none)
        ex = st.exclusions(metric)
        Qh, qg, truth = s["q"], np.where(ex >= 0, ex // 3, -1).astype(np.int32), s["truth"]
    m = Qh.shape[0]
    c = _classifier(knn, s, tuning={"ties": 2})
    c.set_groups(groups)
    assert c.group_max() == 3
    b = st.Poisoned(dev)
    Q = b.inp(Qh, "query") if entry == "gexcl" else None
    G = b.inp(qg, "label") if entry == "gexcl" else None  # (poison -1: nothing excluded)
    T = b.inp(truth, "truth") if entry == "gexcl" else None
    ol = b.out((nk, m), torch.int32)
    oc = b.out((nk,), torch.int64)
    oi = b.out((m, kmax), torch.int64)
    od = b.out((m, kmax), torch.float64)
    of = b.out((m,), torch.int32)

    def call(stream):
        k_list = list(ks)  # a temporary: nothing may read the host list after the call
        if entry == "lgo":
            c.lgo_sweep_device(r0, m, k_list, metric, ol.data_ptr(), oc.data_ptr(), oi.data_ptr(),
                               od.data_ptr(), of.data_ptr(), stream=stream)
        else:
            c.classify_sweep_gexcl_device(Q.data_ptr(), m, G.data_ptr(), k_list, metric,
                                          ol.data_ptr(), T.data_ptr(), oc.data_ptr(),
                                          oi.data_ptr(), od.data_ptr(), of.data_ptr(),
                                          stream=stream)

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    want = lgo.expected_gexcl(s["tr"], s["lab"], groups, Qh, qg, list(ks), True, s["classes"])
    plain = lgo.expected_gexcl(s["tr"], s["lab"], groups, Qh, np.full(m, -1), list(ks), True,
                               s["classes"])
    assert (want["labels"] != plain["labels"]).any(), "the exclusions matter"
    np.testing.assert_array_equal(b.result(ol), want["labels"])
    np.testing.assert_array_equal(b.result(oc), (want["labels"] == truth).sum(axis=1))
    _check_rows(knn, None, b.result(oi), b.result(od), b.result(of),
                (None, want["idx"], want["dist"]), ties2=True)
    finish(dev, [c])

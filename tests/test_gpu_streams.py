"""Stream order of every `*_device` entry point: each call is made on a HELD
caller stream S -- a fresh non-blocking stream, ordered with neither the
context's own stream nor the legacy default stream -- with poisoned inputs that
a copy on S replaces and sentinel outputs that a copy on S reads (protocol and
data: tests/streams.py).  A missing piece of a call, shared state that is not
stream-ordered or a call that waits for the device fails a test here.  So does
a piece that runs on the context's own stream or the default stream, because
every run on a caller stream carries a canary on those streams and counts only
if the canary overtook S (st.Canary: two streams that the runtime placed on
one hardware queue execute in submission order, and a run in which they did
is repeated on another stream).  Expected values are the CPU oracle's.

Entry point -> test (every function of knn_amd.h with a `void* stream`):

    knn_classify_device             test_classify_held
    knn_classify_sweep_device       test_sweep_held
    knn_classify_sweep_excl_device  test_sweep_held
    knn_loo_sweep_device            test_sweep_held
    knn_classify_sweep_eval_device  test_sweep_held
    knn_loo_sweep_eval_device       test_sweep_held
    knn_vote_sweep_device           test_vote_blocks_held
    knn_vote_sweep_weighted_device  test_vote_blocks_held
    knn_vote_weights_device         test_vote_blocks_held
    knn_vote_counts_device          test_vote_counts_held
    knn_confusion_device            test_confusion_held
    knn_search_partial_device       test_partial_merge_resolve_held
    knn_merge_vote_device           test_partial_merge_resolve_held
    knn_shard_distances_device      test_partial_merge_resolve_held
    knn_tie_resolve_device          test_partial_merge_resolve_held
    knn_minmax_device               test_minmax_normalize_held
    knn_normalize_device            test_minmax_normalize_held

Part B (test_candidate_paths_held, test_rescan_paths_held) runs every candidate
path under knn_classify_device, part C (test_back_to_back) a sequence of calls
that share the context's workspaces, part D (test_hip_ties_held_stream)
knn_dist.HipTies under a non-default current stream.
"""
import re

import numpy as np
import pytest

import oracle
import streams as st
from test_gpu_normalize import _same_bits
from test_gpu_parity import assert_neighbors_match
from test_gpu_sharded import hip_ties_case

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


def _ptr(t):
    return None if t is None else t.data_ptr()


RETRIES = {"runs": 0, "ordered": 0}  # held runs, and those repeated for an ordered canary


def held_run(dev, ctxs, bufs, call, default_hold=False, check=None, tries=6):
    """Warm-up of the identical call on the context's own stream (workspaces
    are grow-only and hipFree waits for the device, images are built lazily
    with a host wait: either would end the hold), everything back to poison /
    sentinel, then the call on the held stream.  With a caller stream the run
    carries st.Canary: a run in which a canary was ordered behind S could not
    have shown a launch misplaced on that canary's stream, so the run is
    repeated on the next fresh stream until one run shows every other stream
    overtaking S.  With `check` (several contexts: more streams than hardware
    queues, one of them always shares S's) every run is checked, and the runs
    go on until each stream has overtaken S in one of them.  The test fails if
    that does not happen.  Returns (still_held, keep)."""
    import torch
    bufs.produce()
    torch.cuda.synchronize(dev)
    call(None)
    for c in ctxs:
        c.sync()
    torch.cuda.synchronize(dev)
    if default_hold:  # the call runs on the context's own stream: nothing to overtake
        bufs.reset()
        S, keep = st.hold_on_default(dev)
        return st.run_on_stream(S, bufs.produce, call, bufs.consume), keep
    canary = st.Canary(dev, ctxs)

    def produce():
        bufs.produce()
        canary.produce()

    def canary_then_call(stream):
        canary.launch()
        call(stream)

    seen = [False] * (len(ctxs) + 1)
    for _ in range(tries):
        bufs.reset()
        canary.reset()
        S, keep = st.held_stream(dev)
        held = st.run_on_stream(S, produce, canary_then_call, bufs.consume)
        for c in ctxs:
            c.sync()
        torch.cuda.synchronize(dev)
        RETRIES["runs"] += 1
        over = canary.overtook()
        if check is not None:
            assert held, st.HOLD_MSG
            check()
            seen = [a or b for a, b in zip(seen, over)]
        if all(over) or all(seen):
            return held, keep
        RETRIES["ordered"] += 1
    pytest.fail("in %d runs the context's own stream or the default stream never ran ahead of "
                "the held caller stream: a misplaced launch could not be told apart" % tries)


def finish(dev, ctxs):
    """After the comparison: everything drained before anything is freed."""
    import torch
    for c in ctxs:
        c.sync()
    torch.cuda.synchronize(dev)
    for c in ctxs:
        c.close()


def _classifier(knn, s, precision=st.AUTO, tuning=None, vote=None):
    c = knn.Classifier(0)
    c.set_precision(precision)
    for key, value in (tuning or {}).items():
        c.set_tuning(key, value)
    c.set_train(s["tr"], s["lab"], s["classes"])
    if vote is not None:
        c.set_vote(vote)
    return c


def _check_rows(knn, got, idx, dist, flags, want, ties2=False):
    wlab, widx, wdist = want
    assert not (flags == st.SENTINEL).any(), "flags left at the sentinel"
    assert not (flags & knn.FLAG_NONFINITE).any(), "poisoned (NaN) queries were read"
    if got is not None:
        np.testing.assert_array_equal(got, wlab)
    if ties2:
        np.testing.assert_array_equal(idx, widx)
        np.testing.assert_array_equal(dist.view(np.int64), np.asarray(wdist).view(np.int64))
    else:
        assert_neighbors_match(idx, dist, np.asarray(widx), np.asarray(wdist), flags)


def _classify_held(knn, dev, name, metric, k, precision=st.AUTO, tuning=None, vote=None,
                   rows=True, timing=False):
    """One knn_classify_device on the held stream; returns (context, labels,
    idx, dist, flags) with the context still open (finish() closes it)."""
    import torch
    s = st.any_set(name)
    m = s["q"].shape[0]
    c = _classifier(knn, s, precision, tuning, vote)
    if timing:
        c.set_timing(True)
    b = st.Poisoned(dev)
    Q = b.inp(s["q"], "query")
    ol = b.out((m,), torch.int32)
    of = b.out((m,), torch.int32)
    oi = b.out((m, max(k, 1)), torch.int64) if rows else None
    od = b.out((m, max(k, 1)), torch.float64) if rows else None

    def call(stream):
        c.classify_device(Q.data_ptr(), m, k, metric, ol.data_ptr(), _ptr(oi), _ptr(od),
                          of.data_ptr(), stream=stream)

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    out = (b.result(ol), b.result(oi)[:, :k] if rows else None,
           b.result(od)[:, :k] if rows else None, b.result(of))
    return (c,) + out


class MergeOnHeldStream:
    """hip_ties_case's hooks: the merge reads poisoned lists (no neighbour
    anywhere) that copies on a held stream S replace, its outputs start at the
    sentinel, and S is the current stream from the merge to the read-back."""

    def begin(self, dev, lists, outs):
        import torch
        self.real = lists
        self.live = [torch.full_like(t, p) for t, p in
                     zip(lists, (st.POISON["dist"], st.POISON["idx"], st.POISON["label"]))]
        for t in outs:
            t.fill_(st.SENTINEL)
        self.S, self.keep = st.held_stream(dev)
        self.scope = torch.cuda.stream(self.S)
        self.scope.__enter__()
        for live, real in zip(self.live, self.real):
            live.copy_(real, non_blocking=True)
        return self.live

    def merged(self):
        self.still_held = not self.S.query()

    def end(self, ties):
        assert ties.stream == self.S.cuda_stream != 0
        self.S.synchronize()

    def close(self):
        self.scope.__exit__(None, None, None)


# ------------------------------------------------- A. one call per entry point
@pytest.mark.parametrize("case", ["k0", "k10", "k10-norows", "weighted", "weighted-norows",
                                  "timed", "k1100"])
def test_classify_held(knn, dev, case):
    """knn_classify_device: the fill kernels (k = 0), the search, the large-k
    path, the weighted vote over caller rows and over the context's own
    (sw_idx / sw_dist / sw_ks), and the five timing events with the
    hipExtLaunchKernelGGL start / stop pair."""
    vote = knn.VOTE_DISTANCE if case.startswith("weighted") else None
    name, k = (("largek", 1100) if case == "k1100" else ("noisy8", 10) if vote
               else ("gauss128", 0 if case == "k0" else 10))
    rows = not case.endswith("norows")
    c, got, idx, dist, flags = _classify_held(knn, dev, name, st.L2, k, vote=vote, rows=rows,
                                              timing=case == "timed")
    if k == 0:
        np.testing.assert_array_equal(got, np.full_like(got, -1))
        np.testing.assert_array_equal(flags, np.zeros_like(flags))
    else:
        want = st.expected_knn(name, st.L2, k)
        np.testing.assert_array_equal(
            got, st.expected_weighted(name, st.L2, k) if vote else want[0])
        if rows:
            _check_rows(knn, None, idx, dist, flags, want)
        assert not (flags & knn.FLAG_NONFINITE).any() and not (flags == st.SENTINEL).any()
    if case == "k1100":
        assert c.last_kernel_name().startswith("large_k_kernel")
    if case == "timed":
        assert c.last_phase_ms(knn.PHASE_CANDIDATE) > 0
    finish(dev, [c])


@pytest.mark.parametrize("ties,metric", [(1, 0), (2, 1)])
@pytest.mark.parametrize("entry", ["sweep", "excl", "loo", "sweep_eval", "excl_eval",
                                   "loo_eval"])
def test_sweep_held(knn, dev, entry, ties, metric):
    """The K-sweep calls on the tie set (a 0, a duplicate and kmax in the
    list): the pageable K list's upload, the search, the sweep tie scan and the
    reference-order pass, the prefix votes, the zeroed counts and the
    confusion pass, all on S.  With "ties" = 2 the indices are the oracle's."""
    import torch
    name = "ties%d" % metric
    s = st.tie_set(metric)
    ks = st.KS_SWEEP
    nk, kmax, C = len(ks), max(ks), s["classes"]
    loo, ev = entry.startswith("loo"), entry.endswith("eval")
    r0, r1 = st.LOO_ROWS
    m = r1 - r0 if loo else s["q"].shape[0]
    c = _classifier(knn, s, tuning={"ties": ties})
    b = st.Poisoned(dev)
    Q = None if loo else b.inp(s["q"], "query")
    T = None if loo else b.inp(s["truth"], "truth")
    E = b.inp(st.exclusions(metric), "excl") if entry.startswith("excl") else None
    ol = b.out((nk, m), torch.int32)
    oc = b.out((nk,), torch.int64)
    if ev:
        ocf = b.out((nk, C, C), torch.int64)
        ou = b.out((nk,), torch.int64)
    else:
        oi = b.out((m, kmax), torch.int64)
        od = b.out((m, kmax), torch.float64)
        of = b.out((m,), torch.int32)

    def call(stream):
        k_list = list(ks)  # a temporary: nothing may read the host list after the call
        if entry == "loo":
            c.loo_sweep_device(r0, m, k_list, metric, ol.data_ptr(), oc.data_ptr(),
                               oi.data_ptr(), od.data_ptr(), of.data_ptr(), stream=stream)
        elif entry == "loo_eval":
            c.loo_sweep_eval_device(r0, m, k_list, metric, ol.data_ptr(), oc.data_ptr(),
                                    ocf.data_ptr(), ou.data_ptr(), stream=stream)
        elif ev:
            c.classify_sweep_eval_device(Q.data_ptr(), m, k_list, metric, T.data_ptr(),
                                         d_labels=ol.data_ptr(), d_correct=oc.data_ptr(),
                                         d_conf=ocf.data_ptr(), d_unl=ou.data_ptr(),
                                         d_excl=_ptr(E), stream=stream)
        else:
            c.classify_sweep_device(Q.data_ptr(), m, k_list, metric, ol.data_ptr(), T.data_ptr(),
                                    oc.data_ptr(), oi.data_ptr(), od.data_ptr(), of.data_ptr(),
                                    stream=stream, d_excl=_ptr(E))

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    want = (st.expected_loo(name, metric, ks, r0, r1) if loo
            else st.expected_excl(metric, ks) if E is not None
            else st.expected_sweep(name, metric, ks))
    np.testing.assert_array_equal(b.result(ol), want["labels"])
    np.testing.assert_array_equal(b.result(oc), want["correct"])
    if ev:
        np.testing.assert_array_equal(b.result(ocf), want["conf"])
        np.testing.assert_array_equal(b.result(ou), want["unl"])
    else:
        _check_rows(knn, None, b.result(oi), b.result(od), b.result(of),
                    (None, want["idx"], want["dist"]), ties2=ties == 2)
    finish(dev, [c])


def _syn_inputs(b, s):
    return (b.inp(s["idx"], "idx"), b.inp(s["dist"], "dist"), b.inp(s["lab"], "label"),
            b.inp(s["truth"], "truth"))


@pytest.mark.parametrize("kmax", sorted(st.SYN_KS))
def test_vote_blocks_held(knn, dev, kmax):
    """knn_vote_sweep_device, knn_vote_sweep_weighted_device and
    knn_vote_weights_device over synthetic rows, one after the other on S
    (kmax = 600 crosses the 512-entry LDS chunk of wvote_sweep_kernel); the two
    sweeps upload their K lists into the same device buffer."""
    import torch
    s = st.synthetic(kmax)
    m, ks, k, C = st.SYN_M, s["ks"], s["k"], s["C"]
    c = knn.Classifier(0)
    b = st.Poisoned(dev)
    I, D, L, T = _syn_inputs(b, s)
    ou, ocu = b.out((len(ks), m), torch.int32), b.out((len(ks),), torch.int64)
    ow, ocw = b.out((len(ks), m), torch.int32), b.out((len(ks),), torch.int64)
    os_ = b.out((m, C), torch.float64)

    def call(stream):
        c.vote_sweep_device(I.data_ptr(), m, kmax, L.data_ptr(), list(ks), ou.data_ptr(),
                            d_truth=T.data_ptr(), d_correct=ocu.data_ptr(), stream=stream)
        c.vote_sweep_weighted_device(I.data_ptr(), D.data_ptr(), m, kmax, L.data_ptr(),
                                     list(reversed(ks)), ow.data_ptr(), d_truth=T.data_ptr(),
                                     d_correct=ocw.data_ptr(), stream=stream)
        c.vote_weights_device(I.data_ptr(), D.data_ptr(), m, kmax, L.data_ptr(), k, C,
                              os_.data_ptr(), stream=stream)

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    np.testing.assert_array_equal(b.result(ou), s["uniform"])
    np.testing.assert_array_equal(b.result(ocu), s["uniform_correct"])
    np.testing.assert_array_equal(b.result(ow), s["weighted"][::-1])
    np.testing.assert_array_equal(b.result(ocw), s["weighted_correct"][::-1])
    np.testing.assert_array_equal(b.result(os_), s["sums"])
    finish(dev, [c])


@pytest.mark.parametrize("C", st.COUNTS_CS)
def test_vote_counts_held(knn, dev, C):
    """knn_vote_counts_device with LDS counters (C = 3) and on the
    hipMemsetAsync + global atomics route (C = COUNTS_LDS_C + 1)."""
    import torch
    s = st.synthetic(65, C)
    m = st.SYN_M
    c = knn.Classifier(0)
    b = st.Poisoned(dev)
    I, L = b.inp(s["idx"], "idx"), b.inp(s["lab"], "label")
    oc = b.out((m, C), torch.int32)

    def call(stream):
        c.vote_counts_device(I.data_ptr(), m, 65, L.data_ptr(), s["k"], C, oc.data_ptr(),
                             stream=stream)

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    np.testing.assert_array_equal(b.result(oc), s["counts"])
    finish(dev, [c])


@pytest.mark.parametrize("C", st.CONFUSION_CS)
def test_confusion_held(knn, dev, C):
    """knn_confusion_device in its three regimes (per-wave LDS, per-workgroup
    LDS, global atomics).  It ADDS: the zeroes arrive by a copy on S."""
    s = st.confusion_case(C)
    nk, m = s["labels"].shape
    c = knn.Classifier(0)
    b = st.Poisoned(dev)
    L, T = b.inp(s["labels"], "label"), b.inp(s["truth"], "truth")
    ocf = b.inout(np.zeros((nk, C, C), np.int64), "sentinel")
    ou = b.inout(np.zeros(nk, np.int64), "sentinel")

    def call(stream):
        c.confusion_device(L.data_ptr(), nk, m, T.data_ptr(), C, ocf.data_ptr(), ou.data_ptr(),
                           stream=stream)

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    np.testing.assert_array_equal(b.result(ocf), s["conf"])
    np.testing.assert_array_equal(b.result(ou), s["unl"])
    finish(dev, [c])


@pytest.mark.parametrize("k,mq", [(10, st.TIE_M), (1500, 41)])
def test_partial_merge_resolve_held(knn, dev, k, mq):
    """Three shard contexts' knn_search_partial_device, one after the other on
    S, knn_merge_vote_device (w = 11: the LDS merge; w = 1501 over 3 parts: the
    rank merge), every shard's knn_shard_distances_device for the flagged
    queries and knn_tie_resolve_device, as one chain on S.  Which queries the
    merge flags is read once from a run on the contexts' own streams (the
    host has to size the exchange); their rows reach d_qsel / d_orow on S."""
    import torch
    metric = st.L2
    s = st.tie_set(metric)
    q = s["q"][:mq]
    w, n, d = k + 1, st.TIE_N, s["tr"].shape[1]
    rows = [r1 - r0 for r0, r1 in st.TIE_SHARDS]
    ctxs = []
    for r0, r1 in st.TIE_SHARDS:
        c = knn.Classifier(0)
        Xs = torch.from_numpy(s["tr"][r0:r1].copy()).to(dev)
        Ls = torch.from_numpy(s["lab"][r0:r1].copy()).to(dev)
        c.set_train_device(Xs.data_ptr(), Ls.data_ptr(), r1 - r0, d, s["classes"], idx_offset=r0,
                           keep=(Xs, Ls))
        ctxs.append(c)
    b = st.Poisoned(dev)
    Q = b.inp(q, "query")
    lab_all = b.inp(s["lab"], "label")
    gd = b.out((3, mq, w), torch.float64)
    gi = b.out((3, mq, w), torch.int64)
    gl = b.out((3, mq, w), torch.int32)
    ol, of = b.out((mq,), torch.int32), b.out((mq,), torch.int32)
    oi, od = b.out((mq, k), torch.int64), b.out((mq, k), torch.float64)

    def search_merge(stream):
        for p, c in enumerate(ctxs):
            c.search_partial_device(Q.data_ptr(), mq, w, metric, gd[p].data_ptr(),
                                    gi[p].data_ptr(), gl[p].data_ptr(), stream=stream)
            if stream is None:  # each context's own stream: the merge's is another
                c.sync()
        ctxs[0].merge_vote_device(gd.data_ptr(), gi.data_ptr(), gl.data_ptr(), 3, mq, w, k,
                                  ol.data_ptr(), oi.data_ptr(), od.data_ptr(), of.data_ptr(),
                                  stream=stream)

    b.produce()
    torch.cuda.synchronize(dev)
    search_merge(None)
    for c in ctxs:
        c.sync()
    torch.cuda.synchronize(dev)
    pend = np.nonzero(of.cpu().numpy() & knn.FLAG_TIE_PENDING)[0].astype(np.int32)
    T = int(pend.size)
    assert T > 20, "the tie set leaves queries to the cross-shard exchange"
    qsel, orow = b.inp(pend, "qsel"), b.inp(pend, "orow")
    Dall = b.out((T * n,), torch.float64)

    def call(stream):
        search_merge(stream)
        off = 0
        for c, nr in zip(ctxs, rows):
            c.shard_distances_device(Q.data_ptr(), qsel.data_ptr(), T, metric,
                                     Dall.data_ptr() + 8 * off, stream=stream)
            off += T * nr
        ctxs[0].tie_resolve_device(Dall.data_ptr(), rows, T, lab_all.data_ptr(), orow.data_ptr(),
                                   k, ol.data_ptr(), oi.data_ptr(), od.data_ptr(), of.data_ptr(),
                                   stream=stream)

    wlab, widx, wdist = oracle.knn(s["tr"], s["lab"], q, k, True, s["classes"], n_out=k)

    def check():
        got, idx, dist, flags = b.result(ol), b.result(oi), b.result(od), b.result(of)
        assert not (flags & knn.FLAG_TIE_PENDING).any()
        _check_rows(knn, got, idx, dist, flags, (wlab, widx, wdist))
        ref = (flags & knn.FLAG_TIE_REF) != 0
        assert ref.sum() == T
        np.testing.assert_array_equal(idx[ref], widx[ref])

    held, keep = held_run(dev, ctxs, b, call, check=check, tries=16)
    assert held, st.HOLD_MSG
    finish(dev, ctxs)


def test_minmax_normalize_held(knn, dev):
    """knn_minmax_device (init = 1, then init = 0 on a second set) and
    knn_normalize_device as one chain on S against oracle.normalize."""
    import torch
    s = st.normalize_case()
    d = s["d"]
    c = knn.Classifier(0)
    b = st.Poisoned(dev)
    X1 = b.inout(s["x1"], "data")
    X2 = b.inp(s["x2"], "data")
    mx = b.out((d,), torch.float64, fill=st.POISON["bound"])
    mn = b.out((d,), torch.float64, fill=st.POISON["bound"])

    def call(stream):
        c.minmax_device(X1.data_ptr(), X1.shape[0], d, mx.data_ptr(), mn.data_ptr(), init=True,
                        stream=stream)
        c.minmax_device(X2.data_ptr(), X2.shape[0], d, mx.data_ptr(), mn.data_ptr(), init=False,
                        stream=stream)
        c.normalize_device(X1.data_ptr(), X1.shape[0], d, mx.data_ptr(), mn.data_ptr(),
                           stream=stream)

    held, keep = held_run(dev, [c], b, call)
    assert held, st.HOLD_MSG
    assert _same_bits(b.result(mx), s["mx"]) and _same_bits(b.result(mn), s["mn"])
    assert _same_bits(b.result(X1), s["want1"])
    finish(dev, [c])


# ------------------------------------------- B. every candidate path on S
def _path_case(knn, dev, spec, k):
    name, metric, precision, tuning, paths, pattern = spec
    c, got, idx, dist, flags = _classify_held(knn, dev, name, metric, k, precision, tuning)
    assert c.last_candidate_path() in paths, c.last_candidate_path()
    assert re.fullmatch(pattern, c.last_kernel_name()), c.last_kernel_name()
    _check_rows(knn, got, idx, dist, flags, st.expected_knn(name, metric, k))
    return c, flags


@pytest.mark.parametrize("case", sorted(st.PATHS))
def test_candidate_paths_held(knn, dev, case):
    """knn_classify_device on S through every candidate kernel family, the
    region order's query sort and scatter kernels and the norm blocks; the
    path and the kernel name are asserted so that no case rides another
    kernel."""
    c, _ = _path_case(knn, dev, st.PATHS[case], st.PATH_K)
    finish(dev, [c])


@pytest.mark.parametrize("case", sorted(st.RESCANS))
def test_rescan_paths_held(knn, dev, case):
    """The duplicate sets: the rescan filters (fp32, and int8 on the 32x32x32
    image) and the full exact scan on S."""
    c, flags = _path_case(knn, dev, st.RESCANS[case], st.DUP_K)
    assert c.last_rescan_count() > 0
    assert (flags[:st.DUP_QUERIES] & knn.FLAG_EXACT_RESCAN).all()
    finish(dev, [c])


# ------------------------------- C. back-to-back calls, one context, one hold
@pytest.mark.parametrize("where", ["caller-stream", "context-stream"])
def test_back_to_back(knn, dev, where):
    """Nine calls enqueued without a host wait share sw_ks, the pinned counts
    and the grow-only workspaces: two sweeps with different K lists (handed
    over as temporaries), classify at descending batch sizes (the larger
    call's lists stay in the padding), another metric, the weighted vote
    (which rewrites sw_ks[0]), the first sweep again and a leave-one-out
    evaluation.  On a held caller stream, and on the context's own stream
    behind a hold on the legacy default stream.  Every call's outputs are the
    oracle's."""
    import torch
    name = "noisy8"
    s = st.dataset(name)
    m, C = s["q"].shape[0], s["classes"]
    c = _classifier(knn, s)
    b = st.Poisoned(dev)
    Q = b.inp(s["q"], "query")
    T = b.inp(s["truth"], "truth")
    i32, i64, f64 = torch.int32, torch.int64, torch.float64

    def sweep_out(nk, rows):
        return b.out((nk, rows), i32), b.out((nk,), i64)

    def cls_out(mm, k):
        return (b.out((mm,), i32), b.out((mm, k), i64), b.out((mm, k), f64), b.out((mm,), i32))

    sA, sB, sA2 = sweep_out(3, m), sweep_out(5, m), sweep_out(3, m)
    c257, c37, c1 = cls_out(m, 7), cls_out(37, 7), cls_out(1, 7)
    cL1 = cls_out(m, 3)
    wl = b.out((m,), i32)
    loo_l, loo_c = sweep_out(3, 40)
    loo_f, loo_u = b.out((3, C, C), i64), b.out((3,), i64)

    def sweep(stream, ks, out):
        c.classify_sweep_device(Q.data_ptr(), m, list(ks), st.L2, out[0].data_ptr(), T.data_ptr(),
                                out[1].data_ptr(), stream=stream)

    def classify(stream, mm, k, metric, out):
        c.classify_device(Q.data_ptr(), mm, k, metric, out[0].data_ptr(), out[1].data_ptr(),
                          out[2].data_ptr(), out[3].data_ptr(), stream=stream)

    def call(stream):
        sweep(stream, st.KS_A, sA)
        sweep(stream, st.KS_B, sB)
        classify(stream, m, 7, st.L2, c257)
        classify(stream, 37, 7, st.L2, c37)
        classify(stream, 1, 7, st.L2, c1)
        classify(stream, m, 3, st.L1, cL1)
        c.set_vote(knn.VOTE_DISTANCE)
        c.classify_device(Q.data_ptr(), m, 7, st.L2, wl.data_ptr(), stream=stream)
        c.set_vote(knn.VOTE_UNIFORM)
        sweep(stream, st.KS_A, sA2)
        c.loo_sweep_eval_device(10, 40, list(st.KS_A), st.L2, loo_l.data_ptr(), loo_c.data_ptr(),
                                loo_f.data_ptr(), loo_u.data_ptr(), stream=stream)

    held, keep = held_run(dev, [c], b, call, default_hold=where == "context-stream")
    assert held, st.HOLD_MSG
    wA, wB = st.expected_sweep(name, st.L2, st.KS_A), st.expected_sweep(name, st.L2, st.KS_B)
    for out, want in ((sA, wA), (sB, wB), (sA2, wA)):
        np.testing.assert_array_equal(b.result(out[0]), want["labels"])
        np.testing.assert_array_equal(b.result(out[1]), want["correct"])
    w7, w3 = st.expected_knn(name, st.L2, 7), st.expected_knn(name, st.L1, 3)
    for out, want, mm in ((c257, w7, m), (c37, w7, 37), (c1, w7, 1), (cL1, w3, m)):
        _check_rows(knn, b.result(out[0]), b.result(out[1]), b.result(out[2]), b.result(out[3]),
                    tuple(a[:mm] for a in want))
    np.testing.assert_array_equal(b.result(wl), st.expected_weighted(name, st.L2, 7))
    wl_ = st.expected_loo(name, st.L2, st.KS_A, 10, 50)
    np.testing.assert_array_equal(b.result(loo_l), wl_["labels"])
    np.testing.assert_array_equal(b.result(loo_c), wl_["correct"])
    np.testing.assert_array_equal(b.result(loo_f), wl_["conf"])
    np.testing.assert_array_equal(b.result(loo_u), wl_["unl"])
    finish(dev, [c])


# --------------------------------- D. HipTies under a non-default current stream
@pytest.mark.parametrize("metric", [0, 1])
def test_hip_ties_held_stream(knn, dev, metric):
    """The body of test_hip_ties_default_stream inside torch.cuda.stream(S),
    S held and the merge inputs produced on S: HipTies' default stream is then
    S.  (resolve_ties reads counts back, which ends the hold: it is asserted
    after the merge's enqueue.  No canary here: knn_merge_vote_device's own
    held run is test_partial_merge_resolve_held.)"""
    hold = MergeOnHeldStream()
    hip_ties_case(knn, metric, hold)
    assert hold.still_held, st.HOLD_MSG

"""Cost of a K sweep against single searches (recorded, not gated).

Device-resident inputs on one GPU; per shape:
  (a) classify_device at K = kmax,
  (b) classify_sweep_device over ks = 1..kmax,
  (c) kmax separate classify_device calls (K = 1..kmax),
each timed with events on the stream the calls run on, after warm-up, as the
median over --steps.  Also: the sweep with "ties" = 0 (no scan / tie-order
pass), the prefix-vote kernel alone (vote_sweep_device over the sweep's rows)
and the queries the sweep re-ordered per call (tie counters).  Prints one JSON
line per shape.  --profile runs a few sweeps only (for a kernel trace).

  python tools/sweep_time.py --set mnist|cfg2 [--steps 5] [--warmup 2] [--profile]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _knn():
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(ROOT, "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make(name):
    rng = np.random.default_rng(3)
    if name == "mnist":  # the reference's published shape, normalised random data
        n, m, d, kmax, classes = 60000, 10000, 784, 50, 10
        X = rng.random((n + m, d))
    else:  # cfg2 shape: byte features (dense exact ties)
        n, m, d, kmax, classes = 1000000, 10000, 128, 10, 10
        centres = rng.uniform(40, 215, (classes, d))
        lab_all = rng.integers(0, classes, n + m)
        X = np.empty((n + m, d))
        for s in range(0, n + m, 100000):
            e = min(n + m, s + 100000)
            X[s:e] = np.clip(np.rint(centres[lab_all[s:e]] +
                                     25 * rng.standard_normal((e - s, d))), 0, 255)
        return X[:n], lab_all[:n].astype(np.int32), X[n:], lab_all[n:].astype(np.int32), kmax, classes
    lab = rng.integers(0, classes, n + m).astype(np.int32)
    return X[:n], lab[:n], X[n:], lab[n:], kmax, classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="mnist", choices=["mnist", "cfg2"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    knn = _knn()
    tr, lab, te, truth, kmax, classes = make(a.set)
    n, d = tr.shape
    m = te.shape[0]
    dev = torch.device("cuda", 0)
    X = torch.from_numpy(tr).to(dev)
    L = torch.from_numpy(lab).to(dev)
    Q = torch.from_numpy(te).to(dev)
    T = torch.from_numpy(truth).to(dev)
    ks = list(range(1, kmax + 1))
    nk = len(ks)
    c = knn.Classifier(0)
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, classes, keep=(X, L))
    one = torch.empty(m, dtype=torch.int32, device=dev)
    out = torch.empty((nk, m), dtype=torch.int32, device=dev)
    corr = torch.empty(nk, dtype=torch.int64, device=dev)
    idx = torch.empty((m, kmax), dtype=torch.int64, device=dev)
    flags = torch.empty(m, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream

    def single(k=kmax):
        c.classify_device(Q.data_ptr(), m, k, knn.L2, one.data_ptr(), stream=sp)

    def sweep():
        c.classify_sweep_device(Q.data_ptr(), m, ks, knn.L2, out.data_ptr(), T.data_ptr(),
                                corr.data_ptr(), d_idx=idx.data_ptr(), d_flags=flags.data_ptr(),
                                stream=sp)

    def singles():
        for k in ks:
            single(k)

    def vote():
        c.vote_sweep_device(idx.data_ptr(), m, kmax, L.data_ptr(), ks, out.data_ptr(),
                            d_truth=T.data_ptr(), d_correct=corr.data_ptr(), stream=sp)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        st.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    torch.cuda.synchronize()
    if a.profile:
        for _ in range(3):
            sweep()
        st.synchronize()
        return
    res = {"set": a.set, "n": n, "m": m, "d": d, "kmax": kmax, "nk": nk}
    res["a_single_kmax_ms"] = timed(single, a.steps, a.warmup)
    res["b_sweep_ms"] = timed(sweep, a.steps, a.warmup)
    c.sync()
    c.tie_totals(reset=True)
    sweep()
    c.sync()
    res["queued_queries"] = c.tie_totals(reset=True)
    res["flag_tie_ref"] = int(((flags.cpu().numpy() & knn.FLAG_TIE_REF) != 0).sum())
    single()
    c.sync()
    res["queued_queries_single_kmax"] = c.tie_totals(reset=True)
    res["vote_kernel_ms"] = timed(vote, a.steps, a.warmup)
    c.set_tuning("ties", 0)
    res["sweep_ties0_ms"] = timed(sweep, a.steps, a.warmup)
    res["single_ties0_ms"] = timed(single, a.steps, a.warmup)
    c.set_tuning("ties", 1)
    res["c_singles_ms"] = timed(singles, max(1, a.steps // 2), 1)
    res["b_over_a"] = res["b_sweep_ms"] / res["a_single_kmax_ms"]
    res["c_over_b"] = res["c_singles_ms"] / res["b_sweep_ms"]
    res["candidate_path"] = c.last_candidate_path()
    print(json.dumps(res))
    sys.stdout.flush()
    c.close()


if __name__ == "__main__":
    main()

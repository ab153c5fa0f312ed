"""Cost of the leave-one-out K sweep against the plain sweep (recorded, not gated).

Device-resident inputs on one GPU, the MNIST shape (60000 x 784, uniform
random data: no ties), ks = 1..50:
  (a) loo_sweep_device over train rows [0, 10000),
  (b) classify_sweep_device of the same 10000 rows as queries at ks = 1..51
      (the plain sweep's code path at the width (a) searches at),
each timed with events on the stream the calls run on, after warm-up, as the
median over --steps.  Also alternates the two (a, b, a, b, ...) so both see
the same machine state.  Prints one JSON line.

  python tools/loo_time.py [--steps 7] [--warmup 2] [--rows 10000]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--d", type=int, default=784)
    ap.add_argument("--kmax", type=int, default=50)
    a = ap.parse_args()
    knn = _knn()
    rng = np.random.default_rng(3)
    n, d, m, kmax, classes = a.n, a.d, a.rows, a.kmax, 10
    tr = rng.random((n, d))
    lab = rng.integers(0, classes, n).astype(np.int32)
    dev = torch.device("cuda", 0)
    X = torch.from_numpy(tr).to(dev)
    L = torch.from_numpy(lab).to(dev)
    ks_a = list(range(1, kmax + 1))
    ks_b = list(range(1, kmax + 2))
    c = knn.Classifier(0)
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, classes, keep=(X, L))
    out = torch.empty((kmax + 1, m), dtype=torch.int32, device=dev)
    corr = torch.empty(kmax + 1, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream

    def loo():
        c.loo_sweep_device(0, m, ks_a, knn.L2, out.data_ptr(), corr.data_ptr(), stream=sp)

    def sweep():
        c.classify_sweep_device(X.data_ptr(), m, ks_b, knn.L2, out.data_ptr(), L.data_ptr(),
                                corr.data_ptr(), stream=sp)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    torch.cuda.synchronize()
    for _ in range(a.warmup):
        loo()
        sweep()
    st.synchronize()
    ta, tb = [], []
    for _ in range(a.steps):  # alternating
        ta.append(once(loo))
        tb.append(once(sweep))
    c.sync()
    c.tie_totals(reset=True)
    loo()
    c.sync()
    res = {"n": n, "d": d, "rows": m, "kmax": kmax, "steps": a.steps,
           "a_loo_ms": statistics.median(ta), "b_sweep_kmax1_ms": statistics.median(tb),
           "a_min_ms": min(ta), "a_max_ms": max(ta), "b_min_ms": min(tb), "b_max_ms": max(tb),
           "queued_queries": c.tie_totals(reset=True),
           "loo_accuracy_k1": float(corr.cpu().numpy()[0]) / m,
           "candidate_path": c.last_candidate_path()}
    res["a_over_b"] = res["a_loo_ms"] / res["b_sweep_kmax1_ms"]
    print(json.dumps(res))
    sys.stdout.flush()
    c.close()


if __name__ == "__main__":
    main()

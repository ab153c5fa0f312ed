"""K-fold sweep on fold shards against the only other route to the same numbers,
the leave-group-out sweep with groups = folds (recorded, not gated).

Device-resident inputs on one GPU, timed as tools/lgo_time.py does (events on
the stream the calls run on, after warm-up, the two routes interleaved, median
of --steps).  Folds are contiguous (row // (n / F)), so fold 0 is rows [0, n /
F) and both calls answer the same queries:
  kfold: kfold_sweep_device of fold 0 (n / F rows);
  lgo:   lgo_sweep_device of rows [0, --lgo_rows) -- at gmax = n / F the search
         runs at kmax + gmax entries, the exact large-k path, so the route is
         timed on a slice and both are reported per row.
Shapes: mnist = 60000 x 784 uniform data, F = 5, both metrics; cfg2 = bench.py's
grid data (128 dims) cut to 200000 rows, F = 10, L2.  ks = 1..50.
Prints one JSON line per shape and metric.

  python tools/kfold_time.py [--shape mnist|cfg2] [--steps 5] [--warmup 1] [--lgo_rows 256]
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
    ap.add_argument("--shape", default="mnist", choices=["mnist", "cfg2"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lgo_rows", type=int, default=256)
    a = ap.parse_args()
    knn = _knn()
    dev = torch.device("cuda", 0)
    classes, kmax = 10, 50
    if a.shape == "mnist":
        n, d, F, metrics = 60000, 784, 5, (knn.L2, knn.L1)
        rng = np.random.default_rng(3)
        X = torch.from_numpy(rng.random((n, d))).to(dev)
        L = torch.from_numpy(rng.integers(0, classes, n).astype(np.int32)).to(dev)
    else:
        sys.path.insert(0, ROOT)
        import bench
        n, d, F, metrics = 200000, 128, 10, (knn.L2,)
        X, L, _, _ = bench.synth(n, 1, d, classes, 1, 2, dev)
        L = L.to(torch.int32)
    nf = n // F
    folds = (np.arange(n) // nf).astype(np.int32)
    ks = list(range(1, kmax + 1))
    c = knn.Classifier(0)
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, classes, keep=(X, L))
    c.set_folds(folds, F)
    c.set_groups(folds, F)
    assert c.fold_max() == nf == c.group_max()
    out = torch.empty((len(ks), nf), dtype=torch.int32, device=dev)
    corr = torch.empty(len(ks), dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream
    lgo_rows = min(a.lgo_rows, nf)

    def timed(fns):
        ms = {name: [] for name in fns}
        for step in range(a.warmup + a.steps):
            for name, fn in fns.items():  # interleaved
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                e1.synchronize()
                if step >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
                for k, v in ms.items()}

    for metric in metrics:
        fns = {
            "kfold": lambda: c.kfold_sweep_device(0, ks, metric, out.data_ptr(), corr.data_ptr(),
                                                  stream=sp),
            "lgo": lambda: c.lgo_sweep_device(0, lgo_rows, ks, metric, out.data_ptr(),
                                              corr.data_ptr(), stream=sp),
        }
        torch.cuda.synchronize()
        res = {"shape": a.shape, "n": n, "d": d, "F": F, "metric": int(metric), "kmax": kmax,
               "steps": a.steps, "kfold_rows": nf, "lgo_rows": lgo_rows}
        res.update(timed(fns))
        res["kfold"]["us_per_row"] = 1e3 * res["kfold"]["median_ms"] / nf
        res["lgo"]["us_per_row"] = 1e3 * res["lgo"]["median_ms"] / lgo_rows
        print(json.dumps(res))
        sys.stdout.flush()
    c.close()


if __name__ == "__main__":
    main()

"""Cost of the leave-group-out sweep against leave-one-out (recorded, not gated).

Device-resident inputs on one GPU, timed as tools/sweep_time.py does (events on
the stream the calls run on, after warm-up): 60000 x 784 uniform data, ks =
1..50, one 16384-row batch of
  loo_sweep_device,
  lgo_sweep_device with every group of one row (gmax = 1),
  lgo_sweep_device with groups of --gmax consecutive rows (default 8, 64, 256).
Prints one JSON line: per case the median and the run-to-run range (min, max)
in ms over --steps.

  python tools/lgo_time.py [--steps 7] [--warmup 2] [--gmax 8,64,256]
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
    ap.add_argument("--gmax", default="8,64,256")
    a = ap.parse_args()
    knn = _knn()
    rng = np.random.default_rng(3)
    n, d, kmax, classes, rows = 60000, 784, 50, 10, 16384
    tr = rng.random((n, d))
    lab = rng.integers(0, classes, n).astype(np.int32)
    dev = torch.device("cuda", 0)
    X = torch.from_numpy(tr).to(dev)
    L = torch.from_numpy(lab).to(dev)
    ks = list(range(1, kmax + 1))
    c = knn.Classifier(0)
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, classes, keep=(X, L))
    out = torch.empty((len(ks), rows), dtype=torch.int32, device=dev)
    corr = torch.empty(len(ks), dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream

    def loo():
        c.loo_sweep_device(0, rows, ks, knn.L2, out.data_ptr(), corr.data_ptr(), stream=sp)

    def lgo():
        c.lgo_sweep_device(0, rows, ks, knn.L2, out.data_ptr(), corr.data_ptr(), stream=sp)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        st.synchronize()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    torch.cuda.synchronize()
    res = {"n": n, "d": d, "rows": rows, "kmax": kmax, "steps": a.steps}
    res["loo"] = timed(loo)
    for g in [1] + [int(v) for v in a.gmax.split(",") if v]:
        c.set_groups((np.arange(n) // g).astype(np.int32))
        assert c.group_max() == g
        res["lgo_gmax%d" % g] = timed(lgo)
        res["lgo_gmax%d" % g]["path"] = c.last_candidate_path()
    res["loo_again"] = timed(loo)
    print(json.dumps(res))
    sys.stdout.flush()
    c.close()


if __name__ == "__main__":
    main()

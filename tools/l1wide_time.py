"""Whole-call time of the Manhattan metric on wide integer rows: the fp32 stream
kernel (candidate path 1, "i8l1" = 0) against the wide pass on int8 codes
(path 7, cand_sad_wide_kernel, "i8l1" = 2) in one process and one build
(recorded, not gated).

Device-resident inputs on one GPU, datagen-"int"-style data (integers 0..255
per dim), one classifier per setting over the same train set.  Each call
(prep + candidate + re-rank + rescan) is timed with events on the stream it
runs on, after warm-up; the two settings alternate (a, b, a, b, ...) so both
see the same machine state.  Prints one JSON line per shape with the median
and range of --steps repetitions and each setting's rescan count.

  python tools/l1wide_time.py [--steps 7] [--warmup 2] [--shape mnist|second|all]
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
SHAPES = {"mnist": (60000, 10000, 784, 50), "second": (1000000, 4096, 512, 10)}


def _knn():
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(ROOT, "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(knn, name, n, m, d, k, steps, warmup):
    classes = 10
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    X = torch.randint(0, 256, (n, d), device=dev, generator=g).to(torch.float64)
    Q = torch.randint(0, 256, (m, d), device=dev, generator=g).to(torch.float64)
    L = torch.randint(0, classes, (n,), device=dev, generator=g).to(torch.int32)
    out = {v: torch.empty(m, dtype=torch.int32, device=dev) for v in (0, 2)}
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream
    clf = {}
    for v in (0, 2):
        c = knn.Classifier(0)
        c.set_tuning("i8l1", v)
        c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, classes, keep=(X, L))
        clf[v] = c
    torch.cuda.synchronize()

    def call(v):
        clf[v].classify_device(Q.data_ptr(), m, k, knn.L1, out[v].data_ptr(), stream=sp)

    def once(v):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call(v)
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        call(0)
        call(2)
    st.synchronize()
    t = {0: [], 2: []}
    for _ in range(steps):
        t[0].append(once(0))
        t[2].append(once(2))
    res = {"shape": name, "n": n, "m": m, "d": d, "k": k, "steps": steps}
    for v, tag in ((0, "path1"), (2, "wide")):
        res[tag + "_ms"] = statistics.median(t[v])
        res[tag + "_min_ms"], res[tag + "_max_ms"] = min(t[v]), max(t[v])
        res[tag + "_rescans"] = clf[v].last_rescan_count()
        res[tag + "_candidate_path"] = clf[v].last_candidate_path()
        res[tag + "_kernel"] = clf[v].last_kernel_name()
    res["labels_equal"] = bool((out[0] == out[2]).all().item())
    res["path1_over_wide"] = res["path1_ms"] / res["wide_ms"]
    print(json.dumps(res))
    sys.stdout.flush()
    for c in clf.values():
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", default="all", choices=["all"] + sorted(SHAPES))
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps must be >= 5 (median and range of at least 5 repetitions)")
    knn = _knn()
    for name in (sorted(SHAPES) if a.shape == "all" else [a.shape]):
        run(knn, name, *SHAPES[name], a.steps, a.warmup)


if __name__ == "__main__":
    main()

"""Time of the Manhattan metric on continuous data above 256 dims: the fp32
VALU stream pass (candidate path 1, "u16l1w" = 0) against the wide pass on
16-bit fixed-point codes (path 8, cand_fix16_wide_kernel, "u16l1w" = 1) in one
process and one build (recorded, not gated).

Device-resident inputs on one GPU: uniform data generated on the device and
min-max normalised over train and queries together (the reference's
transductive normalisation: everything in [0, 1]), one classifier per setting
over the same train set.  Whole calls (prep + candidate + re-rank + rescan)
are timed with events on the stream they run on, after warm-up; the settings
alternate (a, b, a, b, ...) so both see the same machine state.  A second
round with knn_set_timing on gives the per-phase means.  Prints one JSON line
per shape: median and range of --steps repetitions, phases, rescans per call.

  python tools/l1fixwide_time.py [--steps 7] [--warmup 2] [--shape mnist|wide1m|all]
      [--pkg DIR]   the package directory to load (knn_amd.py + lib/), e.g. a
                    build of another commit; default this tree's
      [--only-off]  time "u16l1w" = 0 alone and never set the key (a build
                    that does not know it)
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's default shape (MNIST: 60000 x 784, 10000 queries) and a
# million rows at the one-slab width
SHAPES = {"mnist": (60000, 10000, 784, 50), "wide1m": (1000000, 4096, 512, 10)}
PHASES = ("prep", "cand", "merge", "rescan")


def _knn(pkg):
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(pkg, "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(knn, name, n, m, d, k, steps, warmup, settings):
    classes = 10
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(n + d)
    A = torch.rand((n + m, d), device=dev, generator=g, dtype=torch.float64)
    lo, hi = A.min(0).values, A.max(0).values
    A = (A - lo) / (hi - lo)
    X, Q = A[:n].contiguous(), A[n:].contiguous()
    del A
    L = torch.randint(0, classes, (n,), device=dev, generator=g).to(torch.int32)
    out = {v: torch.empty(m, dtype=torch.int32, device=dev) for v in settings}
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream
    clf = {}
    for v in settings:
        c = knn.Classifier(0)
        if v:
            c.set_tuning("u16l1w", v)
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
        for v in settings:
            call(v)
    st.synchronize()
    t = {v: [] for v in settings}
    resc = {v: [] for v in settings}
    for _ in range(steps):
        for v in settings:
            t[v].append(once(v))
            resc[v].append(clf[v].last_rescan_count())
    # per phase: the same alternation with the library's own events
    for v in settings:
        clf[v].set_timing(True)
        clf[v].timing_totals(reset=True)
    for _ in range(steps):
        for v in settings:
            call(v)
            st.synchronize()
    res = {"shape": name, "n": n, "m": m, "d": d, "k": k, "steps": steps}
    for v in settings:
        tag = "u16w" if v else "path1"
        res[tag + "_ms"] = statistics.median(t[v])
        res[tag + "_min_ms"], res[tag + "_max_ms"] = min(t[v]), max(t[v])
        res[tag + "_rescans_per_call"] = statistics.mean(resc[v])
        ms, calls = clf[v].timing_totals(reset=True)
        res[tag + "_phase_ms"] = {p: x / max(calls, 1) for p, x in zip(PHASES, ms)}
        res[tag + "_candidate_path"] = clf[v].last_candidate_path()
        res[tag + "_kernel"] = clf[v].last_kernel_name()
    if len(settings) == 2:
        res["labels_equal"] = bool((out[0] == out[1]).all().item())
        res["path1_over_u16w"] = res["path1_ms"] / res["u16w_ms"]
    print(json.dumps(res))
    sys.stdout.flush()
    for c in clf.values():
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", default="all", choices=["all"] + sorted(SHAPES))
    ap.add_argument("--pkg", default=os.path.join(ROOT, "-mpi-knn-_amd"))
    ap.add_argument("--only-off", action="store_true")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps must be >= 5 (median and range of at least 5 repetitions)")
    knn = _knn(a.pkg)
    for name in (sorted(SHAPES) if a.shape == "all" else [a.shape]):
        run(knn, name, *SHAPES[name], a.steps, a.warmup, (0,) if a.only_off else (0, 1))


if __name__ == "__main__":
    main()

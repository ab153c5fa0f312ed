"""Cost of the per-class evaluation inside a K sweep (recorded, not gated).

Device-resident inputs on one GPU, the method of tools/sweep_time.py; per shape:
  (a) classify_sweep_device over ks = 1..kmax (labels and correct counts),
  (b) classify_sweep_eval_device over the same ks with conf and unl,
timed with events on the stream the calls run on: --warmup steps of each, then
--steps timed steps ALTERNATING (a), (b), (a), (b), ...; the median and the
range of each.  --pkg DIR times the library under DIR (knn_amd.py + lib/),
e.g. a build of the parent commit, which has (a) only.  Prints one JSON line.
--profile enqueues the two new kernels alone a few times (for a kernel trace):
the confusion pass over a [50][10000] label array at C = 10 and at C = 97 (the
global-atomics regime), the vote counts over [10000][50] rows at C = 10 and at
C = 1025.

  python tools/eval_time.py --set mnist|cfg2 [--steps 7] [--warmup 2] [--pkg DIR] [--profile]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_time  # noqa: E402  (the shapes)


def _knn(pkg):
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(pkg, "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def profile(knn, dev):
    rng = np.random.default_rng(5)
    c = knn.Classifier(0)
    nk, m, kmax = 50, 10000, 50
    truth = torch.from_numpy(rng.integers(0, 10, m).astype(np.int32)).to(dev)
    for C in (10, 97):
        t = truth % C
        # ~90 % of the labels on the diagonal, as a classifier's are
        lab = torch.where(torch.rand((nk, m), device=dev) < 0.9, t.expand(nk, m),
                          torch.randint(0, C, (nk, m), device=dev, dtype=torch.int32))
        lab = lab.to(torch.int32).contiguous()
        conf = torch.zeros((nk, C, C), dtype=torch.int64, device=dev)
        unl = torch.zeros(nk, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        for _ in range(5):
            c.confusion_device(lab.data_ptr(), nk, m, t.data_ptr(), C, conf.data_ptr(),
                               unl.data_ptr())
        c.sync()
        assert int(conf.sum().item()) == 5 * nk * m
    idx = torch.randint(0, 60000, (m, kmax), device=dev, dtype=torch.int64)
    for C in (10, 1025):
        tl = torch.randint(0, C, (60000,), device=dev, dtype=torch.int32)
        cnt = torch.empty((m, C), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for _ in range(5):
            c.vote_counts_device(idx.data_ptr(), m, kmax, tl.data_ptr(), kmax, C, cnt.data_ptr())
        c.sync()
        assert int(cnt.sum().item()) == m * kmax
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="mnist", choices=["mnist", "cfg2"])
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "-mpi-knn-_amd"))
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    knn = _knn(a.pkg)
    dev = torch.device("cuda", 0)
    if a.profile:
        profile(knn, dev)
        return
    tr, lab, te, truth, kmax, classes = sweep_time.make(a.set)
    n, d = tr.shape
    m = te.shape[0]
    X = torch.from_numpy(tr).to(dev)
    L = torch.from_numpy(lab).to(dev)
    Q = torch.from_numpy(te).to(dev)
    T = torch.from_numpy(truth).to(dev)
    ks = list(range(1, kmax + 1))
    nk = len(ks)
    c = knn.Classifier(0)
    if a.set == "cfg2":
        c.set_tuning("ties", 0)
    c.set_train_device(X.data_ptr(), L.data_ptr(), n, d, classes, keep=(X, L))
    out = torch.empty((nk, m), dtype=torch.int32, device=dev)
    corr = torch.empty(nk, dtype=torch.int64, device=dev)
    conf = torch.empty((nk, classes, classes), dtype=torch.int64, device=dev)
    unl = torch.empty(nk, dtype=torch.int64, device=dev)
    st = torch.cuda.Stream(device=dev)
    sp = st.cuda_stream
    has_eval = hasattr(knn.Classifier, "classify_sweep_eval_device")

    def sweep():
        c.classify_sweep_device(Q.data_ptr(), m, ks, knn.L2, out.data_ptr(), T.data_ptr(),
                                corr.data_ptr(), stream=sp)

    def sweep_eval():
        c.classify_sweep_eval_device(Q.data_ptr(), m, ks, knn.L2, T.data_ptr(),
                                     d_labels=out.data_ptr(), d_correct=corr.data_ptr(),
                                     d_conf=conf.data_ptr(), d_unl=unl.data_ptr(), stream=sp)

    def sweep_eval_nolabels():
        c.classify_sweep_eval_device(Q.data_ptr(), m, ks, knn.L2, T.data_ptr(),
                                     d_correct=corr.data_ptr(), d_conf=conf.data_ptr(),
                                     d_unl=unl.data_ptr(), stream=sp)

    cases = [("a_sweep", sweep)]
    if has_eval:
        cases += [("b_sweep_eval", sweep_eval), ("b_sweep_eval_no_labels", sweep_eval_nolabels)]
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        for _, fn in cases:
            fn()
    st.synchronize()
    ms = {name: [] for name, _ in cases}
    for _ in range(a.steps):
        for name, fn in cases:  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"set": a.set, "pkg": os.path.relpath(a.pkg, ROOT), "n": n, "m": m, "d": d, "nk": nk,
           "classes": classes, "steps": a.steps, "candidate_path": c.last_candidate_path()}
    for name, v in ms.items():
        res[name + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if has_eval:
        res["b_minus_a_ms"] = res["b_sweep_eval_ms"]["median"] - res["a_sweep_ms"]["median"]
        res["trace_equals_correct"] = bool(
            (torch.diagonal(conf, dim1=1, dim2=2).sum(dim=1) == corr).all().item())
    print(json.dumps(res))
    sys.stdout.flush()
    c.close()


if __name__ == "__main__":
    main()

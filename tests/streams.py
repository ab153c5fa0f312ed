"""Stream-order tests (test_gpu_streams.py): data sets with the CPU oracle's
expected results, the held caller stream, poisoned inputs and the run protocol.

Every `*_device` entry point of include/knn_amd.h promises that it is "enqueued
on `stream`", "returns without waiting for the device on every path" and that
"outputs are complete once the stream reaches the end of the call".  The
protocol here makes a violation visible:

  * the caller's stream S (a fresh non-blocking torch stream, ordered with
    neither the context's own stream nor the legacy default stream) is HELD
    behind a chain of fp64 products;
  * every device input of the call exists twice: a staging tensor with the real
    data and the tensor the call reads, pre-filled with POISON -- a valid value
    that gives a visibly different result and can index nothing out of bounds
    (queries NaN -> label -1 / KNN_FLAG_NONFINITE; neighbour idx -1 -> the
    entry never votes; dist +inf; truth -1 -> unlabelled; d_qsel / d_orow 0;
    d_max / d_min 0.0).  The real data reach the call's tensors by a copy
    enqueued on S, after the hold;
  * every output is pre-filled with a sentinel (-7) and has a copy tensor, also
    -7, filled by a copy enqueued on S after the call;
  * only S is synchronised, and only the copies are read.

A piece of the call that ran on another stream runs while S is held: it reads
poison, or the consumer copy overtakes it.  A missing piece leaves sentinels.
`still_held` (S not drained when the last enqueue returned) is asserted by
every held test: without it the test proves nothing, and it is the check of
"returns without waiting for the device".

No GPU code runs at import.  Expected values never come from the library.
"""
import functools
import math
import re

import numpy as np

import datagen
import evalcases
import loo
import oracle
import wvote

L2, L1 = 0, 1
SENTINEL = -7
HOLD_MSG = ("hold elapsed before the last enqueue: the call waited for the device or the hold "
            "is too short")

# ---------------------------------------------------------------- the hold
# One hold unit is one HOLD_DIM x HOLD_DIM fp64 product (2 * 4096^3 = 137
# GFLOP) on S.  Measured on an MI355X (16 host CPUs), with host timers around
# the calls:
#   ENQUEUE_MS: host time from the first to the last enqueue of the longest
#   case, the back-to-back sequence of part C (9 library calls and 43 copies):
#   0.6 ms on a caller stream, 1.0 - 1.6 ms on the context's own stream behind
#   the legacy default stream (the largest is taken);
#   UNIT_MS: device time of one hold unit, 2.15 - 2.3 ms.
# The hold is sized at about 4 x the enqueue time of that longest case (the
# margin covers the run-to-run spread of host launch latency on a shared
# machine), plus one unit for the ~1 ms the host spends enqueuing the hold
# itself while its first product already runs.
HOLD_DIM = 4096
ENQUEUE_MS = 1.6
UNIT_MS = 2.2
HOLD_UNITS = math.ceil(4 * ENQUEUE_MS / UNIT_MS) + 1


def held_stream(dev, units=None):
    """A fresh torch.cuda.Stream with the hold already enqueued on it; returns
    (S, keep): `keep` owns the operands (allocated and synchronised before the
    first product is enqueued) and must outlive the hold."""
    import torch
    units = HOLD_UNITS if units is None else units
    a = torch.ones((HOLD_DIM, HOLD_DIM), dtype=torch.float64, device=dev)
    out = torch.empty_like(a)
    S = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(S):
        for _ in range(units):
            torch.mm(a, a, out=out)
    return S, (a, out)


def hold_on_default(dev, units=None):
    """The same hold on the legacy default stream, which the context's own
    (blocking) stream is ordered after: (default stream, keep)."""
    import torch
    units = HOLD_UNITS if units is None else units
    a = torch.ones((HOLD_DIM, HOLD_DIM), dtype=torch.float64, device=dev)
    out = torch.empty_like(a)
    torch.cuda.synchronize(dev)
    for _ in range(units):
        torch.mm(a, a, out=out)
    return torch.cuda.default_stream(dev), (a, out)


POISON = {"query": float("nan"), "data": float("nan"), "idx": -1, "dist": float("inf"),
          "label": -1, "truth": -1, "excl": -1, "qsel": 0, "orow": 0, "bound": 0.0,
          "sentinel": -7}


class Poisoned:
    """The device buffers of one call (or one chain of calls).  inp(): a
    staging tensor with the real data and the tensor the call reads, poisoned;
    out(): an output tensor and its copy, both at the sentinel.  All tensors
    are allocated up front, on the default stream."""

    def __init__(self, dev):
        self.dev = dev
        self.ins = []   # (staging, live, poison value)
        self.outs = []  # (live, copy)

    def inp(self, host, kind):
        import torch
        staging = torch.from_numpy(np.array(host, order="C")).to(self.dev)
        live = torch.full_like(staging, POISON[kind])
        self.ins.append((staging, live, POISON[kind]))
        return live

    def out(self, shape, dtype, fill=SENTINEL):
        import torch
        live = torch.full(shape, fill, dtype=dtype, device=self.dev)
        self.outs.append((live, torch.full_like(live, fill), fill))
        return live

    def inout(self, host, kind):
        """A tensor the call reads AND writes (rows normalised in place, counts
        the call adds into): staged like an input, copied like an output."""
        import torch
        live = self.inp(host, kind)
        self.outs.append((live, torch.full_like(live, POISON[kind]), None))
        return live

    def reset(self):
        """Inputs back to poison, outputs and copies to the sentinel."""
        for _, live, poison in self.ins:
            live.fill_(poison)
        for live, copy, fill in self.outs:
            if fill is not None:
                live.fill_(fill)
            copy.fill_(SENTINEL)

    def produce(self):
        for staging, live, _ in self.ins:
            live.copy_(staging, non_blocking=True)

    def consume(self):
        for live, copy, _ in self.outs:
            copy.copy_(live, non_blocking=True)

    def result(self, live):
        """The COPY of output `live`, on the host."""
        for l, copy, _ in self.outs:
            if l is live:
                return copy.cpu().numpy()
        raise KeyError("not an output of this set")


def run_on_stream(S, produce, call, consume):
    """The hold is on S already.  On S: the producer copies, the library
    call(s) (`call(stream handle)`; None for the legacy default stream, i.e. the
    context's own), the consumer copies -- no host synchronisation in between;
    then whether S was still held when the last enqueue returned; then S alone
    is synchronised.  Returns still_held."""
    import torch
    with torch.cuda.stream(S):
        produce()
    call(S.cuda_stream or None)
    with torch.cuda.stream(S):
        consume()
    still_held = not S.query()
    S.synchronize()
    return still_held


class Canary:
    """Shows, for one held run, whether the other streams ran apart from S.
    A process has few hardware queues (4 by default), and work of two streams
    that the runtime has placed on one queue executes in submission order: a
    launch on the context's own stream then waits for the hold and the producer
    copies on S like the rest of the call, and a misplaced launch could not be
    told from a correct one.  The canary is such a misplaced launch made on
    purpose: a poisoned one-cell neighbour row that a producer copy on S
    replaces, read right after the producer copies by knn_vote_counts_device
    (it needs no train set) on each context's OWN stream and by a copy on the
    legacy default stream.  A canary that saw the poison overtook S, as any
    misplaced piece of the call would have; one that saw the real row was
    ordered behind S, and that run proves nothing."""

    def __init__(self, dev, ctxs):
        import torch
        self.dev, self.ctxs = dev, ctxs
        self.real = torch.zeros(1, dtype=torch.int64, device=dev)
        self.row = torch.full_like(self.real, POISON["idx"])
        self.lab = torch.zeros(1, dtype=torch.int32, device=dev)
        self.counts = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in ctxs]
        self.seen = torch.zeros(1, dtype=torch.int64, device=dev)

    def reset(self):
        self.row.fill_(POISON["idx"])
        self.seen.fill_(SENTINEL)
        for cnt in self.counts:
            cnt.fill_(SENTINEL)

    def produce(self):
        self.row.copy_(self.real, non_blocking=True)

    def launch(self):
        import torch
        # the default stream first: launched last, its copy would wait for the
        # contexts' (blocking) streams and be ordered whenever one of them is
        with torch.cuda.stream(torch.cuda.default_stream(self.dev)):
            self.seen.copy_(self.row, non_blocking=True)
        for c, cnt in zip(self.ctxs, self.counts):
            c.vote_counts_device(self.row.data_ptr(), 1, 1, self.lab.data_ptr(), 1, 1,
                                 cnt.data_ptr())

    def overtook(self):
        """After everything has drained: per context, then for the default
        stream, whether its canary read the poison."""
        return ([int(cnt.item()) == 0 for cnt in self.counts]
                + [int(self.seen.item()) == POISON["idx"]])


# ------------------------------------------------------------------ data sets
def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


CLASSES = 5
#        kind     n     m    d
SETS = {
    "gauss128": ("gauss", 4099, 257, 128),
    "int128": ("int", 4099, 257, 128),
    "gauss288": ("gauss", 2051, 129, 288),
    "gauss300": ("gauss", 2051, 129, 300),
    "gauss320": ("gauss", 2051, 129, 320),
    "int300": ("int", 2051, 129, 300),
    "noisy8": ("noisy", 4099, 257, 8),   # overlapping classes: labels depend on K and the vote
    "largek": ("gauss", 1301, 37, 8),
    "dup_gauss": ("gauss", 3001, 65, 32),
    "dup_int": ("int", 3001, 65, 32),
}
DUP_ROWS, DUP_QUERIES, DUP_K = 400, 32, 9


@functools.lru_cache(maxsize=None)
def dataset(name):
    """dict(tr, lab, q, truth, classes, kind): seeded, ragged n and m."""
    if name == "noisy8":  # off its 1/1024 grid: no exact ties, the reported rows are the oracle's
        return _noisy8()
    kind, n, m, d = SETS[name]
    seed = 9000 + sum(map(ord, name))
    tr, lab, q, truth, _, _ = datagen.make_sets(kind, seed, n, m, 0, d, CLASSES)
    if name.startswith("dup_"):
        # more than k identical nearest rows: no candidate list can certify the
        # top k, the exact rescan must run (test_duplicates_force_rescan)
        rng = np.random.default_rng(seed)
        tr[1000:1000 + DUP_ROWS] = tr[5]
        lab[1000:1000 + DUP_ROWS] = rng.integers(0, CLASSES, DUP_ROWS)
        q[:DUP_QUERIES] = tr[5]
    return _freeze(dict(tr=tr, lab=lab, q=q, truth=truth, classes=CLASSES, kind=kind))


def _noisy8():
    kind, n, m, d = SETS["noisy8"]
    tr, lab, q, truth, _, _ = datagen.make_sets(kind, 9008, n, m, 0, d, CLASSES)
    rng = np.random.default_rng(9008)
    tr = tr + rng.uniform(-2.0 ** -12, 2.0 ** -12, tr.shape)
    return _freeze(dict(tr=tr, lab=lab, q=q, truth=truth, classes=CLASSES, kind=kind))


def on_byte_grid(x):
    """plan_cases' criterion ("int" sets sit on the byte grid, "gauss" sets span
    more than 256 codes of their grid): every value c / 2^s for one s, the
    codes of each dimension spanning at most 255."""
    for s in range(0, 31):
        c = x * 2.0 ** s
        if (c == np.rint(c)).all():
            return bool(((c.max(0) - c.min(0)) <= 255).all())
    return False


TIE_N, TIE_M, TIE_CLASSES = 4001, 250, 5
TIE_SHARDS = [(0, 1300), (1300, 2701), (2701, TIE_N)]


@functools.lru_cache(maxsize=None)
def tie_set(metric):
    """The tie set of test_gpu_sharded.py (integer codes 0..9 in 6 dims, labels
    independent of position) with a seeded truth."""
    from test_gpu_sharded import _tie_set
    tr, lab, q = _tie_set(metric, n=TIE_N, m=TIE_M)
    truth = np.random.default_rng(77 + metric).integers(0, TIE_CLASSES, TIE_M).astype(np.int32)
    return _freeze(dict(tr=tr, lab=lab, q=q, truth=truth, classes=TIE_CLASSES, kind="ties"))


def any_set(name):
    return tie_set(int(name[-1])) if name.startswith("ties") else dataset(name)


@functools.lru_cache(maxsize=None)
def expected_knn(name, metric, k):
    """The oracle's (labels, idx [m, k], dist [m, k]) of set `name`."""
    s = any_set(name)
    lab, idx, dist = oracle.knn(s["tr"], s["lab"], s["q"], k, metric == L2, s["classes"],
                                n_out=max(k, 1))
    for a in (lab, idx, dist):
        a.setflags(write=False)
    return lab, idx[:, :k], dist[:, :k]


@functools.lru_cache(maxsize=None)
def expected_weighted(name, metric, k):
    """KNN_VOTE_DISTANCE labels [m] over the oracle's rows (sets without exact
    ties: the rows the call reports are the oracle's)."""
    s = any_set(name)
    _, idx, dist = expected_knn(name, metric, k)
    return wvote.labels(wvote.lab_rows(s["lab"], idx), dist, [k])[0]


# K lists: a 0, a duplicate and kmax (part A); the two lists of the sequence
KS_SWEEP = (5, 0, 37, 5, 10)
KS_A = (3, 0, 7)
KS_B = (1, 5, 2, 11, 4)


@functools.lru_cache(maxsize=None)
def expected_sweep(name, metric, ks):
    """dict(labels [nk, m], correct [nk], conf [nk, C, C], unl [nk], idx, dist
    [m, kmax]) of the plain sweep."""
    s = any_set(name)
    _, idx, dist = expected_knn(name, metric, max(ks))
    labels = evalcases.oracle_labels(s["tr"], s["lab"], s["q"], list(ks), metric == L2,
                                     s["classes"])
    return _freeze(_scored(labels, s["truth"], s["classes"], idx, dist))


def _scored(labels, truth, classes, idx, dist):
    conf, unl = evalcases.confusion(labels, truth, classes)
    return dict(labels=labels, correct=(labels == truth).sum(axis=1).astype(np.int64), conf=conf,
                unl=unl, idx=idx, dist=dist)


@functools.lru_cache(maxsize=None)
def exclusions(metric):
    """One excluded global train row per tie-set query (every fifth: none),
    chosen among the query's nearest rows so that the exclusion matters."""
    _, idx, _ = expected_knn("ties%d" % metric, metric, max(KS_SWEEP))
    rng = np.random.default_rng(5 + metric)
    excl = idx[np.arange(TIE_M), rng.integers(0, 8, TIE_M)].astype(np.int64)
    excl[::5] = -1
    excl.setflags(write=False)
    return excl


@functools.lru_cache(maxsize=None)
def expected_excl(metric, ks):
    s = tie_set(metric)
    want = loo.expected_excl(s["tr"], s["lab"], s["q"], exclusions(metric), list(ks),
                             metric == L2, s["classes"])
    return _freeze(_scored(want["labels"], s["truth"], s["classes"], want["idx"], want["dist"]))


LOO_ROWS = (100, 229)  # 129 train rows of the tie set


@functools.lru_cache(maxsize=None)
def expected_loo(name, metric, ks, row0, row1):
    """Leave-one-out over train rows [row0, row1): truth = the rows' labels."""
    s = any_set(name)
    rows = np.arange(row0, row1)
    want = loo.expected_excl(s["tr"], s["lab"], s["tr"][row0:row1], rows, list(ks), metric == L2,
                             s["classes"])
    return _freeze(_scored(want["labels"], s["lab"][row0:row1], s["classes"], want["idx"],
                           want["dist"]))


# ------------------------------------------- synthetic rows (building blocks)
SYN_M, SYN_NLAB = 385, 1500
SYN_KS = {65: (5, 0, 65, 5, 10), 600: (17, 0, 600, 17, 513)}


def uniform_labels(lrows, ks):
    """cpp:324-337 over the first K entries of each row; empty slots (label -1)
    count nothing, a row without entries gives -1."""
    out = np.empty((len(ks), lrows.shape[0]), np.int32)
    for q in range(lrows.shape[0]):
        for j, k in enumerate(ks):
            row = lrows[q, :k]
            out[j, q] = loo.vote(row[row >= 0])
    return out


@functools.lru_cache(maxsize=None)
def synthetic(kmax, C=3):
    """wvote.synthetic_rows with labels in [0, C), a truth, and the expected
    uniform / weighted labels, counts and class sums."""
    idx, dist = wvote.synthetic_rows(SYN_M, kmax, SYN_NLAB, C, seed=300 + kmax + C)
    rng = np.random.default_rng(kmax + C)
    lab = rng.integers(0, C, SYN_NLAB).astype(np.int32)
    truth = rng.integers(0, min(C, 3), SYN_M).astype(np.int32)
    ks = SYN_KS[kmax]
    lrows = wvote.lab_rows(lab, idx)
    k = kmax - 3
    uni = uniform_labels(lrows, ks)
    wtd = wvote.labels(lrows, dist, list(ks))
    return _freeze(dict(idx=idx, dist=dist, lab=lab, truth=truth, ks=ks, k=k, C=C, uniform=uni,
                        weighted=wtd, uniform_correct=(uni == truth).sum(1).astype(np.int64),
                        weighted_correct=(wtd == truth).sum(1).astype(np.int64),
                        counts=evalcases.vote_counts(lab, idx, k, C),
                        sums=wvote.sums(lrows, dist, k, C)))


@functools.lru_cache(maxsize=None)
def confusion_case(C):
    """Labels [nk, m] and truth [m] over C classes, some of both outside [0, C),
    and the expected confusion matrices."""
    rng = np.random.default_rng(40 + C)
    nk, m = 3, SYN_M
    labels = rng.integers(-1, C, (nk, m)).astype(np.int32)
    truth = rng.integers(0, C, m).astype(np.int32)
    truth[::41] = C + 2
    conf, unl = evalcases.confusion(labels, truth, C)
    return _freeze(dict(labels=labels, truth=truth, C=C, conf=conf, unl=unl))


CONFUSION_CS = (10, evalcases.SMALL_C + 1, evalcases.LDS_C + 1)
COUNTS_CS = (3, evalcases.COUNTS_LDS_C + 1)


@functools.lru_cache(maxsize=None)
def normalize_case():
    """Two sets for minmax (init = 1, then init = 0) and the oracle's bounds and
    normalised first set (oracle.normalize scans train, then test)."""
    rng = np.random.default_rng(808)
    d = 137
    x1 = rng.normal(0, 3, (1031, d))
    x2 = rng.normal(0, 5, (257, d))
    x1[:, 0] = 2.5                           # constant dim: untouched
    x2[:, 0] = 2.5
    w1, w2 = x1.copy(), x2.copy()
    oracle.normalize(w1, w2, None)
    mx = np.maximum(np.maximum(x1.max(0), x2.max(0)), -1.0)
    mn = np.minimum(np.minimum(x1.min(0), x2.min(0)), 999999.0)
    return _freeze(dict(x1=x1, x2=x2, want1=w1, mx=mx, mn=mn, d=d))


# ----------------------------------------------------------- part B: the paths
AUTO, FP32, BF16X3, FP16 = 0, 1, 2, 3
PATH_K = 10
# id: (set, metric, precision, tuning, candidate path(s), kernel-name pattern)
# cand_kernel<DP, R, kernel metric, waves>: the third parameter names the pass
PATHS = {
    "fp32-resident": ("gauss128", L2, FP32, {}, (0,), r"cand_kernel<128,\d+,0,\d+>"),
    "fp32-stream-d300": ("gauss300", L2, FP32, {}, (0,), r"cand_stream_kernel<\d+,\d+,0>"),
    "bf16x3-32x32x16": ("gauss128", L2, BF16X3, {"mfma16": 0}, (2,), r"cand_kernel<128,\d+,2,\d+>"),
    "bf16x3-mfma16": ("gauss128", L2, BF16X3, {"mfma16": 1}, (3,), r"cand_kernel<128,\d+,3,\d+>"),
    "bf16x3-s3-d288": ("gauss288", L2, BF16X3, {}, (2,), r"cand_s3_kernel<\d+,false,\w+>"),
    "fp16-resident-gk0": ("gauss128", L2, FP16, {"gk": 0}, (4,), r"cand_kernel<128,\d+,4,\d+>"),
    "fp16-resident-gk1": ("gauss128", L2, FP16, {"gk": 1}, (4,), r"cand_kernel<128,\d+,4,\d+>"),
    "fp16-s3-d320": ("gauss320", L2, FP16, {"s3q": 1, "qres": 0}, (4,),
                     r"cand_s3_kernel<\d+,true,\w+>"),
    "fp16-qres-d320": ("gauss320", L2, FP16, {"s3q": 1, "qres": 1}, (4,), r"cand_qres_kernel<10>"),
    "int8-16x16x64": ("int128", L2, AUTO, {"i8": 1, "i8w": 0}, (5,), r"cand_kernel<128,\d+,5,\d+>"),
    "int8-32x32x32": ("int128", L2, AUTO, {"i8": 1, "i8w": 1}, (6,), r"cand_kernel<128,\d+,6,\d+>"),
    "l1-codes-d128": ("int128", L1, AUTO, {"i8l1": 1}, (7,), r"cand_sad_kernel<128,.*>"),
    "l1-codes-wide-d300": ("int300", L1, AUTO, {"i8l1": 2}, (7,), r"cand_sad_wide_kernel<.*>"),
    "l1-fix16": ("gauss128", L1, AUTO, {"u16l1": 1}, (8,), r"cand_fix16_kernel<128,.*>"),
    "l1-fp32": ("gauss128", L1, AUTO, {}, (1,), r"cand_kernel<128,\d+,1,\d+>"),
    "l1-fp32-stream-d300": ("gauss300", L1, AUTO, {}, (1,), r"cand_stream_kernel<\d+,\d+,1>"),
    "region-order5": ("int128", L2, AUTO, {"i8": 1, "i8w": 1, "order": 5}, (6,),
                      r"cand_kernel<128,\d+,6,\d+>"),
    "norm-blocks": ("int128", L2, AUTO, {"i8": 1, "i8w": 0, "nblk": 1}, (5,),
                    r"cand_kernel<128,\d+,5,\d+>"),
}
# the duplicate sets: the rescan filters (fp32; int8 on the 32x32x32 image) and
# the full exact scan
RESCANS = {
    "rescan-fp32-filter": ("dup_gauss", L2, AUTO, {}, (2, 3), r"cand_kernel<32,\d+,[23],\d+>"),
    "rescan-int8-filter": ("dup_int", L2, AUTO, {"i8": 1, "i8w": 1}, (6,),
                           r"cand_kernel<32,\d+,6,\d+>"),
}
KERNEL_FAMILIES = ("cand_kernel", "cand_stream_kernel", "cand_s3_kernel", "cand_qres_kernel",
                   "cand_sad_kernel", "cand_sad_wide_kernel", "cand_fix16_kernel")


def kernel_family(name):
    return re.match(r"\w+", name).group(0)


# ------------------------------------------------- the contract's entry points
def stream_entry_points(header_text):
    """Names of the functions of knn_amd.h that take a `void* stream`."""
    flat = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    return sorted(set(m.group(1) for m in
                      re.finditer(r"\bint\s+(knn_\w+)\s*\(([^;{]*?)\)\s*;", flat, flags=re.S)
                      if re.search(r"void\s*\*\s*stream", m.group(2))))

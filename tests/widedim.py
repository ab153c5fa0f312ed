"""Inputs above 1024 dims, and the arithmetic that shows they bite.  Plain
numpy, deterministic from a seed.

Above 256 dims a width pads to a multiple of 32 (fp32 stream kernel, fp16 S3)
or of 16 (bf16x3 S3) and runs the stream kernels; several paths change only
above 1024 dims ("Widths"):

  d > 1024    rescan_finish_fast_kernel reads the query in place; the wide L1
              code passes ("i8l1" = 2, "u16l1w" = 1) hand over to the fp32 L1
              stream kernel
  DP >= 2048  the wide rescan filter's LDS (8 (DP + 1) floats) passes 64 KiB
  d <= 4096   the merge stages the query in LDS (82 KiB at most), above it
              reads it in place
  DP >= 5120  the filter's 8 query rows no longer fit a CU's 160 KiB: it
              runs 4 queries per pass (rescan_wide_queries)

Isotropic Gaussian data at these widths has all distances nearly equal: no
reduced-precision pass could certify anything and only the rescan would run.
The rows here come from a low intrinsic dimension instead: Z @ A with Z in
R^{rows x 8} (class centres plus noise) and A in R^{8 x d}, rounded to the
1/1024 grid; the byte family is clip(rint(.), 0, 255).

Per width a family of constructions on one base set:
  plain  nothing special: most queries certify;
  dups   DUPS exact copies of train row 5, relabelled at random, and 16
         queries on it: more than kRescanCap rows at the k-th distance, so
         the fast rescan cannot finish those queries and the full scan runs
         (400 copies, test_rescan_paths_large_d's count, stay below
         kRescanCap = 1024 and are finished by the fast rescan: that count is
         the `near` construction's);
  near   NEAR rows equal to row 5 up to 1e-9 per coordinate and the same 16
         queries: uncertifiable (the proxies cannot tell them apart), fewer
         than kRescanCap rows within the filter's reach: the fast rescan
         finishes them;
and, apart from the families, ties(d): byte data with duplicated rows under
different labels and queries on them -- exact ties across the k-th place.
"""
import functools

import numpy as np

ZDIM = 8
CLASSES = 5
K_RESCAN_CAP = 1024      # knn_kernels.h kRescanCap
SPECIAL = 16             # queries placed on train row 5
ROW = 5
DUPS = 1100              # > kRescanCap
NEAR = 400               # < kRescanCap
FIRST = 300              # the copies are train rows [FIRST, FIRST + count)
TIE_PAIRS = 300          # ties: train row TIE_AT + i is a copy of row i
TIE_AT = 600
TIE_QUERIES = 24         # ties: query i sits on train row i

# d -> (n, m, k): ragged n (no multiple of 256), ragged m, k over {1, 10, 50};
# the oracle costs at most 2.4 GFLOP per case
SHAPES = {
    1025: (2999, 130, 10),   # first past 1024: DP 1056 (fp32, fp16 S3), 1040 (bf16x3 S3)
    1536: (2203, 33, 50),    # an embedding width
    2016: (1901, 33, 10),    # the wide filter's LDS just under 64 KiB ...
    2048: (1901, 130, 1),    # ... and just over
    3072: (1777, 33, 10),    # raw CIFAR bytes' width (continuous data here)
    4096: (1733, 33, 50),    # the last width whose query the merge stages in LDS ...
    4097: (1733, 130, 10),   # ... and the first it reads in place
    5088: (1699, 33, 50),    # the last DP with 8 filter queries in 160 KiB ...
    5089: (1699, 33, 10),    # ... and the first with 4 (DP 5120)
    6000: (1651, 33, 10),    # clearly beyond
}
BYTES = "3072b"              # byte data at d = 3072
SHAPES[BYTES] = (1777, 33, 10)
WIDTHS = tuple(SHAPES)
# k = n - 1 on a small set (every row re-ranked, C2 = 1024: the merge's
# largest LDS footprint) and a single query
KMAX = dict(d=2048, n=601, m=1, k=600)

# the configurations of test_gpu_widedim.py: name -> (precision name, tuning)
CONFIGS = {
    "fp32": ("FP32", {}),
    "bf16x3": ("BF16X3", {}),
    "auto": ("AUTO", {}),
    "fp16": ("FP16", {}),
    "fp16w": ("FP16", {"s3q": 0}),
    "fp16qres": ("FP16", {"qres": 1}),
}


def dim_of(width):
    return 3072 if width == BYTES else int(width)


# ---------------------------------------------------------------- padding
def pad_fp32(d):
    """pad_dim above 256 dims: the stream kernel's 32-dim chunks."""
    return (d + 31) // 32 * 32


def pad_bf16x3(d):
    """pad_dim_bf16x3 above 256 dims: any multiple of 16."""
    return (d + 15) // 16 * 16


def pad_fp16_s3(d):
    """pad_dim_fp16_s3: any multiple of 32."""
    return (d + 31) // 32 * 32


def rescan_wide_queries(DP, lds_limit=160 * 1024):
    """knn_plan.cpp rescan_wide_queries: the wide filter's queries per pass."""
    for fqw in (8, 4, 2, 1):
        if fqw * (DP + 1) * 4 + 128 <= lds_limit:
            return fqw
    return 0


def merge_lds_bytes(d, C2, NT):
    """launch_mr's dynamic LDS with the query row staged (d <= 4096)."""
    return (d if d <= 4096 else 0) * 8 + C2 * 8 + min(NT, C2) * 17 * 8 + C2 * 8


# ------------------------------------------------------------- error bounds
def err_factor(kmetric, DP):
    """knn_plan.cpp err_factor for kernel metrics 0, 1, 2 and 4."""
    u = 2.0 ** -24
    u2 = 2.0 ** -23
    if kmetric == 4:
        n = DP + 1
        return n * u2 / (1.0 - n * u2) * 1.02
    if kmetric == 2:
        n = 3 * DP + 1
        return (n * u2 / (1.0 - n * u2) + 2.0 ** -15) * 1.02
    n = DP + 1 if kmetric == 0 else DP
    gam = n * u / (1.0 - n * u)
    return (gam + (5.0 if kmetric == 0 else 3.0) * u) * 1.01


class Operands:
    """The centred operands of a train set as build_train forms them: column
    means rounded to the 2^-(jx+2) grid, scale 2^jx with max |x - mu| 2^jx in
    [2^8, 2^9), and the fp16 operands' measured representation error."""

    def __init__(self, train):
        mu = train.mean(axis=0)
        amax = np.abs(train - mu).max()
        e = int(np.frexp(amax)[1]) if amax > 0 else 0
        self.jx = min(9 - e, 450)
        g = 2.0 ** (self.jx + 2)
        self.mu = np.rint(mu * g) / g
        x = train - self.mu
        self.x2max = float((x * x).sum(axis=1).max())
        self.x1max = float(np.abs(x).sum(axis=1).max())
        s = 2.0 ** self.jx
        with np.errstate(over="ignore"):
            dx = (x * s).astype(np.float16).astype(np.float64) / s - x
        self.dxmax = float(np.sqrt((dx * dx).sum(axis=1).max())) + 2.0 ** -50 * np.sqrt(self.x2max)

    def fp16_bound(self, q, DP):
        """E of merge_rerank_kernel for fp16 operands:
        accumulation (err_factor(4, DP)), the seed's rounding, and the train
        and query operands' representation errors."""
        x = q - self.mu
        qn = float(np.sqrt((x * x).sum()))
        s = 2.0 ** self.jx
        with np.errstate(over="ignore"):
            op = (-2.0 * x * s).astype(np.float16).astype(np.float64)
        dq = float(np.sqrt(((op * (-0.5 / s) - x) ** 2).sum())) + 2.0 ** -50 * qn
        xm = np.sqrt(self.x2max)
        f = err_factor(4, DP)
        return (f * (self.x2max + 2.0 * (qn + dq) * (xm + self.dxmax) * 1.001) +
                3.01 * 2.0 ** -24 * self.x2max +
                2.0 * (qn * self.dxmax + dq * (xm + self.dxmax)) * 1.001)

    def filter_slack(self, q, metric, DP):
        """How far beyond tau (L2: tau^2) the fast rescan's fp32 filter may
        reach: its threshold adds E = f (x2max + 2.1 |q'| xmax) (L1: f (|q'|_1
        + x1max)) and a row's proxy is within E of its exact value."""
        x = q - self.mu
        if metric == 0:
            qn = float(np.sqrt((x * x).sum()))
            return 2.0 * err_factor(0, DP) * (self.x2max + 2.1 * qn * np.sqrt(self.x2max))
        return 2.0 * err_factor(1, DP) * (float(np.abs(x).sum()) + self.x1max)


# ------------------------------------------------------------------- data
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _seed(width):
    return 7000 + dim_of(width) + (1 if width == BYTES else 0)


def low_rank(rng, rows, d, classes=CLASSES):
    """rows x d values Z @ A: Z = class centres (uniform in [-1.5, 1.5]^8) plus
    standard normal noise, A standard normal / sqrt(8); the class of each row."""
    cls = rng.integers(0, classes, rows)
    centres = rng.uniform(-1.5, 1.5, (classes, ZDIM))
    Z = centres[cls] + rng.standard_normal((rows, ZDIM))
    A = rng.standard_normal((ZDIM, d)) / np.sqrt(ZDIM)
    return Z @ A, cls.astype(np.int32)


@functools.lru_cache(maxsize=2)
def base(width):
    """(train, labels, queries, k) of a width's plain construction (read-only)."""
    n, m, k = SHAPES[width]
    d = dim_of(width)
    rng = _rng(_seed(width))
    X, cls = low_rank(rng, n + m, d)
    if width == BYTES:
        X = np.clip(np.rint(128.0 + 40.0 * X), 0, 255)
    else:
        X = np.round(X * 1024.0) / 1024.0
    tr, te, lab = np.ascontiguousarray(X[:n]), np.ascontiguousarray(X[n:]), cls[:n].copy()
    for a in (tr, te, lab):
        a.setflags(write=False)
    return tr, lab, te, k


KINDS = ("plain", "dups", "near")


def case(width, kind):
    """(train, labels, queries, k) of a width's construction; fresh arrays
    except for `plain` (shared, read-only)."""
    tr, lab, te, k = base(width)
    if kind == "plain":
        return tr, lab, te, k
    rng = _rng(_seed(width) + {"dups": 11, "near": 12}[kind])
    tr, lab, te = tr.copy(), lab.copy(), te.copy()
    d = tr.shape[1]
    if kind == "dups":
        tr[FIRST:FIRST + DUPS] = tr[ROW]
        lab[FIRST:FIRST + DUPS] = rng.integers(0, CLASSES, DUPS)
        te[:SPECIAL] = tr[ROW]
    elif kind == "near":
        tr[FIRST:FIRST + NEAR] = tr[ROW] + rng.standard_normal((NEAR, d)) * 1e-9
        lab[FIRST:FIRST + NEAR] = rng.integers(0, CLASSES, NEAR)
        te[:SPECIAL] = tr[ROW]
    else:
        raise ValueError(kind)
    return tr, lab, te, k


def ties(d, n=1777, m=33):
    """Byte data at width d with TIE_PAIRS duplicated rows under other labels
    and TIE_QUERIES queries on them: (train, labels, queries)."""
    rng = _rng(9000 + d)
    X, cls = low_rank(rng, n + m, d)
    X = np.clip(np.rint(128.0 + 40.0 * X), 0, 255)
    tr, te, lab = np.ascontiguousarray(X[:n]), np.ascontiguousarray(X[n:]), cls[:n].copy()
    tr[TIE_AT:TIE_AT + TIE_PAIRS] = tr[:TIE_PAIRS]
    lab[TIE_AT:TIE_AT + TIE_PAIRS] = (lab[:TIE_PAIRS] + 1 +
                                      rng.integers(0, CLASSES - 1, TIE_PAIRS)) % CLASSES
    te[:TIE_QUERIES] = tr[:TIE_QUERIES]
    return tr, lab, te


TIE_WIDTHS = (3072, 5089)


def sized(d, n, m, seed):
    """A plain low-rank set of any shape on the 1/1024 grid (the further tests
    of test_gpu_widedim.py: large k, shards, sweeps, the context walk)."""
    rng = _rng(seed)
    X, cls = low_rank(rng, n + m, d)
    X = np.round(X * 1024.0) / 1024.0
    return np.ascontiguousarray(X[:n]), cls[:n].copy(), np.ascontiguousarray(X[n:]), cls[n:].copy()


# --------------------------------------------------------------- the plan
def rerank_window(k, n):
    """C of plan_search before the lists cap it: max(2W, W + 16), W = k + 1."""
    W = k + 1
    return min(n, max(2 * W, W + 16), 1024)


def _list_len(W, n_tiles, lps):
    """choose_geometry's R for the stream kernels (lists of 8 where a split
    count S >= 5 W / (4 lps) exists among min(64, n_tiles), else 16)."""
    s8 = (W * 5 + 4 * lps - 1) // (4 * lps)
    return 8 if s8 <= min(64, n_tiles) else 16


def kernel_name(config, metric, n, k):
    """The candidate kernel plan_search names above 1024 dims (W <= 1001)."""
    W = k + 1
    prec, tune = CONFIGS[config]
    n_stream = (n + 255) // 256 * 256 // 128     # 128-row tiles of the fp32 image
    n_s3 = (n + 255) // 256                      # 256-row tiles of the S3 images
    if metric == 1 or prec == "FP32":
        return "cand_stream_kernel<32,%d,%d>" % (_list_len(W, n_stream, 2), metric)
    if prec == "BF16X3":
        return "cand_s3_kernel<%d,false,false>" % _list_len(W, n_s3, 2)
    # fp16 S3 (AUTO takes it above 256 dims): quad lists of 8 on 16x16x32
    # where 5 W / 16 splits exist (and "s3q" allows), else the 32x32x16 form
    s3q_S = (W * 5 + 15) // 16
    if tune.get("s3q", -1) != 0 and s3q_S <= 32 and s3q_S <= n_s3:
        return "cand_s3_kernel<8,true,true>"
    return "cand_s3_kernel<%d,true,false>" % _list_len(W, n_s3, 2)

"""Inputs at the numeric edges of operand preparation and of AUTO's path
choice (knn_prep.hip; build_train, detect_i8, use_fp16 / use_i8 and auto_check
in knn_api.cpp), and their oracle results.  Plain numpy on top of
test_gpu_parity's generators, deterministic from a seed; test_numedge_data.py
checks on the CPU what test_gpu_numedge.py takes for granted.

  degenerate   train sets whose spread max |x - mu| is 0 or nearly (operand
               scale 2^jx at its cap, the frexp that a zero maximum skips);
  ladder       one continuous case scaled by 2^e: exact scalings (nothing
               under- or overflows) and scalings under which squares go
               denormal, flush to zero, or the inputs themselves are denormal;
  range        |x - mean| just below and just above the 2^400 the library
               accepts;
  aniso        features whose scales span 2^-40: the small dimensions leave
               the fp16 / fp32 operand range and only the bound's absolute
               terms cover them; clusters separated in those dimensions only;
  overflow     finite queries whose reference distance to every row is +inf;
  grid_*       integer-coded train sets on either side of each limit of the
               int8 grid detection, and queries at the edge of the code range;
  offset40     continuous data under per-dimension offsets of about 2^40;
  auto_*       batches of 4096 queries that keep or retire AUTO's int8 / fp16
               pass.
"""
import numpy as np

import oracle
from test_gpu_parity import _grid_codes, _mix

CLASSES = 5

# ------------------------------------------------------------ 1. operand scale
DEGENERATE = ("deg_one", "deg_same", "deg_onedim")
LADDER_EXACT = (-300, 300, 390)      # nothing under- or overflows: metamorphic
LADDER_LOSSY = (-1060, -600, -520)   # inputs denormal / squares flush / squares denormal
LADDER_K = 10
RANGE_LIMIT = 400                    # build_train: |x - mean| < 2^400
ANISO = {"aniso16": 16, "aniso300": 300}
ANISO_K = 10
ANISO_SMALL = 33                     # dimensions scaled by <= 2^-33 separate the clusters
OVERFLOW_Q = {0: (3, 17, 40), 1: (5, 29)}   # metric: the overflowing queries


def _rng(seed):
    return np.random.default_rng(seed)


def _degenerate(name):
    rng = _rng(2101)
    d, m = 16, 40
    base = np.round(rng.standard_normal(d) * 64) / 64
    n = 1 if name == "deg_one" else 300
    tr = np.tile(base, (n, 1))
    if name == "deg_onedim":
        # rows differ in dimension 3 only, by multiples of 2^-30 (37 levels:
        # ties among the rows of a level, distinct distances across levels)
        tr[:, 3] += (np.arange(n) % 37) * 2.0 ** -30
    lab = rng.integers(0, CLASSES, n).astype(np.int32)
    te = base + rng.standard_normal((m, d))
    te[:6] = base                     # queries sitting on the rows
    te[6:10] = base
    te[6:10, 3] += 2.0 ** -31         # between two levels of deg_onedim
    return tr, lab, np.ascontiguousarray(te)


def degenerate_ks(name):
    n = case(name)[0].shape[0]
    return sorted({1, min(7, n), n})


def _ladder_base():
    return _mix(_rng(2102), 4000, 200, 24, CLASSES)


def _ladder(e):
    tr, lab, te = case("ladder0")
    return np.ldexp(tr, e), lab, np.ldexp(te, e)


def _range(above):
    """_mix rows scaled so that max |x - column mean| is 2^400 (1 -+ 2^-20):
    the margin is far beyond the rounding of the mean (1e-16 relative)."""
    tr, lab, te = _mix(_rng(2103), 600, 50, 8, CLASSES)
    a = np.abs(tr - tr.mean(axis=0)).max()
    s = 2.0 ** RANGE_LIMIT / a * (1.0 + (1 if above else -1) * 2.0 ** -20)
    return tr * s, lab, te * s


def aniso_scales(d):
    return 2.0 ** -((4 * np.arange(d)) % 44).astype(np.float64)


def _aniso(d):
    """Bulk: standard normal rows times the per-dimension scales 2^-(4 i mod
    44).  Two clusters (40 and 600 train rows, 4 queries each): every point
    of a cluster equals its centre in the dimensions scaled by more than
    2^-33 and is N(0, 1) x scale in the others, so (q_i - x_i) is exactly 0
    in the large dimensions and the reference's distance is the plain sum
    over the small ones.  Returns (train, labels, queries, info): info[i] is
    the cluster size of query i, or 0 for a bulk query."""
    rng = _rng(2104 + d)
    sc = aniso_scales(d)
    small = sc <= 2.0 ** -ANISO_SMALL
    train = [rng.standard_normal((3000, d)) * sc]
    queries, info = [], []
    for size in (40, 600):
        pts = np.tile(rng.standard_normal(d) * sc, (size + 4, 1))
        pts[:, small] = rng.standard_normal((size + 4, int(small.sum()))) * sc[small]
        train.append(pts[:size])
        queries.append(pts[size:])
        info += [size] * 4
    queries.append(rng.standard_normal((40, d)) * sc)
    info += [0] * 40
    train = np.concatenate(train)
    train = np.ascontiguousarray(train[rng.permutation(train.shape[0])])
    lab = rng.integers(0, CLASSES, train.shape[0]).astype(np.int32)
    return train, lab, np.ascontiguousarray(np.concatenate(queries)), info


def _overflow(metric):
    tr, lab, te = _mix(_rng(2105), 3000, 60, 16, CLASSES)
    tr -= 0.5                         # train values of both signs
    te -= 0.5
    for i, q in enumerate(OVERFLOW_Q[metric]):
        if metric == 0:
            te[q, 5 + i] = 1e160 if i % 2 == 0 else -1e160   # squares to +inf
        else:
            te[q, 2] = 1.5e308        # |q - x| finite, their sum +inf
            te[q, 9] = -1.5e308
    return tr, lab, te


# ------------------------------------------------------ 2. int8 grid detection
GRID_N, GRID_M, GRID_K = 6000, 300, 10
# the limits of detect_i8 (knn_api.cpp): fractional bits, code span, magnitude
GRID_MAX_FRAC, GRID_MAX_SPAN, GRID_MAX_ABS = 30, 255, 2.0 ** 50
GRID_MAX_D = 256
# name: does the detection accept the train set?
GRID_CASES = {
    "grid_span255": True, "grid_span256": False,
    "grid_half254": True, "grid_half257": False,
    "grid_frac30": True, "grid_frac31": False,
    "grid_offsets": True, "grid_big": False,
    "grid_const1": True, "grid_const33": True, "grid_const200": True, "grid_const256": True,
    "grid_d257": False,
}
# query edges on grid_span255 (dimension 0: codes 0..255 at scale 1/256,
# centre 128): block b of 30 queries has dimension 0 at EDGE_CODES[b] codes
# from the centre; the rest of the batch is interior
EDGE_BLOCK = 30
EDGE_CODES = (-128, 127, -129, 128, -1128, 1127)
EDGE_OFFGRID = (6 * EDGE_BLOCK, 7 * EDGE_BLOCK)   # 2^-31 off a grid point


def _codes(rng, n, m, d, lo, hi):
    """_grid_codes' shape at scale 1: integer codes in [lo, hi]."""
    return _grid_codes(rng, n, m, d, CLASSES, lo=lo, hi=hi, scale=1.0)


def _span_case(rng, d=48):
    """Codes 0..200 in every dimension but 0, which is uniform over 0..255
    (both ends present); scale 1/256."""
    tr, lab, te = _codes(rng, GRID_N, GRID_M, d, 0, 200)
    tr[:, 0] = rng.integers(0, 256, GRID_N)
    te[:, 0] = rng.integers(0, 256, GRID_M)
    tr[11, 0], tr[4321, 0] = 0.0, 255.0
    return tr / 256.0, lab, te / 256.0


def _grid(name):
    rng = _rng(2200 + sorted(GRID_CASES).index(name))
    if name in ("grid_span255", "grid_span256"):
        tr, lab, te = _span_case(rng)
        if name == "grid_span256":
            tr[4321, 0] = 256.0 / 256.0           # one code further
        return tr, lab, te
    if name in ("grid_half254", "grid_half257"):
        top = 127 if name == "grid_half254" else 128
        tr, lab, te = _codes(rng, GRID_N, GRID_M, 48, 0, top)
        tr[5, 1], tr[6, 1] = 0.0, float(top)      # the whole range in one dimension
        tr[777, 1] = 63.5 if name == "grid_half254" else top + 0.5
        return tr, lab, te
    if name in ("grid_frac30", "grid_frac31"):
        tr, lab, te = _codes(rng, GRID_N, GRID_M, 48, 0, 255)
        tr[5, 1], tr[6, 1], tr[7, 1] = 0.0, 255.0, 101.0   # (an odd code: s = 30)
        if name == "grid_frac31":
            tr[777, 2] += 0.5                     # 31 fractional bits after the scaling
        return np.ldexp(tr, -30), lab, np.ldexp(te, -30)
    if name in ("grid_offsets", "grid_big"):
        d = 48
        tr, lab, te = _codes(rng, GRID_N, GRID_M, d, 0, 255)
        off = np.rint(rng.uniform(-1.0, 1.0, d) * 2.0 ** 49)
        off[0], off[1] = 2.0 ** 49 - 1, -(2.0 ** 49 - 1)
        if name == "grid_big":
            off[7] = 2.0 ** 50                    # |hi| >= 2^50 in one dimension
        return tr + off, lab, te + off
    d = int(name[len("grid_const"):] if name.startswith("grid_const") else name[len("grid_d"):])
    tr, lab, te = _codes(rng, GRID_N, GRID_M, d, 0, 255)
    if name.startswith("grid_const") and d > 1:
        for c in range(1, d, 3):                  # constant dimensions (span 0)
            tr[:, c] = te[:, c] = float(c % 200)
    return tr / 256.0, lab, te / 256.0


def _grid_edges():
    tr, lab, te = case("grid_span255")
    te = te.copy()
    for b, code in enumerate(EDGE_CODES):
        te[b * EDGE_BLOCK:(b + 1) * EDGE_BLOCK, 0] = (128 + code) / 256.0
    te[EDGE_OFFGRID[0]:EDGE_OFFGRID[1], 0] += 2.0 ** -31
    return tr, lab, te


def frac_bits(x):
    """Largest number of fractional bits of any value of x (0 for integers),
    or 64 if beyond 63: the s of `x = c / 2^s`."""
    x = np.abs(np.asarray(x, np.float64)).ravel()
    for s in range(64):
        y = np.ldexp(x, s)
        if (y == np.floor(y)).all():
            return s
    return 64


def grid_rule(train):
    """(accept, s, largest per-dimension code span, largest |code|) of a
    train set under the int8 rule of knn_amd.h -- every value c / 2^s with the
    codes of each dimension spanning <= 255 -- with the limits detect_i8 puts
    on it (s <= 30, |codes| < 2^50, d <= 256), recomputed in numpy."""
    s = frac_bits(train)
    codes = np.ldexp(train, min(s, 63))
    span = float((codes.max(axis=0) - codes.min(axis=0)).max())
    top = float(np.abs(codes).max())
    ok = (s <= GRID_MAX_FRAC and span <= GRID_MAX_SPAN and top < GRID_MAX_ABS
          and train.shape[1] <= GRID_MAX_D)
    return ok, s, span, top


# ------------------------------------------- 3. large offset, continuous data
def _offset40():
    tr, lab, te = _mix(_rng(2301), 4000, 200, 40, CLASSES)
    rng = _rng(2302)
    off = rng.uniform(1.0, 2.0, 40) * 2.0 ** 40 * rng.choice([-1.0, 1.0], 40)
    return tr + off, lab, te + off


# ------------------------------------------------ 4. AUTO choice, retirement
AUTO_N, AUTO_M, AUTO_D, AUTO_K, AUTO_BAD = 9000, 4096, 64, 10, 400
AUTO_CLASSES = 7


def _auto(name):
    """auto_grid / auto_cont: batch A.  auto_grid_b: A with the first 400
    queries 1000 codes beyond the code range in dimension 0;
    auto_cont_b: A with the first 400 queries scaled by 1e4 (beyond the fp16
    operand range: void proxies)."""
    if name == "auto_grid":
        return _grid_codes(_rng(2401), AUTO_N, AUTO_M, AUTO_D, AUTO_CLASSES)
    if name == "auto_cont":
        return _mix(_rng(2402), AUTO_N, AUTO_M, AUTO_D, AUTO_CLASSES)
    tr, lab, te = case(name[:-2])
    te = te.copy()
    if name == "auto_grid_b":
        te[:AUTO_BAD, 0] = (255.0 + 1000.0) / 256.0
    else:
        te[:AUTO_BAD] *= 1e4
    return tr, lab, te


# ------------------------------------------------------------------- accessors
_data = {}
_oracle = {}


def classes(name):
    return AUTO_CLASSES if name.startswith("auto_") else CLASSES


def case(name):
    """(train, labels, queries[, info]) of a named case; built once per
    process and shared (read-only arrays)."""
    if name not in _data:
        if name in DEGENERATE:
            out = _degenerate(name)
        elif name == "ladder0":
            out = _ladder_base()
        elif name.startswith("ladder"):
            out = _ladder(int(name[len("ladder"):]))
        elif name in ("range_below", "range_above"):
            out = _range(name == "range_above")
        elif name in ANISO:
            out = _aniso(ANISO[name])
        elif name in ("overflow_l2", "overflow_l1"):
            out = _overflow(0 if name == "overflow_l2" else 1)
        elif name in GRID_CASES:
            out = _grid(name)
        elif name == "grid_edges":
            out = _grid_edges()
        elif name == "offset40":
            out = _offset40()
        elif name.startswith("auto_"):
            out = _auto(name)
        else:
            raise KeyError(name)
        for a in out[:3]:
            a.setflags(write=False)
        _data[name] = out
    return _data[name]


def oracle_knn(name, k, metric, n_out=None):
    """(labels, idx[m, n_out], dist[m, n_out]) of the oracle for a named case;
    n_out defaults to k.  Computed once, shared, left unchanged.  The *_b
    batches of section 4 differ from their batch A in the first AUTO_BAD
    queries only: the rest is taken from A's result."""
    n_out = k if n_out is None else n_out
    key = (name, k, metric, n_out)
    if key not in _oracle:
        tr, lab, te = case(name)[:3]
        if name in ("auto_grid_b", "auto_cont_b"):
            head = oracle.knn(tr, lab, te[:AUTO_BAD], k, metric == 0, classes(name), n_out=n_out)
            rest = oracle_knn(name[:-2], k, metric, n_out)
            out = [np.concatenate([h, r[AUTO_BAD:]]) for h, r in zip(head, rest)]
        else:
            out = list(oracle.knn(tr, lab, te, k, metric == 0, classes(name), n_out=n_out))
        for a in out:
            a.setflags(write=False)
        _oracle[key] = out
    return _oracle[key]

"""Inputs of test_gpu_l1kcap.py: parity at k = 101 .. 1000 (W = k + 1 up to
1001) on the three L1 code passes -- candidate path 7 on byte codes
(cand_sad_kernel, "i8l1" = 1), its wide form at 256 < d <= 1024
(cand_sad_wide_kernel, "i8l1" = 2) and path 8 on 16-bit fixed-point codes
(cand_fix16_kernel, "u16l1" = 1) -- and their oracle results.

The case table extends tests/kcap.py's: a name found there is kcap's own case
(same arrays, same oracle cache), the others are built the same way from
test_gpu_parity's generators.  Continuous cases (`_mix`) go to path 8 and
have strictly increasing L1 oracle distances; grid cases (`_grid_codes`,
codes / 256) go to path 7 and tie inherently.  test_l1kcap_data.py checks on
the CPU what the GPU tests take for granted.
"""
import numpy as np

import kcap
import l1fix
import oracle
from test_gpu_parity import _grid_codes, _mix

CLASSES = kcap.CLASSES
GRID_S = 8  # _grid_codes: values code / 256, so the common scale is 2^8

# the passes: tuning keys, candidate path, kernel name (DP, R, NW filled in)
PASSES = {
    "sad": ({"i8l1": 1}, 7, "cand_sad_kernel<%(DP)d,%(R)d,%(NW)d>"),
    "wide": ({"i8l1": 2}, 7, "cand_sad_wide_kernel<%(R)d,%(NW)d>"),
    "fix16": ({"u16l1": 1}, 8, "cand_fix16_kernel<%(DP)d,%(R)d,%(NW)d>"),
}


def pad_dim(tag, d):
    """The padded width the pass runs at (pad_dim_i8w / _i8l1w / _u16l1)."""
    if tag == "wide":
        return (d + 15) // 16 * 16
    return next(p for p in (32, 64, 96, 128, 160, 192, 256) if p >= d)


def tile_rows(tag, d):
    """Train rows per tile of the kernel that runs (sad_tile_rows,
    sad_wide_tile_rows, fix16_tile_rows)."""
    DP = pad_dim(tag, d)
    if tag == "wide":
        return 64
    return (64 if DP > 128 else 128) if tag == "sad" else (64 if DP > 64 else 128)


def kernel_name(tag, d, R, NW):
    return PASSES[tag][2] % {"DP": pad_dim(tag, d), "R": R, "NW": NW}


# name: (generator, seed, n, m, d, largest W asked of it); kcap's names are
# not repeated here
CASES = {
    # section 1: the k ladder, one width on each side of every tile-row switch
    "grid200": ("grid", 2101, 20000, 96, 200, 1001),
    "grid300": ("grid", 2102, 20000, 64, 300, 1001),
    "ladder130": ("mix", 2103, 20000, 96, 130, 1001),
    # section 2: every (R, NW) form; m = 300 is a 256-query tile and a padded one
    "gforms100": ("grid", 2204, 8000, 300, 100, 151),
    "gforms300": ("grid", 2105, 8000, 300, 300, 151),
    "forms48": ("mix", 2106, 8000, 300, 48, 151),
    "forms128": ("mix", 2107, 8000, 300, 128, 151),
    # section 3: lists that cannot hold W (fewer than 32 tiles of 64 rows)
    "gsmall200": ("grid", 2608, 1500, 64, 200, 1001),
    "gsmall300": ("grid", 2909, 1500, 64, 300, 1001),
    "small130": ("mix", 2110, 1500, 64, 130, 1001),
    # (kcap's gsmall48 and gedge1000 hold a query whose code leaves the byte
    # about the train centre of its dim: the pass hands such queries over)
    "gsmall48b": ("grid", 2114, 3000, 64, 48, 1001),
    "gedge1000b": ("grid", 2115, 1000, 40, 16, 1000),
    # section 6: partial lists and the sharded merge on the grid
    "gpart32": ("grid", 2111, 12000, 64, 32, 1001),
    # section 8 / 9
    "gsweep300": ("grid", 2112, 8000, 70, 300, 1001),
    "gnonfin32": ("grid", 2113, 8000, 70, 32, 1001),
}
# section 4's small-n edges of the wide kernel: kcap.EDGES at d = 272.  Codes
# in [64, 191]: a few hundred rows do not reach both ends of the byte in each
# of 272 dims, and with a range of 127 codes every query code stays within a
# byte about the train centre whatever the sample
GRID_RANGE = {}
for _n, _k in kcap.EDGES:
    CASES["wedge%d" % _n] = ("grid", 2300 + _n, _n, 40, 272, min(_k + 1, _n))
    GRID_RANGE["wedge%d" % _n] = (64, 191)

# the kcap cases these tests run, with the largest W asked of them here
KCAP_CASES = {"ladder48": 1001, "grid48": 1001, "small48": 1001, "part32": 1001,
              "sweep40": 1001, "gsweep64": 1001, "nonfin32": 1001}
for _n, _k in kcap.EDGES:
    KCAP_CASES["edge%d" % _n] = min(_k + 1, _n)
    if _n != 1000:
        KCAP_CASES["gedge%d" % _n] = min(_k + 1, _n)

# section 1: pass, case, d
LADDER_KS = [101, 102, 103, 127, 128, 255, 256, 511, 512, 999, 1000]
WIDE_LADDER_KS = [101, 103, 256, 512, 1000]
LADDER = [("sad", "grid48"), ("sad", "grid200"), ("wide", "grid300"), ("fix16", "ladder48"),
          ("fix16", "ladder130")]
# section 2
FORMS = [("sad", "gforms100"), ("wide", "gforms300"), ("fix16", "forms48"), ("fix16", "forms128")]
FORMS_KS = (30, 150)
FORMS_BLOCK, FORMS_TILES = 64, 64  # the m = 4096 batch: 64 queries tiled 64 times
# section 3: pass, case
SMALL = [("sad", "gsmall48b"), ("sad", "gsmall200"), ("wide", "gsmall300"), ("fix16", "small48"),
         ("fix16", "small130")]


def edge_case(tag, n):
    """Section 4: the case of kcap.EDGES' n for a pass (d = 16, wide: 272)."""
    if tag == "sad":
        return "gedge1000b" if n == 1000 else "gedge%d" % n
    return ("wedge%d" if tag == "wide" else "edge%d") % n


# section 5 on the grid: (copies, [k, ...]); a variant (b) cannot exist there
GRID_RESCAN = {"a": (1500, [600]), "c": (700, [1000])}
GRID_RESCAN_SEED = {32: 2411, 300: 2412}
# section 8
SWEEP = [("sad", "gsweep64"), ("wide", "gsweep300"), ("fix16", "sweep40")]
SWEEP_KS = [1, 100, 101, 512, 1000]
LOO = [("sad", "gsmall48b"), ("fix16", "small48")]
LOO_KS = [1, 500, 999]

_data = {}
_oracle = {}
_models = {}


def spec(name):
    """(generator, seed, n, m, d, W) of a case of either table."""
    if name in CASES:
        return CASES[name]
    return kcap.CASES[name][:5] + (KCAP_CASES[name],)


def is_grid(name):
    if isinstance(name, tuple):
        return name[0] == "grescan"
    return spec(name)[0] == "grid"


def case(name):
    """(train, labels, queries), built once per process, read-only."""
    if name not in CASES:
        return kcap.case(name)
    if name not in _data:
        kind, seed, n, m, d, _ = CASES[name]
        rng = np.random.default_rng(seed)
        if kind == "mix":
            sets = _mix(rng, n, m, d, CLASSES)
        else:
            lo, hi = GRID_RANGE.get(name, (0, 255))
            sets = _grid_codes(rng, n, m, d, CLASSES, lo=lo, hi=hi)
        _data[name] = kcap._freeze(sets)
    return _data[name]


def grid_rescan_case(d, variant):
    """kcap.rescan_case on the grid: _grid_codes(n = 6000, m = 64) with rows
    [1000, 1000 + copies) exact copies of row 5 under random labels and the
    first 16 queries sitting on row 5."""
    key = ("grescan", d, variant)
    if key not in _data:
        copies, _ = GRID_RESCAN[variant]
        rng = np.random.default_rng(GRID_RESCAN_SEED[d])
        tr, lab, te = _grid_codes(rng, kcap.RESCAN_N, kcap.RESCAN_M, d, CLASSES)
        lo, hi = kcap.RESCAN_AT, kcap.RESCAN_AT + copies
        tr[lo:hi] = tr[kcap.RESCAN_ROW]
        lab[lo:hi] = rng.integers(0, CLASSES, copies)
        te[:kcap.RESCAN_SITTING] = tr[kcap.RESCAN_ROW]
        _data[key] = kcap._freeze((tr, lab, te))
    return _data[key]


def _own(name):
    return name in CASES or name == "ties" or (isinstance(name, tuple) and name[0] == "grescan")


def arrays(name):
    if name == "ties":
        return tie_order_sets()
    if isinstance(name, tuple):
        return grid_rescan_case(*name[1:]) if name[0] == "grescan" else kcap.rescan_case(*name[1:])
    return case(name)


def oracle_knn(name, k, n_out=None):
    """(labels, idx[m, n_out], dist[m, n_out]) of the L1 oracle for a case of
    either table, ("rescan", d, variant), ("grescan", d, variant) or "ties"
    (tie_order_sets); computed once, shared (kcap's cache for kcap's cases),
    left unchanged."""
    if not _own(name):
        return kcap.oracle_knn(name, k, 1, n_out)
    n_out = k if n_out is None else n_out
    key = (name, k, n_out)
    if key not in _oracle:
        tr, lab, te = arrays(name)
        _oracle[key] = kcap._freeze(list(oracle.knn(tr, lab, te, k, False, CLASSES, n_out=n_out)))
    return _oracle[key]


def grid_codes(tr, te, s=GRID_S):
    """Path 7's operands as l1codes.proxy_model derives them -- the centre
    floor((lo + hi + 1) / 2) of the scaled train range per dim, signed codes,
    top bit flipped -- as int16 arrays (train [n, d], queries [m, d]), so that
    a query's proxies against 20000 rows cost one small array.  Raises if a
    value is off the grid or a code leaves the byte."""
    T, Q = np.ldexp(tr, s), np.ldexp(te, s)
    cent = np.floor((T.min(0) + T.max(0) + 1.0) / 2.0)
    ct, cq = T - cent, Q - cent
    assert (ct == np.rint(ct)).all() and (cq == np.rint(cq)).all(), "off the grid"
    assert ct.min() >= -128 and ct.max() <= 127 and cq.min() >= -128 and cq.max() <= 127
    flip = lambda c: ((c.astype(np.int64) & 0xFF) ^ 0x80).astype(np.int16)  # noqa: E731
    return flip(ct), flip(cq)


def grid_proxies(ut, uq, q):
    """Integer proxies of query q against every train row (int64 [n])."""
    return np.abs(ut - uq[q]).sum(1, dtype=np.int64)


def fix16_model(name):
    """l1fix.Model of a continuous case, built once."""
    if name not in _models:
        tr, _, te = arrays(name)
        _models[name] = l1fix.Model(tr, te)
    return _models[name]


def window_counts(sorted_prox, W, slack):
    """Rows whose proxy is at most the W-th smallest + slack (proxies sorted)."""
    return int(np.searchsorted(sorted_prox, sorted_prox[W - 1] + slack, side="right"))


def tie_order_sets():
    """test_tie_order_large_k's integer data under L1: 5000 x 12 train rows,
    300 queries, full of exact ties."""
    if "ties" not in _data:
        rng = np.random.default_rng(72)
        centres = rng.integers(0, 256, (5, 12))
        lab = rng.integers(0, 5, 5300).astype(np.int32)
        X = np.clip(centres[lab] + rng.integers(-5, 6, (5300, 12)), 0, 255).astype(np.float64)
        _data["ties"] = kcap._freeze((X[:5000].copy(), lab[:5000].copy(), X[5000:].copy()))
    return _data["ties"]

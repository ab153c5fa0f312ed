"""Inputs of test_gpu_kcap.py: parity at k = 101 .. 1000 (W = k + 1 up to 1001,
the candidate pipeline's capacity limits), and their oracle results.  Plain
numpy on top of test_gpu_parity's generators, deterministic from a seed;
test_kcap_data.py checks on the CPU what the GPU tests take for granted.

Continuous cases (`_mix`): every query's first W oracle distances are strictly
increasing (W the largest the GPU tests ask of the case), so the GPU tests
demand index-for-index equality and no tie flag.  Grid cases (`_grid_codes`,
the int8 paths' data) tie inherently and go through the parity suite's tie
rules.  rescan_case() plants exact or near duplicates of one row under 16
queries: more rows within reach of the W-th distance than the fast rescan
keeps (a, b), or few enough for it to finish (c).
"""
import numpy as np

import oracle
from test_gpu_parity import _grid_codes, _mix

CLASSES = 5

# name: (generator, seed, n, m, d, largest W asked of it)
CASES = {
    # section 1: the k ladder (d = 64: the smallest width >= 48 that has a
    # bf16x3 kernel on the 16x16x32 layout, which needs DP % 32 == 0)
    "ladder48": ("mix", 1101, 20000, 96, 48, 1001),
    "ladder64": ("mix", 1102, 20000, 96, 64, 1001),
    "grid48": ("grid", 1103, 20000, 96, 48, 1001),
    "grid96": ("grid", 1104, 20000, 96, 96, 1001),
    # section 2: d > 256 (320: a width the query-resident kernel serves as is)
    "ladder300": ("mix", 1105, 20000, 64, 300, 1001),
    "qres320": ("mix", 1106, 20000, 64, 320, 102),
    # section 3: forced wide union
    "wide24": ("mix", 1107, 20000, 64, 24, 601),
    # section 4: lists that cannot hold W
    "small48": ("mix", 1108, 3000, 64, 48, 1001),
    "gsmall48": ("grid", 1109, 3000, 64, 48, 1001),
    "gsmall96": ("grid", 1110, 3000, 64, 96, 1001),
    # section 6: partial lists and the sharded merge
    "part32": ("mix", 1111, 12000, 64, 32, 1001),
    # section 7: sweep
    "sweep40": ("mix", 1112, 8000, 130, 40, 1001),
    "gsweep64": ("grid", 1113, 8000, 130, 64, 1001),
    "nonfin32": ("mix", 1114, 8000, 70, 32, 1001),
}
# section 4's small-n edges: (n, k) at d = 16, m = 40
EDGES = [(1000, 1000), (1001, 1000), (1024, 1000), (1025, 1000), (257, 256), (300, 299)]
for _n, _k in EDGES:
    CASES["edge%d" % _n] = ("mix", 1200 + _n, _n, 40, 16, min(_k + 1, _n))
    CASES["gedge%d" % _n] = ("grid", 1300 + _n, _n, 40, 16, min(_k + 1, _n))

# section 5: rescan at large W; (copies, noise, [k, ...]) per variant
RESCAN = {"a": (1500, 0.0, [600]), "b": (1500, 1e-9, [600, 1000]), "c": (700, 0.0, [1000])}
RESCAN_N, RESCAN_M, RESCAN_SITTING, RESCAN_ROW, RESCAN_AT = 6000, 64, 16, 5, 1000
RESCAN_SEED = {32: 1401, 300: 1402}

_data = {}
_oracle = {}


def is_grid(name):
    return CASES[name][0] == "grid"


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def case(name):
    """(train, labels, queries) of a named case; built once per process and
    shared (read-only arrays)."""
    if name not in _data:
        kind, seed, n, m, d, _ = CASES[name]
        rng = np.random.default_rng(seed)
        gen = _mix if kind == "mix" else _grid_codes
        _data[name] = _freeze(gen(rng, n, m, d, CLASSES))
    return _data[name]


def rescan_case(d, variant):
    """_mix(n = 6000, m = 64) with rows [1000, 1000 + copies) set to row 5
    (+ noise * N(0, 1) per coordinate), random labels on them, and the first
    16 queries sitting exactly on row 5."""
    key = ("rescan", d, variant)
    if key not in _data:
        copies, noise, _ = RESCAN[variant]
        rng = np.random.default_rng(RESCAN_SEED[d])
        tr, lab, te = _mix(rng, RESCAN_N, RESCAN_M, d, CLASSES)
        lo, hi = RESCAN_AT, RESCAN_AT + copies
        tr[lo:hi] = tr[RESCAN_ROW]
        if noise:
            tr[lo:hi] += noise * rng.standard_normal((copies, d))
        lab[lo:hi] = rng.integers(0, CLASSES, copies)
        te[:RESCAN_SITTING] = tr[RESCAN_ROW]
        _data[key] = _freeze((tr, lab, te))
    return _data[key]


def _arrays(name):
    return rescan_case(*name[1:]) if isinstance(name, tuple) else case(name)


def oracle_knn(name, k, metric, n_out=None):
    """(labels, idx[m, n_out], dist[m, n_out]) of the oracle for a named case
    (or ("rescan", d, variant)); n_out defaults to k.  Computed once, shared,
    left unchanged."""
    n_out = k if n_out is None else n_out
    key = (name, k, metric, n_out)
    if key not in _oracle:
        tr, lab, te = _arrays(name)
        _oracle[key] = _freeze(list(oracle.knn(tr, lab, te, k, metric == 0, CLASSES, n_out=n_out)))
    return _oracle[key]


def rerank_count(W, n):
    """Rows the merge re-ranks exactly where the lists can hold them:
    min(n, max(2W, W + 16), 1024)."""
    return min(n, max(2 * W, W + 16), 1024)

"""Row orders that steer the reference's std::sort, and a CPU port of it.

The reference orders a query's n records with libstdc++'s std::sort on the
distance alone (cpp:323/366); the library emulates that sort on the GPU
(knn_select.hip, ref_sort_prefix) for the queries whose label or neighbour
order depends on it.  On random data the sort sees a random permutation with
duplicates: introsort never reaches its depth limit there, and its partitions
never meet the orders at which an unguarded scan or a cut computed in
parallel could go wrong.  This module dictates the sequence instead.

With d = 1, a query at -c and non-negative integer train values x_i, row i's
distance is x_i + c bit for bit in both metrics (L2: sqrt((x + c)^2), L1:
|x + c|), so any sequence of integer keys, in any row order, can be put in
front of the sort through the public API (as_train()).

  std_sort_port   libstdc++ (GCC 11) std::sort over record ids in plain
                  Python, written from bits/stl_algo.h and bits/stl_heap.h,
                  with a trace of the ranges that took the heap-sort fallback;
  killer          McIlroy's adversary ("A Killer Adversary for Quicksort",
                  1999) run against the port: a row order on which the
                  median-of-3 introsort exhausts its depth limit;
  with_ties       integer division of the keys (tied groups);
  SEQUENCES       named edge orders, each a function of n.

test_sortorder_data.py pins the port to the oracle's real std::sort and
checks that the cases below do what they are meant to; test_gpu_sortorder.py
runs them on the GPU.
"""
import functools

import numpy as np

THRESHOLD = 16  # _S_threshold


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


class Trace:
    """What a std_sort_port run did: `heap` the (first, last) ranges that hit
    depth limit 0 and were heap-sorted, `depth` the deepest level of
    __unguarded_partition_pivot reached (the limit is 2 * floor(lg n))."""

    def __init__(self):
        self.heap = []
        self.depth = 0


def std_sort_port(keys=None, less=None, n=None, fallback="heap"):
    """std::sort(first, last, comp) of the records 0..n-1 in row order.

    `keys`: the record's key per row (compared with strict < only), or
    `less(i, j)`: a comparator on record ids (n given).  Returns (order,
    trace): order[p] is the record left at position p.

    `fallback` = "stable" replaces the heap sort of a range that ran out of
    depth by a stable sort of that range -- a WRONG std::sort, the model of a
    kernel whose fallback sorts correctly but not as libstdc++ does."""
    if less is None:
        kl = [float(v) for v in keys]
        n = len(kl)

        def less(i, j):
            return kl[i] < kl[j]
    a = list(range(n))
    tr = Trace()

    def move_median_to_first(result, x, y, z):
        if less(a[x], a[y]):
            if less(a[y], a[z]):
                m = y
            elif less(a[x], a[z]):
                m = z
            else:
                m = x
        elif less(a[x], a[z]):
            m = x
        elif less(a[y], a[z]):
            m = z
        else:
            m = y
        a[result], a[m] = a[m], a[result]

    def unguarded_partition(first, last, pivot):
        while True:
            while less(a[first], a[pivot]):
                first += 1
            last -= 1
            while less(a[pivot], a[last]):
                last -= 1
            if not first < last:
                return first
            a[first], a[last] = a[last], a[first]
            first += 1

    def push_heap(first, hole, top, value):
        parent = (hole - 1) // 2
        while hole > top and less(a[first + parent], value):
            a[first + hole] = a[first + parent]
            hole = parent
            parent = (hole - 1) // 2
        a[first + hole] = value

    def adjust_heap(first, hole, length, value):
        top = hole
        child = hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if less(a[first + child], a[first + child - 1]):
                child -= 1
            a[first + hole] = a[first + child]
            hole = child
        if length & 1 == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            a[first + hole] = a[first + child - 1]
            hole = child - 1
        push_heap(first, hole, top, value)

    def make_heap(first, last):
        length = last - first
        if length < 2:
            return
        parent = (length - 2) // 2
        while True:
            adjust_heap(first, parent, length, a[first + parent])
            if parent == 0:
                return
            parent -= 1

    def sort_heap(first, last):
        while last - first > 1:
            last -= 1
            value = a[last]  # __pop_heap(first, last, last)
            a[last] = a[first]
            adjust_heap(first, 0, last - first, value)

    def partial_sort_all(first, last):
        # __partial_sort(first, last, last): __heap_select's loop over
        # [middle, last) is empty, leaving __make_heap + __sort_heap
        tr.heap.append((first, last))
        if fallback == "heap":
            make_heap(first, last)
            sort_heap(first, last)
        elif fallback == "stable":
            a[first:last] = sorted(a[first:last], key=functools.cmp_to_key(
                lambda i, j: -1 if less(i, j) else (1 if less(j, i) else 0)))
        else:
            raise ValueError(fallback)

    def introsort_loop(first, last, depth_limit, level):
        while last - first > THRESHOLD:
            if depth_limit == 0:
                partial_sort_all(first, last)
                return
            depth_limit -= 1
            level += 1
            tr.depth = max(tr.depth, level)
            mid = first + (last - first) // 2
            move_median_to_first(first, first + 1, mid, last - 1)
            cut = unguarded_partition(first + 1, last, first)
            introsort_loop(cut, last, depth_limit, level)
            last = cut

    def unguarded_linear_insert(last):
        value = a[last]
        nxt = last - 1
        while less(value, a[nxt]):
            a[last] = a[nxt]
            last = nxt
            nxt -= 1
        a[last] = value

    def insertion_sort(first, last):
        for i in range(first + 1, last):
            if less(a[i], a[first]):
                value = a[i]
                a[first + 1:i + 1] = a[first:i]
                a[first] = value
            else:
                unguarded_linear_insert(i)

    if n:
        introsort_loop(0, n, 2 * (n.bit_length() - 1), 0)
        if n > THRESHOLD:
            insertion_sort(0, THRESHOLD)
            for i in range(THRESHOLD, n):
                unguarded_linear_insert(i)
        else:
            insertion_sort(0, n)
    return np.array(a, np.int64), tr


def killer(n):
    """McIlroy's adversary against std_sort_port: every row starts as "gas"
    (larger than any fixed key, undecided among themselves); comparing two gas
    rows fixes the one that is not the current pivot candidate at the next
    key, and a gas row compared with a fixed one becomes the candidate.  The
    keys so decided, in row order (a permutation of 0..n-1), make the
    median-of-3 partitions peel off a couple of records per level."""
    gas = n
    val = [gas] * n
    st = {"solid": 0, "cand": 0}

    def less(x, y):
        if val[x] == gas and val[y] == gas:
            if x == st["cand"]:
                val[x] = st["solid"]
            else:
                val[y] = st["solid"]
            st["solid"] += 1
        if val[x] == gas:
            st["cand"] = x
        elif val[y] == gas:
            st["cand"] = y
        return val[x] < val[y]

    std_sort_port(less=less, n=n)
    for i in range(n):  # rows the sort never had to decide
        if val[i] == gas:
            val[i] = st["solid"]
            st["solid"] += 1
    return np.array(val, np.int64)


def with_ties(keys, div):
    """Keys // div: tied groups of `div` consecutive keys."""
    return np.asarray(keys, np.int64) // int(div)


def few_values(seed, n, values=4):
    """n seeded draws from `values` distinct keys."""
    return _rng(seed).integers(0, values, n).astype(np.int64)


def _i(n):
    return np.arange(n, dtype=np.int64)


SEQUENCES = {
    "all_equal": lambda n: np.full(n, 7, np.int64),
    "alternating": lambda n: _i(n) % 2,
    "two_blocks": lambda n: (_i(n) < n // 2).astype(np.int64),  # 1 ... 1 0 ... 0
    "ascending": lambda n: _i(n),
    "descending": lambda n: n - 1 - _i(n),
    "organ_pipe": lambda n: np.minimum(_i(n), n - 1 - _i(n)),
    "sawtooth3": lambda n: _i(n) % 3,
    "sawtooth17": lambda n: _i(n) % 17,
    "ascending_pairs": lambda n: _i(n) // 2,
    "random4": lambda n: few_values(1000 + n, n),
}
EDGE_N = [16, 17, 33, 1024, 1025, 2049]
EDGE_K = lambda n: sorted({min(k, n) for k in (1, 2, 16, 17, n - 1, n)})  # noqa: E731

FILL = 3  # the constant of the columns beyond the first


def as_train(keys, d, m=1):
    """(train [n, d], queries [m, d]) in fp64: the keys in column 0 of the
    train rows, -c in column 0 of query c (c = 0..m-1), FILL elsewhere.  Query
    c's distance to row i is keys[i] + c exactly, in both metrics."""
    keys = np.asarray(keys, np.float64)
    assert (keys >= 0).all() and (keys == np.rint(keys)).all() and keys.max() + m < 2 ** 26
    train = np.full((keys.shape[0], d), float(FILL))
    train[:, 0] = keys
    queries = np.full((m, d), float(FILL))
    queries[:, 0] = -np.arange(m, dtype=np.float64)
    return train, queries


def labels(seed, n, classes):
    """Seeded labels independent of the keys."""
    return _rng(seed).integers(0, classes, n).astype(np.int32)


def vote(labs):
    """cpp:324-337: the first label whose count strictly exceeds the running max."""
    cnt, best, win = {}, 0, -1
    for v in labs:
        c = cnt.get(int(v), 0) + 1
        cnt[int(v)] = c
        if c > best:
            best, win = c, int(v)
    return win


def index_order(keys):
    """The (distance, train index) order: what the library reports without
    the reference-order pass."""
    return np.argsort(np.asarray(keys), kind="stable")


# Killer cases: keys = with_ties(killer(n), div), vote at k over `classes`
# labels drawn from `seed`.  test_sortorder_data.py holds each to the
# conditions that make it a test of the heap-sort fallback (a heap range
# [f, l) with l - f > 16 and f < k -- or k <= f for the "skip" case -- and a
# label that the two wrong orders get wrong); the heap ranges in the comments
# are the port's trace.
KILLERS = {
    "n2000": dict(n=2000, div=2, k=100, classes=3, seed=47),       # heap [40, 2000)
    "n300": dict(n=300, div=2, k=100, classes=3, seed=1034),       # heap [32, 300)
    "n2049": dict(n=2049, div=2, k=1100, classes=2, seed=6),       # heap [44, 2049), k > 1000
    "n2000_large_k": dict(n=2000, div=2, k=1200, classes=3, seed=241),  # heap [40, 2000)
}
# Further k on a case's data: at and below the heap range's start (the range
# starts at or beyond k and must be skipped), just above it, and k = n.
EXTRA_K = {"n2000": [10, 40, 42, 2000], "n300": [32, 300]}
SWEEP_KS = [1, 10, 40, 41, 42, 100]  # straddles n2000's f = 40
CLASSES = 3  # class_cnt of every call (a case may use fewer)

_cache = {}


def killer_case(name):
    """(keys, labels, k) of a KILLERS entry; built once per process and
    shared (callers must not modify the arrays)."""
    if name not in _cache:
        c = KILLERS[name]
        keys = with_ties(killer(c["n"]), c["div"])
        lab = labels(c["seed"], c["n"], c["classes"])
        keys.setflags(write=False)
        lab.setflags(write=False)
        _cache[name] = (keys, lab, c["k"])
    return _cache[name]

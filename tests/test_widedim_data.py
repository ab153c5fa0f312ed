"""The inputs of test_gpu_widedim.py, checked on the CPU: conditions on the
data (oracle distances and the bounds' arithmetic), not on the kernels.

1. plain and near: every query's k+1 oracle distances are pairwise distinct,
   so the GPU test can demand index-for-index equality;
2. dups: more than kRescanCap = 1024 rows lie within the oracle's k-th
   distance of each of the 16 special queries (the fast rescan cannot finish
   them: the full scan must); near: fewer than 1024 do, even with the k-th
   distance widened by the fp32 filter's slack (err_factor(0, DP) and
   err_factor(1, DP), widedim.Operands.filter_slack): the fast rescan can;
3. plain: for at least half the queries the gap between the k-th squared
   distance and the first row outside the re-rank window C = max(2W, W + 16)
   exceeds twice the fp16 bound E of DESIGN.md section 2 at that DP (a proxy
   is within E of its exact value on either side of the cut), so the fp16
   pass -- the loosest of the four -- can certify them;
4. ties: queries whose k-th and (k+1)-th oracle distances are equal, under
   both metrics;
5. the padded widths, the wide filter's queries per pass and the kernel
   names of widedim.py equal what csrc/knn_plan.cpp gives (tools/plan_check).
"""
import os
import subprocess

import numpy as np
import pytest

import oracle
import widedim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "-mpi-knn-_amd")

# d -> (pad_dim, pad_dim_bf16x3, pad_dim_fp16_s3, filter queries per pass)
PADS = {
    1025: (1056, 1040, 1056, 8), 1536: (1536, 1536, 1536, 8), 2016: (2016, 2016, 2016, 8),
    2048: (2048, 2048, 2048, 8), 3072: (3072, 3072, 3072, 8), 4096: (4096, 4096, 4096, 8),
    4097: (4128, 4112, 4128, 8), 5088: (5088, 5088, 5088, 8), 5089: (5120, 5104, 5120, 4),
    6000: (6016, 6000, 6016, 4),
}


@pytest.fixture(scope="module")
def plan_check():
    built = subprocess.run(["make", "-s", "-C", PKG, "bin/plan_check"], capture_output=True,
                           text=True)
    if built.returncode != 0:  # no sanitizer runtimes on this machine: the plain program
        built = subprocess.run(["make", "-s", "-C", PKG, "bin/plan_check", "SAN="],
                               capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr

    def run(*args):
        out = subprocess.run([os.path.join(PKG, "bin", "plan_check")] + [str(a) for a in args],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")[:-1]
    return run


def test_padded_widths_match_the_plan(plan_check):
    assert sorted(PADS) == sorted({widedim.dim_of(w) for w in widedim.WIDTHS})
    for line in plan_check("pads", *sorted(PADS)):
        d, dp, dpb, dph, i8w, u16w, fqw = (int(v) for v in line.split())
        assert (dp, dpb, dph, fqw) == PADS[d], line
        assert (widedim.pad_fp32(d), widedim.pad_bf16x3(d), widedim.pad_fp16_s3(d),
                widedim.rescan_wide_queries(dp)) == PADS[d]
        assert i8w == -1 and u16w == -1  # the wide L1 code passes end at 1024 dims
    # the filter's LDS on either side of 64 KiB and of a CU's 160 KiB
    assert 8 * (2016 + 1) * 4 < 65536 <= 8 * (2048 + 1) * 4
    assert 8 * (5088 + 1) * 4 + 72 <= 163840 < 8 * (5120 + 1) * 4
    # the merge's LDS with the query staged: past 64 KiB at d = 4096, 82 KiB at most
    assert widedim.merge_lds_bytes(4096, 1024, 256) == 83968
    assert widedim.merge_lds_bytes(4096, 128, 256) + 32768 > 65536
    assert widedim.merge_lds_bytes(4097, 1024, 256) == 83968 - 32768


@pytest.mark.parametrize("width", widedim.WIDTHS)
def test_kernel_names_match_the_plan(plan_check, width):
    n, m, k = widedim.SHAPES[width]
    d = widedim.dim_of(width)
    prec = {"AUTO": 0, "FP32": 1, "BF16X3": 2, "FP16": 3}
    for config, (p, tune) in widedim.CONFIGS.items():
        for metric in (0, 1):
            got = plan_check("name", d, n, m, k + 1, metric, prec[p],
                             *["%s=%d" % kv for kv in tune.items()])[0]
            assert got == widedim.kernel_name(config, metric, n, k), (config, metric)
    # the wide L1 code passes hand over to the fp32 L1 stream kernel
    for key in ("i8l1=2", "u16l1w=1"):
        assert plan_check("name", d, n, m, k + 1, 1, 0, key)[0] == \
            widedim.kernel_name("auto", 1, n, k)
    assert plan_check("name", 1024, n, m, k + 1, 1, 0, "u16l1w=1")[0].startswith(
        "cand_fix16_wide_kernel<")


_ORACLE = {}


def oracle_of(width, kind, metric, n_out):
    """Oracle (idx, dist) with at least n_out columns; computed once, shared."""
    key = (width, kind, metric)
    if key not in _ORACLE or _ORACLE[key][0].shape[1] < n_out:
        tr, lab, te, k = widedim.case(width, kind)
        _ORACLE[key] = oracle.knn(tr, lab, te, k, metric == 0, widedim.CLASSES, n_out=n_out)[1:]
    return _ORACLE[key]


@pytest.mark.parametrize("width", widedim.WIDTHS)
def test_plain_distinct_and_certifiable(width):
    tr, lab, te, k = widedim.case(width, "plain")
    n, d = tr.shape
    C = widedim.rerank_window(k, n)
    for metric in (0, 1):
        widx, wdist = oracle_of(width, "plain", metric, C + 1)
        gaps = np.diff(wdist[:, :k + 1], axis=1)
        assert (gaps > 0).all(), "tied oracle distances (metric %d): change the seed" % metric
    widx, wdist = oracle_of(width, "plain", 0, C + 1)
    ops = widedim.Operands(tr)
    DP = widedim.pad_fp16_s3(d)
    E = np.array([ops.fp16_bound(q, DP) for q in te])
    gap = wdist[:, C] ** 2 - wdist[:, k - 1] ** 2
    ok = int((gap > 2.0 * E).sum())
    print("width %s: %d of %d queries have a gap beyond 2E (median gap / 2E %.3g)"
          % (width, ok, len(te), np.median(gap / (2.0 * E))))
    assert 2 * ok >= len(te)


@pytest.mark.parametrize("width", [w for w in widedim.WIDTHS if w != widedim.BYTES])
def test_dups_beyond_and_near_within_the_fast_rescan(width):
    S = widedim.SPECIAL
    for metric in (0, 1):
        tr, lab, te, k = widedim.case(width, "dups")
        widx, wdist = oracle_of(width, "dups", metric, k + 1)
        for q in range(S):
            dist = oracle.row_distances(te[q], tr, metric == 0)
            assert (dist <= wdist[q, k - 1]).sum() > widedim.K_RESCAN_CAP
        tr, lab, te, k = widedim.case(width, "near")
        widx, wdist = oracle_of(width, "near", metric, k + 1)
        assert (np.diff(wdist, axis=1) > 0).all(), "tied oracle distances: change the seed"
        ops = widedim.Operands(tr)
        DP = widedim.pad_fp32(tr.shape[1])
        worst = 0
        for q in range(S):
            dist = oracle.row_distances(te[q], tr, metric == 0)
            slack = ops.filter_slack(te[q], metric, DP)
            tau = wdist[q, k]  # the (k+1)-th: W = k + 1 rows are kept
            within = (dist ** 2 <= tau ** 2 + slack) if metric == 0 else (dist <= tau + slack)
            worst = max(worst, int(within.sum()))
            assert k + 1 <= within.sum() < widedim.K_RESCAN_CAP
            # ... and beyond what the proxies can tell apart: the NEAR rows'
            # distances all lie inside the slack
            assert within.sum() >= widedim.NEAR
        print("width %s metric %d: at most %d rows within the filter's reach" % (width, metric, worst))


@pytest.mark.parametrize("d", widedim.TIE_WIDTHS)
def test_ties_cross_the_kth_place(d):
    tr, lab, te = widedim.ties(d)
    assert tr.min() >= 0 and tr.max() <= 255 and (tr == np.rint(tr)).all()
    for metric in (0, 1):
        for k in (1, 10):
            _, widx, wdist = oracle.knn(tr, lab, te, k, metric == 0, widedim.CLASSES, n_out=k + 1)
            edge = wdist[:, k - 1] == wdist[:, k]
            print("ties metric %d k %d: %d queries tied across the k-th place" % (metric, k, edge.sum()))
            if k == 1:
                # query i sits on train row i and on its copy under another label
                assert edge[:widedim.TIE_QUERIES].all()
                q = np.arange(widedim.TIE_QUERIES)
                assert (lab[q] != lab[widedim.TIE_AT + q]).all()
            inside = (np.diff(wdist[:, :k], axis=1) == 0).any(axis=1) | edge
            assert inside[:widedim.TIE_QUERIES].all()


def test_generators_are_deterministic():
    a = widedim.sized(1030, 40, 3, 5)
    b = widedim.sized(1030, 40, 3, 5)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (a[0] * 1024 == np.rint(a[0] * 1024)).all()
    assert np.linalg.matrix_rank(a[0] - a[0].mean(axis=0), tol=0.05) <= widedim.ZDIM

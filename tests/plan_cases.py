"""Cases of the search-plan parity test (test_gpu_plan.py) and of the tool
that records them (tools/record_plans.py): the smallest shapes that reach
each branch of the host-side plan (csrc/knn_plan.cpp) -- candidate path,
waves per workgroup, list geometry, thresholds, query order.

Data are seeded (datagen.make_sets): "int" sets sit on the byte grid (the
int8 passes), "gauss" sets are continuous for the plan's purposes (their
1/1024 grid spans more than 256 codes)."""
import functools
import hashlib

import numpy as np

import datagen

CLASSES = 5
AUTO, FP32, BF16X3, FP16 = 0, 1, 2, 3
L2, L1 = 0, 1


def _case(cid, kind, n, m, d, k, metric=L2, precision=AUTO, **tune):
    return {"id": cid, "kind": kind, "n": n, "m": m, "d": d, "k": k, "metric": metric,
            "precision": precision, "tune": tune}


def _cases():
    out = []
    # the AUTO batch threshold (4095 / 4096 queries): nw 4 -> 8, fp16 / int8 / mfma16 on
    for kind in ("gauss", "int"):
        for n in (2000, 40000):
            for m in (4095, 4096):
                out.append(_case("%s-n%d-m%d-d128" % (kind, n, m), kind, n, m, 128, 10))
    for kind in ("gauss", "int"):
        for d in (16, 24, 96, 256):
            out.append(_case("%s-d%d-m4096" % (kind, d), kind, 2000, 4096, d, 10))
    for d in (16, 24, 96, 256):
        out.append(_case("gauss-d%d-m4095" % d, "gauss", 2000, 4095, d, 10))
    # d > 256: fp16 S3 on 16x16x32 (AUTO), the query-resident kernel, bf16x3 S3, fp32 stream
    for d in (288, 320):
        out.append(_case("s3q-d%d" % d, "gauss", 4096, 512, d, 10))
    out.append(_case("qres-d320", "gauss", 4096, 512, 320, 10, qres=1))
    out.append(_case("s3-bf16x3-d288", "gauss", 4096, 512, 288, 10, precision=BF16X3))
    out.append(_case("stream-fp32-d300", "gauss", 4096, 512, 300, 10, precision=FP32))
    for d in (24, 300):
        out.append(_case("l1-d%d" % d, "gauss", 2000, 512, d, 10, metric=L1))
    # W = k + 1 on the edges the plan names: gk <= 4 up to W = 11 and the
    # resident kernel's K <= 4 up to W = 27, kQuadMaxW = 64, s3q up to W = 102
    for k in (1, 10, 11, 26, 27, 63, 64, 100, 101, 102):
        for kind in ("gauss", "int"):
            out.append(_case("%s-k%d" % (kind, k), kind, 40000, 4096, 128, k))
    for k in (100, 101, 102):
        out.append(_case("s3q-d288-k%d" % k, "gauss", 4096, 512, 288, k))
    # n_qt >= 512: quad lists take S >= 4 W
    for kind in ("gauss", "int"):
        out.append(_case("%s-m131072" % kind, kind, 20000, 131072, 32, 10))
    # region order of train rows and queries
    for ophase in (0, -1):
        out.append(_case("order5-ophase%d" % ophase, "int", 40000, 700, 128, 7, order=5, i8=1,
                         ophase=ophase))
    # tuning keys, one at a time
    for R in (4, 8, 16):
        out.append(_case("bf16x3-R%d" % R, "gauss", 40000, 4095, 128, 10, precision=BF16X3, R=R))
    out.append(_case("bf16x3-S3", "gauss", 40000, 4095, 128, 10, precision=BF16X3, S=3))
    for nw in (4, 8):
        out.append(_case("bf16x3-nw%d" % nw, "gauss", 40000, 4095, 128, 10, precision=BF16X3, nw=nw))
        out.append(_case("fp16-nw%d" % nw, "gauss", 40000, 4096, 128, 10, nw=nw))
    for gk in (0, 1):
        out.append(_case("fp16-gk%d" % gk, "gauss", 40000, 4096, 128, 10, gk=gk))
    for gg in (4, 8):
        out.append(_case("fp16-gg%d" % gg, "gauss", 40000, 4096, 128, 10, gg=gg))
    for i8w in (0, 1):
        out.append(_case("int-i8w%d" % i8w, "int", 40000, 4096, 128, 10, i8w=i8w))
    out.append(_case("int-R8", "int", 40000, 4096, 128, 10, R=8))
    out.append(_case("int-i8w0-R8", "int", 40000, 4096, 128, 10, i8w=0, R=8))
    for m16 in (0, 1):
        out.append(_case("bf16x3-mfma16-%d" % m16, "gauss", 40000, 4096, 128, 10,
                         precision=BF16X3, mfma16=m16))
    out.append(_case("s3q0-d288", "gauss", 4096, 512, 288, 10, s3q=0))
    out.append(_case("s3gq2-d288", "gauss", 4096, 512, 288, 10, s3gq=2))
    out.append(_case("int-i8resc0", "int", 40000, 4096, 128, 10, i8resc=0))
    out.append(_case("fp16-qblk4", "gauss", 40000, 4096, 128, 10, qblk=4))
    out.append(_case("fp16-seed8192", "gauss", 80000, 4096, 128, 10, seed=8192))
    return out


CASES = _cases()
FIELDS = ("kernel", "path", "geometry", "rescans", "sha1")


@functools.lru_cache(maxsize=2)
def _sets(kind, n, m, d):
    seed = 1000 + n % 997 + 7 * d + (m % 13)
    tr, trl, te, _, _, _ = datagen.make_sets(kind, seed, n, m, 0, d, CLASSES)
    return tr, trl, te


def run_case(knn, case):
    """One fresh classifier, set_train and one classify; the recorded fields."""
    tr, trl, te = _sets(case["kind"], case["n"], case["m"], case["d"])
    c = knn.Classifier(0)
    try:
        c.set_precision(case["precision"])
        for key, value in case["tune"].items():
            c.set_tuning(key, value)
        c.set_train(tr, trl, CLASSES)
        labels, _, _, flags = c.classify(te, case["k"], case["metric"], return_neighbors=True)
        g = c.last_geometry()
        return {"kernel": c.last_kernel_name(), "path": int(c.last_candidate_path()),
                "geometry": [int(g[f]) for f in ("workgroups", "splits", "lists", "rerank")],
                "rescans": int(c.last_rescan_count()),
                "sha1": hashlib.sha1(np.ascontiguousarray(labels).tobytes() +
                                     np.ascontiguousarray(flags).tobytes()).hexdigest()}
    finally:
        c.close()

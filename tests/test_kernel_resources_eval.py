"""CPU check of the per-class evaluation kernels' code objects
(csrc/knn_eval.hip): eval_confusion_kernel<0 | 1 | 2> (per-wave LDS copies,
one LDS histogram per workgroup, global atomics) and eval_vote_counts_kernel<
true | false> (LDS counters, global atomics) are in the gfx950 code objects,
none uses scratch, and the static LDS of each is what its regime's threshold
allows (per-wave copies up to C = 16, one histogram up to C = 96,
vote counters up to C = 1024; 32-bit counters, 4 waves per workgroup).  Reads
the AMDGPU metadata notes as test_kernel_resources.py does (whose reader does
not keep the LDS size: the notes are read once more for it); no GPU needed."""
import os
import re
import subprocess

import evalcases
from test_kernel_resources import LLVM, kernel_metadata

WAVES = 4
# static LDS bytes of each variant, from the thresholds alone
LDS_WANT = {
    ("eval_confusion_kernel", 0): WAVES * evalcases.SMALL_C ** 2 * 4,
    ("eval_confusion_kernel", 1): evalcases.LDS_C ** 2 * 4,
    ("eval_confusion_kernel", 2): 0,
    ("eval_vote_counts_kernel", 1): WAVES * evalcases.COUNTS_LDS_C * 4,
    ("eval_vote_counts_kernel", 0): 0,
}


def _variant(name):
    m = re.search(r"eval_confusion_kernelILi(\d)E", name)
    if m:
        return "eval_confusion_kernel", int(m.group(1))
    m = re.search(r"eval_vote_counts_kernelILb(\d)E", name)
    if m:
        return "eval_vote_counts_kernel", int(m.group(1))
    return None


def _eval_kernels(tmp):
    return {_variant(k): v for k, v in kernel_metadata(tmp).items() if _variant(k)}


def _lds_bytes(tmp):
    """.group_segment_fixed_size of the eval kernels, from the code objects
    kernel_metadata left in tmp."""
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes",
                                os.path.join(tmp, f)], check=True, capture_output=True,
                               text=True).stdout
        entry = {}
        for line in notes.splitlines() + ["  - .end"]:
            if re.match(r"\s+- \.", line):
                if "name" in entry and "lds" in entry and _variant(entry["name"]):
                    out[_variant(entry["name"])] = entry["lds"]
                entry = {}
            m = re.match(r"\s+(?:- )?\.name:\s+(\S+)", line)
            if m:
                entry["name"] = m.group(1)
            m = re.match(r"\s+(?:- )?\.group_segment_fixed_size:\s+(\d+)", line)
            if m:
                entry["lds"] = int(m.group(1))
    return out


def test_every_variant_is_built(tmp_path):
    assert set(_eval_kernels(str(tmp_path))) == set(LDS_WANT)


def test_eval_kernels_use_no_scratch(tmp_path):
    built = _eval_kernels(str(tmp_path))
    assert built, "no eval kernel in the code objects"
    spilled = sorted(k for k, v in built.items() if v.get("private_segment_fixed_size", 0) != 0)
    assert not spilled, "variants using scratch: %s" % spilled


def test_static_lds_within_the_thresholds(tmp_path):
    built = _eval_kernels(str(tmp_path))
    lds = _lds_bytes(str(tmp_path))
    assert set(lds) == set(built) == set(LDS_WANT)
    for key, want in sorted(LDS_WANT.items()):
        print("%s<%d>: %d B of LDS (threshold allows %d)" % (key + (lds[key], want)))
        assert lds[key] <= want
        if want:  # the LDS regimes do keep their counters there
            assert lds[key] > 0
    # the largest (one histogram at C = 96) leaves room for 4 workgroups in a
    # CU's 160 KB
    assert 4 * max(lds.values()) <= 160 * 1024

"""CPU check of the weighted-vote kernels' code objects (csrc/knn_wvote.hip):
wvote_sweep_kernel and wvote_sums_kernel are in the gfx950 code objects,
neither uses scratch, and their LDS stays within 64 KB per workgroup: the
static part from the AMDGPU metadata notes (read as
test_kernel_resources_eval.py reads them) plus, for the sweep kernel, the
dynamic part its launch asks for (knnk::wvote_sweep_lds_bytes, the host
function the launch itself uses) at every row length and list size the API
admits.  No GPU needed."""
import ctypes
import os
import re
import subprocess

from test_kernel_resources import LIB, LLVM, kernel_metadata

KERNELS = ("wvote_sweep_kernel", "wvote_sums_kernel")
LDS_LIMIT = 64 * 1024
WAVES, CHUNK = 4, 512  # waves per workgroup, row entries per LDS chunk


def _which(name):
    for k in KERNELS:
        if k in name:
            return k
    return None


def _built(tmp):
    return {_which(k): v for k, v in kernel_metadata(tmp).items() if _which(k)}


def _static_lds(tmp):
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
                if "name" in entry and "lds" in entry and _which(entry["name"]):
                    out[_which(entry["name"])] = entry["lds"]
                entry = {}
            m = re.match(r"\s+(?:- )?\.name:\s+(\S+)", line)
            if m:
                entry["name"] = m.group(1)
            m = re.match(r"\s+(?:- )?\.group_segment_fixed_size:\s+(\d+)", line)
            if m:
                entry["lds"] = int(m.group(1))
    return out


def test_both_kernels_are_built_without_scratch(tmp_path):
    built = _built(str(tmp_path))
    assert set(built) == set(KERNELS)
    spilled = sorted(k for k, v in built.items() if v.get("private_segment_fixed_size", 0) != 0)
    assert not spilled, "kernels using scratch: %s" % spilled


def test_lds_within_64_kb(tmp_path):
    _built(str(tmp_path))
    lds = _static_lds(str(tmp_path))
    assert set(lds) == set(KERNELS)
    fn = getattr(ctypes.CDLL(LIB), "_ZN4knnk21wvote_sweep_lds_bytesEiib")
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_bool]
    fn.restype = ctypes.c_size_t
    worst = 0
    for kmax in (0, 1, 64, 65, 511, 512, 513, 1000, 1100, 100000, 2 ** 31 - 1):
        for nk in (1, 7, 4095, 4096):
            for truth in (False, True):
                dyn = fn(kmax, nk, truth)
                # the layout of DESIGN 6d: per wave 20 B per chunk entry + 768 B
                # of staging, the per-K counters in front
                ch = max(64, min(CHUNK, (kmax + 63) // 64 * 64))
                assert dyn == WAVES * (20 * ch + 768) + (8 * ((nk + 1) // 2) if truth else 0)
                worst = max(worst, dyn)
    print("wvote_sweep_kernel: %d B static + at most %d B dynamic LDS; wvote_sums_kernel: %d B"
          % (lds["wvote_sweep_kernel"], worst, lds["wvote_sums_kernel"]))
    assert lds["wvote_sweep_kernel"] + worst <= LDS_LIMIT
    assert 0 < lds["wvote_sums_kernel"] <= LDS_LIMIT

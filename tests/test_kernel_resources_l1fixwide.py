"""CPU check of the wide 16-bit fixed-point L1 kernel's code objects
(csrc/knn_cand_fix16_wide.hip, cand_fix16_wide_kernel<R, NW>): every variant
the plan can name is in the library, uses no scratch, stays within 256
registers per lane, and holds the LDS its design gives it: two buffers of one
(tile, slab) unit -- 32 rows x 512 dims x 2 bytes = 32 KB each -- and two rows
of 32 seeds.  Reads the AMDGPU metadata notes as test_kernel_resources.py
does; no GPU needed."""
import os
import re
import subprocess

from test_kernel_resources import LLVM, kernel_metadata

VARIANTS = {(8, 4), (8, 8), (16, 4), (16, 8)}  # (R, NW): knn_plan.cpp, resident_variant
LDS_BYTES = 2 * 32 * 512 * 2 + 2 * 32 * 4  # 65792: two workgroups per CU (160 KB)


def _wide(tmp):
    meta = kernel_metadata(tmp)
    out = {}
    for name, v in meta.items():
        m = re.search(r"cand_fix16_wide_kernelILi(\d+)ELi(\d+)E", name)
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = v
    return out


def test_every_planned_variant_is_built(tmp_path):
    assert set(_wide(str(tmp_path))) == VARIANTS


def test_wide_kernels_use_no_scratch(tmp_path):
    wide = _wide(str(tmp_path))
    assert wide, "no cand_fix16_wide_kernel in the code objects"
    spilled = sorted(k for k, v in wide.items() if v.get("private_segment_fixed_size", 0) != 0)
    assert not spilled, "variants (R, NW) using scratch: %s" % spilled


def test_wide_kernels_stay_within_256_registers(tmp_path):
    wide = _wide(str(tmp_path))
    assert wide, "no cand_fix16_wide_kernel in the code objects"
    for (r, nw), v in sorted(wide.items()):
        regs = v.get("vgpr_count", 0) + v.get("agpr_count", 0)
        print("cand_fix16_wide_kernel<%d,%d>: %d registers per lane" % (r, nw, regs))
        assert 0 < regs <= 256, ((r, nw), v)


def _lds_bytes(tmp):
    """(R, NW) -> .group_segment_fixed_size, from the code objects that
    kernel_metadata left in tmp (a kernel's .name follows that key)."""
    out = {}
    for f in sorted(os.listdir(tmp)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)],
                               check=True, capture_output=True, text=True).stdout
        lds = None
        for line in notes.splitlines():
            if re.match(r"\s+- \.", line):
                lds = None
            m = re.match(r"\s+(?:- )?\.group_segment_fixed_size:\s+(\d+)", line)
            if m:
                lds = int(m.group(1))
            m = re.match(r"\s+(?:- )?\.name:\s+\S*cand_fix16_wide_kernelILi(\d+)ELi(\d+)E", line)
            if m:
                assert lds is not None
                out[(int(m.group(1)), int(m.group(2)))] = lds
    return out


def test_wide_kernels_hold_two_slab_buffers_in_lds(tmp_path):
    assert _wide(str(tmp_path)), "no cand_fix16_wide_kernel in the code objects"
    lds = _lds_bytes(str(tmp_path))
    assert set(lds) == VARIANTS
    for key, size in sorted(lds.items()):
        assert size == LDS_BYTES, (key, size)

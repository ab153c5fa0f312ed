"""CPU check of the wide L1-on-codes kernel's code objects
(csrc/knn_cand_sad_wide.hip, cand_sad_wide_kernel<R, NW>): every variant the
plan can name is in the library, uses no scratch, and stays within the
registers its launch bounds leave a lane.  Reads the AMDGPU metadata notes as
test_kernel_resources.py does; no GPU needed."""
import re

from test_kernel_resources import kernel_metadata

# __launch_bounds__(NW * 64): a workgroup's NW waves sit on the CU's 4 SIMDs,
# NW / 4 per SIMD, which share the SIMD's 512 registers per lane (VGPR + AGPR)
BUDGET = {4: 512, 8: 256}
VARIANTS = {(8, 4), (8, 8), (16, 4), (16, 8)}  # (R, NW): knn_plan.cpp, resident_variant


def _wide(tmp):
    meta = kernel_metadata(tmp)
    out = {}
    for name, v in meta.items():
        m = re.search(r"cand_sad_wide_kernelILi(\d+)ELi(\d+)E", name)
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = v
    return out


def test_every_planned_variant_is_built(tmp_path):
    assert set(_wide(str(tmp_path))) == VARIANTS


def test_wide_kernels_use_no_scratch(tmp_path):
    wide = _wide(str(tmp_path))
    assert wide, "no cand_sad_wide_kernel in the code objects"
    spilled = sorted(k for k, v in wide.items() if v.get("private_segment_fixed_size", 0) != 0)
    assert not spilled, "variants (R, NW) using scratch: %s" % spilled


def test_wide_kernels_fit_their_waves_per_simd(tmp_path):
    wide = _wide(str(tmp_path))
    assert wide, "no cand_sad_wide_kernel in the code objects"
    for (r, nw), v in sorted(wide.items()):
        regs = v.get("vgpr_count", 0) + v.get("agpr_count", 0)
        print("cand_sad_wide_kernel<%d,%d>: %d registers per lane" % (r, nw, regs))
        assert 0 < regs <= BUDGET[nw], ((r, nw), v)

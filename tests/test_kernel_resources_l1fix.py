"""CPU check of the 16-bit fixed-point L1 kernel's code objects
(csrc/knn_cand_fix16.hip, cand_fix16_kernel<DP, R, NW>): every variant the
plan can name is in the library and no other, none uses scratch, and each
stays within the registers its launch bounds leave a lane.  Reads the AMDGPU
metadata notes as test_kernel_resources.py does; no GPU needed."""
import re

import l1fix
from test_kernel_resources import kernel_metadata

# __launch_bounds__(NW * 64): a workgroup's NW waves sit on the CU's 4 SIMDs,
# NW / 4 per SIMD, which share the SIMD's 512 registers per lane (VGPR + AGPR)
BUDGET = {4: 512, 8: 256}
# (DP, R, NW): knn_plan.cpp, resident_variant -- 8 waves only up to DP = 128,
# where the resident query (DP / 2 registers) leaves room
VARIANTS = {(dp, r, nw) for dp in l1fix.WIDTHS for r in (8, 16) for nw in (4, 8)
            if nw == 4 or dp <= 128}


def _fix16(tmp):
    out = {}
    for name, v in kernel_metadata(tmp).items():
        m = re.search(r"cand_fix16_kernelILi(\d+)ELi(\d+)ELi(\d+)E", name)
        if m:
            out[tuple(int(g) for g in m.groups())] = v
    return out


def test_every_planned_variant_is_built(tmp_path):
    assert set(_fix16(str(tmp_path))) == VARIANTS


def test_fix16_kernels_use_no_scratch(tmp_path):
    built = _fix16(str(tmp_path))
    assert built, "no cand_fix16_kernel in the code objects"
    spilled = sorted(k for k, v in built.items() if v.get("private_segment_fixed_size", 0) != 0)
    assert not spilled, "variants (DP, R, NW) using scratch: %s" % spilled


def test_fix16_kernels_fit_their_waves_per_simd(tmp_path):
    built = _fix16(str(tmp_path))
    assert built, "no cand_fix16_kernel in the code objects"
    for (dp, r, nw), v in sorted(built.items()):
        regs = v.get("vgpr_count", 0) + v.get("agpr_count", 0)
        print("cand_fix16_kernel<%d,%d,%d>: %d registers per lane" % (dp, r, nw, regs))
        # the resident query alone takes DP / 2 of them
        assert dp // 2 < regs <= BUDGET[nw], ((dp, r, nw), v)

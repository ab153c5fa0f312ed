"""CPU check of the int8 L1-on-codes kernel's code objects
(csrc/knn_cand_sad.hip, cand_sad_kernel<DP, R, NW>): every variant the plan
can name is in the library and no other, none uses scratch, and each stays
within the registers its launch bounds leave a lane.  Reads the AMDGPU
metadata notes as test_kernel_resources.py does; no GPU needed."""
import re

from test_kernel_resources import kernel_metadata

# __launch_bounds__(NW * 64): a workgroup's NW waves sit on the CU's 4 SIMDs,
# NW / 4 per SIMD, which share the SIMD's 512 registers per lane (VGPR + AGPR)
BUDGET = {4: 512, 8: 256}
WIDTHS = (32, 64, 96, 128, 160, 192, 256)  # pad_dim_i8w's values
# (DP, R, NW): knn_plan.cpp, resident_variant
VARIANTS = {(dp, r, nw) for dp in WIDTHS for r in (8, 16) for nw in (4, 8)}


def _sad(tmp):
    out = {}
    for name, v in kernel_metadata(tmp).items():
        m = re.search(r"cand_sad_kernelILi(\d+)ELi(\d+)ELi(\d+)E", name)
        if m:
            out[tuple(int(g) for g in m.groups())] = v
    return out


def test_every_planned_variant_is_built(tmp_path):
    assert len(VARIANTS) == 28
    assert set(_sad(str(tmp_path))) == VARIANTS


def test_sad_kernels_use_no_scratch(tmp_path):
    built = _sad(str(tmp_path))
    assert built, "no cand_sad_kernel in the code objects"
    spilled = sorted(k for k, v in built.items() if v.get("private_segment_fixed_size", 0) != 0)
    assert not spilled, "variants (DP, R, NW) using scratch: %s" % spilled


def test_sad_kernels_fit_their_waves_per_simd(tmp_path):
    built = _sad(str(tmp_path))
    assert built, "no cand_sad_kernel in the code objects"
    for (dp, r, nw), v in sorted(built.items()):
        regs = v.get("vgpr_count", 0) + v.get("agpr_count", 0)
        print("cand_sad_kernel<%d,%d,%d>: %d registers per lane" % (dp, r, nw, regs))
        # the resident query alone takes DP / 4 of them
        assert dp // 4 < regs <= BUDGET[nw], ((dp, r, nw), v)

"""CPU check of knn_fold.hip's kernels in the built gfx950 code objects: the
fold gather and the list index map use no scratch and stay within the register
bound the file states (32 VGPRs, no AGPRs).  Reads the code objects' metadata
as test_kernel_resources.py does; no GPU needed."""
from test_kernel_resources import kernel_metadata

KERNELS = ("fold_gather_kernel", "fold_map_idx_kernel")


def test_fold_kernels_use_no_scratch_and_few_registers(tmp_path):
    meta = kernel_metadata(str(tmp_path))
    for name in KERNELS:
        found = {k: v for k, v in meta.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        (k, v), = found.items()
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
        assert v.get("vgpr_count", 0) <= 32 and v.get("agpr_count", 0) == 0, (k, v)

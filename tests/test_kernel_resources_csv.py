"""CPU check of the CSV reader's code objects (csrc/knn_csv.hip): the count,
scan, convert and scatter kernels are in the gfx950 code objects of the built
library and none uses scratch (the conversion's tables are read from global
memory, no token is copied to a private buffer).  Reads the AMDGPU metadata
notes as test_kernel_resources.py does; no GPU needed."""
from test_kernel_resources import kernel_metadata

KERNELS = ("csv_count_kernel", "csv_scan_kernel", "csv_convert_kernel", "csv_scatter_kernel")


def _csv_kernels(tmp):
    out = {}
    for name, meta in kernel_metadata(tmp).items():
        for k in KERNELS:
            if k in name:
                out[k] = meta
    return out


def test_every_kernel_is_built(tmp_path):
    assert set(_csv_kernels(str(tmp_path))) == set(KERNELS)


def test_csv_kernels_use_no_scratch(tmp_path):
    built = _csv_kernels(str(tmp_path))
    assert built, "no CSV kernel in the code objects"
    spilled = sorted(k for k, v in built.items() if v.get("private_segment_fixed_size", 0) != 0)
    assert not spilled, "kernels using scratch: %s" % spilled

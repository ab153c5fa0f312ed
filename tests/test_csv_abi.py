"""CPU checks of the CSV reader's boundary: the header declares its entry
points with the documented prototypes and states the token rule and the tiers,
the built library exports them, the Python mirror lists and binds them, the
calls refuse the null handle without a device, and the driver knows --csv.
No GPU calls are made."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest
import torch

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "-mpi-knn-_amd")
HEADER = os.path.join(ROOT, "include", "knn_amd.h")
# name -> the parameter types of the header's declaration, in order
CSV = {
    "knn_csv_parse_device": [
        "knn_ctx*", "const char*", "int64_t", "int32_t", "int32_t", "int64_t", "double*",
        "int32_t*", "int64_t*", "int64_t*", "int64_t", "int64_t*", "void*"],
    "knn_csv_read": [
        "knn_ctx*", "const char*", "int32_t", "int32_t", "int64_t", "double*", "int32_t*",
        "int64_t*"],
    "knn_csv_read_device": [
        "knn_ctx*", "const char*", "int32_t", "int32_t", "int64_t", "double*", "int32_t*",
        "int64_t*"],
}
EXTRA = ("knn_csv_last_slow", "knn_csv_last_phases")


@pytest.fixture(scope="module")
def knn():
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(PKG, "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not (os.path.exists(mod.LIB_PATH) and os.path.exists(mod.DRIVER_PATH)):
        mod.build()
    return mod


def test_header_declares_the_prototypes():
    assert set(CSV) | set(EXTRA) <= set(declared_functions())
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in CSV.items():
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
        assert m, name
        got = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            got.append(re.sub(r"\s*\w+$", "", p).replace(" *", "*"))  # drop the parameter name
        assert got == want, name
    text = open(HEADER).read()
    # the token rule, the tiers and the reference's values are stated
    assert "TERMINATES" in text and "Clinger" in text and "Eisel-Lemire" in text
    assert "bit for bit" in text and "KNN_CSV_BLOCK_BYTES" in text


def test_library_exports_the_calls(knn):
    out = subprocess.run(["nm", "-D", "--defined-only", knn.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (knn_\w+)", out))
    assert set(CSV) | set(EXTRA) <= exported


def test_mirror_lists_and_binds_the_calls(knn):
    assert set(CSV) | set(EXTRA) <= set(knn.EXPORTED)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    for name, params in CSV.items():
        fn = getattr(knn.lib(), name)
        assert fn.restype is ctypes.c_int
        want = []
        for k, t in enumerate(params):
            if t == "const char*" and name != "knn_csv_parse_device":
                want.append(ctypes.c_char_p)  # the path
            else:
                want.append(P if t.endswith("*") else {"int32_t": i32, "int64_t": i64}[t])
        assert list(fn.argtypes) == want, name
    sig = inspect.signature(knn.Classifier.read_csv)
    assert list(sig.parameters)[1:5] == ["path", "dim", "with_label", "rows"]
    assert sig.parameters["device"].default is False
    assert callable(knn.Classifier.csv_parse_device)
    m = re.search(r"#define\s+KNN_CSV_BLOCK_BYTES\s+(\d+)", open(HEADER).read())
    assert int(m.group(1)) == knn.CSV_BLOCK_BYTES


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly(knn, tmp_path):
    """Without a HIP device no context exists to parse on (no CPU fallback):
    the calls refuse the null handle instead of reading the file themselves."""
    L = knn.lib()
    p = tmp_path / "a.csv"
    p.write_text("1,2,3\n")
    data = (ctypes.c_double * 3)()
    tokens = ctypes.c_int64(0)
    assert L.knn_csv_read(None, str(p).encode(), 3, 0, 1, data, None, ctypes.byref(tokens)) == -1
    assert L.knn_csv_read_device(None, str(p).encode(), 3, 0, 1, data, None,
                                 ctypes.byref(tokens)) == -1
    assert L.knn_csv_parse_device(None, None, 0, 3, 0, 1, data, None, ctypes.byref(tokens), None,
                                  0, ctypes.byref(tokens), None) == -1
    assert L.knn_csv_last_slow(None) == -1
    assert list(data) == [0.0, 0.0, 0.0]


def test_driver_help_names_csv(knn):
    r = subprocess.run([knn.DRIVER_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--csv host|gpu" in r.stderr + r.stdout

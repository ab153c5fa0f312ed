"""CPU checks of the distance-weighted vote's boundary: the header declares its
entry points and constants and says which calls stay uniform, the built library
exports them, the Python mirror lists and binds them, the calls refuse the null
handle, and the driver knows --weights.  No GPU calls are made."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest

from test_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "-mpi-knn-_amd")
HEADER = os.path.join(ROOT, "include", "knn_amd.h")
# name -> the parameter types of the header's declaration, in order
WVOTE = {
    "knn_set_vote": ["knn_ctx*", "int"],
    "knn_get_vote": ["knn_ctx*"],
    "knn_group_set_vote": ["knn_group*", "int"],
    "knn_vote_sweep_weighted_device": [
        "knn_ctx*", "const int64_t*", "const double*", "int64_t", "int32_t", "const int32_t*",
        "int64_t", "const int32_t*", "int32_t", "int32_t*", "const int32_t*", "int64_t*", "void*"],
    "knn_vote_weights_device": [
        "knn_ctx*", "const int64_t*", "const double*", "int64_t", "int32_t", "const int32_t*",
        "int64_t", "int32_t", "int32_t", "double*", "void*"],
}


@pytest.fixture(scope="module")
def knn():
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(PKG, "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not (os.path.exists(mod.LIB_PATH) and os.path.exists(mod.DRIVER_PATH)):
        mod.build()
    return mod


def test_header_declares_the_prototypes_and_constants():
    assert set(WVOTE) <= set(declared_functions())
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, want in WVOTE.items():
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
        assert m, name
        got = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            got.append(re.sub(r"\s*\w+$", "", p).replace(" *", "*"))  # drop the parameter name
        assert got == want, name
    assert re.search(r"^#define KNN_VOTE_UNIFORM 0\s*$", src, flags=re.M)
    assert re.search(r"^#define KNN_VOTE_DISTANCE 1\s*$", src, flags=re.M)
    # the header says which calls stay uniform in every mode
    m = re.search(r"stay UNIFORM in every mode:(.*?)\*/", text, flags=re.S)
    assert m
    for name in ("knn_vote_sweep_device", "knn_vote_counts_device", "knn_merge_vote_device",
                 "knn_tie_resolve_device"):
        assert name in m.group(1)


def test_library_exports_the_calls(knn):
    out = subprocess.run(["nm", "-D", "--defined-only", knn.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (knn_\w+)", out))
    assert set(WVOTE) <= exported


def test_mirror_lists_and_binds_the_calls(knn):
    assert set(WVOTE) <= set(knn.EXPORTED)
    assert (knn.VOTE_UNIFORM, knn.VOTE_DISTANCE) == (0, 1)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    ctype = lambda t: P if t.endswith("*") else {"int32_t": i32, "int64_t": i64,  # noqa: E731
                                                 "int": ctypes.c_int}[t]
    for name, params in WVOTE.items():
        fn = getattr(knn.lib(), name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [ctype(t) for t in params], name
    for meth in ("set_vote", "get_vote", "vote_sweep_weighted_device", "vote_weights_device"):
        assert callable(getattr(knn.Classifier, meth))
    assert callable(knn.Group.set_vote)
    sig = inspect.signature
    assert sig(knn.Classifier.classify).parameters["return_weights"].default is False
    assert "--weights" in knn.run_driver.__doc__


def test_null_handles_are_refused(knn):
    L = knn.lib()
    idx = (ctypes.c_int64 * 4)()
    dist = (ctypes.c_double * 4)()
    lab = (ctypes.c_int32 * 4)()
    ks = (ctypes.c_int32 * 1)(1)
    w = (ctypes.c_double * 8)()
    assert L.knn_set_vote(None, 1) == -1
    assert L.knn_get_vote(None) == -1
    assert L.knn_group_set_vote(None, 1) == -1
    assert L.knn_vote_sweep_weighted_device(None, idx, dist, 4, 1, lab, 0, ks, 1, lab, None, None,
                                            None) == -1
    assert L.knn_vote_weights_device(None, idx, dist, 4, 1, lab, 0, 1, 2, w, None) == -1


def test_driver_help_names_weights(knn):
    r = subprocess.run([knn.DRIVER_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--weights uniform|distance" in r.stderr + r.stdout
    r = subprocess.run([knn.DRIVER_PATH, "--weights", "cubic"], capture_output=True, text=True)
    assert r.returncode == 1 and "--weights takes uniform or distance" in r.stderr

"""CPU checks of the leave-one-out sweep's boundary: the header declares its
four entry points, the built library exports them with the documented
prototypes, the Python mirror lists and binds them, without a device no
context can be created (KNN_ERR_DEVICE) and the calls refuse the null handle,
and the driver knows --loo and refuses it without --K_list before any device
call.
No GPU calls are made."""
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "-mpi-knn-_amd")
HEADER = os.path.join(ROOT, "include", "knn_amd.h")
# name -> the parameter types of the header's declaration, in order
LOO = {
    "knn_classify_sweep_excl_device": [
        "knn_ctx*", "const double*", "int64_t", "const int64_t*", "const int32_t*", "int32_t",
        "int32_t", "int32_t*", "const int32_t*", "int64_t*", "int64_t*", "double*", "int32_t*",
        "void*"],
    "knn_loo_sweep_device": [
        "knn_ctx*", "int64_t", "int64_t", "const int32_t*", "int32_t", "int32_t", "int32_t*",
        "int64_t*", "int64_t*", "double*", "int32_t*", "void*"],
    "knn_loo_sweep": [
        "knn_ctx*", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*", "int64_t*",
        "double*", "int32_t*"],
    "knn_group_loo_sweep": [
        "knn_group*", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*"],
}


@pytest.fixture(scope="module")
def knn():
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(PKG, "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not (os.path.exists(mod.LIB_PATH) and os.path.exists(mod.DRIVER_PATH)):
        mod.build()
    return mod


def test_header_declares_the_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in LOO.items():
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
        assert m, name
        got = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            got.append(re.sub(r"\s*\w+$", "", p).replace(" *", "*"))  # drop the parameter name
        assert got == want, name
    assert "cpp:308-343" in open(HEADER).read()


def test_library_exports_the_calls(knn):
    out = subprocess.run(["nm", "-D", "--defined-only", knn.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (knn_\w+)", out))
    assert set(LOO) <= exported


def test_mirror_lists_and_binds_the_calls(knn):
    assert set(LOO) <= set(knn.EXPORTED)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    ctype = lambda t: P if t.endswith("*") else {"int32_t": i32, "int64_t": i64}[t]  # noqa: E731
    for name, params in LOO.items():
        fn = getattr(knn.lib(), name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [ctype(t) for t in params], name
    for meth in ("classify_sweep", "loo_sweep", "loo_sweep_device"):
        assert callable(getattr(knn.Classifier, meth))
    assert callable(knn.Group.loo_sweep)
    import inspect
    assert "exclude" in inspect.signature(knn.Classifier.classify_sweep).parameters
    assert "d_excl" in inspect.signature(knn.Classifier.classify_sweep_device).parameters


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly(knn):
    """Without a HIP device knn_create fails with KNN_ERR_DEVICE, so no context
    exists to sweep on (no CPU fallback): the mirror raises, and the new calls
    refuse the null handle (KNN_ERR_ARG / KNN_ERR_STATE) instead of computing."""
    L = knn.lib()
    h = ctypes.c_void_p()
    assert L.knn_create(ctypes.byref(h), 0) == -2
    assert "no CPU fallback" in L.knn_last_error().decode()
    with pytest.raises(knn.KnnError, match="no CPU fallback"):
        knn.Classifier(0)
    with pytest.raises(knn.KnnError):
        knn.Group([0], mode=0)
    ks = (ctypes.c_int32 * 2)(1, 3)
    out = (ctypes.c_int32 * 8)()
    corr = (ctypes.c_int64 * 2)()
    excl = (ctypes.c_int64 * 1)(-1)
    for d_excl in (None, excl):
        assert L.knn_classify_sweep_excl_device(None, None, 0, d_excl, ks, 2, 0, out, None, None,
                                                None, None, None, None) == -1
    assert L.knn_loo_sweep_device(None, 0, 0, ks, 2, 0, out, corr, None, None, None, None) == -1
    assert L.knn_loo_sweep(None, ks, 2, 0, out, corr, None, None, None) == -1
    assert L.knn_group_loo_sweep(None, ks, 2, 0, out, corr) == -3


def test_driver_help_names_loo(knn):
    r = subprocess.run([knn.DRIVER_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--loo" in r.stderr + r.stdout


def test_driver_loo_needs_k_list(knn, tmp_path):
    """Refused while the flags are checked: no file is read, no device call made."""
    r = subprocess.run([knn.DRIVER_PATH, "--loo"], cwd=str(tmp_path), capture_output=True,
                       text=True)
    assert r.returncode != 0
    assert "--loo needs --K_list" in r.stderr
    assert "accuracy" not in r.stdout


def test_driver_loo_k_below_n_train(knn, tmp_path):
    r = subprocess.run([knn.DRIVER_PATH, "--loo", "--K_list", "1,100", "--N_train", "100"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode != 0
    assert "N_train - 1" in r.stderr

"""CPU checks of the per-class evaluation's boundary: the header declares its
eight entry points, the built library exports them with the documented
prototypes, the Python mirror lists and binds them, without a device no
context can be created (KNN_ERR_DEVICE) and the calls refuse the null handle,
and the driver knows --confusion.
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
EVAL = {
    "knn_confusion_device": [
        "knn_ctx*", "const int32_t*", "int32_t", "int64_t", "const int32_t*", "int32_t",
        "int64_t*", "int64_t*", "void*"],
    "knn_vote_counts_device": [
        "knn_ctx*", "const int64_t*", "int64_t", "int32_t", "const int32_t*", "int64_t", "int32_t",
        "int32_t", "int32_t*", "void*"],
    "knn_classify_sweep_eval_device": [
        "knn_ctx*", "const double*", "int64_t", "const int64_t*", "const int32_t*", "int32_t",
        "int32_t", "int32_t*", "const int32_t*", "int64_t*", "int64_t*", "int64_t*", "void*"],
    "knn_loo_sweep_eval_device": [
        "knn_ctx*", "int64_t", "int64_t", "const int32_t*", "int32_t", "int32_t", "int32_t*",
        "int64_t*", "int64_t*", "int64_t*", "void*"],
    "knn_classify_sweep_eval": [
        "knn_ctx*", "const double*", "int64_t", "const int32_t*", "int32_t", "int32_t", "int32_t*",
        "const int32_t*", "int64_t*", "int64_t*", "int64_t*"],
    "knn_loo_sweep_eval": [
        "knn_ctx*", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*", "int64_t*",
        "int64_t*"],
    "knn_group_classify_sweep_eval": [
        "knn_group*", "const double*", "int64_t", "const int32_t*", "int32_t", "int32_t",
        "int32_t*", "const int32_t*", "int64_t*", "int64_t*", "int64_t*"],
    "knn_group_loo_sweep_eval": [
        "knn_group*", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*", "int64_t*",
        "int64_t*"],
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
    assert set(EVAL) <= set(declared_functions())
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in EVAL.items():
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
        assert m, name
        got = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            got.append(re.sub(r"\s*\w+$", "", p).replace(" *", "*"))  # drop the parameter name
        assert got == want, name
    text = open(HEADER).read()
    # the accumulate convention and the tie note are stated
    assert "ADDS" in text and "ZEROED" in text
    assert '"ties" = 2' in text and "KNN_FLAG_TIE_BOUNDARY" in text


def test_library_exports_the_calls(knn):
    out = subprocess.run(["nm", "-D", "--defined-only", knn.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (knn_\w+)", out))
    assert set(EVAL) <= exported


def test_mirror_lists_and_binds_the_calls(knn):
    assert set(EVAL) <= set(knn.EXPORTED)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    ctype = lambda t: P if t.endswith("*") else {"int32_t": i32, "int64_t": i64}[t]  # noqa: E731
    for name, params in EVAL.items():
        fn = getattr(knn.lib(), name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [ctype(t) for t in params], name
    for meth in ("confusion_device", "vote_counts_device", "classify_sweep_eval_device",
                 "loo_sweep_eval_device"):
        assert callable(getattr(knn.Classifier, meth))
    sig = inspect.signature
    assert sig(knn.Classifier.classify_sweep).parameters["confusion"].default is False
    assert sig(knn.Classifier.loo_sweep).parameters["confusion"].default is False
    assert sig(knn.Classifier.loo_sweep).parameters["labels"].default is True
    assert sig(knn.Classifier.classify).parameters["return_counts"].default is False
    assert sig(knn.Group.classify_sweep).parameters["confusion"].default is False
    assert sig(knn.Group.loo_sweep).parameters["confusion"].default is False
    assert sig(knn.Group.loo_sweep).parameters["labels"].default is True


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly(knn):
    """Without a HIP device knn_create fails with KNN_ERR_DEVICE, so no context
    exists to evaluate on (no CPU fallback): the mirror raises, and the new
    calls refuse the null handle (KNN_ERR_ARG / KNN_ERR_STATE) instead of
    computing."""
    L = knn.lib()
    h = ctypes.c_void_p()
    assert L.knn_create(ctypes.byref(h), 0) == -2
    assert "no CPU fallback" in L.knn_last_error().decode()
    with pytest.raises(knn.KnnError, match="no CPU fallback"):
        knn.Classifier(0)
    ks = (ctypes.c_int32 * 2)(1, 3)
    lab = (ctypes.c_int32 * 8)()
    truth = (ctypes.c_int32 * 4)()
    corr = (ctypes.c_int64 * 2)()
    conf = (ctypes.c_int64 * 8)()
    unl = (ctypes.c_int64 * 2)()
    idx = (ctypes.c_int64 * 4)()
    q = (ctypes.c_double * 4)()
    assert L.knn_confusion_device(None, lab, 2, 4, truth, 2, conf, unl, None) == -1
    assert L.knn_vote_counts_device(None, idx, 4, 1, lab, 0, 1, 2, lab, None) == -1
    assert L.knn_classify_sweep_eval_device(None, q, 4, None, ks, 2, 0, lab, truth, corr, conf,
                                            unl, None) == -1
    assert L.knn_loo_sweep_eval_device(None, 0, 0, ks, 2, 0, lab, corr, conf, unl, None) == -1
    assert L.knn_classify_sweep_eval(None, q, 4, ks, 2, 0, lab, truth, corr, conf, unl) == -1
    assert L.knn_loo_sweep_eval(None, ks, 2, 0, lab, corr, conf, unl) == -1
    assert L.knn_group_classify_sweep_eval(None, q, 4, ks, 2, 0, lab, truth, corr, conf,
                                           unl) == -3
    assert L.knn_group_loo_sweep_eval(None, ks, 2, 0, lab, corr, conf, unl) == -3


def test_driver_help_names_confusion(knn):
    r = subprocess.run([knn.DRIVER_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--confusion" in r.stderr + r.stdout

"""CPU checks of the K-fold sweep's boundary: the header declares its entry
points, the built library exports them with the documented prototypes, the
Python mirror lists and binds them, without a device the calls refuse the null
handle, and the driver knows --kfold / --folds and refuses their misuse before
any device call.  The per-fold device call takes its stream as `on_stream`,
like the leave-group-out calls; its held-stream test is in test_gpu_kfold.py.
No GPU calls are made."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "-mpi-knn-_amd")
HEADER = os.path.join(ROOT, "include", "knn_amd.h")
# name -> (return type, the parameter types of the header's declaration, in order)
KFOLD = {
    "knn_set_folds": ("int", ["knn_ctx*", "const int32_t*", "int32_t"]),
    "knn_get_fold_max": ("int32_t", ["knn_ctx*"]),
    "knn_kfold_sweep_device": ("int", [
        "knn_ctx*", "int32_t", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*",
        "int64_t*", "double*", "int32_t*", "void*"]),
    "knn_kfold_sweep": ("int", [
        "knn_ctx*", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*", "int64_t*",
        "int64_t*", "int64_t*", "double*", "int32_t*"]),
    "knn_group_set_folds": ("int", ["knn_group*", "const int32_t*", "int32_t"]),
    "knn_group_kfold_sweep": ("int", [
        "knn_group*", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*", "int64_t*",
        "int64_t*"]),
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
    for name, (ret, want) in KFOLD.items():
        m = re.search(r"^%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), src, flags=re.M)
        assert m, name
        got = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            got.append(re.sub(r"\s*\w+$", "", p).replace(" *", "*"))  # drop the parameter name
        assert got == want, name
    text = open(HEADER).read()
    assert "fold shards" in text and "FOLD f REMOVED" in text
    assert re.search(r"knn_kfold_sweep_device\([^;]*void\s*\*\s*on_stream\)", src, flags=re.S)


def test_library_exports_the_calls(knn):
    out = subprocess.run(["nm", "-D", "--defined-only", knn.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (knn_\w+)", out))
    assert set(KFOLD) <= exported


def test_mirror_lists_and_binds_the_calls(knn):
    assert set(KFOLD) <= set(knn.EXPORTED)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    ctype = lambda t: P if t.endswith("*") else {"int32_t": i32, "int64_t": i64}[t]  # noqa: E731
    for name, (ret, params) in KFOLD.items():
        fn = getattr(knn.lib(), name)
        assert fn.restype is (ctypes.c_int if ret == "int" else i32)
        assert list(fn.argtypes) == [ctype(t) for t in params], name
    for meth in ("set_folds", "kfold_sweep", "kfold_sweep_device", "fold_max"):
        assert callable(getattr(knn.Classifier, meth))
    assert callable(knn.Group.set_folds) and callable(knn.Group.kfold_sweep)
    assert list(inspect.signature(knn.Classifier.kfold_sweep).parameters) == list(
        inspect.signature(knn.Classifier.lgo_sweep).parameters)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly(knn):
    """Without a HIP device no context exists to sweep on (no CPU fallback):
    the new calls refuse the null handle instead of computing."""
    L = knn.lib()
    h = ctypes.c_void_p()
    assert L.knn_create(ctypes.byref(h), 0) == -2
    ks = (ctypes.c_int32 * 2)(1, 3)
    out = (ctypes.c_int32 * 8)()
    corr = (ctypes.c_int64 * 2)()
    folds = (ctypes.c_int32 * 4)(0, 1, 1, 0)
    assert L.knn_set_folds(None, folds, 2) == -1
    assert L.knn_get_fold_max(None) == 0
    assert L.knn_kfold_sweep_device(None, 0, ks, 2, 0, out, corr, None, None, None, None) == -1
    assert L.knn_kfold_sweep(None, ks, 2, 0, out, corr, None, None, None, None, None) == -1
    assert L.knn_group_set_folds(None, folds, 2) == -3
    assert L.knn_group_kfold_sweep(None, ks, 2, 0, out, corr, None, None) == -3
    assert "before set_train" in L.knn_last_error().decode()


def test_mirror_checks_the_fold_array(knn):
    """Refused in the mirror, before any device call."""
    c = knn.Classifier.__new__(knn.Classifier)
    c.class_cnt, c.n_train, c.device, c._h = 3, 4, 0, ctypes.c_void_p()
    with pytest.raises(ValueError, match="one id per train row"):
        c.set_folds([0, 1])
    with pytest.raises(ValueError, match="labels=False needs confusion=True"):
        c.kfold_sweep([1], labels=False)


def test_driver_help_names_kfold(knn):
    r = subprocess.run([knn.DRIVER_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--kfold" in r.stderr + r.stdout and "--folds" in r.stderr + r.stdout


@pytest.mark.parametrize("args, msg", [
    (["--kfold", "5", "--loo", "--K_list", "1,3"], "--kfold and --loo exclude each other"),
    (["--kfold", "5"], "--kfold needs --K_list"),
    (["--kfold", "1", "--K_list", "1,3"], "fold count in [2, 64]"),
    (["--kfold", "65", "--K_list", "1,3"], "fold count in [2, 64]"),
    (["--folds", "folds.csv", "--K_list", "1,3"], "--folds needs --kfold"),
])
def test_driver_usage_errors(knn, tmp_path, args, msg):
    """Refused while the flags are checked: no file is read, no device call made."""
    r = subprocess.run([knn.DRIVER_PATH] + args, cwd=str(tmp_path), capture_output=True,
                       text=True)
    assert r.returncode == 1
    assert msg in r.stderr
    assert "accuracy" not in r.stdout

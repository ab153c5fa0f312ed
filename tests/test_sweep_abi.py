"""CPU checks of the K sweep's boundary: the header declares its four entry
points, the built library exports them, the Python mirror lists and binds
them, and the driver knows --K_list and refuses it without a validation pass
before any device call.  No GPU calls are made."""
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "-mpi-knn-_amd")
HEADER = os.path.join(ROOT, "include", "knn_amd.h")
SWEEP = ("knn_vote_sweep_device", "knn_classify_sweep_device", "knn_classify_sweep",
         "knn_group_classify_sweep")


@pytest.fixture(scope="module")
def knn():
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(PKG, "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not (os.path.exists(mod.LIB_PATH) and os.path.exists(mod.DRIVER_PATH)):
        mod.build()
    return mod


def test_header_declares_the_sweep():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SWEEP:
        assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), name


def test_library_exports_the_sweep(knn):
    out = subprocess.run(["nm", "-D", "--defined-only", knn.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (knn_\w+)", out))
    assert set(SWEEP) <= exported
    L = ctypes.CDLL(knn.LIB_PATH)
    for name in SWEEP:
        assert hasattr(L, name)


def test_mirror_lists_and_binds_the_sweep(knn):
    assert set(SWEEP) <= set(knn.EXPORTED)
    for name in SWEEP:
        fn = getattr(knn.lib(), name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert callable(knn.Classifier.classify_sweep)
    assert callable(knn.Classifier.vote_sweep_device)
    assert callable(knn.Group.classify_sweep)


def test_driver_help_names_k_list(knn):
    r = subprocess.run([knn.DRIVER_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--K_list" in r.stderr + r.stdout


def test_driver_k_list_needs_validation(knn, tmp_path):
    """Refused while the flags are checked: no file is read, no device call made."""
    r = subprocess.run([knn.DRIVER_PATH, "--K_list", "1,3", "--Validation", "false"],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode != 0
    assert "--K_list needs --Validation true" in r.stderr
    assert "accuracy" not in r.stdout


@pytest.mark.parametrize("bad", ["", "1,,3", "1,x", "-2", "3,"])
def test_driver_k_list_syntax(knn, tmp_path, bad):
    r = subprocess.run([knn.DRIVER_PATH, "--K_list=" + bad], cwd=str(tmp_path),
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "--K_list" in r.stderr

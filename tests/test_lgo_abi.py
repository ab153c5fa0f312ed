"""CPU checks of the leave-group-out sweep's boundary: the header declares its
entry points, the built library exports them with the documented prototypes,
the Python mirror lists and binds them, without a device the calls refuse the
null handle, and the driver knows --groups and refuses it without --loo
--K_list before any device call.
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
LGO = {
    "knn_set_groups": ("int", ["knn_ctx*", "const int32_t*", "int32_t"]),
    "knn_set_groups_device": ("int", ["knn_ctx*", "const int32_t*", "int32_t"]),
    "knn_get_group_max": ("int32_t", ["knn_ctx*"]),
    "knn_classify_sweep_gexcl_device": ("int", [
        "knn_ctx*", "const double*", "int64_t", "const int32_t*", "const int32_t*", "int32_t",
        "int32_t", "int32_t*", "const int32_t*", "int64_t*", "int64_t*", "double*", "int32_t*",
        "void*"]),
    "knn_lgo_sweep_device": ("int", [
        "knn_ctx*", "int64_t", "int64_t", "const int32_t*", "int32_t", "int32_t", "int32_t*",
        "int64_t*", "int64_t*", "double*", "int32_t*", "void*"]),
    "knn_lgo_sweep": ("int", [
        "knn_ctx*", "const int32_t*", "int32_t", "int32_t", "int32_t*", "int64_t*", "int64_t*",
        "int64_t*", "int64_t*", "double*", "int32_t*"]),
    "knn_group_set_groups": ("int", ["knn_group*", "const int32_t*", "int32_t"]),
    "knn_group_lgo_sweep": ("int", [
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
    for name, (ret, want) in LGO.items():
        m = re.search(r"^%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), src, flags=re.M)
        assert m, name
        got = []
        for p in m.group(1).split(","):
            p = " ".join(p.split())
            got.append(re.sub(r"\s*\w+$", "", p).replace(" *", "*"))  # drop the parameter name
        assert got == want, name
    text = open(HEADER).read()
    assert "leave-one-group-out" in text and "candidate pass" in text


def test_stream_tables_hold_every_entry_point():
    """The two new device calls take a stream (a `void*` parameter whose name
    ends in `stream`).  They and every entry point that tests/streams.py
    counts are in the entry point -> test table of test_gpu_streams.py or of
    test_gpu_lgo_streams.py, with a test that exists in that file; the two new
    calls are in the latter."""
    import streams
    text = open(HEADER).read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    new = sorted(
        m.group(1) for m in re.finditer(r"\bint\s+(knn_\w+)\s*\(([^;{]*?)\)\s*;", flat, flags=re.S)
        if m.group(1) in LGO and re.search(r"void\s*\*\s*\w*stream\b", m.group(2)))
    assert new == ["knn_classify_sweep_gexcl_device", "knn_lgo_sweep_device"]
    names = sorted(set(streams.stream_entry_points(text)) | set(new))
    here = os.path.dirname(os.path.abspath(__file__))
    tables = {}
    for fname in ("test_gpu_streams.py", "test_gpu_lgo_streams.py"):
        text = open(os.path.join(here, fname)).read()
        doc = text.split('"""')[1]
        tests = set(re.findall(r"^def (test_\w+)", text, flags=re.M))
        for n in names:
            m = re.search(r"^\s*%s\s+(test_\w+)" % re.escape(n), doc, flags=re.M)
            if m:
                assert m.group(1) in tests, "%s -> %s: no such test in %s" % (n, m.group(1), fname)
                tables[n] = fname
        body = text.split('"""', 2)[2]
        assert "xfail" not in body and "skip" not in body
    assert sorted(tables) == names, set(names) - set(tables)
    assert tables["knn_lgo_sweep_device"] == tables["knn_classify_sweep_gexcl_device"] \
        == "test_gpu_lgo_streams.py"


def test_library_exports_the_calls(knn):
    out = subprocess.run(["nm", "-D", "--defined-only", knn.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (knn_\w+)", out))
    assert set(LGO) <= exported


def test_mirror_lists_and_binds_the_calls(knn):
    assert set(LGO) <= set(knn.EXPORTED)
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    ctype = lambda t: P if t.endswith("*") else {"int32_t": i32, "int64_t": i64}[t]  # noqa: E731
    for name, (ret, params) in LGO.items():
        fn = getattr(knn.lib(), name)
        assert fn.restype is (ctypes.c_int if ret == "int" else i32)
        assert list(fn.argtypes) == [ctype(t) for t in params], name
    for meth in ("set_groups", "lgo_sweep", "lgo_sweep_device", "classify_sweep_gexcl_device",
                 "group_max"):
        assert callable(getattr(knn.Classifier, meth))
    assert callable(knn.Group.set_groups) and callable(knn.Group.lgo_sweep)
    assert "exclude_group" in inspect.signature(knn.Classifier.classify_sweep).parameters
    for par in ("return_neighbors", "confusion", "labels"):
        assert par in inspect.signature(knn.Classifier.lgo_sweep).parameters


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
    grp = (ctypes.c_int32 * 4)(0, 1, 1, 2)
    assert L.knn_set_groups(None, grp, 3) == -1
    assert L.knn_set_groups_device(None, None, 0) == -1
    assert L.knn_get_group_max(None) == 0
    for d_qgroup in (None, grp):
        assert L.knn_classify_sweep_gexcl_device(None, None, 0, d_qgroup, ks, 2, 0, out, None,
                                                 None, None, None, None, None) == -1
    assert L.knn_lgo_sweep_device(None, 0, 0, ks, 2, 0, out, corr, None, None, None, None) == -1
    assert L.knn_lgo_sweep(None, ks, 2, 0, out, corr, None, None, None, None, None) == -1
    assert L.knn_group_set_groups(None, grp, 3) == -3
    assert L.knn_group_lgo_sweep(None, ks, 2, 0, out, corr, None, None) == -3
    assert "before set_train" in L.knn_last_error().decode()
    assert L.knn_group_lgo_sweep(None, ks, 2, 0, None, corr, None, None) == -1


def test_mutually_exclusive_exclusions(knn):
    """Refused in the mirror, before any device call."""
    c = knn.Classifier.__new__(knn.Classifier)
    c.class_cnt, c.n_train, c.device, c._h = 3, 4, 0, ctypes.c_void_p()
    import numpy as np
    with pytest.raises(ValueError, match="mutually exclusive"):
        c.classify_sweep(np.zeros((2, 3)), [1], exclude=np.array([-1, -1]),
                         exclude_group=np.array([0, 0]))
    with pytest.raises(ValueError, match="one group id"):
        c.classify_sweep(np.zeros((2, 3)), [1], exclude_group=np.array([0]))
    with pytest.raises(ValueError, match="one id per train row"):
        c.set_groups([0, 1])


def test_driver_help_names_groups(knn):
    r = subprocess.run([knn.DRIVER_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--groups" in r.stderr + r.stdout


@pytest.mark.parametrize("extra", [[], ["--loo"], ["--K_list", "1,3"]])
def test_driver_groups_needs_loo_and_k_list(knn, tmp_path, extra):
    """Refused while the flags are checked: no file is read, no device call made."""
    r = subprocess.run([knn.DRIVER_PATH, "--groups", "groups.csv"] + extra, cwd=str(tmp_path),
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "--groups needs --loo --K_list" in r.stderr or "--loo needs --K_list" in r.stderr
    assert "accuracy" not in r.stdout

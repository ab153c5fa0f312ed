"""The reference's CSV reader on the GPU (knn_csv_read, knn_csv_read_device,
knn_csv_parse_device, Classifier.read_csv, the driver's --csv gpu) against the
oracle's restatement of the reference's reader (cpp:154-222: getline /
stringstream split on ',' / atof / atoi), bit for bit (tobytes()) plus the
token count.  Files come from tests/csvcases.py (checked on a CPU by
tests/test_csvcases_data.py); B = KNN_CSV_BLOCK_BYTES, the bytes one workgroup
owns."""
import os

import numpy as np
import pytest

import csvcases
import oracle

pytestmark = pytest.mark.gpu

B = csvcases.B


@pytest.fixture(scope="module")
def knn():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "knn_amd", os.path.join(root, "-mpi-knn-_amd", "knn_amd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if mod.lib().knn_device_count() < 1:
        pytest.fail("no HIP device visible: the KNN path has no CPU fallback")
    return mod


@pytest.fixture(scope="module")
def clf(knn):
    """A context without a train set: the reader needs none."""
    c = knn.Classifier(0)
    yield c
    c.close()


def _same(clf, path, dim, with_label, rows, what=""):
    """read_csv on the GPU == the oracle's reader: values, labels, tokens."""
    want, wlab, wn = oracle.read_csv(str(path), dim, with_label, rows)
    got, glab, gn = clf.read_csv(str(path), dim, with_label, rows)
    assert gn == wn, what
    assert got.dtype == np.float64 and got.shape == (rows, dim)
    assert got.tobytes() == want.tobytes(), what
    if with_label:
        assert glab.dtype == np.int32 and glab.tobytes() == wlab.tobytes(), what
    else:
        assert glab is None
    return gn


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text)
    return p


@pytest.mark.parametrize("reps", [1, 8])
def test_tricky_tokens(clf, tmp_path, reps):
    """Every fallback of the conversion, mixed line ends; once with the last
    line open, and eight times over so the text spans several blocks."""
    text, dim, rows = csvcases.tricky_text(reps)
    p = _write(tmp_path, "tricky.csv", text)
    # (rows ending in the empty token lose it, as in the reference: fewer tokens)
    assert rows * dim < _same(clf, p, dim, True, rows) < rows * (dim + 1)
    assert clf.csv_last_slow() > rows  # blanks, '+', '\r', hex, inf / nan ... went to the host


def test_block_edges(clf, tmp_path):
    """Files of exactly B-1, B, B+1, 3B-1, 3B, 3B+1 bytes, token lengths 1..24
    cycling; a terminator, '-', '.', 'e' and a look-back byte on a block's
    first and last byte."""
    for name, text in csvcases.edge_cases():
        p = _write(tmp_path, "edge.csv", text)
        n = len(csvcases.rule_tokens(text)[0])
        for dim, with_label in ((5, True), (3, False)):
            rows = n // (dim + with_label) + 1
            assert _same(clf, p, dim, with_label, rows, name) == n, name


@pytest.mark.parametrize("name", sorted(csvcases.LINE_CASES))
def test_line_structure(clf, tmp_path, name):
    p = _write(tmp_path, name + ".csv", csvcases.LINE_CASES[name])
    _same(clf, p, 2, True, 5, name)
    _same(clf, p, 3, False, 4, name)


@pytest.mark.parametrize("with_label", [True, False])
def test_bounds(clf, knn, tmp_path, with_label):
    """More tokens than rows * (dim [+ 1]): counted, not stored.  Fewer: the
    remaining cells of sentinel-filled arrays are untouched."""
    import ctypes
    dim = 4
    per = dim + with_label
    labs = ["3.0", " 7", "-1", "12345678901", "5"]
    rows = 10
    text = "".join((labs[r % 5] + "," if with_label else "") +
                   ",".join("%d.25" % (r * dim + j) for j in range(dim)) + "\n"
                   for r in range(rows)).encode()
    p = _write(tmp_path, "b.csv", text)
    # more tokens than cells
    assert _same(clf, p, dim, with_label, 6) == rows * per
    assert _same(clf, p, dim, with_label, 0) == rows * per
    # fewer: sentinels stay (the C call on caller-filled arrays)
    big = 16
    data = np.full((big, dim), -77.5)
    lab = np.full(big, -99, np.int32)
    tokens = ctypes.c_int64(0)
    rc = knn.lib().knn_csv_read(clf.handle, str(p).encode(), dim, int(with_label), big,
                                data.ctypes.data, lab.ctypes.data if with_label else None,
                                ctypes.byref(tokens))
    assert rc == 0 and tokens.value == rows * per
    want, wlab, _ = oracle.read_csv(str(p), dim, with_label, rows)
    assert data[:rows].tobytes() == want.tobytes()
    assert (data[rows:] == -77.5).all()
    if with_label:
        assert lab[:rows].tobytes() == wlab.tobytes()
        assert (lab[rows:] == -99).all()
    # a partial last row: tokens end in the middle of row 3
    cut = text.split(b"\n")
    part = b"\n".join(cut[:3]) + b"\n" + b",".join(cut[3].split(b",")[:2])
    p2 = _write(tmp_path, "b2.csv", part)
    data[:] = -77.5
    lab[:] = -99
    rc = knn.lib().knn_csv_read(clf.handle, str(p2).encode(), dim, int(with_label), big,
                                data.ctypes.data, lab.ctypes.data if with_label else None,
                                ctypes.byref(tokens))
    assert rc == 0 and tokens.value == 3 * per + 2
    want = np.full((big, dim), -77.5)
    wl = np.full(big, -99, np.int32)
    ref, rlab, _ = oracle.read_csv(str(p2), dim, with_label, 4)
    nd = 3 * dim + (1 if with_label else 2)
    want.reshape(-1)[:nd] = ref.reshape(-1)[:nd]
    assert data.tobytes() == want.tobytes()
    if with_label:
        wl[:4] = rlab
        assert lab.tobytes() == wl.tobytes()


@pytest.mark.parametrize("length", [65, 200, 5000])
def test_long_tokens(clf, tmp_path, length):
    """Tokens beyond the kernel's 64-byte walk go to the host, wherever they
    stand: digits and garbage, at the start, middle, end, across a block edge."""
    for garbage in (False, True):
        for where in ("start", "middle", "end", "edge"):
            text = csvcases.long_token_text(length, garbage, where)
            p = _write(tmp_path, "long.csv", text)
            n = len(csvcases.rule_tokens(text)[0])
            what = "%d %s %s" % (length, garbage, where)
            assert _same(clf, p, 4, False, n // 4 + 1, what) == n
            assert clf.csv_last_slow() >= 1
            _same(clf, p, 4, True, n // 5 + 1, what)


def test_slow_list_overflow(clf, tmp_path):
    """100 KB of '+1,': about 33k slow tokens against a first capacity of
    4096, so the conversion runs once more with room for all."""
    text = csvcases.all_slow_text()
    p = _write(tmp_path, "slow.csv", text)
    n = len(text) // 3
    assert max(4096, len(text) // 64) < n
    assert _same(clf, p, 7, False, n // 7 + 1) == n
    assert clf.csv_last_slow() == n
    got, _, _ = clf.read_csv(str(p), 7, False, n // 7)
    assert (got == 1.0).all()


def test_tier1_files_have_no_slow_token(clf, tmp_path):
    """bench.write_grid_csv's k/256 values and integers 0..255 are tier 1."""
    import bench
    codes, lab = csvcases.grid_codes()
    for labels in (lab, None):
        p = tmp_path / "grid.csv"
        bench.write_grid_csv(str(p), codes, labels, chunk=300)
        got, glab, n = clf.read_csv(str(p), codes.shape[1], labels is not None, codes.shape[0])
        assert n == codes.shape[0] * (codes.shape[1] + (labels is not None))
        assert got.tobytes() == (codes.astype(np.float64) / 256.0).tobytes()
        assert clf.csv_last_slow() == 0
        if labels is not None:
            np.testing.assert_array_equal(glab, lab)
    text, dim, rows = csvcases.int_text()
    p = _write(tmp_path, "ints.csv", text)
    assert _same(clf, p, dim, True, rows) == rows * (dim + 1)
    assert clf.csv_last_slow() == 0


def test_missing_file_and_bad_arguments(clf, knn, tmp_path):
    with pytest.raises(knn.KnnError, match="nope.csv"):
        clf.read_csv(str(tmp_path / "nope.csv"), 3, False, 2)
    p = _write(tmp_path, "a.csv", b"1,2,3\n")
    with pytest.raises(knn.KnnError):
        clf.read_csv(str(p), 0, False, 2)
    import ctypes
    data = np.zeros(3)
    tokens = ctypes.c_int64(0)
    L = knn.lib()  # rows < 0 (numpy refuses it before the library sees it)
    assert L.knn_csv_read(clf.handle, str(p).encode(), 3, 0, -1, data.ctypes.data, None,
                          ctypes.byref(tokens)) == -1
    assert L.knn_csv_parse_device(clf.handle, None, -1, 3, 0, 1, None, None, None, None, 0, None,
                                  None) == -1


def test_device_path_equals_host(clf, tmp_path):
    import torch
    text, dim, rows = csvcases.tricky_text(1)
    p = _write(tmp_path, "tricky.csv", text)
    want, wlab, wn = oracle.read_csv(str(p), dim, True, rows)
    d, l, n = clf.read_csv(str(p), dim, True, rows, device=True)
    assert isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.float64
    assert l.dtype == torch.int32 and n == wn
    assert d.cpu().numpy().tobytes() == want.tobytes()
    assert l.cpu().numpy().tobytes() == wlab.tobytes()
    text = csvcases.edge_cases()[-1][1]
    p = _write(tmp_path, "e.csv", text)
    want, _, wn = oracle.read_csv(str(p), 3, False, 5000)
    d, l, n = clf.read_csv(str(p), 3, False, 5000, device=True)
    assert l is None and n == wn and d.cpu().numpy().tobytes() == want.tobytes()


def test_parse_device_on_a_caller_stream(clf, tmp_path):
    """The building block on a non-default torch stream: the text is uploaded
    on that stream, no host sync before the call, results read after syncing
    that stream; the slow tokens are finished here with Python's float / int."""
    import torch
    dev = torch.device("cuda", 0)
    text, dim, rows = csvcases.int_text(rows=900, dim=28, seed=4)
    text = text.replace(b"\n", b"\r\n", 40)  # forty slow tokens
    p = _write(tmp_path, "s.csv", text)
    want, wlab, wn = oracle.read_csv(str(p), dim, True, rows)
    host = torch.frombuffer(bytearray(text), dtype=torch.uint8).pin_memory()
    cap = 64
    S = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(S):
        d_text = host.to(dev, non_blocking=True)
        data = torch.zeros((rows, dim), dtype=torch.float64, device=dev)
        lab = torch.zeros(rows, dtype=torch.int32, device=dev)
        misc = torch.full((2,), -1, dtype=torch.int64, device=dev)
        slow = torch.zeros((cap, 2), dtype=torch.int64, device=dev)
        clf.csv_parse_device(d_text.data_ptr(), len(text), dim, True, rows, data.data_ptr(),
                             lab.data_ptr(), misc.data_ptr(), slow.data_ptr(), cap,
                             misc.data_ptr() + 8, stream=S.cuda_stream)
    S.synchronize()
    tokens, nslow = misc.cpu().tolist()
    assert tokens == wn and nslow == 40
    got, glab = data.cpu().numpy(), lab.cpu().numpy()
    for c, pos in slow.cpu().numpy()[:nslow].tolist():
        b = max(text.rfind(b",", 0, pos), text.rfind(b"\n", 0, pos)) + 1
        assert c % (dim + 1) != 0
        got.reshape(-1)[c - c // (dim + 1) - 1] = float(text[b:pos])
    assert got.tobytes() == want.tobytes()
    assert glab.tobytes() == wlab.tobytes()


def test_driver_csv_gpu_equals_host(knn, tmp_path):
    """--csv gpu and --csv host: byte-identical Test_label.csv, stdout identical
    apart from the Running time line."""
    paths = csvcases.driver_files(tmp_path)
    cfg = knn.KnnConfig(dim=7, K=5, N_train=300, N_test=100, N_val=100, class_cnt=4,
                        train_file_name=paths["train"], validation_file_name=paths["val"],
                        test_file_name=paths["test"])
    outs = {}
    for mode in ("host", "gpu"):
        wd = tmp_path / mode
        wd.mkdir()
        stdout = knn.run_driver(cfg, str(wd), extra=["--csv", mode])
        lines = [ln for ln in stdout.splitlines() if not ln.startswith("Running time")]
        outs[mode] = (lines, (wd / "Test_label.csv").read_bytes())
    assert outs["gpu"][0] == outs["host"][0] and outs["host"][0]
    assert outs["gpu"][1] == outs["host"][1] and len(outs["host"][1].splitlines()) == 100

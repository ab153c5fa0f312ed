"""CSV files for the GPU reader's tests (tests/test_gpu_csv.py), built from
seeds, and a numpy restatement of the byte-parallel token rule the kernels use
(include/knn_amd.h), which tests/test_csvcases_data.py checks against the
oracle's reader on every file built here.  No GPU is needed to build them."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "knn_amd.h")
_m = re.search(r"#define\s+KNN_CSV_BLOCK_BYTES\s+(\d+)", open(HEADER).read())
# bytes one workgroup owns (0: the header has no reader yet)
B = int(_m.group(1)) if _m else 0
TOKEN_MAX = 64  # longer tokens go to the host

# tests/test_csv_parse.py's list: every fallback of the conversion
TRICKY = ["0.1", "-0.0", "1e-310", "  5.5", "+3", "0x1p-3", "inf", "-INF", "nan", "1.5abc", "",
          ".5", "5.", "1e400", "4.9e-324", "-7", "0.30000000000000004", "123456789012345678901",
          "  -2.5e+3", "1E5", "abc", "0000.25"]


def rule_tokens(text):
    """(terminator positions, token starts) by the byte-parallel rule: p ends a
    token iff text[p] == ',' or (text[p] == '\\n' or p == len) and p > 0 and
    text[p-1] is neither; the token starts after the previous ',' or '\\n'."""
    a = np.frombuffer(text + b"\n", np.uint8)  # the end of the file acts as a newline
    n = len(text)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    comma, nl = a == ord(","), a == ord("\n")
    delim = comma | nl
    prev = np.concatenate([[True], delim[:-1]])
    term = np.flatnonzero(comma | (nl & ~prev))
    dpos = np.concatenate([[-1], np.flatnonzero(delim[:n])])  # (-1: the start of the file)
    start = dpos[np.searchsorted(dpos, term, side="left") - 1] + 1  # after the last one before p
    return term.astype(np.int64), start.astype(np.int64)


def tricky_text(reps=1):
    """4000 rows, dim 7, labels; tricky tokens, every fifth row %.17g normals,
    every third line CRLF; reps == 1: the last line without its newline."""
    rng = np.random.default_rng(5)
    dim, rows = 7, 4000
    lines = []
    for r in range(rows):
        toks = [TRICKY[i] for i in rng.integers(0, len(TRICKY), dim)]
        if r % 5 == 0:
            toks = ["%.17g" % v for v in rng.standard_normal(dim)]
        lines.append("%d," % (r % 10) + ",".join(toks) + ("\r\n" if r % 3 == 0 else "\n"))
    text = "".join(lines)
    return (text[:-1] if reps == 1 else text * reps).encode(), dim, rows * reps


def _token(L, i):
    """A numeric token of exactly L bytes (L >= 1) with '-', '.', 'e' where
    the length allows."""
    d = "%d" % (1 + i % 9)
    if L == 1:
        return d
    if L == 2:
        return "-" + d
    if L < 7:
        return (d + "." + "5274" * 6)[:L]
    tail = "e-3" if i % 2 else "e+2"
    return ("-" + d + "." + "618033" * 5)[:L - 3] + tail


def _fill(n, i0, close=True):
    """Exactly n bytes of tokens with lengths 1..24 cycling, ',' after each,
    '\\n' after every seventh; close=False: the last token runs to the end."""
    out, i = [], i0
    left = n
    while left > 0:
        L = 1 + i % 24
        if L + 1 >= left:
            L = left - 1 if close else left
        tok = _token(L, i) if L > 0 else ""
        out.append(tok)
        left -= len(tok)
        if left > 0:
            out.append("\n" if i % 7 == 6 else ",")
            left -= 1
        i += 1
    s = "".join(out)
    assert len(s) == n
    return s


# (snippet, index of the marked byte): the byte that must land on a block edge
EDGE_MARKS = [("7,", 1), ("7\n", 1), ("-1.5e-3,", 0), ("-1.5e-3,", 2), ("-1.5e-3,", 4),
              (",\n", 1), ("\n\n", 1), ("3,\n", 1), ("25\r\n", 3)]


def edge_text(nbytes, mark, at, close):
    """A file of exactly nbytes bytes whose marked snippet byte stands at
    position `at` (None when it does not fit)."""
    snip, k = mark
    s0 = at - k
    if s0 < 2 or s0 + len(snip) > nbytes:
        return None
    head = _fill(s0, 3)
    tail = _fill(nbytes - s0 - len(snip), 11, close)
    text = (head + snip + tail).encode()
    assert len(text) == nbytes and text[at] == ord(snip[k])
    return text


def edge_cases():
    """[(name, text)] over the sizes B-1, B, B+1, 3B-1, 3B, 3B+1: each mark on
    the last byte of a block and on the first byte of the next."""
    out = []
    for n in (B - 1, B, B + 1, 3 * B - 1, 3 * B, 3 * B + 1):
        for edge in (B, 3 * B):
            for at in (edge - 1, edge):
                for j, mark in enumerate(EDGE_MARKS):
                    text = edge_text(n, mark, at, close=(j + at) % 2 == 0)
                    if text is not None:
                        out.append(("n%d_at%d_m%d" % (n, at, j), text))
        out.append(("n%d_plain" % n, _fill(n, 0, close=n % 2 == 0).encode()))
    return out


# name -> text: the line structures the reference's getline pair decides
LINE_CASES = {
    "empty": b"",
    "newlines": b"\n\n\n\n",
    "comma_newline": b",\n",
    "trailing_comma_line": b"1,2,\n",
    "leading_comma": b",1,2",
    "blank_lines": b"1,2,3\n\n\n4,5,6\n\n7,8,9\n",
    "ends_in_comma": b"1,2,3\n4,5,",
    "crlf": b"1,2,3\r\n4,5,6\r\n7,8,9\r\n",
    "one_token": b"42",
    "one_comma": b",",
    "one_newline": b"\n",
    "crlf_blank_lines": b"1,2\r\n\r\n3,4\r\n",
}


def long_token_text(length, garbage, where):
    """Rows of short tokens with one token of `length` bytes (digits, or
    garbage) at the start, the middle, the end, or across the first block edge
    ('edge': it begins 10 bytes in front of position B)."""
    tok = ("x" if garbage else "") + "1234567890" * (length // 10 + 1)
    tok = tok[:length]
    if where == "start":
        return (tok + "," + _fill(3000, 1)).encode()
    if where == "middle":
        return (_fill(3000, 1) + tok + "," + _fill(3000, 5)).encode()
    if where == "end":
        return (_fill(3000, 1) + tok).encode()
    assert where == "edge"
    return (_fill(B - 10, 1) + tok + "\n" + _fill(500, 2)).encode()


def all_slow_text():
    """100 KB of '+1,' tokens: every token is slow."""
    return b"+1," * (100 * 1024 // 3)


def grid_codes(rows=500, dim=24, seed=8):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (rows, dim)).astype(np.uint8),
            rng.integers(0, 10, rows).astype(np.int32))


def int_text(rows=700, dim=28, seed=3):
    """An MNIST-like file: a label and integers 0..255 per row."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (rows, dim))
    lab = rng.integers(0, 10, rows)
    return "".join("%d," % lab[r] + ",".join("%d" % x for x in v[r]) + "\n"
                   for r in range(rows)).encode(), dim, rows


def driver_files(d, n_train=300, n_val=100, n_test=100, dim=7, seed=21):
    """Generated CSVs in the reference's three formats under directory d."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 10, (4, dim))

    def block(n):
        lab = rng.integers(0, 4, n)
        return lab, centres[lab] + rng.standard_normal((n, dim))

    paths = {}
    for name, n, with_label in (("train", n_train, True), ("val", n_val, True),
                                ("test", n_test, False)):
        lab, X = block(n)
        rows = [("%d," % lab[r] if with_label else "") + ",".join("%.17g" % v for v in X[r])
                for r in range(n)]
        paths[name] = os.path.join(str(d), name + ".csv")
        with open(paths[name], "w") as f:
            f.write("\n".join(rows) + "\n")
    return paths

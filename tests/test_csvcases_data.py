"""CPU checks of the files tests/csvcases.py builds for the GPU reader's tests:
their sizes relative to KNN_CSV_BLOCK_BYTES, the bytes that must stand on a
block's first and last position, and that the byte-parallel token rule the
kernels use (csvcases.rule_tokens) finds exactly the tokens the oracle's
restatement of the reference's reader finds, with the same text."""
import numpy as np

import csvcases
import oracle

B = csvcases.B


def _oracle_tokens(tmp_path, text, name="f.csv"):
    p = tmp_path / name
    p.write_bytes(text)
    return oracle.read_csv(str(p), 1, False, 1)[2]


def test_block_size_is_declared():
    assert B >= 4096 and B % 4096 == 0


def test_edge_files_have_the_sizes_and_marks(tmp_path):
    cases = csvcases.edge_cases()
    sizes = sorted({len(t) for _, t in cases})
    assert sizes == sorted({B - 1, B, B + 1, 3 * B - 1, 3 * B, 3 * B + 1})
    # each marked byte lands on a block's last and first byte in some file
    want = {ord(s[k]) for s, k in csvcases.EDGE_MARKS}
    last = {t[B - 1] for _, t in cases if len(t) > B}
    first = {t[B] for _, t in cases if len(t) > B}
    assert want <= last and want <= first
    # a look-back byte on an edge decides: '\n' at a block's first byte after a
    # ',' (no token) and after a digit (a token)
    assert any(len(t) > B and t[B] == 10 and t[B - 1] == ord(",") for _, t in cases)
    assert any(len(t) > B and t[B] == 10 and chr(t[B - 1]).isdigit() for _, t in cases)
    # token lengths 1..24 all occur
    term, start = csvcases.rule_tokens(cases[-1][1])
    assert set(range(1, 25)) <= set((term - start).tolist())
    for name, text in cases[::7] + cases[-6:]:
        term, _ = csvcases.rule_tokens(text)
        assert len(term) == _oracle_tokens(tmp_path, text), name


def test_rule_matches_the_oracle_on_line_structures(tmp_path):
    for name, text in csvcases.LINE_CASES.items():
        term, start = csvcases.rule_tokens(text)
        assert len(term) == _oracle_tokens(tmp_path, text), name
        assert (start <= term).all()


def test_tricky_text_spans_blocks_and_matches(tmp_path):
    text, dim, rows = csvcases.tricky_text(1)
    assert not text.endswith(b"\n") and b"\r\n" in text
    big, _, rows8 = csvcases.tricky_text(8)
    assert rows8 == 8 * rows and len(big) > 4 * B
    term, start = csvcases.rule_tokens(text)
    # (a row ending in the empty token loses it: the count is the oracle's, not
    # rows * (dim + 1), and the rows drift as in the reference)
    n = _oracle_tokens(tmp_path, text)
    assert len(term) == n and 0 < rows * (dim + 1) - n < rows
    assert len(csvcases.rule_tokens(big)[0]) == _oracle_tokens(tmp_path, big)


def test_long_and_slow_files(tmp_path):
    for length in (65, 200, 5000):
        for where in ("start", "middle", "end", "edge"):
            text = csvcases.long_token_text(length, False, where)
            term, start = csvcases.rule_tokens(text)
            assert (term - start).max() == length > csvcases.TOKEN_MAX
            assert len(term) == _oracle_tokens(tmp_path, text)
    text = csvcases.long_token_text(200, False, "edge")
    term, start = csvcases.rule_tokens(text)
    i = int(np.argmax(term - start))
    assert start[i] < B <= term[i]
    slow = csvcases.all_slow_text()
    assert 99 * 1024 < len(slow) <= 100 * 1024
    assert len(csvcases.rule_tokens(slow)[0]) == len(slow) // 3 > 8 * 4096


def test_driver_files_hold_the_rows(tmp_path):
    paths = csvcases.driver_files(tmp_path)
    data, lab, n = oracle.read_csv(paths["train"], 7, True, 300)
    assert n == 300 * 8 and set(lab.tolist()) <= {0, 1, 2, 3}
    assert oracle.read_csv(paths["test"], 7, False, 100)[2] == 700

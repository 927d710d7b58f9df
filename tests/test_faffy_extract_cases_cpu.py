"""The inputs of the extract plan tests (tests/extract_device_lib.py) hit the cases they are named after: shown on the checker
(tests/faffy_lib.py), without a GPU."""
import ctypes

import pytest

import extract_device_lib as X
import faffy_lib as F


def case(cid):
    return next(c for c in X.CASES if c[0] == cid)


def checker(c):
    return F.extract(X.FILES, c[1], c[2], c[3], skip_missing=c[4])


def test_the_atol_table_equals_libc():
    libc = ctypes.CDLL("libc.so.6")
    libc.atol.restype = ctypes.c_long
    libc.atol.argtypes = [ctypes.c_char_p]
    assert set(X.ATOL) == set(X.NUMBER_TOKENS)
    for tok, want in X.ATOL.items():
        assert libc.atol(tok) == want == F.atol(tok), tok


def test_the_covering_interval_yields_one_item():
    out, status, _ = checker(case("pmax-covering"))
    assert status == 0 and X.items(out) == [b">big|200000|0"]
    assert len(out) == len(b">big|200000|0\n") + 10000 + 1
    assert len(X.items(checker(case("pmax-covering-joins"))[0])) == 1
    assert X.items(checker(case("pmax-covering-new-item"))[0]) == [b">big|200000|0", b">big|200000|10001"]
    assert len(X.items(checker(case("pmax-covering-flank-joins"))[0])) == 1
    assert len(X.items(checker(case("pmax-covering-flank-at-flank"))[0])) == 1
    assert len(X.items(checker(case("pmax-covering-flank-new-item"))[0])) == 2


def test_of_the_two_touching_inputs_one_merges():
    assert X.items(checker(case("sweep-touching"))[0]) == [b">chr1|3000|95"]
    assert X.items(checker(case("sweep-one-apart"))[0]) == [b">chr1|3000|95", b">chr1|3000|206"]
    assert len(X.items(checker(case("sweep-dropped-between-merging"))[0])) == 1
    assert len(X.items(checker(case("sweep-dropped-between-separate"))[0])) == 2
    assert len(X.items(checker(case("sweep-min-size-equal-and-below"))[0])) == 1
    assert len(X.items(checker(case("sweep-min-size-one-more"))[0])) == 0


def test_the_run_inputs_have_long_runs():
    c = case("pmax-run-of-5000")
    assert X.longest_run(c[1], c[2], c[3]) == 5000
    big = X.big_case()
    assert len(F.bed_lines(big[1])) == 100001
    assert X.longest_run(big[1], big[2], big[3]) > 4096
    assert checker(big)[1] == 0


def test_the_duplicate_name_means_the_last_record():
    out, status, _ = checker(case("name-duplicate-last-wins"))
    assert status == 0 and X.items(out) == [b">dup|1200|0", b">dup|1200|1000"]
    assert checker(case("name-duplicate-first-length"))[1] == 0
    assert checker(case("name-space-header"))[1:] == (1, b"Missing sequence: has\n")


def test_the_edge_inputs_lie_on_the_edges():
    for at in (X.SLICE, X.TILE):
        for tok in range(3):
            bed = case("edge-straddle-%d-token%d" % (at, tok))[1]
            line = next(ln for ln in F.bed_lines(bed) if ln.startswith(b"chr1_random"))
            s = bed.index(line)
            a = s + line.index(line.split()[tok])
            assert a < at < a + len(line.split()[tok]), (at, tok)
    assert len(case("edge-exactly-a-tile")[1]) == X.TILE and case("edge-exactly-a-tile")[1].endswith(b"\n")
    assert len(case("edge-a-tile-less-one")[1]) == X.TILE - 1 and len(case("edge-a-tile-and-one")[1]) == X.TILE + 1
    bed = case("first-fail-at-slice-start")[1]
    assert bed[X.SLICE:].startswith(b"nope") and bed[X.SLICE - 1:X.SLICE] == b"\n"
    bed = case("first-fail-at-tile-start")[1]
    assert bed[X.TILE:].startswith(b"nope")
    bed = case("first-fail-last-line-alone-in-its-slice")[1]
    assert len(bed) % X.SLICE == 6 and bed.endswith(b"\nchr1 7")
    assert len(case("edge-long-first-token-skip")[1].split()[0]) == 70000


@pytest.mark.parametrize("c", X.CASES + [X.big_case()], ids=lambda c: c[0])
def test_every_input_ends_with_the_status_the_helper_predicts(c):
    out, status, msg = checker(c)
    code, record = X.expected(X.FILES, c[1], c[2], c[3], c[4])
    assert status == {0: 0, X.ASSERT: 134, X.MISSING: 1}[code]
    if code == X.MISSING:
        assert msg == b"Missing sequence: %s\n" % F.bed_lines(c[1])[record].split()[0]


def test_the_error_inputs_cover_both_kinds_and_both_stages():
    got = {X.expected(X.FILES, c[1], c[2], c[3], c[4]) for c in X.ERROR_CASES}
    assert {code for code, _ in got} == {X.ASSERT, X.MISSING}
    assert max(r for _, r in got) >= 2048 and len(X.ERROR_CASES) >= 30

"""The decomposition of the device name sort (tests/name_sort_cases.model) against sorted(), and what every named case is there for."""
import random

import pytest

import name_sort_cases as N

CASES = N.named_cases()


def flags_of(headers, order):
    keys = [N.key_of(h) for h in headers]
    return [1 if k == 0 or keys[order[k]] != keys[order[k - 1]] else 0 for k in range(len(order))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_equals_checker(name):
    headers = CASES[name]
    order, flag, rounds, tied = N.model(headers)
    want = N.check(headers)
    assert order == want[0] and flag == flags_of(headers, want[0]) and sum(flag) == want[2]
    print(name, len(headers), rounds, tied)


def test_model_on_small_random_inputs():
    rnd = random.Random(42)
    for t in range(3000):
        n = rnd.randrange(0, 201)
        alphabet = [b"a", b"b", b"\x80", b"\xff"]
        pool = [b"".join(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 41))) for _ in range(rnd.randrange(1, n + 2))]
        headers = [rnd.choice(pool) for _ in range(n)]
        if t % 3 == 0:  # NUL-cut headers among them
            headers = [h + b"\0tail" if rnd.random() < 0.2 else h for h in headers]
        order, flag, rounds, _ = N.model(headers)
        want = N.check(headers)
        assert order == want[0] and flag == flags_of(headers, want[0]), headers
        assert rounds <= 6 and (rounds > 0) == (n >= 2)


def test_rounds_of_the_named_cases():
    rounds = {name: N.model(CASES[name])[2:] for name in ("edges", "long", "nested", "scaffolds_plain", "scaffolds_spread", "all_equal", "genome")}
    assert rounds["nested"] == (5, 66) and len(CASES["nested"]) == 69
    assert rounds["scaffolds_spread"] == (2, 17994)
    assert rounds["scaffolds_plain"][0] <= 2
    assert rounds["long"][0] <= 2  # two 5 000-byte names cost no more rounds than two short ones
    assert rounds["all_equal"] == (1, 0)
    assert rounds["genome"] == (1, 0)
    assert N.model([])[2:] == (0, 0) and N.model([b"only"])[2:] == (0, 0)


def test_edges_hold_what_they_are_there_for():
    headers = N.edges()
    keys = [N.key_of(h) for h in headers]
    assert 30 <= len(headers) <= 45 and b"" in keys
    for n in N.EDGE_LENGTHS:
        assert sum(1 for k in keys if len(k) == n and k[:-1] == N.SHARED[:n - 1]) == 2
    for short, ext in ((b"ab", b"abc"), (b"pre8byte", b"pre8byteZ"), (b"pre16bytes_key__", b"pre16bytes_key__Z")):
        assert short in keys and ext in keys and ext[:-1] == short
    assert len(b"pre8byte") == 8 and len(b"pre16bytes_key__") == 16
    for dup in (N.DUP8, N.DUP16):  # the key ends at a word boundary: its last word has no zero byte
        at = [r for r, k in enumerate(keys) if k == dup]
        assert len(dup) % 8 == 0 and len(at) == 3 and all(b - a > 1 for a, b in zip(at, at[1:]))
    order, name_of, n_names, name_rec = N.check(headers)
    place = {keys[r]: k for k, r in enumerate(order)}
    assert place[b"hi\x7f"] < place[b"hi\x80"] < place[b"hi\xff"]
    assert place[b"a\tb"] < place[b"a b"]
    # "ab": two whole headers and a NUL-cut one that comes last in the input
    ab = [r for r, k in enumerate(keys) if k == b"ab"]
    assert len(ab) == 3 and headers[ab[-1]] == b"ab\0zz"
    assert name_rec[name_of[ab[0]]] == ab[1]
    assert [order[k] for k in range(len(order)) if keys[order[k]] == b"ab"] == ab  # input order inside a name
    cut = [r for r, k in enumerate(keys) if k == b"cut"]
    assert len(cut) == 2 and name_rec[name_of[cut[0]]] == -1
    assert n_names == len(set(keys))


def test_long_and_random_shapes():
    long_keys = N.long_names()
    assert {len(k) for k in long_keys} == {4999, 5000, 4101}
    a, b = [k for k in long_keys if k[:1] == b"y"]
    assert a[:4096] == b[:4096] and a[4096] != b[4096]
    for n in N.RANDOM_SIZES:
        headers = CASES["random_%d" % n]
        assert len(headers) == n
        if n >= 63:
            letters = set(b"".join(headers))
            assert 0x80 in letters and 0xff in letters and 2 <= len(letters) <= 4
            assert len(set(headers)) < n and max(map(len, headers)) <= 40
    assert N.genome()[0] == b"chr1" and len(N.genome()) == 25

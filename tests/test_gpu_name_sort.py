"""The device name sort (paffy_hip_fasta_name_order, name_sort_kernel.h) against sorted() on the cases of tests/name_sort_cases.py, its
round counts against the CPU model, and the tables it builds through their consumers: the sequence store under add_mismatches against
the host-string path, to_bed -q's name query against a set lookup, faffy extract against tests/faffy_lib.py."""
import ctypes as C

import pytest

import faffy_lib as F
import name_sort_cases as N

pytestmark = pytest.mark.gpu

CASES = N.named_cases()
CONSUMER_CASES = ("edges", "nested", "random_20000")


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected():
    """per case: the checker's tables and the model's rounds, computed once"""
    return {name: (N.check(h), N.model(h)[2:]) for name, h in CASES.items()}


def index(eng, headers, bases=None):
    return eng._files([N.fasta(headers, bases)])


@pytest.mark.parametrize("name", sorted(CASES))
def test_order_names_and_rounds(eng, expected, name):
    headers = CASES[name]
    (order, name_of, n_names, _), (rounds, tied) = expected[name]
    text = index(eng, headers)
    got = eng.fasta_name_order()
    stats = eng.name_sort_stats()
    del text
    print(name, stats)
    assert got[2] == n_names and got[0] == order and got[1] == name_of
    assert stats == {"records": len(headers), "rounds": rounds, "tied_after_first": tied, "names": n_names}


def test_rounds_whatever_the_model_says(eng):
    rounds = {}
    for name in ("long", "scaffolds_plain", "scaffolds_spread", "nested"):
        text = index(eng, CASES[name])
        eng.fasta_name_order()
        rounds[name] = eng.name_sort_stats()["rounds"]
        del text
    assert rounds["long"] <= 2 and rounds["scaffolds_plain"] <= 3 and rounds["scaffolds_spread"] <= 3 and rounds["nested"] >= 3, rounds


def test_empty_and_one_record(eng):
    text = eng._files([b""])
    assert eng.fasta_name_order() == ([], [], 0)
    assert eng.name_sort_stats() == {"records": 0, "rounds": 0, "tied_after_first": 0, "names": 0}
    text = eng._files([b">only one\nACGT\n"])
    assert eng.fasta_name_order() == ([0], [0], 1)
    assert eng.name_sort_stats() == {"records": 1, "rounds": 0, "tied_after_first": 0, "names": 1}
    text = eng._files([b">\nACGT\n>\nA\n"])  # no header byte at all
    assert eng.fasta_name_order() == ([0, 1], [0, 0], 1)
    del text


def test_a_second_index_gets_its_own_tables(eng):
    first, second = [b"b", b"a", b"c", b"a"], [b"z", b"y", b"x"]
    text = index(eng, first)
    assert eng.fasta_name_order() == ([1, 3, 0, 2], [1, 0, 2, 0], 3)
    assert eng.fasta_name_order() == ([1, 3, 0, 2], [1, 0, 2, 0], 3)  # the table is built once per index
    text = index(eng, second)
    assert eng.fasta_name_order() == ([2, 1, 0], [2, 1, 0], 3)
    got = eng.faffy_extract([N.fasta(second, [b"ACGTACGTACGT"] * 3)], b"y\t2\t9\n", flank=0, min_size=1)
    assert got == b">y|12|2\nGTACGTA\n"
    del text


def test_capacity_and_state():
    import paffy_amd
    from paffy_amd import engine as E

    e = paffy_amd.Engine()
    n = C.c_int64()
    assert E.lib().paffy_hip_fasta_name_order(e._ctx, 0, None, None, C.byref(n)) == -5  # PAFFY_E_STATE: no index
    text = e._files([N.fasta([b"b", b"a"])])
    assert E.lib().paffy_hip_fasta_name_order(e._ctx, 1, None, None, C.byref(n)) == -4  # PAFFY_E_CAPACITY: cap < records
    assert E.lib().paffy_hip_fasta_name_order(e._ctx, 2, None, None, C.byref(n)) == 0 and n.value == 2  # either pointer may be NULL
    del text
    e.close()


# ---- through the consumers ----

def paf_naming(headers, bases):
    """one line per key that a PAF field can hold, query and target, each inside the shortest record of its name; then a missing name"""
    keys = []
    for h in headers:
        k = N.key_of(h)
        if k and b"\t" not in k and k not in keys:
            keys.append(k)
    length = len(bases[0])
    lines = []
    for i, q in enumerate(keys):
        t = keys[(i * 7 + 3) % len(keys)]
        lines.append(b"%s\t%d\t0\t%d\t%c\t%s\t%d\t0\t%d\t%d\t%d\t60\tcg:Z:%dM\n" % (q, length, length, b"+-"[i & 1], t, length, length, length, length, length))
    return b"".join(lines), b"no such name\t5\t0\t5\t+\t%s\t%d\t0\t5\t5\t5\t60\tcg:Z:5M\n" % (keys[0], length)


@pytest.fixture(scope="module")
def key_sets():
    return {name: {N.key_of(h) for h in CASES[name]} for name in CONSUMER_CASES}


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_store_equals_host_string_path(name):
    import paffy_amd
    from paffy_amd import engine as E

    headers = CASES[name]
    bases = N.distinct_bases(len(headers))
    good, missing = paf_naming(headers, bases)
    outs = []
    for device in (True, False):
        e = paffy_amd.Engine()
        if device:
            assert e.set_sequences_fasta([N.fasta(headers, bases)]) == len(headers)
            assert e.name_sort_stats()["records"] == len(headers)
        else:
            names = (C.c_char_p * len(headers))(*[N.key_of(h) for h in headers])
            seqs = (C.c_char_p * len(headers))(*bases)
            lens = (C.c_int64 * len(headers))(*[len(b) for b in bases])
            e._check(E.lib().paffy_hip_set_sequences(e._ctx, len(headers), names, seqs, lens), "paffy_hip_set_sequences")
        for paf in (good, good[:len(good) // 2] + missing + good[len(good) // 2:]):
            out, info = e.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], paf, raise_on_error=False)
            outs.append((device, out, info.error.code, info.error.record))
        e.close()
    dev, host = [o[1:] for o in outs if o[0]], [o[1:] for o in outs if not o[0]]
    assert dev == host
    assert dev[0][1] == 0 and b"X" in dev[0][0] and b"=" in dev[0][0]
    assert dev[1][1] != 0 and dev[1][2] == good[:len(good) // 2].count(b"\n")


@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_fasta_seen_equals_a_set_lookup(eng, key_sets, name, with_target):
    headers = CASES[name]
    keys = sorted(k for k in key_sets[name] if b"\t" not in k)
    named_q, named_t = set(keys[0::3]), set(keys[1::3])
    lines = [b"%s\t9\t0\t1\t+\tnobody\t9\t0\t1\t1\t1\t60\n" % q for q in sorted(named_q)]
    lines += [b"not here\t9\t0\t1\t+\t%s\t9\t0\t1\t1\t1\t60\n" % t for t in sorted(named_t)]
    got = eng.fasta_seen([N.fasta(headers)], b"".join(lines), with_target=with_target)
    named = named_q | named_t if with_target else named_q
    assert [(k, s) for k, _, s in got] == [(N.key_of(h), N.key_of(h) in named) for h in headers]
    assert eng.name_sort_stats()["names"] == len(key_sets[name])


@pytest.mark.parametrize("name", CONSUMER_CASES)
def test_faffy_extract_equals_the_checker(eng, key_sets, name):
    headers = CASES[name]
    bases = N.distinct_bases(len(headers))
    files = [N.fasta(headers, bases)]
    tokens = sorted(k for k in key_sets[name] if k and not set(k) & set(b" \t\r\x0b\x0c"))
    assert (b"cut" in tokens) == (name == "edges")  # the name that only NUL-cut headers bear: no record is meant by it
    bed = b"".join(b"%s\t%d\t%d\n" % (t, 1 + i % 3, 8 + i % 4) for i, t in enumerate(tokens)) + b"missing_name\t1\t9\n"
    want, status, _ = F.extract(files, bed, flank=1, min_size=1, skip_missing=True)
    assert status == 0 and want.count(b">") >= len(tokens) - 1
    assert eng.faffy_extract(files, bed, flank=1, min_size=1, skip_missing=True) == want
    want, status, msg = F.extract(files, bed, flank=1, min_size=1)
    assert status == 1
    with pytest.raises(Exception):
        eng.faffy_extract(files, bed, flank=1, min_size=1)

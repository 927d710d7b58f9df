"""The device FASTA loaders (paffy_hip_set_sequences_fasta, paffy_hip_set_intervals_fasta, paffy_hip_fasta_seen) against the host-string
calls on the records tests/faffy_lib.fasta_read makes of the same files, and against the oracle."""
import ctypes as C

import pytest

import chunk_lib as K
import faffy_lib as F
import fasta_corpus as FC
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import paffy_amd.engine as E

    return E


def engine():
    import paffy_amd

    return paffy_amd.Engine()


def set_host(E, eng, recs):
    """paffy_hip_set_sequences on the records as the host held them (duplicate names kept, names up to a NUL byte)"""
    names = [h.split(b"\0", 1)[0] for h, _ in recs]
    vals = [s for _, s in recs]
    n = len(recs)
    a = (C.c_char_p * max(1, n))(*names)
    b = (C.c_char_p * max(1, n))(*vals)
    ln = (C.c_int64 * max(1, n))(*[len(v) for v in vals])
    eng._check(E.lib().paffy_hip_set_sequences(eng._ctx, n, a, b, ln), "paffy_hip_set_sequences")


def add_mismatches_both(E, files, paf, keep_raw=False):
    import paffy_amd

    outs = []
    for device in (True, False):
        eng = engine()
        if keep_raw:
            eng.keep_raw_sequences(True)
        if device:
            assert eng.set_sequences_fasta(files) == len(FC.records(files))
        else:
            set_host(E, eng, FC.records(files))
        out, info = eng.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], paf, raise_on_error=False)
        outs.append((out, info.error.code, info.error.record))
        eng.close()
    return outs


@pytest.mark.parametrize("keep_raw", [False, True])
def test_adversarial_store_equals_host_path(E, keep_raw):
    files = FC.adversarial()
    paf = FC.paf(files, 3000)
    dev, host = add_mismatches_both(E, files, paf, keep_raw)
    assert dev == host and dev[1] == 0
    assert b"=" in dev[0] and b"X" in dev[0]
    # the oracle on the records whose names are unique (which duplicate wins is not pinned)
    recs = FC.records(files)
    names = [h for h, _ in recs]
    uniq = {h: s for h, s in recs if names.count(h) == 1}
    lines = [ln + b"\n" for ln in paf.splitlines() if ln.split(b"\t")[0] in uniq and ln.split(b"\t")[5] in uniq]
    sub = b"".join(lines)
    want, werr = O.run([O.stage(O.ADD_MISMATCHES)], sub, uniq)
    eng = engine()
    eng.set_sequences_fasta(files)
    import paffy_amd

    got, info = eng.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], sub)
    eng.close()
    assert werr.code == 0 and got == want and len(lines) > 100


def test_paths_and_clean_layout(E, tmp_path):
    """paths load as bytes do; the adversarial files give the store their clean rewrite gives"""
    files = FC.adversarial(5)
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / ("f%d.fa" % k)
        p.write_bytes(f)
        paths.append(str(p))
    paf = FC.paf(files, 1500, seed=9)
    import paffy_amd

    outs = []
    for src in (files, paths, FC.clean(files)):
        eng = engine()
        eng.set_sequences_fasta(src)
        outs.append(eng.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], paf)[0])
        eng.close()
    assert outs[0] == outs[1] == outs[2]


def test_missing_sequence_same_error(E):
    files = FC.adversarial()
    paf = FC.paf(files, 50) + b"nosuch\t10\t0\t5\t+\tlen16\t16\t0\t5\t5\t5\t60\tcg:Z:5M\n" + FC.paf(files, 20, seed=4)
    dev, host = add_mismatches_both(E, files, paf)
    assert dev == host and dev[1] != 0 and dev[2] == 50


def test_scaffolds(E):
    files = FC.scaffolds()
    paf = FC.paf(files, 20000, seed=11)
    dev, host = add_mismatches_both(E, files, paf)
    assert dev == host and dev[1] == 0


def test_empty_and_headerless():
    import paffy_amd

    eng = engine()
    assert eng.set_sequences_fasta([]) == 0
    assert eng.set_sequences_fasta([b"", b"ACGT\nno header\n"]) == 0
    assert eng.set_sequences_fasta([b">a\nAC\n"]) == 1
    got = eng.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], b"a\t2\t0\t2\t+\ta\t2\t0\t2\t2\t2\t60\tcg:Z:2M\n")[0]
    assert got.endswith(b"cg:Z:2=\n")
    eng.close()


# ---- intervals (upconvert) ----

IV_FILES = [b">chrB|50000|20000\n" + b"A" * 5000 + b"\n>chrA|100000|0\r\n" + b"C" * 600 + b"\n" + b"G" * 400 + b"\n>chrA|100000|2000\n" + b"T" * 1000
            + b"\n>chrA|100000|1000\n" + b"a c\tg" * 250 + b"\n",
            b"junk\n>chrB|50000|10000\n" + b"N" * 10000 + b"\n>chrA|100000|40000\n" + b"A" * 30000 + b"\n>chrA|100000|3000\n" + b"A" * 500
            + b"\n>x|y|70|0x10\n" + b"A" * 20]


def iv_records(files):
    return [(h, len(s)) for h, s in F.fasta_read_files(files)]


def run_iv(eng, data, files=None, fasta=None):
    import paffy_amd

    if files is not None:
        assert eng.set_intervals_fasta(files) == len(iv_records(files))
    else:
        eng.set_intervals([h for h, _ in fasta], [n for _, n in fasta])
    out, info = eng.run([paffy_amd.stage(paffy_amd.UPCONVERT)], data, raise_on_error=False)
    return out, info.error.code, info.error.record


def upconvert_records(n, seed):
    import random

    rnd = random.Random(seed)
    fasta = iv_records(IV_FILES)
    out = []
    while len(out) < n:
        side = []
        for _ in range(2):
            nm, ln = rnd.choice([(b"chrA", 100000), (b"chrB", 50000), (b"chrD", 7000)])
            s = rnd.choice([0, 1000, 2000, 3000, 20000, rnd.randrange(0, ln - 1)]) if nm != b"chrD" else rnd.randrange(0, ln - 1)
            side.append((nm, ln, s, min(ln, s + rnd.choice([0, 1, 5]))))
        (qn, ql, qs, qe), (tn, tl, ts, te) = side
        line = b"%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t5\t9\t60\ttp:A:P\n" % (qn, ql, qs, qe, tn, tl, ts, te)
        if line not in out and K.upconvert(line, fasta)[1] is None:  # valid records (the failing ones have tests of their own)
            out.append(line)
    return b"".join(out)


def test_intervals_equal_host_and_checker():
    data = upconvert_records(400, 1)
    fasta = iv_records(IV_FILES)
    want, fail = K.upconvert(data, fasta)
    assert fail is None and b"chrA|100000|1000\t" in want
    eng = engine()
    got = run_iv(eng, data, files=IV_FILES)
    host = run_iv(eng, data, fasta=fasta)
    bad = data + b"chrA\t100000\t1500\t2600\t+\tchrB\t50000\t100\t200\t5\t9\t60\n"  # starts in [1000, 2000], ends beyond it
    got_bad, host_bad = run_iv(eng, bad, files=IV_FILES), run_iv(eng, bad, fasta=fasta)
    eng.close()
    assert got == host and got[0] == want and got[1] == 0
    assert got_bad == host_bad and (got_bad[1], got_bad[2]) == K.upconvert(bad, fasta)[1]


def test_intervals_equal_keys():
    """two intervals with the same (name, start): the qsort order of the same array decides, as on the host path"""
    files = [b">c|1000|100\n" + b"A" * 50 + b"\n>c|1000|100\n" + b"A" * 80 + b"\n>c|1000|0\n" + b"A" * 100 + b"\n"]
    data = b"".join(b"c\t1000\t%d\t%d\t+\tc\t1000\t%d\t%d\t5\t9\t60\n" % (s, s + 10, t, t + 20) for s, t in ((100, 0), (120, 130), (140, 99), (0, 150)))
    eng = engine()
    got = run_iv(eng, data, files=files)
    host = run_iv(eng, data, fasta=iv_records(files))
    eng.close()
    assert got == host


def test_intervals_bad_header():
    eng = engine()
    with pytest.raises(RuntimeError, match="header"):
        eng.set_intervals_fasta([b">good|10|0\nAAAA\n>not a chunk header\nAC\n"])
    eng.close()


def test_module_upconvert_fasta_files():
    import paffy_amd

    data = upconvert_records(50, 2)
    fasta = iv_records(IV_FILES)
    want, fail = K.upconvert(data, fasta)
    assert fail is None and paffy_amd.upconvert(data, fasta_files=IV_FILES) == want


# ---- to_bed -q names ----

def test_fasta_seen():
    files = [b">q1\nAC\n>t1\nA\n>q1\nG\n>x y\nAAA\n>nope\n\n>\nA\n", b">t2\r\nACGT"]
    paf = (b"q1\t2\t0\t1\t+\tt1\t1\t0\t1\t1\t1\t60\n"
           b"x y\t3\t0\t1\t+\tt2\t4\t0\t1\t1\t1\t60"  # the last line has no newline
           )
    eng = engine()
    got = eng.fasta_seen(files, paf)
    assert got == [(b"q1", 2, True), (b"t1", 1, False), (b"q1", 1, True), (b"x y", 3, True), (b"nope", 0, False), (b"", 1, False), (b"t2", 4, False)]
    got = eng.fasta_seen(files, paf, with_target=True)
    assert [s for _, _, s in got] == [True, True, True, True, False, False, True]
    # a line of one field, a tab-led line (names the empty header), no target column
    got = eng.fasta_seen(files, b"nope\n\tx\n", with_target=True)
    assert [s for _, _, s in got] == [False, False, False, False, False, True, False]
    eng.close()

"""`faffy chunk | extract | merge` on the GPU (engine and bin/faffy) against the checker (tests/faffy_lib.py), the reference's own
chunk-and-merge and extract tests (tests/fasta_chunk_and_merge_test.c, tests/fasta_extract_test.c) restated, exit statuses, and the
hand-offs to `paffy dechunk` and `paffy upconvert`."""
import os
import random
import subprocess

import pytest

import chunk_lib as K
import faffy_lib as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAFFY = os.path.join(ROOT, "bin", "faffy")
PAFFY = os.path.join(ROOT, "bin", "paffy")


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


_BASES = bytes(b"ACGTacgt"[i % 8] for i in range(256))


def genome(seed, n_rec, max_len, width=60, names=None, min_len=0):
    """FASTA text and its records: mixed case, N runs, names with '|' and spaces"""
    rnd = random.Random(seed)
    recs, out = [], bytearray()
    for k in range(n_rec):
        name = names[k] if names else (b"chr%d|part %d" % (k, rnd.randrange(9)) if k % 3 == 0 else b"seq%d" % k)
        n = rnd.randrange(min_len, max_len + 1)
        s = bytearray(rnd.randbytes(n).translate(_BASES))
        for _ in range(n // 5000 + (n > 50)):
            a, r = rnd.randrange(n - 40), rnd.randrange(1, 40)
            s[a:a + r] = b"N" * r
        s = bytes(s)
        recs.append((name, s))
        out += b">" + name + b"\n" + b"".join(s[i:i + width] + b"\n" for i in range(0, n, width))
    return bytes(out), recs


def faffy(args, stdin=b"", cwd=None):
    p = subprocess.run([FAFFY] + args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=cwd)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("c,o", [(1000, 100), (777, 0), (50, 49), (5000, 1000), (1, 0), (3, -2), (100000, 10)])
def test_chunk_engine(eng, c, o):
    a, _ = genome(1, 30, 4000)
    b, _ = genome(2, 5, 20000, width=77)
    want, st = F.chunk([a, b], c, o, d="out")
    assert st == 0
    assert eng.faffy_chunk([a, b], c, o, d="out") == want


@pytest.mark.parametrize("f,m", [(10, 100), (0, 0), (25, 5), (1000, 1)])
def test_extract_engine(eng, f, m):
    a, recs = genome(3, 12, 5000)
    rnd = random.Random(f * 7 + m)
    lines = []
    for _ in range(400):
        name, s = rnd.choice(recs)
        if not s:
            continue
        st = rnd.randrange(len(s))
        en = rnd.randrange(st, len(s) + 1)
        lines.append(b"%s\t%d\t%d\textra\n" % (name.split(b" ")[0] if b" " in name else name, st, en))
    bed = b"".join(lines)
    want, status, _ = F.extract([a], bed, f, m, skip_missing=True)
    assert status == 0
    assert eng.faffy_extract([a], bed, f, m, skip_missing=True) == want


def test_merge_engine(eng):
    a, recs = genome(4, 20, 9000)
    chunks, _ = F.chunk([a], 1000, 100)
    files = [b for _, b in chunks]
    want, st = F.merge(files)
    assert st == 0 and eng.faffy_merge(files) == want
    # merge gives the records back, names without their last two '|'-tokens ("chr0|part 3" keeps its own '|')
    back = F.fasta_read(want)
    assert back == [(n, s) for n, s in recs if s]


def test_cli_chunk_and_merge_20mb(tmp_path):
    """tests/fasta_chunk_and_merge_test.c: a seeded 20 Mb FASTA through `faffy chunk -c 1000000 -o 10000`, then `faffy merge -i`"""
    text, recs = genome(5, 7, 6_000_000)
    fa = tmp_path / "in.fa"
    fa.write_bytes(text)
    d = tmp_path / "chunks"
    rc, out, err = faffy(["chunk", str(fa), "-c", "1000000", "-o", "10000", "-d", str(d)])
    assert rc == 0, err
    want, _ = F.chunk([text], 1000000, 10000, d=str(d))
    assert out == b"".join(p.encode() + b"\n" for p, _ in want)
    for p, b in want:
        assert open(p, "rb").read() == b
    lst = tmp_path / "list.txt"
    lst.write_bytes(out)
    rc, merged, err = faffy(["merge", "-i", str(lst)])
    assert rc == 0, err
    assert F.fasta_read(merged) == [(n, s) for n, s in recs if s]
    rc, merged2, _ = faffy(["merge", "-o", str(tmp_path / "m.fa")], stdin=out)
    assert rc == 0 and (tmp_path / "m.fa").read_bytes() == merged


def test_cli_extract(tmp_path):
    text, recs = genome(6, 9, 3000)
    fa = tmp_path / "g.fa"
    fa.write_bytes(text)
    bed = b"".join(b"%s %d %d\n" % (n, 10 * k, 10 * k + 150) for k, (n, s) in enumerate(recs) if len(s) > 10 * k + 150 and b" " not in n)
    (tmp_path / "x.bed").write_bytes(bed)
    rc, out, err = faffy(["extract", str(fa), "-i", str(tmp_path / "x.bed"), "-f", "7", "-m", "20"])
    assert rc == 0, err
    assert out == F.extract([text], bed, 7, 20)[0]
    rc, out2, _ = faffy(["extract", str(fa), "-o", str(tmp_path / "o.fa")], stdin=bed)
    assert rc == 0 and (tmp_path / "o.fa").read_bytes() == F.extract([text], bed)[0]


def test_extract_property_200_trials(eng):
    """tests/fasta_extract_test.c: every base of every interval (with flanks, at least min_size long) is written exactly once, from the
    right place of its sequence"""
    rnd = random.Random(2024)
    for trial in range(200):
        seqs = {b"%d" % i: bytes(rnd.choice(b"ACGT") for _ in range(rnd.randrange(0, 1001))) for i in range(rnd.randrange(1, 11))}
        text = b"".join(F.write_record(k, v) for k, v in seqs.items())
        flank, min_size = rnd.randrange(0, 11), rnd.randrange(0, 11)
        marked = {k: bytearray(v) for k, v in seqs.items()}
        lines, total = [], 0
        for _ in range(rnd.randrange(0, 101)):
            name = b"%d" % rnd.randrange(0, len(seqs))
            s = seqs[name]
            if not s:
                continue
            st = rnd.randrange(0, len(s))
            en = rnd.randrange(st, len(s) + 1)
            lines.append(b"%s %d %d\n" % (name, st, en))
            if en - st >= min_size:
                for j in range(max(0, st - flank), min(len(s), en + flank)):
                    if marked[name][j] != ord("X"):
                        total += 1
                        marked[name][j] = ord("X")
        out = eng.faffy_extract([text], b"".join(lines), flank, min_size)
        seen = {k: bytearray(v) for k, v in seqs.items()}
        n_out = 0
        for hdr, sub in F.fasta_read(out):
            toks = hdr.split(b"|")
            name, start = toks[0], int(toks[2])
            for i, c in enumerate(sub):
                assert c == seen[name][i + start], f"trial {trial}"
                seen[name][i + start] = ord("X")
            n_out += len(sub)
        assert n_out == total, f"trial {trial}"


def test_exit_statuses(eng, tmp_path):
    import paffy_amd

    bad = b">a\nACGTU\n"
    with pytest.raises(paffy_amd.PafError) as e:
        eng.faffy_chunk([bad], 10, 1)
    assert e.value.exit_status == 134
    with pytest.raises(paffy_amd.PafError) as e:
        eng.faffy_extract([bad], b"a 0 5\n", 0, 1)
    assert e.value.exit_status == 134
    assert eng.faffy_extract([bad], b"a 0 4\n", 0, 1) == b">a|5|0\nACGT\n"  # only the written bases are checked
    with pytest.raises(paffy_amd.PafError) as e:
        eng.faffy_extract([bad], b"a 0 4\nb 0 1\n", 0, 1)
    assert e.value.exit_status == 1
    assert eng.faffy_extract([bad], b"b 0 1\na 0 4\n", 0, 1, skip_missing=True) == b">a|5|0\nACGT\n"
    for files in ([b">s|10|4\nAC\n"], [b">s|10|0\nAC\n>s|10|5\nAC\n"], [b">0\nAC\n"]):
        with pytest.raises(paffy_amd.PafError) as e:
            eng.faffy_merge(files)
        assert e.value.exit_status == 134
    assert eng.faffy_merge([b">U|3|0\nUUU\n"]) == b">U\nUUU\n"  # merge checks no bases
    with pytest.raises(paffy_amd.PafError) as e:
        eng.faffy_chunk([b">a\n\n"], 5, 5)  # c <= o: the assert fires at the first record, empty or not
    assert e.value.exit_status == 134
    # the CLI ends the same way, and writes nothing
    fa = tmp_path / "bad.fa"
    fa.write_bytes(bad)
    rc, out, _ = faffy(["chunk", str(fa), "-d", str(tmp_path / "d1")])
    assert rc in (134, -6) and out == b""
    (tmp_path / "b.bed").write_bytes(b"a 0 4\nnope 1 2\n")
    rc, out, err = faffy(["extract", str(fa), "-i", str(tmp_path / "b.bed"), "-o", str(tmp_path / "o.fa"), "-m", "1"])
    assert rc == 1 and err.endswith(b"Missing sequence: nope\n") and (tmp_path / "o.fa").read_bytes() == b""
    rc, out, _ = faffy(["extract", str(fa), "-n", "-i", str(tmp_path / "b.bed"), "-m", "1", "-f", "0"])
    assert rc == 0 and out == b">a|5|0\nACGT\n"
    (tmp_path / "c.fa").write_bytes(b">s|10|0\nAC\n>s|10|5\nAC\n")
    rc, _, _ = faffy(["merge"], stdin=str(tmp_path / "c.fa").encode())
    assert rc in (134, -6)
    rc, _, _ = faffy(["chunk", str(fa), "-c", "4", "-o", "4", "-d", str(tmp_path / "d2")])
    assert rc in (134, -6)


def paf(qn, ql, qs, qe, tn, tl, ts, te):
    return b"%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t5\t9\t60\ttp:A:P\tcg:Z:%dM\n" % (qn, ql, qs, qe, tn, tl, ts, te, qe - qs)


def test_chunk_headers_through_paffy_dechunk(eng, tmp_path):
    """records whose sides lie inside one chunk, renamed with the headers of faffy chunk's files, come back through paffy dechunk"""
    a, recs = genome(8, 6, 30000, names=[b"q%d" % k for k in range(6)])
    chunks = eng.faffy_chunk([a], 5000, 500)
    pieces = [(h, s) for _, b in chunks for h, s in F.fasta_read(b)]
    rnd = random.Random(9)
    orig, renamed = [], []
    for _ in range(300):
        (qh, qs_), (th, ts_) = rnd.choice(pieces), rnd.choice(pieces)
        if not qs_ or not ts_:
            continue
        qn, ql, qc = qh.rsplit(b"|", 2)
        tn, tl, tc = th.rsplit(b"|", 2)
        qa, ta = rnd.randrange(len(qs_)), rnd.randrange(len(ts_))
        n = min(rnd.randrange(1, 200), len(qs_) - qa, len(ts_) - ta)
        qc, tc, ql, tl = int(qc), int(tc), int(ql), int(tl)
        orig.append(paf(qn, ql, qc + qa, qc + qa + n, tn, tl, tc + ta, tc + ta + n))
        renamed.append(paf(qh, len(qs_), qa, qa + n, th, len(ts_), ta, ta + n))
    data = b"".join(renamed)
    p = subprocess.run([PAFFY, "dechunk"], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    want, fail = K.dechunk(data)
    assert fail is None and p.stdout == want
    assert [ln.split(b"\t")[:9] for ln in p.stdout.split(b"\n")[:-1]] == [ln.split(b"\t")[:9] for ln in b"".join(orig).split(b"\n")[:-1]]


def test_extract_output_through_paffy_upconvert(eng, tmp_path):
    a, recs = genome(10, 5, 20000, names=[b"t%d" % k for k in range(5)], min_len=18001)
    rnd = random.Random(12)
    bed = b"".join(b"t%d %d %d\n" % (k, s, s + rnd.randrange(100, 3000)) for k in range(5) for s in sorted(rnd.sample(range(0, 15000), 4))
                   if len(recs[k][1]) > 18000)
    ext = eng.faffy_extract([a], bed, 20, 50)
    fa = tmp_path / "ext.fa"
    fa.write_bytes(ext)
    subs = F.fasta_read(ext)
    lines, keys = [], set()
    for _ in range(200):
        h, s = rnd.choice(subs)
        name, ln, st = h.rsplit(b"|", 2)
        qa, ts = int(st) + rnd.randrange(len(s) - 50), rnd.randrange(10**6 - 100)
        if (name, qa, ts) in keys:  # no two records with one key (the checker's writer is dedupe's)
            continue
        keys.add((name, qa, ts))
        lines.append(paf(name, int(ln), qa, qa + 40, b"other", 10**6, ts, ts + 40))
    data = b"".join(lines)
    p = subprocess.run([PAFFY, "upconvert", str(fa)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    want, fail = K.upconvert(data, [(h, len(s)) for h, s in subs])
    assert fail is None and p.stdout == want

"""`bin/paffy view` through the pipelined stream in view mode, in the three situations where the order of events is the behaviour:
a failing record in the third chunk, a line that does not parse behind a record that fails a stage in the same chunk, and rows that
reach outside a sequence in the second chunk. Input above 2 MiB (lines padded with a tag of 110 KB, as in
tests/test_gpu_alignment_rows.py), read in one chunk (PAFFY_CHUNK_MB unset) and in chunks of 1 MiB; -s, -a -s and -s -t. The expected
bytes are the oracle's text of the chunks in front of the failing one (a chunk with a failing record writes nothing; a chunk is the longest
run of whole lines within PAFFY_CHUNK_MB), the expected stderr and status those of the oracle's error."""
import os
import subprocess

import pytest

import oracle_lib as O
from test_gpu_alignment_rows import sequences
from test_gpu_flat import cigar_of, record
from test_gpu_view_text import oracle_text, row_lines, total_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
ERR_MISSING_QUERY, ERR_SEQ_RANGE = 17, 21
PAD = b"\tzz:Z:" + b"p" * 110_000
FLAGS = [("-s",), ("-a", "-s"), ("-s", "-t")]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def padded(ln):
    at = ln.find(b"\tcg:Z:")
    return ln[:at] + PAD + ln[at:] if at >= 0 else ln[:-1] + PAD + b"\n"


def chunks_of(lines, cap):
    """the chunks the CLI reads: whole lines, as many as fit cap bytes -> [(first, end)]"""
    out, first = [], 0
    while first < len(lines):
        end, held = first, 0
        while end < len(lines) and held + len(lines[end]) <= cap:
            held += len(lines[end])
            end += 1
        assert end > first
        out.append((first, end))
        first = end
    return out


def message(code, record, aux):
    if code == O.ERR_STRAND:
        return b"Got an unexpected strand character (%c) in a paf string\n" % aux
    if code == ERR_MISSING_QUERY:
        return b"No query sequence found for record %d\n" % record
    assert code == ERR_SEQ_RANGE
    return b"alignment reaches outside a sequence (record %d)\n" % record


_CASE = {}


def case():
    """25 padded records (2.8 MB) on the sequences of test_gpu_alignment_rows.py and three spoilers of the same length"""
    if not _CASE:
        seqs = sequences()
        lines = [padded(ln) for ln in (row_lines() * 2)[:25]]  # with one or two spoilers: three chunks of 1 MiB, nine lines each at most
        assert len(b"".join(lines)) > 2 << 20 and len(chunks_of(lines, 1 << 20)) == 3
        kw = dict(qlen=len(seqs["qb"]), tlen=len(seqs["tb"]), qs=12_000, ts=13_000)
        lost = padded(record([(20, "M")], "+", qname="nobody", tname="tb", **kw).encode())
        torn = padded(b"qb\t30000\t5\t9\tx\ttb\t30000\t5\t9\t4\t4\t60\ttp:A:P\n")  # no such strand
        # = and I ops alone, the query range 52 bases past the 30 000 loaded (the line says 40 000): the plan passes, the rows do not
        far = padded(record([(50, "="), (2, "I"), (50, "=")], "-", qname="qb", tname="tb", qlen=40_000, tlen=len(seqs["tb"]), qs=29_950, ts=14_000).encode())
        _CASE["c"] = (seqs, lines, lost, torn, far)
    return _CASE["c"]


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    fa = tmp_path_factory.mktemp("fa") / "g.fa"
    with open(fa, "wb") as fh:
        for name, s in sequences().items():
            fh.write(b">" + name.encode() + b"\n" + s + b"\n")
    return str(fa)


def text_of(lines, flags):
    """the oracle's per-record text of lines that all pass"""
    if "-t" in flags or not lines:
        return b""
    seqs = sequences()
    enc, err = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines), seqs)
    assert err.code == 0
    return b"".join(oracle_text(enc.splitlines(keepends=True), seqs, "-a" in flags))


def view(paf, fa, flags, chunk_mb):
    env = dict(os.environ)
    env.pop("PAFFY_CHUNK_MB", None)
    env.pop("PAFFY_GPUS", None)
    if chunk_mb:
        env["PAFFY_CHUNK_MB"] = str(chunk_mb)
    r = subprocess.run([PAFFY, "view", *flags, "-i", paf, fa], capture_output=True, env=env, timeout=120)
    return r.returncode, r.stdout, r.stderr


def returncode_of(code):
    status = O.lib().po_error_exit_status(code) if code != ERR_SEQ_RANGE else 139  # the reference reads outside the string there
    return {134: -6, 139: -11}.get(status, status or 1)


def check(tmp_path, fasta, lines, flags, expect):
    """expect(chunks) -> (the index of the failing chunk, code, record, aux, the text of that chunk that is written all the same)"""
    paf = tmp_path / "in.paf"
    paf.write_bytes(b"".join(lines))
    for chunk_mb in (None, 1):
        chunks = chunks_of(lines, (chunk_mb or 64) << 20)  # view reads chunks of 64 MiB unless told otherwise
        assert len(chunks) == (3 if chunk_mb else 1)
        k, code, rec, aux, tail = expect(chunks)
        want = text_of(lines[:chunks[k][0]], flags) + tail
        status, out, err = view(str(paf), fasta, flags, chunk_mb)
        assert (status, err) == (returncode_of(code), message(code, rec, aux)), (flags, chunk_mb, status, err[-300:])
        assert out == want, (flags, chunk_mb, len(out), len(want))


@pytest.mark.parametrize("flags", FLAGS, ids=["s", "a_s", "s_t"])
def test_a_failing_record_in_the_third_chunk(tmp_path, fasta, flags):
    seqs, lines, lost, torn, far = case()
    at = 22
    lines = lines[:at] + [lost] + lines[at:]
    assert [a <= at < b for a, b in chunks_of(lines, 1 << 20)] == [False, False, True]
    _, err = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines), seqs)
    assert (err.code, err.record) == (ERR_MISSING_QUERY, at)

    def expect(chunks):
        k = [i for i, (a, b) in enumerate(chunks) if a <= at < b][0]
        return k, err.code, err.record, err.aux, b""

    check(tmp_path, fasta, lines, flags, expect)


@pytest.mark.parametrize("flags", FLAGS, ids=["s", "a_s", "s_t"])
def test_a_line_that_does_not_parse_behind_a_stage_failure_in_one_chunk(tmp_path, fasta, flags):
    """with per-record text the lines' fields are read before the stages run, so the line that does not parse speaks; under -t only the
    stages' first failing record is known"""
    seqs, lines, lost, torn, far = case()
    lines = lines[:10] + [lost] + lines[10:12] + [torn] + lines[12:]
    assert [(a <= 10 < b, a <= 13 < b) for a, b in chunks_of(lines, 1 << 20)] == [(False, False), (True, True), (False, False)]
    _, staged = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines), seqs)
    _, parsed = O.run([O.stage(O.PASS)], b"".join(lines))
    assert (staged.code, staged.record) == (ERR_MISSING_QUERY, 10) and (parsed.code, parsed.record, parsed.aux) == (O.ERR_STRAND, 13, ord("x"))
    err = staged if "-t" in flags else parsed

    def expect(chunks):
        k = [i for i, (a, b) in enumerate(chunks) if a <= 10 < b][0]
        return k, err.code, err.record, err.aux, b""

    check(tmp_path, fasta, lines, flags, expect)


@pytest.mark.parametrize("flags", FLAGS, ids=["s", "a_s", "s_t"])
def test_a_rows_failure_in_the_second_chunk(tmp_path, fasta, flags):
    seqs, lines, lost, torn, far = case()
    at = 12
    lines = lines[:at] + [far] + lines[at:]
    assert [a <= at < b for a, b in chunks_of(lines, 1 << 20)] == [False, True, False]
    enc, err = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines), seqs)
    assert err.code == 0  # the encoder looks at no base of the record
    if "-a" not in flags or "-t" in flags:  # no rows are written: nothing fails
        paf = tmp_path / "in.paf"
        paf.write_bytes(b"".join(lines))
        tot = [0] * 6
        for ln in enc.splitlines(keepends=True):
            if b"cg:Z:" in ln:
                tot = O.cigar_stats(cigar_of(ln).decode(), tot, zero=False)
        want = (b"" if "-t" in flags else b"".join(oracle_text(enc.splitlines(keepends=True)))) + total_line(len(lines), tot)
        for chunk_mb in (None, 1):
            assert view(str(paf), fasta, flags, chunk_mb) == (0, want, b""), chunk_mb
        return

    def expect(chunks):  # every block of the chunk in front of the record, and the record's stats line
        k = [i for i, (a, b) in enumerate(chunks) if a <= at < b][0]
        return k, ERR_SEQ_RANGE, at, 0, text_of(lines[chunks[k][0]:at], flags) + oracle_text([far])[0]

    check(tmp_path, fasta, lines, flags, expect)

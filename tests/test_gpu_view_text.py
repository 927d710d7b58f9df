"""What `paffy view` writes per record, written on the GPU into device memory (k_view_line_size / k_view_line_emit,
paffy_amd/csrc/view_line_kernel.h, in front of the rows of pretty_kernel.h) and fetched through the C-ABI (paffy_hip_plan_view_sizes /
_view_text: Engine.view_sizes / view_text), against the oracle's paf_pretty_print of the same lines byte for byte. Every fetch lies
between guard bytes that Engine.view_text asserts are untouched. The batches are the smallest that reach each mechanism: every value of
the two %f fields at which glibc's rounding decides (exact ties, the carry into the integer digit, the NaN of an empty record), every
decimal width of the integers, names round the 16 bytes a lane copies, every residue mod 16 of where a name is read and where a line is
written. The same batches go through `bin/paffy view` in test_gpu_view_cli_text.py."""
import random
import re

import pytest

import oracle_lib as O
import synth_lib
from test_gpu_alignment_rows import place, sequences
from test_gpu_flat import cigar_of, record  # noqa: F401 -- cigar_of: for the sums of the encoded lines

pytestmark = pytest.mark.gpu

STATS = 10  # PAFFY_STATS (the oracle has no such stage: it changes no line)
ERR_MISSING_QUERY = 17
GUARD = 256
E_ARG, E_STATE = r"\(-2\)", r"\(-5\)"

# matches, mismatches -> the text of (float)m / (m + x) as glibc prints it
F_TABLE = [((0, 0), "-nan"), ((0, 7), "0.000000"), ((1, 127), "0.007812"), ((3, 125), "0.023438"), ((5, 123), "0.039062"), ((1, 2), "0.333333"),
           ((2, 1), "0.666667"), ((1999999, 1), "1.000000"), ((16777217, 1), "1.000000")]


def ratio_lines():
    """[(line, Identity text or None, Identity-with-gaps text or None)]: the table through = and X ops, the same quotients through insert
    and delete bases in the gapped denominator, a record of I ops alone, a record without a cigar"""
    out = []
    for k, ((m, x), text) in enumerate(F_TABLE):
        ops = ([(m, "=")] if m else []) + ([(x, "X")] if x else [])
        strand = "+-"[k % 2]
        if ops:
            out.append((record(ops, strand, qname="q%d" % k, tname="t%d" % k), text, text))
        if m and x:  # identity 1.000000, the table's value with gaps: the x bases as inserts, as deletes, as both
            out.append((record([(m, "="), (x, "I")], strand, qname="qi%d" % k, tname="ti%d" % k), "1.000000", text))
            out.append((record([(x, "D"), (m, "=")], strand, qname="qd%d" % k, tname="td%d" % k), "1.000000", text))
            if x > 1:
                out.append((record([(1, "I"), (m, "="), (x - 1, "D")], strand, qname="qb%d" % k, tname="tb%d" % k), "1.000000", text))
        if not m and x:  # no match: 0.000000 both ways whatever the gaps
            out.append((record([(x, "X"), (3, "I"), (2, "D")], strand, qname="qz", tname="tz"), "0.000000", "0.000000"))
    out.append((record([(5, "I"), (200, "I")], "+", qname="only_i", tname="t_only_i"), "-nan", "0.000000"))
    nocg = record([(10, "M")], "-", qname="no_cg", tname="t_no_cg")
    out.append((nocg[:nocg.index("\tcg:Z:")] + "\n", "-nan", "-nan"))
    return [(ln.encode(), a, b) for ln, a, b in out]


def width_lines():
    """records without a cigar (nothing ties their lengths to an op): starts and lengths of 0 and of 10^k - 1 and 10^k for k = 1..18 in
    each of the four fields, both strands; scores negative, 0, of 19 digits, and absent"""
    vals = [0] + [v for k in range(1, 19) for v in (10 ** k - 1, 10 ** k)]
    scores = ["AS:i:-1", "AS:i:0", "AS:i:1234567890123456789", "AS:i:-1234567890123456789", None, "AS:i:-9", "AS:i:99999999", "AS:i:100000000"]
    n = len(vals)
    out = []
    for i, v in enumerate(vals):
        qs, qspan, ts, tspan = v, vals[(i + 9) % n], vals[(i + 18) % n], vals[(i + 27) % n]
        tags = "tp:A:P" + ("\t" + scores[i % len(scores)] if scores[i % len(scores)] else "")
        out.append("qw\t%d\t%d\t%d\t%s\ttw\t%d\t%d\t%d\t0\t0\t60\t%s\n" % (4 * 10 ** 18, qs, qs + qspan, "+-"[i % 2], 4 * 10 ** 18, ts, ts + tspan, tags))
    return [ln.encode() for ln in out]


NAME_LENS = (1, 15, 16, 17, 48, 255, 5000)


def name_lines():
    """query and target names of every length of NAME_LENS against each other; one record at every offset mod 16 of the batch text
    (the line in front of it is padded to get it there); the lines' lengths differ enough that the output offsets of the batch pass
    every residue mod 16 (test_names_and_alignment asserts both)"""
    rng = random.Random(0x71E7)

    def name(n, tag):
        return (tag + "".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789_.|") for _ in range(n)))[:n]

    out = []
    for i, qn in enumerate(NAME_LENS):
        for j, tn in enumerate(NAME_LENS):
            out.append(record([(7 + i, "="), (1 + j, "X")], "+-"[(i + j) % 2], qname=name(qn, "Q"), tname=name(tn, "T")))
    same = record([(40, "="), (2, "I"), (5, "X")], "-", qname="same_record_16_bytes", tname="same_target_17_bytes")
    at = sum(len(ln) for ln in out)
    for k in range(16):  # the same record at offset k mod 16 of the text: the line in front of it is padded to get it there
        pad = record([(3, "=")], "+", qname="pad", tname="p")
        pad = record([(3, "=")], "+", qname="pad" + "x" * ((k - at - len(pad)) % 16), tname="p")
        out += [pad, same]
        at += len(pad) + len(same)
    return [ln.encode() for ln in out]


def name_sequences(lines):
    """{name: a few bases} for every name of the lines: what the CLI's add_mismatches stage wants to find (no record here has an M op)"""
    seqs = {}
    for ln in lines:
        f = ln.split(b"\t")
        seqs[f[0].decode()] = b"ACGT"
        seqs[f[5].decode()] = b"ACGT"
    return seqs


def oracle_text(lines, seqs=None, rows=False):
    out = []
    for ln in lines:
        f = ln.split(b"\t")
        rc, text = O.pretty_print(ln, seqs[f[0].decode()] if rows else b"", seqs[f[5].decode()] if rows else b"", rows)
        assert rc == 0
        out.append(text)
    return out


def offsets_of(sizes):
    off = [0]
    for b in sizes:
        off.append(off[-1] + b)
    return off


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def plan(eng, stages, lines):
    import paffy_amd

    data = b"".join(lines)
    d_in = eng.to_device(data)
    info = eng.plan([paffy_amd.stage(*s) for s in stages], d_in, len(data))
    return d_in, info


def check_batch(eng, lines, want):
    """a [STATS] plan of the lines: the sizes are the oracle's lengths, the whole batch and every record alone are the oracle's bytes"""
    d_in, info = plan(eng, [(STATS, 0.0, 0.0)], lines)
    assert info.error.code == 0 and info.n_records == len(lines)
    sizes = eng.view_sizes(0, len(lines))
    assert sizes == [len(w) for w in want]
    whole = eng.view_text(0, len(lines), guard=GUARD)
    got, at = [], 0
    for b in sizes:
        got.append(whole[at:at + b])
        at += b
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:300], w[:300])
    return d_in, sizes, whole


def test_the_two_ratios_are_glibcs_text(eng):
    cases = ratio_lines()
    lines = [c[0] for c in cases]
    want = oracle_text(lines)
    _, _, whole = check_batch(eng, lines, want)
    got = whole.splitlines()
    assert len(got) == len(cases)
    for g, (ln, ident, gaps) in zip(got, cases):
        m = re.search(rb"\tIdentity:([^\t]+)\tIdentity-with-gaps([^\t]+)\t", g)
        assert (m.group(1).decode(), m.group(2).decode()) == (ident, gaps), (ln[:80], g)
    seen = {t for _, a, b in cases for t in (a, b)}
    assert seen == {t for _, t in F_TABLE}


def test_integer_widths(eng):
    lines = width_lines()
    want = oracle_text(lines)
    assert any(b"Q-start:0\t" in w for w in want) and any(b"Score:-1234567890123456789\t" in w for w in want)
    assert any(b"T-length:1000000000000000000\t" in w for w in want) and any(b"Q-length:999999999999999999\t" in w for w in want)
    assert {w.split(b"Same-strand:")[1][:1] for w in want} == {b"0", b"1"}
    check_batch(eng, lines, want)


def test_names_and_alignment(eng):
    lines = name_lines()
    want = oracle_text(lines)
    d_in, sizes, whole = check_batch(eng, lines, want)
    off_in, at = set(), 0
    for ln in lines:
        if ln.startswith(b"same_record_16_bytes"):
            off_in.add(at % 16)
        at += len(ln)
    assert off_in == set(range(16)), "the same record at every offset mod 16 of the batch text"
    assert {o % 16 for o in offsets_of(sizes)} == set(range(16)), "output offsets of every residue mod 16"
    assert max(len(ln.split(b"\t")[0]) for ln in lines) == 5000


def test_ranges_and_capacity(eng):
    lines = name_lines()[:40] + width_lines()[:9] + [c[0] for c in ratio_lines()]
    n = len(lines)
    want = b"".join(oracle_text(lines))
    d_in, info = plan(eng, [(STATS, 0.0, 0.0)], lines)
    assert info.error.code == 0
    off = offsets_of(eng.view_sizes(0, n))
    assert eng.view_text(0, n, guard=GUARD) == want
    for cuts in ([0, 1, 7, n], list(range(n + 1))):
        pieces = []
        for a, b in zip(cuts, cuts[1:]):
            assert eng.view_sizes(a, b - a) == [y - x for x, y in zip(off[a:b], off[a + 1:b + 1])]
            pieces.append(eng.view_text(a, b - a, offsets=off[a:b + 1], guard=GUARD))  # a slice of the batch's offsets: h_off[0] > 0
        assert b"".join(pieces) == want
    assert eng.view_text(3, 0) == b"" and eng.view_text(n, 0) == b"" and eng.view_sizes(2, 0) == []
    with pytest.raises(RuntimeError, match=E_ARG):  # one byte short
        eng.view_text(0, n, offsets=off, guard=GUARD, out_cap=off[n] - 1)
    with pytest.raises(RuntimeError, match=E_ARG):
        eng.view_text(7, n - 7, offsets=off[7:], guard=GUARD, out_cap=off[n] - off[7] - 1)
    assert eng.view_text(7, n - 7, offsets=off[7:], guard=GUARD, out_cap=off[n] - off[7]) == want[off[7]:]
    for first, count in ((0, n + 1), (n, 1), (n - 1, 2), (-1, 1)):
        with pytest.raises(RuntimeError, match=E_ARG):
            eng.view_sizes(first, count)
        with pytest.raises(RuntimeError, match=E_ARG):
            eng.view_text(first, count, offsets=[0] * (count + 1))
    # offsets that are not the sizes' running sums write nothing and are refused
    wrong = list(off)
    wrong[3] += 1
    with pytest.raises(RuntimeError, match=E_ARG):
        eng.view_text(0, n, offsets=wrong, guard=GUARD)


# ---- with rows: [ADD_MISMATCHES, STATS] on records that lie on sequences ----
ADD_ST = [(O.ADD_MISMATCHES, 0.05, 1.0), (STATS, 0.0, 0.0)]


def row_lines():
    """column totals round the windows of 150, a record without a cigar, both strands"""
    seqs = sequences()
    out = []
    for k, total in enumerate((1, 149, 150, 151, 300, 451)):
        ops = [(total, "M")] if total < 3 else [(total // 3, "M"), (1, "I"), (total - total // 3 - 2, "M"), (1, "D")]
        assert sum(n for n, _ in ops) == total
        for s in "+-":
            out.append(place(ops, s, 2 * k + (s == "-")))
    out.insert(5, b"qb\t%d\t10100\t10200\t+\ttb\t%d\t10300\t10400\t100\t100\t60\ttp:A:P\n" % (len(seqs["qb"]), len(seqs["tb"])))
    return out


_ROWS = {}


def row_case():
    """(lines, the oracle's blocks with rows, the oracle's stats lines alone) of row_lines() as add_mismatches encodes them"""
    if not _ROWS:
        seqs = sequences()
        lines = row_lines()
        enc, err = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines), seqs)
        assert err.code == 0
        enc = enc.splitlines(keepends=True)
        assert len(enc) == len(lines)
        _ROWS["case"] = (lines, oracle_text(enc, seqs, True), oracle_text(enc))
    return _ROWS["case"]


@pytest.fixture(scope="module")
def raw_eng():
    import paffy_amd

    e = paffy_amd.Engine()
    e.keep_raw_sequences(True)
    e.set_sequences(sequences())
    yield e
    e.close()


def test_lines_with_rows(raw_eng):
    import paffy_amd

    e = raw_eng
    lines, blocks, stats_lines = row_case()
    n = len(lines)
    d_in, info = plan(e, ADD_ST, lines)
    assert info.error.code == 0 and info.n_records == n
    sizes = e.view_sizes(0, n, with_rows=True)
    assert sizes == [len(b) for b in blocks]
    assert [a + b for a, b in zip(e.view_sizes(0, n), e.alignment_sizes(0, n))] == sizes
    assert e.view_text(0, n, with_rows=True, guard=GUARD) == b"".join(blocks)
    off = offsets_of(sizes)
    assert b"".join(e.view_text(a, 1, True, offsets=off[a:a + 2], guard=GUARD) for a in range(n)) == b"".join(blocks)
    assert e.view_text(0, n, guard=GUARD) == b"".join(stats_lines)  # the same plan without the rows
    with pytest.raises(RuntimeError, match=E_ARG):
        e.view_text(0, n, True, offsets=off, guard=GUARD, out_cap=off[n] - 1)
    # a name that is among no sequences: add_mismatches would fail the plan on it, so the rows' own report is reached behind a plan of
    # STATS alone, as in test_gpu_alignment_rows.py -- the record's index in the batch, wherever the call starts
    seqs = sequences()
    kw = dict(qlen=len(seqs["qb"]), tlen=len(seqs["tb"]), qs=12_000, ts=13_000)
    good = record([(20, "M")], "+", qname="qb", tname="tb", **kw).encode()
    lost = record([(20, "M")], "+", qname="nobody", tname="tb", **kw).encode()
    d_in, info = plan(e, [(STATS, 0.0, 0.0)], [good, good, lost, good])
    assert info.error.code == 0
    for first, count in ((0, 4), (2, 2), (2, 1)):
        with pytest.raises(paffy_amd.PafError) as ei:
            e.view_text(first, count, with_rows=True, guard=GUARD)
        assert (ei.value.info.code, ei.value.info.record) == (ERR_MISSING_QUERY, 2)
    assert e.view_text(0, 2, with_rows=True, guard=GUARD) == b"".join(oracle_text([good, good], seqs, True))
    assert e.view_text(0, 4, guard=GUARD) == b"".join(oracle_text([good, good, lost, good]))  # the lines alone need no sequence


def test_sums_only_plan_writes_the_same_lines(raw_eng):
    import paffy_amd

    e = raw_eng
    lines, blocks, stats_lines = row_case()
    n = len(lines)
    d_in, info = plan(e, ADD_ST, lines)
    default = e.view_text(0, n, guard=GUARD)
    assert default == b"".join(stats_lines)
    e.stats_only(True)
    try:
        d_in, info = plan(e, ADD_ST, lines)
        assert info.error.code == 0 and info.out_bytes == 0
        left = e.flat_stats()[0]
        assert left >= 0, "the sums-only plan did not take the flat pass"
        # the record without a cigar is the record kernels' (a flat piece needs a cigar); every other record is counted on the pieces
        assert left == sum(1 for ln in lines if b"cg:Z:" not in ln)
        assert e.view_sizes(0, n) == [len(s) for s in stats_lines]
        assert e.view_text(0, n, guard=GUARD) == default
        for call in (lambda: e.view_text(0, n, with_rows=True), lambda: e.view_sizes(0, n, with_rows=True)):
            with pytest.raises(RuntimeError, match=E_STATE + r".*paffy_hip_stats_only"):
                call()
        # every record on the pieces: nothing left to the record kernels
        with_cigar = [ln for ln in lines if b"cg:Z:" in ln]
        d_in, info = plan(e, ADD_ST, with_cigar)
        assert info.error.code == 0 and e.flat_stats()[0] == 0
        assert e.view_text(0, len(with_cigar), guard=GUARD) == b"".join(s for ln, s in zip(lines, stats_lines) if b"cg:Z:" in ln)
    finally:
        e.stats_only(False)
    # no STATS stage: no sums to print
    d_in, info = plan(e, [(O.ADD_MISMATCHES, 0.05, 1.0)], lines)
    assert info.error.code == 0
    for call in (lambda: e.view_sizes(0, 1), lambda: e.view_text(0, 1, offsets=[0, 0])):
        with pytest.raises(RuntimeError, match=E_STATE + r".*PAFFY_STATS"):
            call()
    # a plan that reported a failing record
    seqs = sequences()
    lost = record([(20, "M")], "+", qname="nobody", tname="tb", qlen=len(seqs["qb"]), tlen=len(seqs["tb"]), qs=12_000, ts=13_000).encode()
    d_in, info = plan(e, ADD_ST, lines[:3] + [lost])
    assert (info.error.code, info.error.record) == (ERR_MISSING_QUERY, 3)
    for call in (lambda: e.view_sizes(0, 1), lambda: e.view_text(0, 1, offsets=[0, 0])):
        with pytest.raises(RuntimeError, match=E_STATE + r".*failing record"):
            call()
    # another kind of plan since
    d_in, info = plan(e, ADD_ST, lines)
    e.tile(b"".join(with_cigar))  # (tile wants a cigar on every record)
    with pytest.raises(RuntimeError, match=E_STATE + r".*record plan"):
        e.view_sizes(0, 1)


# ---- a stream: the records of tests/test_view_stats.py ----
_STREAM = {}


def stream_case():
    if not _STREAM:
        host = synth_lib.Synth4(0x5EED0004, 2048, n_contigs=6, tlen_min=200_000, tlen_span=200_000)
        data, seqs = host.records(0, 1500), host.genomes()
        enc, err = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs)
        assert err.code == 0
        enc = enc.splitlines(keepends=True)
        tot = [0] * 6
        for ln in enc:
            tot = O.cigar_stats(cigar_of(ln).decode(), tot, zero=False)
        _STREAM["case"] = (data, seqs, oracle_text(enc), oracle_text(enc, seqs, True), tot)
    return _STREAM["case"]


def f32(x):
    import struct

    return struct.unpack("<f", struct.pack("<f", x))[0]


def total_line(n, tot):
    m, x, qi, qd, qib, qdb = tot
    return ("Total-alignments:%d\tAvg-Identity:%f\tAvg-Identity-with-gaps:%f\tAligned-bases:%d\tAligned-bases-with-gaps:%d\tQuery-inserts:%d\tQuery-deletes:%d\n"
            % (n, f32(f32(m) / f32(m + x)), f32(f32(m) / f32(m + x + qib + qdb)), m + x, m + x + qib + qdb, qi, qd)).encode()


@pytest.mark.parametrize("with_rows", [False, True], ids=["lines", "rows"])
def test_a_stream_in_ranges_of_a_mebibyte(with_rows):
    import paffy_amd

    data, seqs, stats_lines, blocks, tot = stream_case()
    want = blocks if with_rows else stats_lines
    e = paffy_amd.Engine()
    try:
        e.keep_raw_sequences(with_rows)
        e.set_sequences(seqs)
        e.stats_only(not with_rows)
        d_in = e.to_device(data)
        info = e.plan([paffy_amd.stage(*s) for s in ADD_ST], d_in, len(data))
        assert info.error.code == 0 and info.n_records == 1500
        off = offsets_of(e.view_sizes(0, 1500, with_rows))
        assert [b - a for a, b in zip(off, off[1:])] == [len(w) for w in want]
        got, first, calls = [], 0, 0
        while first < 1500:
            end = first + 1
            while end < 1500 and off[end + 1] - off[first] <= 1 << 20:
                end += 1
            got.append(e.view_text(first, end - first, with_rows, offsets=off[first:end + 1], guard=GUARD))
            first, calls = end, calls + 1
        assert b"".join(got) == b"".join(want)
        assert calls > 1 if with_rows else calls >= 1
    finally:
        e.close()


@pytest.mark.parametrize("flags", [(), ("s",), ("a", "s"), ("a", "t", "s")], ids=["plain", "s", "a_s", "a_t_s"])
def test_module_level_view(flags):
    import paffy_amd

    data, seqs, stats_lines, blocks, tot = stream_case()
    a, t, s = "a" in flags, "t" in flags, "s" in flags
    want = b"" if t else b"".join(blocks if a else stats_lines)
    if s:
        want += total_line(1500, tot)
    assert paffy_amd.view(data, seqs, include_alignment=a, per_alignment=not t, aggregate=s) == want

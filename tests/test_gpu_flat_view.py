"""The sums of `paffy view` without base-level rows, computed on the pieces of the flat pass (paffy_amd/csrc/flat_view_kernel.h:
Engine.stats_only, the stage list [ADD_MISMATCHES, STATS]) against the oracle: paf_stats_calc of every line `add_mismatches` writes. The
count walk takes the M ops of a piece 64 ops and 64 chunks of 16 columns at a time, so the cases put op lengths round the chunk, op
counts round the window, cigar text round the 1 KiB piece, and = / X ops, both strands and the sequence edge in between; what the pass
leaves goes through the record kernels and must report what the default plan reports."""
import hashlib
import random

import pytest

import oracle_lib as O
import synth_lib
from test_gpu_alignment_rows import STATS, make_seq
from test_gpu_flat import exact_ops, random_ops, record

pytestmark = pytest.mark.gpu

E_STATE = -5  # PAFFY_E_STATE (include/paffy_hip.h)
_SEQS = {}


def sequences():
    """mixed case, runs of N / n, a few letters outside ACGT. A query comes first: the - strand reads it downwards through the
    complemented copy, and nothing lies in front of the first sequence's first base."""
    if not _SEQS:
        rng = random.Random(0x51E3)
        ta = make_seq(rng, 150_000)
        qa = bytearray(ta)  # half of the columns of an M op agree, case aside
        for i in range(0, len(qa), 2):
            qa[i] = rng.choice(b"ACGTacgt")
        tc = make_seq(rng, 200_000)
        qc = bytearray(tc)
        for i in range(0, len(qc), 3):
            qc[i] = rng.choice(b"ACGTacgtNn")
        _SEQS.update({"qa": bytes(qa), "ta": ta, "qb": make_seq(rng, 30_000), "tb": make_seq(rng, 30_000), "qc": bytes(qc), "tc": tc})
    return _SEQS


def place(ops, strand="+", k=0, pair="a", qs=None, ts=None, **kw):
    seqs = sequences()
    qn, tn = "q" + pair, "t" + pair
    return record(ops, strand, qname=qn, tname=tn, qlen=len(seqs[qn]), tlen=len(seqs[tn]), qs=1000 + 37 * k if qs is None else qs,
                  ts=1200 + 53 * k if ts is None else ts, tags="tp:A:P\tAS:i:77", **kw)


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    e.set_sequences(sequences())
    yield e
    e.close()


def stages(*kinds):
    import paffy_amd

    return [paffy_amd.stage(k) for k in kinds]


_WANT = {}


def oracle_stats(data, seqs=None):
    """(error, [six sums per line `add_mismatches` wrote]): computed once per input"""
    key = hashlib.sha256(data).hexdigest()
    if key not in _WANT:
        out, err = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs or sequences())
        per = []
        for ln in out.splitlines():
            f = ln.split(b"cg:Z:")
            per.append(tuple(O.cigar_stats(f[1].split(b"\t")[0].decode())) if len(f) > 1 and f[1].split(b"\t")[0] else (0,) * 6)
        _WANT[key] = ((err.code, err.record), per)
    return _WANT[key]


def plan_view(eng, data, on=True):
    """(PlanInfo, totals, per record, left) of [ADD_MISMATCHES, STATS] with the mode on or off"""
    eng.stats_only(on)
    try:
        info = eng.plan(stages(O.ADD_MISMATCHES, STATS), eng.to_device(data), len(data))
        per = eng.record_stats(info.n_records)
        return info, tuple(eng.plan_stats()), per, eng.flat_stats()[0]
    finally:
        eng.stats_only(False)


def check(eng, lines, want_left=0):
    data = "".join(lines).encode()
    (wcode, wrec), want = oracle_stats(data)
    info, tot, per, left = plan_view(eng, data)
    print("left", left, "records", info.n_records, "error", info.error.code, info.error.record)
    assert info.out_bytes == 0 and info.n_rows == 0 and info.n_records == len(lines)
    assert (info.error.code, info.error.record if wcode else 0) == (wcode, wrec if wcode else 0)
    n_ok = wrec if wcode else len(lines)
    assert len(want) == n_ok
    bad = [i for i in range(n_ok) if per[i] != want[i]]
    assert not bad, (bad[:5], per[bad[0]], want[bad[0]])
    if not wcode:
        assert tot == tuple(sum(w[k] for w in want) for k in range(6))
    if want_left is not None:
        assert left == want_left, left
    return info, per, left


def test_api_presence(eng):
    import paffy_amd

    assert callable(getattr(paffy_amd.Engine, "stats_only", None)) and callable(getattr(paffy_amd, "view_stats", None))
    assert hasattr(paffy_amd.engine.lib(), "paffy_hip_stats_only")


CHUNK_LENS = (1, 15, 16, 17, 31, 32, 33, 2000)


def test_chunks_and_windows(eng):
    rng = random.Random(11)
    lines, k = [], 0
    for s in "+-":
        for n in CHUNK_LENS:  # alone (a record of one op), and between indels
            lines.append(place([(n, "M")], s, k))
            lines.append(place([(3, "M"), (2, "I"), (n, "M"), (1, "D"), (n, "M"), (4, "I"), (5, "M")], s, k + 1))
            k += 2
        for n in (63, 64, 65, 129):  # round the window of 64 ops
            lines.append(place(exact_ops(rng, n, lens=(1, 2, 16, 17, 40), indel=(1, 2, 3)), s, k))
            k += 1
        lines.append(place(random_ops(rng, 301), s, k))
        k += 1
        # more chunks than one round of the item loop takes, from many ops: 64 M ops of 99 columns in one window
        lines.append(place([(99, "M"), (1, "I")] * 64 + [(7, "M")], s, k, pair="c"))
        k += 1
    check(eng, lines)


def test_minus_strand_at_the_first_sequence_edge(eng):
    """the last chunk of a - strand op whose query range starts at base 0..14 of the first loaded sequence: match_mask16 may not read in
    front of the store"""
    assert next(iter(sequences())) == "qa"
    lines = []
    for qs in range(15):
        for n in (1, 5, 16, 33):
            lines.append(place([(n, "M")], "-", qs=qs, ts=40 + qs))
            lines.append(place([(n, "M"), (2, "D"), (3, "M")], "-", qs=qs, ts=90 + qs))
            lines.append(place([(n, "M")], "+", qs=qs, ts=qs))
    check(eng, lines)


def dense_ops(n_bytes):
    """ops whose text has exactly n_bytes: two bytes per op (512 op letters per KiB, the most a piece can hold), one three-byte op for an odd count"""
    ops = [(10, "M")] if n_bytes % 2 else []
    n = (n_bytes - 3 * len(ops)) // 2
    ops += [((1 + i // 2 % 9), "MIMD"[i % 4]) for i in range(n)]
    if ops[-1][1] != "M":
        ops[-1] = (ops[-1][0], "M")
    assert sum(len("%d%s" % o) for o in ops) == n_bytes
    return ops


def test_pieces(eng):
    rng = random.Random(12)
    lines, k = [], 0
    for s in "+-":
        for n_bytes in (1023, 1024, 1025, 4095, 4096, 4097):
            lines.append(place(dense_ops(n_bytes), s, k))
            k += 1
        lines.append(place(exact_ops(rng, 40_001, lens=(1, 2, 3), indel=(1, 2, 3)), s, k))  # 80 KB of text: more than 64 pieces
        k += 1
    lines.append(place(exact_ops(rng, 100_001, lens=(1, 2), indel=(1,)), "-", k))
    # four-digit lengths: a 15-byte cycle over 1.1 KiB, the record's header one byte longer each time, so that a piece boundary falls on
    # every byte of a cycle, inside the numbers and next to the letters
    for j in range(15):
        lines.append(place([(1234, "M"), (1000, "I"), (1001, "D")] * 75 + [(8191, "M")], "+-"[j % 2], pair="c", qs=100 + j, ts=300 + j).replace("AS:i:77", "AS:i:77\tzz:Z:" + "p" * j))
    check(eng, lines)


def test_eq_and_x_ops_in_the_input(eng):
    """= and X ops pass through the encoder: they count as matches and mismatches whatever the bases are; 200 ops other than M in a row
    (the add mode's item word holds 62) do not send the record away"""
    rng = random.Random(13)
    lines = []
    for k, s in enumerate("+-"):
        lines.append(place([(5, "M"), (3, "="), (2, "X"), (17, "M"), (1, "I"), (40, "="), (1, "X"), (33, "M"), (2, "D"), (6, "X")], s, k))
        lines.append(place([(4, "M")] + [(1 + i % 3, "=XID"[i % 4]) for i in range(200)] + [(40, "M"), (2, "X")], s, k + 2))
        lines.append(place([(7, "=")], s, k + 4))
        mixed = [(n, c if c != "M" or i % 4 else "=X"[i // 4 % 2]) for i, (n, c) in enumerate(exact_ops(rng, 1201, lens=(1, 2, 16, 40), indel=(1, 2)))]
        lines.append(place(mixed, s, k + 6))
    check(eng, lines)


GOOD = [(30, "M"), (2, "I"), (17, "M"), (1, "D"), (9, "M")]


def special_batches():
    """one record the pass leaves, between regular ones"""
    seqs = sequences()
    ok = [place(GOOD, "+-"[k % 2], k) for k in range(4)]
    span_q = sum(n for n, c in GOOD if c != "D")
    beyond = record(GOOD, "+", qname="qb", tname="tb", qlen=len(seqs["qb"]) + 500, tlen=len(seqs["tb"]), qs=len(seqs["qb"]) - span_q + 100, ts=50, tags="tp:A:P")
    bad_check = place(GOOD, "+", 9).split("\t")
    bad_check[3] = str(int(bad_check[3]) + 1)  # the query end one base past the cigar's
    empty = place(GOOD, k=4)
    empty = empty[:empty.index("cg:Z:") + 5] + "\n"
    return {
        "missing_query": ok[:2] + [place(GOOD, "+", 7).replace("qa\t", "nobody\t", 1)] + ok[2:],
        "missing_target": ok[:3] + [place(GOOD, "-", 8).replace("\tta\t", "\tnobody\t", 1)] + ok[3:],
        "range_beyond_sequence": ok[:1] + [beyond] + ok[1:],
        "paf_check": ok[:2] + ["\t".join(bad_check)] + ok[2:],
        "length_8192": ok[:2] + [place([(5, "M"), (8192, "M"), (1, "I"), (3, "M")], "-", 1, pair="c")] + ok[2:],
        "no_cigar": ok[:1] + [place(GOOD, k=3).replace("\tcg:Z:", "\tzz:Z:")] + ok[1:],
        "empty_cigar": ok[:3] + [empty] + ok[3:],
    }


KNOWN_CODES = {"missing_query": 17, "missing_target": 18, "range_beyond_sequence": 21, "length_8192": 0}


@pytest.mark.parametrize("name", ["missing_query", "missing_target", "range_beyond_sequence", "paf_check", "length_8192", "no_cigar", "empty_cigar"])
def test_records_left_to_the_record_kernels(eng, name):
    """what the default plan reports, the sums in front of a failure, and where no error ends the plan the one record counted as left"""
    lines = special_batches()[name]
    data = "".join(lines).encode()
    info, per, left = check(eng, lines, want_left=None)
    d_info, d_tot, d_per, d_left = plan_view(eng, data, on=False)
    print(name, "code", info.error.code, "stage", info.error.stage, "record", info.error.record, "aux", info.error.aux, "left", left)
    assert d_left == -1
    if name in KNOWN_CODES:
        assert info.error.code == KNOWN_CODES[name]
    if name == "paf_check":
        assert info.error.code != 0
    assert (info.error.code, info.error.stage, info.error.record) == (d_info.error.code, d_info.error.stage, d_info.error.record)
    if info.error.code:
        assert left >= 1 and per[:info.error.record] == d_per[:info.error.record]
    else:
        assert left == 1 and per == d_per


_SYNTH = {}


def synth4():
    if not _SYNTH:
        host = synth_lib.Synth4(0x5EED0004, 2048, n_contigs=6, tlen_min=200_000, tlen_span=200_000)
        _SYNTH.update(data=host.records(0, 1500), seqs=host.genomes())
    return _SYNTH["data"], _SYNTH["seqs"]


def test_same_answers_as_the_default_plan():
    import paffy_amd

    data, seqs = synth4()
    e = paffy_amd.Engine()
    try:
        e.set_sequences(seqs)
        off = plan_view(e, data, on=False)
        off_out = e.run(stages(O.ADD_MISMATCHES, STATS), data)[0]
        on = plan_view(e, data, on=True)
        assert off[3] == -1 and on[3] == 0, (off[3], on[3])
        assert on[0].error.code == 0 and on[0].n_records == 1500 and on[0].out_bytes == 0 and off[0].out_bytes == len(off_out) > 0
        assert on[1] == off[1] and on[2] == off[2]
        (wcode, _), want = oracle_stats(data, seqs)
        assert wcode == 0 and on[2] == want
        # off again on the same engine: the setting leaves nothing behind
        again = plan_view(e, data, on=False)
        assert again[3] == -1 and again[0].out_bytes == off[0].out_bytes and again[1:3] == off[1:3]
        assert e.run(stages(O.ADD_MISMATCHES, STATS), data)[0] == off_out
        # the package-level call
        assert paffy_amd.view_stats(data, seqs) == (on[1], on[2])
    finally:
        e.close()


def test_refusals_and_other_stage_lists(eng):
    data = "".join(place(GOOD, "+-"[k % 2], k) for k in range(40)).encode()
    d_in = eng.to_device(data)
    eng.stats_only(True)
    try:
        info = eng.plan(stages(O.ADD_MISMATCHES, STATS), d_in, len(data))
        assert info.error.code == 0 and info.out_bytes == 0 and eng.flat_stats()[0] == 0
        for call in (lambda: eng.emit(eng.alloc_out(64)), lambda: eng.alignment_sizes(0, 2), lambda: eng.record_layout(0, 2)):
            with pytest.raises(RuntimeError, match=r"\(%d\).*paffy_hip_stats_only" % E_STATE):
                call()
        assert len(eng.record_stats(info.n_records)) == 40  # the sums are still there
    finally:
        eng.stats_only(False)
    for kinds in ((O.ADD_MISMATCHES,), (STATS,), (O.ADD_MISMATCHES, O.INVERT, STATS)):
        res = []
        for on in (False, True):
            eng.stats_only(on)
            try:
                out, info = eng.run(stages(*kinds), data)
                res.append((out, info.out_bytes, info.n_rows, eng.flat_stats(), eng.plan_stats() if STATS in kinds else None))
            finally:
                eng.stats_only(False)
        assert res[0] == res[1] and len(res[0][0]) > 0, kinds

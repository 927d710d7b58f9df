"""`paffy add_mismatches | paffy trim -r | paffy filter` as the fused stage lists [ADD, TRIM_IDENTITY], [ADD, FILTER] and
[ADD, TRIM_IDENTITY, FILTER] on the pieces of the flat pass (paffy_amd/csrc/flat_add_pipe_kernel.h) against the oracle: error code, stage
and record equal, the output equal by length and SHA-256, then who sized the records (flat_stats). The inputs are those of
add_pipe_lib.py; test_flat_add_pipe_cpu.py proves on the oracle alone that they are sharp."""
import hashlib
import random

import numpy as np
import pytest

import add_pipe_lib as A
import oracle_lib as O
from test_gpu_flat import exact_ops, n_ops_of

pytestmark = pytest.mark.gpu
S = O.stage
ADD, TRIM, FILT = O.ADD_MISMATCHES, O.TRIM_IDENTITY, O.FILTER
LISTS = ([ADD, TRIM], [ADD, FILT], [ADD, TRIM, FILT])
WHY_ENCODER = 11  # FLAT_WHY_ENCODER: the encoder on the pieces did not keep the record


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def gs(kinds, params=None):
    import paffy_amd

    return [paffy_amd.stage(k, *(params or {}).get(k, ())) for k in kinds]


def both(eng, kinds, data, seqs, params=None, left=0):
    """the oracle's run against the engine's; returns (the oracle's output, its error, (left, why))"""
    want, werr = O.run([S(k, *(params or {}).get(k, ())) for k in kinds], data, seqs)
    got, info = eng.run(gs(kinds, params), data, raise_on_error=False)
    stats = eng.flat_stats()
    print("flat stats", kinds, params, stats[0], list(stats[1]))
    assert (info.error.code, info.error.stage, info.error.record) == (werr.code, werr.stage, werr.record), (kinds, info.error.code, werr.code)
    assert len(got) == len(want) and hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest(), (kinds, len(got), len(want))
    if left is not None:
        assert stats[0] == left, (kinds, stats[0], list(stats[1]))
    return want, werr, stats


def test_who_sized_it(eng):
    """T1: some 200 plain records, both strands, 40 to 3 000 ops, homologous sequences with noisy ends. The three lists are sized by the
    flat pass (no record left; -1 before this mode existed) and equal the oracle; the trim cuts a third of the records at least; then
    [ADD], [INVERT] and [ADD, TRIM] again on the same engine: nothing of a plan is left over."""
    b = A.t1_batch()
    data = b.data()
    eng.set_sequences(b.seqs)
    plain, _, _ = both(eng, [ADD], data, b.seqs)
    out = {}
    for kinds in LISTS:
        O.set_filter(min_identity=0.97)
        eng.set_filter(min_identity=0.97)
        try:
            out[tuple(kinds)], werr, _ = both(eng, kinds, data, b.seqs)
        finally:
            O.set_filter()
            eng.set_filter()
        assert werr.code == 0
    trimmed = out[(ADD, TRIM)].splitlines()
    assert len(trimmed) == len(b.lines) and 3 * sum(x != y for x, y in zip(plain.splitlines(), trimmed)) >= len(b.lines)
    assert 0 < len(out[(ADD, FILT)].splitlines()) < len(b.lines) and out[(ADD, FILT)] != out[(ADD, TRIM, FILT)]
    both(eng, [ADD], data, b.seqs)
    both(eng, [O.INVERT], data, b.seqs)
    again, _, _ = both(eng, [ADD, TRIM], data, b.seqs)
    assert again == out[(ADD, TRIM)]


def test_cuts_at_piece_boundaries(eng):
    """T2: front cuts that end on the op before the last new op of the record's piece 0, on that op, on the first new op of piece 1 and
    on the one behind it; the same for the back cut at the last piece boundary. Both strands are built; the positions are read from the
    oracle's output. All eight are seen on the '-' records. A '+' record shows the four of the front: its back is never cut by the
    reference (the second pass runs on the inverted record, and paf_invert reverses the cigar of a '-' record only, impl/paf.c:469-490)."""
    b, _ = A.t2_batch()
    data = b.data()
    eng.set_sequences(b.seqs)
    plain, _, _ = both(eng, [ADD], data, b.seqs)
    trimmed, werr, _ = both(eng, [ADD, TRIM], data, b.seqs)
    assert werr.code == 0
    seen = A.t2_seen(b, plain, trimmed)
    assert {(s, f) for s, f, _ in seen} == {(s, r) for s in "+-" for r in A.RELS}
    assert {k for s, _, k in seen if s == "-"} == set(A.RELS) and {k for s, _, k in seen if s == "+"} == {None}
    both(eng, [ADD, TRIM, FILT], data, b.seqs)


@pytest.mark.parametrize("p0", [0.0, 0.05, 1.0])
def test_parameters(eng, p0):
    """T3: trim -r x trim -t on the T1 batch; a small max_trim stops the walk inside a piece"""
    b = A.t1_batch()
    data = b.data()
    eng.set_sequences(b.seqs)
    outs = set()
    for p1 in (0.0, 0.01, 0.5, 1.0):
        want, werr, _ = both(eng, [ADD, TRIM], data, b.seqs, params={TRIM: (p0, p1)})
        assert werr.code == 0
        outs.add(hashlib.sha256(want).hexdigest())
    assert len(outs) >= (3 if p0 < 1.0 else 1)  # the parameters matter on this batch


def filtered(eng, b, kinds=(ADD, FILT), **thr):
    O.set_filter(**thr)
    eng.set_filter(**thr)
    try:
        want, werr, _ = both(eng, list(kinds), b.data(), b.seqs)
    finally:
        O.set_filter()
        eng.set_filter()
    assert werr.code == 0
    return [l.split(b"\t")[0] for l in want.splitlines()]


def test_filter(eng):
    """T4: min_identity and min_identity_with_gaps at a tie (identity == threshold in float32), one = base more and one less, with and
    without invert; a threshold that drops every record; alignment score, chain score and tile level once each; and, behind a trim, a
    record that passes untrimmed and fails trimmed, and the reverse."""
    for make, key in ((A.t4_identity_batch, "min_identity"), (A.t4_gaps_batch, "min_identity_with_gaps")):
        b, _ = make()
        eng.set_sequences(b.seqs)
        n = len(b.lines)
        kept = filtered(eng, b, **{key: A.TIE})
        assert len(kept) == 2 * n // 3  # the tie and the base more stay
        assert len(filtered(eng, b, **{key: 0.7})) == n // 3  # 0.7 lies above (double)0.7f: the tie goes
        assert len(filtered(eng, b, invert=True, **{key: A.TIE})) == n // 3
        assert filtered(eng, b, **{key: 1.5}) == []  # out_bytes == 0, left == 0
        assert len(filtered(eng, b, invert=True, **{key: 1.5})) == n
    b = A.t4_tags_batch()
    eng.set_sequences(b.seqs)
    assert len(filtered(eng, b, min_alignment_score=500)) == 1
    assert len(filtered(eng, b, min_chain_score=40)) == 2
    assert len(filtered(eng, b, max_tile_level=1)) == 2
    b = A.t4_trim_batch()
    eng.set_sequences(b.seqs)
    thr = A.T4_TRIM_THRESHOLDS
    assert filtered(eng, b, (ADD, FILT), **thr) != filtered(eng, b, (ADD, TRIM, FILT), **thr)
    assert len(filtered(eng, b, (ADD, FILT), **thr)) == 1 and len(filtered(eng, b, (ADD, TRIM, FILT), **thr)) == 1


def small_good(b, rng, strand):
    ops = A.plain_ops(rng, 60)
    cols = A.m_columns(ops)
    return b.add(ops, A.noisy_ends_mask(cols, 30, 20), strand)


def mixed(edit):
    """good, good, the edited record, good, good; edit(batch, index of a good record's twin) -> new line text"""
    rng = random.Random(5105)
    b = A.Batch("e")
    small_good(b, rng, "+")
    small_good(b, rng, "-")
    i = small_good(b, rng, "+")
    small_good(b, rng, "-")
    small_good(b, rng, "+")
    b.lines[i] = edit(b, i)
    return b


def test_mixed_batch(eng):
    """T5: between kept records, each in a batch of its own: a missing sequence, a range outside its sequence, an irregular cigar, an op
    of length 8 192 -- the record kernels report what there is to report, the error triple is the oracle's."""
    def missing(b, i):
        return b.lines[i].replace("eq%d\t" % i, "nope\t", 1)

    def outside(b, i):
        f = b.lines[i].split("\t")
        n = len(b.seqs[b"eq%d" % i])
        span = int(f[3]) - int(f[2])
        f[1], f[2], f[3] = str(n + 10_000), str(n + 10), str(n + 10 + span)
        return "\t".join(f)

    def irregular(b, i):
        L, c = b.ops[i][0]
        return b.lines[i].replace("cg:Z:%d%s" % (L, c), "cg:Z:00%d%s" % (L, c), 1)

    def long_op(b, i):
        ops = [(8192, "M"), (1, "I"), (300, "M")]
        b2 = A.Batch("x")
        b2.add(ops, A.noisy_ends_mask(A.m_columns(ops), 30, 0), "+")
        b.seqs[b"xt0"], b.seqs[b"xq0"] = b2.seqs[b"xt0"], b2.seqs[b"xq0"]
        return b2.lines[0]

    for edit in (missing, outside, irregular, long_op):
        b = mixed(edit)
        eng.set_sequences(b.seqs)
        for kinds in LISTS:
            _, werr, (left, why) = both(eng, kinds, b.data(), b.seqs, left=None)
            print(edit.__name__, kinds, "oracle error", werr.code, werr.stage, werr.record)
            assert left == 1 and why[WHY_ENCODER] == 1, (edit.__name__, kinds, left, list(why))


def test_a_record_without_a_cigar(eng):
    """T5: a record without cg:Z: between two good ones. [ADD, TRIM]: the trim's identity assert (0 / 0), record 1, stage 1, the first
    line alone; [ADD, FILTER] with default thresholds: the record is dropped (NaN identity), both good lines come out -- after an earlier
    batch on the same engine put a record WITH a cigar at that index; [ADD]: the line passes through without a cigar."""
    rng = random.Random(5106)
    b = A.Batch("f")
    small_good(b, rng, "+")
    i = small_good(b, rng, "-")
    small_good(b, rng, "+")
    eng.set_sequences(b.seqs)
    with_cg = b.data()
    both(eng, [ADD, FILT], with_cg, b.seqs)
    both(eng, [ADD, TRIM], with_cg, b.seqs)
    b.lines[i] = b.lines[i][:b.lines[i].index("\tcg:Z:")] + "\n"
    data = b.data()
    want, werr, _ = both(eng, [ADD, FILT], data, b.seqs, left=1)
    assert werr.code == 0 and len(want.splitlines()) == 2 and all(b"cg:Z:" in l for l in want.splitlines())
    want, werr, _ = both(eng, [ADD, TRIM], data, b.seqs, left=1)
    assert (werr.code, werr.stage, werr.record) == (14, 1, 1) and len(want.splitlines()) == 1
    want, werr, _ = both(eng, [ADD], data, b.seqs, left=1)
    assert werr.code == 0 and len(want.splitlines()) == 3 and b"cg:Z:" not in want.splitlines()[1]
    want, werr, _ = both(eng, [ADD, TRIM, FILT], data, b.seqs, left=1)
    assert (werr.code, werr.stage, werr.record) == (14, 1, 1)


SEG, ROWS_MAX = 16_384, 32_768  # ADD_SEG_OPS, PAFFY_ROWS_MAX_OPS


def test_segments(eng):
    """T6: lines of more than 32 768 new ops, written as segments cut at piece boundaries inside the window: uncut; cut inside the first
    and inside the last segment ('-': both ends); and a noisy head so long that more than a whole segment of 16 384 new ops goes."""
    b = A.t6_batch()
    data = b.data()
    eng.set_sequences(b.seqs)
    plain, _, _ = both(eng, [ADD], data, b.seqs)
    trimmed, werr, _ = both(eng, [ADD, TRIM], data, b.seqs)
    assert werr.code == 0
    cut = [A.cuts(x, y) for x, y in zip(plain.splitlines(), trimmed.splitlines())]
    left_ops = [n_ops_of(A.cigar_of(l)) for l in trimmed.splitlines()]
    print("cuts", cut, "ops left", left_ops)
    assert all(n > ROWS_MAX for n in left_ops)
    assert cut[0] == (0, 0) and cut[1] == (0, 0)
    assert 0 < cut[2][0] < SEG and 0 < cut[3][0] < SEG and 0 < cut[3][1] < SEG
    assert cut[4][0] > SEG + 1000 and cut[5][0] > SEG + 1000 and cut[5][1] > SEG + 1000
    O.set_filter(min_identity=0.9)
    eng.set_filter(min_identity=0.9)
    try:
        both(eng, [ADD, TRIM, FILT], data, b.seqs)
        both(eng, [ADD, FILT], data, b.seqs)
    finally:
        O.set_filter()
        eng.set_filter()


@pytest.mark.parametrize("n_ops", [100_001, 1_000_001])
def test_very_long_records(n_ops):
    """T7: records of 100 001 and 1 000 001 input ops with a noisy head and tail, '+' and '-', a fresh engine per case: the trim cuts, the
    window is written as a hundred segments, no record leaves the flat pass."""
    import paffy_amd

    rng = random.Random(5108 + n_ops)
    ops = exact_ops(rng, n_ops, lens=(1, 5, 30, 60, 110), indel=(1, 2, 3))
    cols = A.m_columns(ops)
    b = A.Batch("v")
    b.add(ops, A.noisy_ends_mask(cols, 3000, 2000), "+")
    b.add(ops, None, "-", seqs=b.last_seqs)
    small_good(b, rng, "+")
    data = b.data()
    e2 = paffy_amd.Engine()
    try:
        e2.set_sequences(b.seqs)
        trimmed, werr, _ = both(e2, [ADD, TRIM], data, b.seqs)
        assert werr.code == 0
        # the target range of the written line against the input's: the front of both records was cut, and the back of the '-' record
        # (the reference never cuts the back of a '+' record, see test_cuts_at_piece_boundaries)
        moved = [(int(y.split(b"\t")[7]) - int(x.split("\t")[7]), int(x.split("\t")[8]) - int(y.split(b"\t")[8])) for x, y in zip(b.lines[:2], trimmed.splitlines()[:2])]
        print("target bases cut (front, back)", moved)
        assert moved[0][0] > 1000 and moved[0][1] == 0 and moved[1][0] > 1000 and moved[1][1] > 1000
        assert n_ops_of(A.cigar_of(trimmed.splitlines()[0])) > n_ops
    finally:
        e2.close()


def test_second_try():
    """T8: a fresh engine and records whose M ops of 50 alternating columns become fifty ops each: the first guess of new_ops[] is too
    small, the batch is encoded again, and the trim runs on the second try's ops."""
    import paffy_amd

    b = A.Batch("h")
    ops = [(50, "M") if i % 2 == 0 else (1, "I") for i in range(4999)]
    cols = A.m_columns(ops)
    for k in range(12):
        m = np.zeros(cols, dtype=bool)
        m[1::2] = True
        m[:3000] = False
        m[cols - 3000:] = False
        m[0:80:2] = True
        m[cols - 1:cols - 61:-2] = True
        b.add(ops, m, "+-"[k & 1])
    data = b.data()
    plain, perr = O.run([S(ADD)], data, b.seqs)
    assert perr.code == 0 and sum(n_ops_of(A.cigar_of(l)) for l in plain.splitlines()) > len(data) + (1 << 20)  # more than the first try allows
    e2 = paffy_amd.Engine()
    try:
        e2.set_sequences(b.seqs)
        trimmed, werr, _ = both(e2, [ADD, TRIM], data, b.seqs)
        assert werr.code == 0 and sum(x != y for x, y in zip(plain.splitlines(), trimmed.splitlines())) == 12
    finally:
        e2.close()


def test_summary_overflow(eng):
    """T9: one piece that becomes more than 65 535 new ops (ten 8191M ops on alternating columns in fifty bytes of text). The counts of
    the new ops' summaries are 32 bits wide: the record stays with the flat pass, and the trim's cut ends inside that piece."""
    b = A.t9_batch()
    data = b.data()
    eng.set_sequences(b.seqs)
    plain, _, _ = both(eng, [ADD], data, b.seqs)
    per_piece = A.new_ops_by_piece(b.cigar_start(0), b.ops[0], A.ops_of(plain.splitlines()[0]))
    assert len(per_piece) >= 2 and per_piece[0] > 65_535
    trimmed, werr, _ = both(eng, [ADD, TRIM], data, b.seqs, left=0)
    assert werr.code == 0
    f, k = A.cuts(plain.splitlines()[0], trimmed.splitlines()[0])
    print("new ops per piece", per_piece, "cut", f, k)
    assert per_piece[0] > 65_535 and 0 < f < per_piece[0]
    both(eng, [ADD, FILT], data, b.seqs, left=0)

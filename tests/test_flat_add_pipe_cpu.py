"""The inputs of test_gpu_flat_add_pipe.py on the oracle alone (no GPU): the identity trim behind add_mismatches cuts where the builders
of add_pipe_lib.py say, relative to the 1 KiB pieces of the flat pass; the filter's ties flip with one base; the trim cuts a third of the
plain batch at least."""
import add_pipe_lib as A
import oracle_lib as O

S = O.stage
ADD, TRIM, FILT = O.ADD_MISMATCHES, O.TRIM_IDENTITY, O.FILTER


def run(kinds, b):
    out, err = O.run([S(k) for k in kinds], b.data(), b.seqs)
    assert err.code == 0
    return out.splitlines()


def test_the_trim_cuts_a_third_of_the_plain_batch():
    b = A.t1_batch()
    plain, trimmed = run([ADD], b), run([ADD, TRIM], b)
    assert len(plain) == len(trimmed) == len(b.lines) == 200
    n_cut = sum(x != y for x, y in zip(plain, trimmed))
    assert 3 * n_cut >= len(b.lines) and n_cut < len(b.lines)  # and some stay whole
    assert {l.split("\t")[4] for l in b.lines} == {"+", "-"}
    n_ops = [len(o) for o in b.ops]
    assert min(n_ops) <= 41 and max(n_ops) >= 3000
    # more than a few pieces, and records of one piece
    pieces = [len(A.new_ops_by_piece(b.cigar_start(i), b.ops[i], A.ops_of(plain[i]))) for i in range(len(b.lines))]
    assert min(pieces) == 1 and max(pieces) > 8


def test_the_cuts_land_on_the_piece_boundaries():
    """the front cut ends on the op before the last new op of piece 0, on it, on the first op of piece 1 and on the op behind it, on
    both strands; the back cut the same at the last boundary on the '-' records; the back of a '+' record is never cut"""
    b, want = A.t2_batch()
    plain, trimmed = run([ADD], b), run([ADD, TRIM], b)
    seen = A.t2_seen(b, plain, trimmed)
    for i, ((strand, rf, rb), (cf, cb, wf, wb)) in enumerate(zip(seen, want)):
        f, k = A.cuts(plain[i], trimmed[i])
        assert f == cf and rf == wf, (i, f, cf, rf, wf)
        if strand == "-":
            assert k == cb and rb == wb, (i, k, cb, rb, wb)
        else:
            assert k == 0 and rb is None
    assert {(s, f) for s, f, _ in seen} == {(s, r) for s in "+-" for r in A.RELS}
    assert {k for s, _, k in seen if s == "-"} == set(A.RELS)


def kept(b, kinds=(ADD, FILT), **thr):
    O.set_filter(**thr)
    try:
        return [l.split(b"\t")[0] for l in run(list(kinds), b)]
    finally:
        O.set_filter()


def test_the_filter_ties_flip_with_one_base():
    assert A.TIE < 0.7 and A.quot(70, 100) == A.TIE and A.quot(69, 99) < A.TIE < A.quot(71, 101)
    for make, key, other in ((A.t4_identity_batch, "min_identity", "min_identity_with_gaps"), (A.t4_gaps_batch, "min_identity_with_gaps", "min_identity")):
        b, want = make()
        names = [l.split("\t")[0].encode() for l in b.lines]
        eqs = [eq for eq, _ in want]
        assert kept(b, **{key: A.TIE}) == [n for n, eq in zip(names, eqs) if eq >= 70]
        assert kept(b, **{key: 0.7}) == [n for n, eq in zip(names, eqs) if eq >= 71]
        assert kept(b, invert=True, **{key: A.TIE}) == [n for n, eq in zip(names, eqs) if eq < 70]
        assert kept(b, **{key: 1.5}) == [] and kept(b, invert=True, **{key: 1.5}) == names
        assert kept(b, **{other: A.TIE}) != kept(b, **{key: A.TIE})  # the two identities differ on these records: the gaps count in one
    b = A.t4_tags_batch()
    assert len(kept(b, min_alignment_score=500)) == 1 and len(kept(b, min_chain_score=40)) == 2 and len(kept(b, max_tile_level=1)) == 2


def test_trimming_changes_what_the_filter_sees():
    b = A.t4_trim_batch()
    names = [l.split("\t")[0].encode() for l in b.lines]
    assert kept(b, (ADD, FILT), **A.T4_TRIM_THRESHOLDS) == names[:1]        # passes untrimmed ...
    assert kept(b, (ADD, TRIM, FILT), **A.T4_TRIM_THRESHOLDS) == names[1:]  # ... fails trimmed, and the reverse
    plain, trimmed = run([ADD], b), run([ADD, TRIM], b)
    assert [A.cuts(x, y)[0] > 0 for x, y in zip(plain, trimmed)] == [True, True]


def test_one_piece_of_more_than_65535_new_ops():
    b = A.t9_batch()
    plain, trimmed = run([ADD], b), run([ADD, TRIM], b)
    per_piece = A.new_ops_by_piece(b.cigar_start(0), b.ops[0], A.ops_of(plain[0]))
    f, k = A.cuts(plain[0], trimmed[0])
    assert len(per_piece) >= 2 and 65_535 < per_piece[0] < 131_072 and 0 < f < per_piece[0] and k == 0


def test_the_long_lines_are_cut_where_the_segments_test_says():
    b = A.t6_batch()
    plain, trimmed = run([ADD], b), run([ADD, TRIM], b)
    cut = [A.cuts(x, y) for x, y in zip(plain, trimmed)]
    assert all(len(A.ops_of(l)) > 32_768 for l in trimmed)
    assert cut[0] == (0, 0) and cut[1] == (0, 0)
    assert 0 < cut[2][0] < 16_384 and cut[2][1] == 0 and 0 < cut[3][0] < 16_384 and 0 < cut[3][1] < 16_384
    assert cut[4][0] > 16_384 + 1000 and cut[5][0] > 16_384 + 1000 and cut[5][1] > 16_384 + 1000

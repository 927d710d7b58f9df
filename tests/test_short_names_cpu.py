"""The inputs of tests/test_gpu_short_names.py, proven sharp on the oracle alone (no GPU): the oracle shatters every record, behind
`invert` and `invert | trim` too, and the output rows reach every case of the short-A row writer -- every piece A length from 4 to 15
bytes, and first-16-bytes that span two, three, four and all five of A, `q0 \\t`, `q1`, B and `t0 \\t`."""
import oracle_lib as O
import short_name_cases as S

PIPES = ([O.SHATTER], [O.INVERT, O.SHATTER], [O.INVERT, O.TRIM_IDENTITY, O.SHATTER], [O.INVERT, O.INVERT, O.SHATTER])


def rows_of(lines, pipe):
    out, err = O.run([O.stage(k) for k in pipe], "".join(lines).encode())
    assert err.code == 0, (pipe, err.code, err.record)
    return out.splitlines()


def test_the_oracle_shatters_every_record():
    for name, make in S.ALL.items():
        lines = make()
        assert len(lines) == len(set(lines)) or name in ("deep_heads", "named_checked"), name
        for pipe in PIPES:
            rows = rows_of(lines, pipe)
            assert len(rows) >= (len(lines) if O.TRIM_IDENTITY not in pipe else 1), (name, pipe)
        # an identity trim in front leaves every record of the grid at least one row (the flat pass keeps no empty record)
        if name == "len_a_grid":
            out, err = O.run([O.stage(O.INVERT), O.stage(O.TRIM_IDENTITY)], "".join(lines).encode())
            assert err.code == 0 and all(b"cg:Z:" in l and l.split(b"cg:Z:")[1].strip() for l in out.splitlines()) and len(out.splitlines()) == len(lines)


def test_every_head_shape_occurs():
    seen_len_a, seen_pieces, by_len_a = set(), set(), {}
    for make in S.ALL.values():
        lines = make()
        for pipe in PIPES[:2]:
            for row in rows_of(lines, pipe):
                len_a, n = S.head_pieces(row)
                if len_a < 16:
                    seen_len_a.add(len_a)
                    seen_pieces.add(n)
                    by_len_a.setdefault(len_a, set()).add(n)
    assert seen_len_a == set(range(4, 16)), sorted(seen_len_a)
    assert seen_pieces == {2, 3, 4, 5}, sorted(seen_pieces)
    assert by_len_a[15] == {2} and 5 in by_len_a[4]  # chr1's head is A and one digit; q/9 reaches t0


def test_the_grid_crosses_the_gate_both_ways():
    """piece A of every length 4..17 on the query side and on the target side, and records on all four sides of the 16-byte gate"""
    lines = S.len_a_grid()
    q = {S.piece_a_len(l) for l in lines}
    t = {S.piece_a_len(l, inverted=True) for l in lines}
    assert q == set(range(4, 18)) and t == set(range(4, 18))
    assert {(S.piece_a_len(l) < 16, S.piece_a_len(l, True) < 16) for l in lines} == {(a, b) for a in (False, True) for b in (False, True)}
    ops = {sum(l.split("cg:Z:")[1].count(c) for c in "MID") for l in lines if 6 <= S.piece_a_len(l) and 6 <= S.piece_a_len(l, True)}
    assert ops == set(S.OP_COUNTS), sorted(ops)


def test_two_rows_in_a_lane_has_pairs_at_even_places():
    import re

    n_pairs = 0
    for l in S.two_rows_in_a_lane():
        letters = re.sub(r"[0-9]", "", l.split("cg:Z:")[1].strip())
        n_pairs += sum(1 for k in range(0, len(letters) - 1, 2) if letters[k: k + 2] == "MM")
    assert n_pairs > 100

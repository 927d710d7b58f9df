"""The inputs of test_gpu_flat_fixed_pipe.py (fixed_pipe_lib) hit their cases: shown on the oracle alone. For each record the op either cut
of the fixed trim stopped in, and by how much, is derived from the oracle's output; so is whether the identity trim behind it removed
the shortened op; and the output changes when the decisive length or threshold moves by one.

One case the cases of an identity trim behind a fixed trim cannot have: "the trim removes nothing, but would if the first op had its uncut
length". With an M (or =) op first, a longer first op raises the identity of every prefix and makes every cumulative length reach
max_trim sooner: the hits of the scan (impl/paf.c:820-838) with the uncut length are a subset of those with the cut one. With an X op
first the prefix of that op alone has identity 0 and is a hit whatever its length: the trim never removes nothing. What can be had, and is
here: a shortened X op that goes alone, where with its uncut length a second hit further on would take more ops with it
(x_op_stays_short_of_a_second_hit)."""
import pytest

import fixed_pipe_lib as L
import float_edges as E
import oracle_lib as O


def fixed_out(line, frac):
    return L.run1(L.FIX, line, frac)


@pytest.mark.parametrize("frac", sorted({f for _, f in L.LANDINGS.values()}))
def test_where_the_cuts_land(frac):
    keys, lines = L.landing_batch(frac)
    seen = {}
    for (name, strand), line in zip(keys, lines):
        line = line.encode()
        ops = L.ops_of(line)
        out = fixed_out(line, frac)
        f, s0, b, s1 = L.fixed_cuts(line, out)
        left = L.ops_of(out)
        end = L.end_of(ops, frac)
        seen[name] = (f, s0, b, s1, len(left))
        # each cut took `end` aligned bases: the ops in front of the one it stopped in and s0 / s1 of that op
        assert L.aligned(ops[:f]) + s0 == end and L.aligned(ops[len(ops) - b:]) + s1 == end, (name, f, s0, b, s1, end)
        if name == "inside_first_and_last":
            assert (f, b) == (0, 0) and s0 == s1 == 100
        elif name.startswith("on_boundary"):
            assert (f, b, s0, s1) == (2, 2, 0, 0) and ops[1][1] in "ID" and ops[-2][1] in "ID"  # the op and the indel behind it went, the next op is whole
        elif name == "one_op_record":
            assert (f, b, len(ops)) == (0, 0, 1) and s0 == s1 == 100 and left == [(1800, "M")]
        elif name == "both_cuts_in_one_op":
            assert (f, b) == (2, 2) and s0 == s1 == 60 and left == [(1800, "M")]
        elif name == "digits_1000_to_999_and_10_to_9":
            assert end == 1 and left[0] == (999, "M") and left[-1] == (9, "M")
        elif name == "digits_1099_to_999_and_109_to_9":
            assert left[0] == (999, "M") and left[-1] == (9, "M")
        elif name == "digits_10_to_9_twice":
            assert end == 1 and left[0] == (9, "M") and left[-1] == (9, "M")
        elif name.startswith("middle_"):
            k = int(name.split("_")[1])
            assert (f, b) == (0, 0) and s0 and s1 and sum(len(str(n)) + 1 for n, _ in left[1:-1]) == k
        # one base more in the op a cut stopped in: that op's number in the output moves
        if s0:
            longer = L.with_end_op(line, 0, ops[0][0] + 1) if f == 0 else None
            if longer:
                assert L.ops_of(fixed_out(longer, frac))[0][0] != left[0][0] or L.end_of(L.ops_of(longer), frac) != end
    assert {k for k, _ in keys} == set(seen)


def test_a_second_fixed_trim():
    keys, lines = L.second_batch()
    for (name, strand), line in zip(keys, lines):
        line = line.encode()
        ops = L.ops_of(line)
        one = fixed_out(line, 0.1)
        f, s0, b, s1 = L.fixed_cuts(line, one)
        first_left = L.ops_of(one)
        two = fixed_out(one, 0.1)
        f2, t0, b2, t1 = L.fixed_cuts(one, two)
        end2 = L.end_of(first_left, 0.1)
        assert (f, b) == (0, 0) and s0 == s1 == 100 and end2 == 90, (name, f, s0, b, s1, end2)
        if name == "ends_inside_the_shortened_op":
            assert (f2, b2, t0, t1) == (0, 0, 90, 90) and L.ops_of(two)[0] == (810, "M")
        elif name.startswith("consumes_it_exactly"):
            assert first_left[0][0] == 90 and (f2, b2, t0, t1) == (2, 2, 0, 0)  # the op and the indel behind it; the next op whole
        elif name == "stops_in_the_next_match_op":
            assert first_left[0][0] == 50 and (f2, b2, t0, t1) == (2, 2, 40, 40)
        # decisive by one: a first op one base longer changes what the second trim leaves of it
        longer = L.with_end_op(L.with_end_op(line, 0, ops[0][0] + 1), -1, ops[-1][0] + 1)
        other = L.ops_of(fixed_out(fixed_out(longer, 0.1), 0.1))
        assert other != L.ops_of(two)
        # the pipes of the GPU test give what the two runs give (an invert between them turns the record twice or once)
        want, err = O.run(L.oracle_stages(L.PIPES["fix_fix"], 0.1), line)
        assert err.code == 0 and want == two


@pytest.mark.parametrize("frac", L.TRIM_FRACTIONS)
def test_identity_trim_behind_a_fixed_trim(frac):
    keys, lines = L.trim_batch(frac)
    hit = set()
    for (name, strand), line in zip(keys, lines):
        line = line.encode()
        ops = L.ops_of(line)
        one = fixed_out(line, frac)
        f, s0, b, s1 = L.fixed_cuts(line, one)
        assert (f, b) == (0, 0) and s0 > 0 and s1 > 0, (name, f, s0, b, s1)  # both end ops are shortened, none removed
        two = L.run1(L.TRI, one)
        cf, cb = L.stretch_cuts(one, two)
        back = name.startswith("back_")
        # the end under test, as the text has it; the other end keeps its shortened op
        mine, other = (cb, cf) if back else (cf, cb)
        if back and strand == "+":
            # paf_invert does not turn a '+' record: its second pass scans the front again, the back is never looked at
            assert cb == 0
            continue
        assert other == 0, (name, strand, cf, cb)
        # the same trim when the op at that end has its uncut length
        uncut = L.with_end_op(one, -1 if back else 0, ops[-1 if back else 0][0])
        uf, ub = L.stretch_cuts(uncut, L.run1(L.TRI, uncut))
        umine = ub if back else uf
        base = name[5:] if back else name
        if base == "removes_the_shortened_op_and_more":
            assert mine > 1
        elif base == "removes_only_because_of_the_cut":
            assert mine >= 1 and umine == 0
        elif base == "x_op_stays_short_of_a_second_hit":
            assert mine == 1 and umine > 1
        hit.add((base, back))
        # and the pipe gives what the two runs give
        want, err = O.run(L.oracle_stages(L.PIPES["fix_trim"], frac), line)
        assert err.code == 0 and want == two
    assert len(hit) == len({n for n, _ in keys})  # every case of the batch, at the front and at the back


@pytest.mark.parametrize("name", sorted(L.TIES))
def test_filter_ties_behind_the_trim(name):
    thr, (m, x) = L.tie_thresholds(name)
    lines = [ln.encode() for ln in L.tie_batch(name)]
    raw_m, raw_x = L.window_sums(lines[0])
    assert x > 0 and (m, x) != (raw_m, raw_x)
    f, s0, b, s1 = L.fixed_cuts(lines[0], fixed_out(lines[0], 0.1))
    ops = L.ops_of(lines[0])
    assert "X" in (ops[f][1], ops[len(ops) - 1 - b][1]) and (s0 if ops[f][1] == "X" else s1) > 0  # an X op is shortened
    kept = {}
    for u, t in thr:
        for inv in (False, True):
            with L.Thresholds(min_identity=t, invert=inv):
                out, err = O.run(L.oracle_stages(L.PIPES["fix_filter"], 0.1), b"".join(lines))
            assert err.code == 0
            kept[(u, inv)] = out.count(b"\n")
    # on the tie and below it the records stay, one step above they go; inverted the other way round
    assert kept == {(-1, False): 2, (0, False): 2, (1, False): 0, (-1, True): 0, (0, True): 0, (1, True): 2}
    # the uncut record's identity is on the other side of one of the thresholds: sums that forget the cuts decide otherwise
    raw = float(E.quot(raw_m, raw_m + raw_x))
    assert any((raw >= t) != (float(E.quot(m, m + x)) >= t) for _, t in thr) or raw > thr[2][1] or raw < thr[0][1]
    assert raw > thr[2][1] or raw < thr[0][1]


def test_who_leaves_inputs():
    for ln in L.even_batch().splitlines():
        assert L.aligned(L.ops_of(ln)) % 2 == 0
    out, err = O.run(L.oracle_stages(L.PIPES["fix_invert"], 1.0), L.even_batch())
    print("fixed trim of 1.0 on an even record: oracle error", err.code, err.record, len(out))
    data, n = L.nonplain_batch()
    assert sum(1 for ln in data.splitlines() if set(c for _, c in L.ops_of(ln)) & set("=X")) == n
    assert sum(1 for ln in L.irregular_batch().splitlines() if any(n >= 8192 for n, _ in L.ops_of(ln))) == 1

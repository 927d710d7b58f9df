"""Every family of float_edges.py is SHARP on the oracle: the record one float32 step on the wrong side of a threshold comes out
differently from the record on the threshold, in the way its construction says, and the records on and above it agree. This is what keeps
test_gpu_float_edges.py from passing vacuously -- a comparison that went the wrong way at equality, a band or a pruning margin a hair too
tight, or a conversion that truncates where the reference rounds would change one of these outputs. No GPU; no case is skipped or
filtered at run time."""
import itertools
import re
from fractions import Fraction

import numpy as np
import pytest

import float_edges as E
import oracle_lib as O
from test_gpu_flat import cigar_of, n_ops_of


def ops_cut(batch, params):
    """ops the oracle's identity trim takes off every record of the batch"""
    out, err = O.run([O.stage(O.TRIM_IDENTITY, *params)], batch.data())
    lines = out.splitlines()
    assert err.code == 0 and len(lines) == len(batch.lines)
    return [n_ops_of(cigar_of(src.encode())) - n_ops_of(cigar_of(got)) for src, got in zip(batch.lines, lines)]


@pytest.mark.parametrize("name", sorted(E.TRIM_SETS))
def test_identity_trim_sets_are_sharp(name):
    """q < thr: one step (or 3e-6 to 5e-6) below the threshold the whole prefix up to the probe goes; on it and above it nothing goes, or
    the two ops of the early hit in front of it (the LAST hit wins). q >= id: on the identity and above it the junk alone goes, one step
    below it the whole probe. max_trim: a hit that ends on max_trim goes, one base further on nothing does."""
    batch, cut, params, who = E.trim_set(name)
    got = ops_cut(batch, params)
    assert got == cut
    assert len(set(cut)) >= 2 and max(cut) > 2  # both outcomes are in the set
    pieces = E.pieces_of(batch)
    lo, hi = {"lane": (1, 12), "regs": (13, 64), "hbm": (65, 1 << 20)}.get(who, (1, 1 << 20))
    assert lo <= min(pieces) and max(pieces) <= hi, (who, min(pieces), max(pieces))
    assert max(len(ln) for ln in batch.lines) < 110_000
    if who in ("flat", "lane", "regs", "hbm"):  # which flat kernel is to take each record is decidable from its shape
        lane = E.sized_by_lane(batch, cut)
        assert (who != "lane" or all(lane)) and (who not in ("regs", "hbm") or not any(lane))


def test_probes_are_where_they_claim():
    """near() and near_rel() against the float32 expressions, the pairs that round, and the probes' places in the pieces"""
    thr_f, id_f, max_trim = E.thresholds(E.M0, E.X0, 0.05, 1.0)
    assert float(thr_f) == pytest.approx(0.9313725, abs=1e-7) and max_trim == E.M0 + E.X0
    assert E.quot(95, 102) == thr_f and E.quot(79352, 79352 + 5847) == E.step(thr_f, -1) and E.quot(143423, 143423 + 10568) == E.step(thr_f, 1)
    for u in (-1, 0, 1):
        a, b = E.near(thr_f, u, 140_000, 200_000)
        assert E.quot(a, a + b) == E.step(thr_f, u)
    for rel in (-5e-6, -4e-6, -3e-6, 3e-6, 4e-6, 5e-6):
        a, b = E.near_rel(thr_f, rel, 140_000, 200_000)
        assert abs(float(E.quot(a, a + b)) / float(thr_f) - 1.0 - rel) < 2e-7
    # above 2^24: the float quotient ties (or is a step below) while the exact fraction is on either side of the threshold
    t24, _, _ = E.thresholds(40_000_000, 1_500_000, 0.05, 1.0)
    for u, exact in ((0, "below"), (0, "above"), (-1, "below"), (-1, "above")):
        a, b = E.near(t24, u, rounds=True, exact=exact, lo_den=E.TWO24 + 1, hi_den=E.TWO24 + 20_000)
        assert (a > E.TWO24 and a & 1) or (a + b) & 1
        assert (Fraction(a, a + b) < Fraction(float(t24))) == (exact == "below") and E.quot(a, a + b) == E.step(t24, u)
    # the places: the probe's letter on the last byte of the record's second piece, one byte into its third
    batch, cut, _, _ = E.trim_set("lt")
    at, seen, ops_in_piece, run_in_piece = 0, set(), [], []
    for line, c, where in zip(batch.lines, cut, batch.where):
        cg = at + line.index("cg:Z:") + 5
        if c > 2 and "\t+\t" in line:  # un-mirrored: the probe is the c-th op of the text
            ops = list(re.finditer(r"\d+[MID]", line[line.index("cg:Z:") + 5:]))
            m = ops[c - 1]
            letter = cg + m.end() - 1
            seen.add(((letter >> 10) - (cg >> 10), letter & 1023))
            if where == "drun1":  # in front of the probe, in its own piece: 64 ops and more, the last 99 of them the D run
                mine = [x for x in ops[:c - 1] if (cg + x.end() - 1) >> 10 == letter >> 10]
                ops_in_piece.append(len(mine))
                run_in_piece.append(sum(1 for _ in itertools.takewhile(lambda x: x.group().endswith("D"), reversed(mine))))
        at += len(line)
    assert {(1, 1023), (2, 1), (1, 760), (3, 300)} <= seen, sorted(seen)
    assert min(run_in_piece) >= 99 and min(ops_in_piece) >= 64, (min(run_in_piece), min(ops_in_piece))


def test_fixed_trim_above_2_24():
    """end = (int64)((double)((float)aligned * fraction) / 2): the oracle cuts what the float32 product says; where the product taken in
    double or a truncated conversion says otherwise (2^24 + 3 under every fraction; 10^8 + 1 under 0.3 and 0.7) the outputs would
    differ by two aligned bases"""
    separated = set()
    for aligned in E.FIXED_ALIGNED:
        for frac in E.FIXED_FRACTIONS:
            ref, in_double, truncated = E.fixed_end(aligned, frac)
            for strand in "+-":
                line = E.line_of(E.fixed_ops(aligned), strand)
                out, err = O.run([O.stage(O.TRIM_FIXED, 0.05, frac)], line.encode())
                assert err.code == 0
                left = sum(int(n) for n in re.findall(rb"(\d+)M", cigar_of(out)))
                assert left == aligned - 2 * ref, (aligned, frac, left)
            if ref != in_double:
                separated.add((aligned, frac, "double"))
            if ref != truncated:
                separated.add((aligned, frac, "truncated"))
    assert {(E.TWO24 + 3, f, how) for f in E.FIXED_FRACTIONS for how in ("double", "truncated")} <= separated
    assert {(10 ** 8 + 1, 0.3, "double"), (10 ** 8 + 1, 0.7, "double")} <= separated


def kept_names(out):
    return {ln.split(b"\t")[0].decode() for ln in out.splitlines()}


def test_filter_thresholds():
    """(double)(float)(k / 10) against the double k / 10: 0.1 and 0.3 pass, 0.7 and 0.9 fail, 0.5 is exact; thresholds set to the float32
    quotient itself (kept) and to the next double above it (dropped), sums above 2^24; a record of I ops alone fails every threshold"""
    try:
        for wide in (False, True):
            cases = E.filter_lines(E.TENTHS, wide)
            only_i = E.record(E.ONLY_INSERTS, qname="only_i")
            data = "".join(c[0] for c in cases).encode() + only_i.encode()
            for k in range(1, 10):
                want = {c[0].split("\t")[0] for c in cases if E.filter_keeps(c[1][0], c[1][1], k / 10)}
                for inv in (False, True):
                    O.set_filter(min_identity=k / 10, min_identity_with_gaps=k / 10, invert=inv)
                    out, err = O.run([O.stage(O.FILTER)], data)
                    assert err.code == 0
                    everyone = {c[0].split("\t")[0] for c in cases} | {"only_i"}
                    assert kept_names(out) == ((everyone - want) if inv else want), (k, inv)
            passing = {k for k in range(1, 10) if E.filter_keeps(k, 10 - k, k / 10)}
            assert {1, 3, 5} <= passing and not {7, 9} & passing
            big = E.filter_lines(E.FILTER_BIG, wide)
            bdata = "".join(c[0] for c in big).encode()
            for m, x in E.FILTER_BIG:
                t0 = float(E.quot(m, m + x))
                mine = {c[0].split("\t")[0] for c in big if c[1] == (m, x)}
                for thr, there in ((t0, True), (float(np.nextafter(t0, 2.0)), False)):
                    O.set_filter(min_identity=thr, min_identity_with_gaps=thr)
                    out, err = O.run([O.stage(O.FILTER)], bdata)
                    assert err.code == 0 and (mine <= kept_names(out)) == there and (there or not mine & kept_names(out)), (m, x, thr)
    finally:
        O.set_filter()


def test_chain_trim_decides_by_one_base():
    """Of the three pairs of every length only the one whose B starts exactly on A's trimmed end chains (s1 150 on both lines): the trim
    is the oracle's (int64)((float)length * trim) / 2. Where the product in double or a truncated conversion gives another trim (2^24 + 3
    and 10^9 + 1 under 0.3 and 0.7) that pair would miss."""
    separated = set()
    for trim in E.CHAIN_TRIMS:
        for strand in "+-":
            data, pairs = E.chain_lines(trim, strand)
            out, err, fresh = O.chain(data, trim=trim)
            assert err.code == 0 and fresh == 0
            s1 = {}
            for ln in out.splitlines():
                s1.setdefault(ln.split(b"\t")[0].decode(), []).append(int(re.search(rb"s1:i:(\d+)", ln).group(1)))
            for i, length in enumerate(E.CHAIN_LENGTHS):
                assert sorted(s1["q%d_1" % i]) == [150, 150] and sorted(s1["q%d_0" % i]) == [50, 100] and sorted(s1["q%d_2" % i]) == [50, 100], (trim, strand, length)
        for length in E.CHAIN_LENGTHS:
            ref, in_double, truncated = E.chain_trim(length, trim)
            separated |= {(length, trim, how) for how, v in (("double", in_double), ("truncated", truncated)) if v != ref}
    assert {(E.TWO24 + 3, f, how) for f in E.CHAIN_TRIMS for how in ("double", "truncated")} <= separated
    assert {(10 ** 9 + 1, 0.3, "double"), (10 ** 9 + 1, 0.7, "double")} <= separated


def test_view_ratios_above_2_24():
    """the two %f fields of the view for match and total sums above 2^24 and odd: the oracle prints the float32 quotient's six decimals;
    for VIEW_SHARP they differ from the decimals of the quotient in double and of truncated conversions"""
    for line, ident, gaps in E.view_lines():
        rc, text = O.pretty_print(line, b"", b"", False)
        assert rc == 0
        m = re.search(rb"\tIdentity:([^\t]+)\tIdentity-with-gaps([^\t]+)\t", text)
        assert (m.group(1).decode(), m.group(2).decode()) == (ident, gaps), line[:60]
    for m, x in E.VIEW_SHARP:
        assert E.view_text_of(m, m + x) not in E.view_near_misses(m, m + x)

"""Shatter records whose first constant row piece, `qname \\t qlen \\t` (piece A), is shorter than 16 bytes -- chr1, 2L, q -- for
tests/test_short_names_cpu.py (the oracle alone: the inputs are sharp) and tests/test_gpu_short_names.py (k_emit_rows_short against the
oracle). A row is `A | q0 \\t | q1 | B | t0 \\t | t1 \\t L \\t L | C | L M \\n` with B = `\\t strand \\t tname \\t tlen \\t`; the row writer
composes the first 16 bytes of such a row from the first two to five of these pieces."""
import random

OP_COUNTS = (1, 2, 3, 64, 127, 128, 129, 257, 300)  # a window of the row writer is 128 ops, two per lane


def record(ops, strand="+", qname="chr1", tname="chr2", qlen=248_956_422, tlen=242_193_529, qs=1000, ts=2000, tags="tp:A:P\tAS:i:777\ts1:i:42"):
    """ops: list of (length, letter); the coordinates are consistent with them"""
    qspan = sum(L for L, c in ops if c in "MI")
    tspan = sum(L for L, c in ops if c in "MD")
    assert 0 <= qs and qs + qspan <= qlen and 0 <= ts and ts + tspan <= tlen, (qname, qlen, qs, qspan, tname, tlen, ts, tspan)
    text = "".join(f"{L}{c}" for L, c in ops)
    cols = [qname, str(qlen), str(qs), str(qs + qspan), strand, tname, str(tlen), str(ts), str(ts + tspan), str(qspan), str(qspan + tspan), "60"]
    return "\t".join(cols + ([tags] if tags else []) + ["cg:Z:" + text]) + "\n"


def spans(ops):
    return sum(L for L, c in ops if c in "MI"), sum(L for L, c in ops if c in "MD")


def alternating_ops(rng, n, lens, indel=(1,)):
    """n ops, M at the even places, I / D in turn at the odd ones (no two M ops side by side)"""
    return [(rng.choice(lens), "M") if k % 2 == 0 else (rng.choice(indel), "ID"[(k // 2) & 1]) for k in range(n)]


def side_of_len_a(len_a):
    """(name, sequence length) whose piece A has len_a bytes: as many digits as fit (nine at most), the rest name; the length is all
    nines, so that every coordinate of that many digits is valid"""
    digits = min(len_a - 3, 9)
    name = "chr1XYZab"[: len_a - 2 - digits] if len_a - 2 - digits > 1 else "q"
    assert len(name) + 2 + digits == len_a
    return name, 10 ** digits - 1


def len_a_grid():
    """Every piece A length 4..17 on the query side paired with every one on the target side once per residue (a permutation per strand, so
    an invert moves records across the 16-byte gate in both directions), both strands, every op count that fits the sequence lengths.
    The starts lie near the sequences' ends: few powers of ten inside a record's ranges (the flat pass keeps at most six)."""
    rng = random.Random(2301)
    lines = []
    for si, strand in enumerate("+-"):
        for lq in range(4, 18):
            lt = 4 + (5 * (lq - 4) + 3 + 6 * si) % 14
            (qn, qlen), (tn, tlen) = side_of_len_a(lq), side_of_len_a(lt)
            for n in OP_COUNTS:
                room = min(qlen, tlen)
                lens = (1,) if room < 1000 else (1, 2, 3) if room < 100_000 else (1, 2, 3, 7, 12, 40, 99, 150, 1234)
                ops = alternating_ops(rng, n, lens)
                qspan, tspan = spans(ops)
                if qspan > qlen or tspan > tlen:
                    continue  # a sequence of one or two digits holds the short records only
                qs, ts = qlen - qspan - rng.randrange(min(3, qlen - qspan + 1)), tlen - tspan - rng.randrange(min(3, tlen - tspan + 1))
                lines.append(record(ops, strand, qn, "t" + tn[1:] if tn != "q" else "t", qlen, tlen, qs, ts))
    return lines


def deep_heads():
    """Heads that reach into B and t0 -- names of one and two characters with one-digit lengths, coordinates from 0 --, coordinates that
    gain a digit inside a window (9 -> 10, 99 -> 100, 9 999 -> 10 000), windows whose bases span 20 000 and more (M ops of 4 000 to 8 191:
    the far formatting) and M lengths of 100 and more (no window of short lengths only)."""
    rng = random.Random(2302)
    lines = []
    for strand in "+-":
        for qn, tn in (("q", "t"), ("ab", "t"), ("q", "cd"), ("2L", "3R")):
            for ops in ([(1, "M")], [(9, "M")], [(2, "M"), (1, "I"), (3, "M")], [(1, "M"), (1, "D"), (1, "M"), (1, "I"), (1, "M"), (1, "D"), (2, "M")]):
                qspan, tspan = spans(ops)
                lines.append(record(ops, strand, qn, tn, 9, 9, 0, 0, tags=""))
                lines.append(record(ops, strand, qn, tn, 9, 9, 9 - qspan, 9 - tspan, tags="tp:A:S"))
        # a digit more inside a window: the rows start below 10, 100 and 10 000 and end above
        for qn, tn, start, lens in (("q", "t", 0, (1, 2)), ("q", "t", 3, (1,)), ("X", "2L", 80, (1, 2, 3)), ("ab", "Y", 9_900, (1, 7, 12)), ("q", "chr1", 9_990, (1, 2)),
                                    ("q", "t", 0, (100, 150, 999)), ("2L", "q", 95, (100, 1234))):
            for n in (3, 40, 129):
                ops = alternating_ops(rng, n, lens)
                qspan, tspan = spans(ops)
                qlen, tlen = max(start + qspan, 9), max(start + tspan + 5, 9)
                lines.append(record(ops, strand, qn, tn, qlen, tlen, start if strand == "+" else qlen - qspan, start))
        # far windows: 128 ops of thousands of bases each span far more than 20 000
        for qn, tn, qs in (("q", "t", 0), ("chr1", "chrX", 9_000), ("2L", "q", 99_000), ("ab", "hs.chr10", 5)):
            ops = alternating_ops(rng, 140, (4000, 5555, 8191, 100, 7), indel=(1, 4000))
            qspan, tspan = spans(ops)
            lines.append(record(ops, strand, qn, tn, qs + qspan + 1, 7 + tspan, qs, 7))
    return lines


def two_rows_in_a_lane():
    """Cigars with M ops side by side (2M3M1I4M5M...): a lane of the row writer holds two ops, so some lanes write two rows and the second
    row's head is repaired on its own. Pairs at even and at odd places, with short and with long names."""
    rng = random.Random(2303)
    lines = []
    for strand in "+-":
        for qn, tn, qlen in (("q", "t", 999), ("chr1", "chr2", 248_956_422), ("2L", "hs.chr10", 23_513_712), ("hs.chr10", "X", 9_999)):
            for n in (2, 3, 4, 64, 129, 300, 301):
                lens = (1,) if qlen < 1000 else (1, 2, 3, 9, 150)
                ops = []
                while len(ops) < n:  # pairs of M ops, an indel behind some of them: the pairs fall on even and on odd places
                    ops += [(rng.choice(lens), "M"), (rng.choice(lens), "M")]
                    if rng.random() < 0.4:
                        ops.append((1, "ID"[len(ops) & 1]))
                ops = ops[:n]
                if ops[-1][1] != "M":
                    ops[-1] = (1, "M")
                qspan, tspan = spans(ops)
                lines.append(record(ops, strand, qn, tn, qlen, max(qlen, tspan + 9), 7, 9))
    return lines


def one_long_op():
    """a short-named record the flat pass leaves to the record kernels (an op of 8 192 bases), beside one it keeps"""
    return [record([(5, "M"), (2, "I"), (8192, "M"), (1, "D"), (7, "M")], "+", "chr1", "chr2", qs=1000, ts=2000),
            record([(5, "M"), (2, "I"), (8191, "M"), (1, "D"), (7, "M")], "-", "chrX", "chr1", 156_040_895, 248_956_422, 1000, 2000),
            record([(8192, "M")], "-", "q", "t", 9000, 9000, 3, 5)]


def neighbours():
    """short- and long-named records in turn: k_emit_rows_short and k_emit_rows write adjacent stretches of the output"""
    rng = random.Random(2305)
    lines = []
    for k in range(120):
        names = (("chr1", "chr2"), ("hs.chr3", "pt.chr9"), ("chrX", "hs.chr3"), ("hs.chr10", "2L"))[k & 3]
        ops = alternating_ops(rng, rng.choice((1, 3, 40, 128, 200)), (1, 2, 3, 7, 12, 40, 99, 150, 1234), indel=(1, 2, 3, 9, 25))
        lines.append(record(ops, "+-"[(k >> 2) & 1], names[0], names[1], 250_000_000, 240_000_000, 120_000_000 + 1000 * k, 110_000_000 + 999 * k))
    return lines


def named_checked():
    """the records the issue names: q/9, q/5000, chr1/248956422, chrX/156040895, ab/99999999999, 2L/23513712, both strands"""
    lines = []
    for strand in "+-":
        for qn, qlen in (("q", 9), ("q", 5000), ("chr1", 248_956_422), ("chrX", 156_040_895), ("ab", 99_999_999_999), ("2L", 23_513_712)):
            ops = [(2, "M"), (1, "I"), (1, "M"), (1, "D"), (3, "M")]
            lines.append(record(ops, strand, qn, "chr2", qlen, 242_193_529, qlen - 7, 1_000_000))
    return lines


ALL = {"len_a_grid": len_a_grid, "deep_heads": deep_heads, "two_rows_in_a_lane": two_rows_in_a_lane, "one_long_op": one_long_op, "neighbours": neighbours,
       "named_checked": named_checked}


def piece_a_len(line, inverted=False):
    """bytes of piece A as the row writer sees it: the query side, or the target side behind an odd number of inverts"""
    c = line.split("\t")
    return len(c[5]) + len(c[6]) + 2 if inverted else len(c[0]) + len(c[1]) + 2


def head_pieces(row):
    """(length of piece A, how many of A, q0 \\t, q1, B, t0 \\t the first 16 bytes of an output row span)"""
    c = row.split(b"\t")
    lens = [len(c[0]) + len(c[1]) + 2, len(c[2]) + 1, len(c[3]), len(c[4]) + len(c[5]) + len(c[6]) + 4, len(c[7]) + 1]
    at, n = 0, 0
    for ln in lens:
        if at < 16:
            n += 1
        at += ln
    assert at >= 16, row  # the five pieces always fill the head
    return lens[0], n

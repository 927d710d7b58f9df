"""The op loop of k_flat_parse (paffy_amd/csrc/flat_kernel.h) at its edges, against the oracle: every letter at every byte of a 16-byte
lane chunk behind numbers of one to four digits, numbers whose digits lie on both sides of a lane (16 B), tile (1 KiB) and chunk (four
tiles from the record's first) boundary, each irregular form alone at such a boundary (the record goes to the record kernels and the
bytes stay the oracle's), = and X ops at the same places, the densest tiles (512, 511 and 510 letters) and the largest sums a tile can
hold, and the kernel's other two instantiations (a stats stage, add_mismatches) over the same cigars. A few hundred short records."""
import random
import re

import pytest

import oracle_lib as O
from test_gpu_flat import LEAN_PIPES, STATS, record, run_both

pytestmark = pytest.mark.gpu

LENS = (1, 9, 10, 99, 100, 999, 1000, 8191)
QS, TS = 120_000_000, 110_000_000  # no coordinate of a record crosses a power of ten: the rows of a record keep their digit counts
ANCHOR = [(8000, "M")] * 16        # enough matches behind the ops under test for the identity trim to keep the record
WHY_IRREG = 1                      # FLAT_WHY_IRREG of flat_kernel.h
TILE = 1024


def text_of(ops):
    return "".join(f"{L}{c}" for L, c in ops)


def every_length():
    """L M / 1 I / L D for every L: M, I and D behind one to four digits"""
    ops = []
    for L in LENS:
        ops += [(L, "M"), (1, "I"), (L, "D")]
    return ops


def lane_edge(cg):
    return (cg + 15) // 16 * 16


def tile_edge(cg):
    return (cg // TILE + 1) * TILE


def chunk_edge(cg):
    return (cg // TILE + 4) * TILE


PLACED = []  # stream offset of the tail's first byte, of every record placed() has made


def placed(base, edge, split, tail, strand, by_name_only=False, anchor=ANCHOR, **kw):
    """A record for stream offset `base` in which `split` bytes of the tail's text lie in front of edge(offset of the cigar's first byte)
    and the rest behind it: the name grows by up to 15 characters (by_name_only), or `1M` ops go in front of the tail and the name grows
    by a character where the distance is odd. Returns the line."""
    n, pad = 0, 0
    kw.setdefault("qs", QS)
    kw.setdefault("ts", TS)
    for _ in range(12):
        line = record([(1, "M")] * n + tail + anchor, strand, qname="hs.chr3" + "x" * pad, **kw)
        cg = base + line.index("cg:Z:") + 5
        d = edge(cg) - (cg + 2 * n + split)
        if by_name_only:
            d %= 16
        if d == 0:
            PLACED.append(cg + 2 * n)
            return line
        if by_name_only:
            pad += d
        elif 2 * n + pad + d < 0:  # too close to the boundary: a few bytes further, the next one
            pad += 8
        else:
            n, pad = (2 * n + pad + d) // 2, (2 * n + pad + d) % 2
    raise AssertionError("no placement")


def stream(make):
    """make(base) -> line, for every entry; the lines in stream order"""
    lines, base = [], 0
    for m in make:
        lines.append(m(base))
        base += len(lines[-1])
    return lines


def cigar_starts(lines):
    out, base = [], 0
    for l in lines:
        out.append(base + l.index("cg:Z:") + 5)
        base += len(l)
    return out


def alignment_lines():
    """the cigar's first byte at every offset of a lane chunk; numbers split 1|3, 2|2, 3|1 by a lane, a tile and a chunk boundary"""
    make = []
    for off in range(16):
        for strand in "+-":
            make.append(lambda base, off=off, strand=strand: placed(base, lambda cg, off=off: lane_edge(cg - off) + off, 0, every_length(), strand, by_name_only=True))
    four = {"M": [(8191, "M"), (1, "I"), (1000, "D")] + every_length(), "D": [(1000, "D"), (1, "I"), (8191, "M")] + every_length()}
    for edge in (lane_edge, tile_edge, chunk_edge):
        for split in (1, 2, 3):
            for strand in "+-":
                for first in "MD":
                    make.append(lambda base, e=edge, s=split, st=strand, f=first: placed(base, e, s, four[f], st, by_name_only=e is lane_edge))
    return stream(make)


def test_every_alignment_and_split(eng_edges):
    del PLACED[:]
    lines = alignment_lines()
    starts, first_bytes = cigar_starts(lines), list(PLACED)
    assert {s % 16 for s in starts[:32:2]} == set(range(16)) and {s % 16 for s in starts[1:32:2]} == set(range(16))
    # every letter of L M / 1 I / L D has been at every byte of a lane chunk
    seen = set()
    for s, l in zip(starts[:32], lines[:32]):
        at = s
        for k, (L, c) in enumerate(every_length()):
            at += len(str(L))
            seen.add((k, at % 16))
            at += 1
    assert len(seen) == 16 * 3 * len(LENS)
    # the split numbers do lie across their boundaries
    k, data = 32, "".join(lines)
    for edge in (lane_edge, tile_edge, chunk_edge):
        for split in (1, 2, 3):
            for _ in range(4):
                at = first_bytes[k]
                assert data[at:at + 4] in ("8191", "1000") and not data[at - 1].isdigit() and (at + split) % (16 if edge is lane_edge else TILE) == 0
                assert edge is not chunk_edge or at + split == chunk_edge(starts[k])
                k += 1
    assert k == len(lines)
    run_both(eng_edges, "".join(lines).encode(), kept=True)


@pytest.fixture(scope="module")
def eng_edges():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


IRREGULAR = ("0M", "05M", "12345M", "8192M", "9999M", "5MM", "5N", "5S", "5m")


def irregular_line(base, edge, split, form, strand, where="middle"):
    """a regular record with one irregular form in it: `split` bytes of the form in front of the boundary"""
    head, tail = [(12, "M"), (3, "I")], [(7, "M"), (2, "D"), (30, "M")]
    if where == "first":   # directly behind cg:Z:
        text = form + text_of(tail) + text_of(ANCHOR)
    elif where == "last":  # the last bytes in front of the next line
        text = text_of(head) + text_of(ANCHOR) + form
    else:
        text = text_of(head) + form + text_of(tail) + text_of(ANCHOR)
    parsed = [(int(a) if a else 0, b) for a, b in re.findall(r"(\d*)([A-Za-z=])", text)]
    ops = [(L, c) for L, c in parsed if c in "MIDX="]
    at = text.index(form) if where != "last" else len(text) - len(form)
    n, pad = 0, 0
    for _ in range(12):
        front = [] if where == "first" else [(1, "M")] * n
        line = record(front + ops, strand, qname="hs.chr3" + "x" * pad, qs=QS, ts=TS, cigar=text_of(front) + text)
        cg = base + line.index("cg:Z:") + 5
        d = edge(cg) - (cg + 2 * n + at + split)
        if edge is lane_edge:
            d %= 16
        if d == 0:
            return line
        if where == "first":  # nothing may stand in front of the form: the name alone moves it
            assert edge is lane_edge
            pad += d
        elif 2 * n + pad + d < 0:
            pad += 8
        else:
            n, pad = (2 * n + pad + d) // 2, (2 * n + pad + d) % 2
    raise AssertionError("no placement")


def regular_line(base, strand="+"):
    return placed(base, lane_edge, 0, every_length(), strand, by_name_only=True)


IRREGULAR_PIPES = ([O.SHATTER], [O.INVERT, O.TRIM_IDENTITY, O.SHATTER], [O.INVERT], [O.TRIM_IDENTITY])


def check_left_alone(eng, lines, pipes=IRREGULAR_PIPES):
    """outputs and error codes are the oracle's; the one irregular record of the stream went to the record kernels"""
    data = "".join(lines).encode()
    run_both(eng, data, pipes=pipes)
    for pipe, (_, _, (left, why)) in zip(pipes, STATS[-len(pipes):]):
        assert left >= 1 and why[WHY_IRREG] >= 1, (pipe, left, list(why))
        _, err = O.run([O.stage(k) for k in pipe], data)
        if err.code == 0:
            assert left == 1 and why[WHY_IRREG] == 1, (pipe, left, list(why))


@pytest.mark.parametrize("form", IRREGULAR + ("5M7",))
def test_each_irregular_form_alone(eng_edges, form):
    """the form at a lane and at a tile boundary (its first byte behind the boundary, and one byte in front of it), one stream each"""
    where = "last" if form == "5M7" else "middle"  # a cigar that ends in digits
    for edge in (lane_edge, tile_edge):
        for split in (0, 1):
            for strand in "+-":
                lines = stream([regular_line, lambda b: irregular_line(b, edge, split, form, strand, where), regular_line])
                check_left_alone(eng_edges, lines)


def test_zero_behind_the_tag_and_in_front_of_the_next_line(eng_edges):
    """a '0' as the cigar's first byte (a lane's first and last byte; a tile's first byte: the record in front is as long as that takes)
    and as the last byte in front of the next line (a lane's and a tile's last and first byte)"""
    pipes = ([O.SHATTER], [O.INVERT], [O.TRIM_IDENTITY])
    for form in ("0M", "05M"):
        for split in (0, 15):
            lines = stream([regular_line, lambda b: irregular_line(b, lane_edge, (16 - split) % 16, form, "+", "first"), regular_line])
            assert cigar_starts(lines)[1] % 16 == split and lines[1].split("cg:Z:")[1][0] == "0"
            check_left_alone(eng_edges, lines, pipes=pipes)
        behind = irregular_line(0, lane_edge, 0, form, "-", "first")
        rel = behind.index("cg:Z:") + 5
        fill = every_length() + ANCHOR
        lines = stream([lambda b: placed(b, lambda cg: 2 * TILE - rel - len(text_of(fill)) - 1, 0, every_length(), "+"), lambda b: behind, regular_line])
        assert cigar_starts(lines)[1] == 2 * TILE
        check_left_alone(eng_edges, lines, pipes=pipes)
    for edge in (lane_edge, tile_edge):
        for form, split in (("5M0", 3), ("5M0", 2), ("0", 1), ("0", 0)):
            lines = stream([regular_line, lambda b: irregular_line(b, edge, split, form, "+", "last"), regular_line])
            assert lines[1].endswith("0\n")
            check_left_alone(eng_edges, lines, pipes=pipes)


def test_equal_and_x_ops_at_the_same_places(eng_edges):
    """= and X ops (FLAT_F_NONPLAIN): pipes that keep them stay with the flat pass, shatter goes the record kernels' way"""
    make = []
    tail = [(8191, "="), (1, "X"), (1000, "="), (25, "X"), (3, "I"), (999, "="), (7, "D"), (10, "X"), (5, "M")]
    for edge in (lane_edge, tile_edge, chunk_edge):
        for split in (0, 1, 2, 3, 4):
            for strand in "+-":
                make.append(lambda base, e=edge, s=split, st=strand: placed(base, e, s, tail, st, by_name_only=e is lane_edge))
        make.append(regular_line)
    lines = stream(make)
    data = "".join(lines).encode()
    run_both(eng_edges, data, pipes=([O.INVERT], [O.TRIM_IDENTITY], [O.INVERT, O.TRIM_IDENTITY]), kept=True)
    run_both(eng_edges, data, pipes=([O.SHATTER], [O.INVERT, O.TRIM_IDENTITY, O.SHATTER]))
    run_both(eng_edges, (regular_line(0) + lines[0] + regular_line(0, "-")).encode(), pipes=([O.SHATTER],))


def letters_per_tile(data, lo, hi):
    """op letters of the cigar text data[lo:hi] per 1 KiB tile of the stream"""
    out = {}
    for i in range(lo, hi):
        if data[i] in "MID=X":
            out[i // TILE] = out.get(i // TILE, 0) + 1
    return out


def test_the_densest_tiles(eng_edges):
    """1M1I x 256 from a tile's first byte: 512 letters in the tile; behind 10M and 1000M: 511 and 510. And tiles of 8191M8191D: 204
    ops whose bases add up to more than 16 bits hold (the lanes' 16-bit sums are widened before the wave adds them)."""
    dense = [(1, "M"), (1, "I")] * 256
    make = []
    for lead in ([], [(10, "M")], [(1000, "M")]):
        for strand in "+-":
            make.append(lambda base, lead=lead, strand=strand: placed(base, tile_edge, 0, lead + dense, strand))
    wide = [(8191, "M"), (8191, "D")] * 306
    make.append(lambda base: placed(base, tile_edge, 0, wide, "+", anchor=[(8191, "M")] * 2000))
    make.append(lambda base: placed(base, tile_edge, 3, wide, "-", anchor=[(8191, "M")] * 2000))
    lines = stream(make)
    data = "".join(lines)
    starts = cigar_starts(lines)
    for k, want in enumerate((512, 512, 511, 511, 510, 510)):
        per = letters_per_tile(data, starts[k], starts[k] + lines[k].index("\n") - lines[k].index("cg:Z:") - 5)
        assert per[tile_edge(starts[k]) // TILE] == want == max(per.values()), (k, want)
    per = letters_per_tile(data, starts[6], starts[6] + 3060)
    assert per[tile_edge(starts[6]) // TILE] == 204
    run_both(eng_edges, data.encode(), kept=True)


def test_stats_stage_over_the_same_cigars(eng_edges):
    """k_flat_parse<2> (the I ops counted): the six sums of paf_stats_calc over the alignment cigars, plain and behind an invert"""
    import paffy_amd

    data = "".join(alignment_lines()).encode()
    buf = eng_edges.to_device(data)
    for pipe in ([], [O.INVERT]):
        want, werr = O.run([O.stage(k) for k in pipe] or [O.stage(O.PASS)], data)
        assert werr.code == 0
        acc = [0] * 6
        for ln in want.splitlines():
            acc = O.cigar_stats(ln.split(b"cg:Z:")[1].split(b"\t")[0].decode(), acc, zero=False)
        info = eng_edges.plan([paffy_amd.stage(k) for k in pipe] + [paffy_amd.stage(paffy_amd.STATS)], buf, len(data))
        assert info.error.code == 0 and list(eng_edges.plan_stats()) == acc, pipe
        left, why = eng_edges.flat_stats()
        assert left == 0, (pipe, left, list(why))


def test_add_mismatches_over_the_same_cigars(eng_edges):
    """k_flat_parse<1> (the 16-column chunks of the M ops counted): add_mismatches of a few records with the cigars of the alignment
    case, their first bytes at different offsets of a lane chunk and a four-digit number across a tile boundary"""
    import paffy_amd

    rng = random.Random(611)
    n = 40_000
    q = "".join(rng.choices("ACGT", k=n))
    t = "".join(a if rng.random() < 0.9 else rng.choice("ACGT") for a in q)
    seqs = {"pt.chr9": t}
    make = []
    for k, strand in enumerate("+-+-+-"):
        edge, split = (tile_edge, k - 3) if k >= 4 else (lambda cg, k=k: lane_edge(cg - 5 * k) + 5 * k, 0)
        tail = ([(8191, "M"), (1, "I"), (1000, "D")] if k >= 4 else []) + every_length()
        make.append(lambda base, e=edge, s=split, tl=tail, st=strand, k=k: placed(base, e, s, tl, st, by_name_only=k < 4, anchor=[], qlen=n, tlen=n, qs=100, ts=200, tags="tp:A:P"))
    lines = stream(make)
    for l in lines:
        seqs[l.split("\t")[0]] = q
    data = "".join(lines).encode()
    stages = [O.stage(O.ADD_MISMATCHES)]
    want, werr = O.run(stages, data, seqs)
    eng_edges.set_sequences(seqs)
    got, info = eng_edges.run([paffy_amd.Stage(s.kind, s.p0, s.p1) for s in stages], data, raise_on_error=False)
    assert info.error.code == werr.code == 0 and got == want and b"X" in got

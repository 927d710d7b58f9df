"""Edges of the flat pass's writers against the oracle (error code, length and SHA-256 of the whole output): window texts to either side of
FLAT_COPY_MAX, where the copy writer hands over to the four-wave line writer; the copy writer's rewritten end ops after a fixed trim, with
copied middles too short for its 16-byte loop; add_mismatches and tile on records of 100 001 and 1 000 001 ops; and a batch of
add_mismatches lines with more segments than the item list holds."""
import hashlib
import random
import re
import time

import pytest

import oracle_lib as O
from test_gpu_flat import STATS, cigar_of, exact_ops, n_ops_of, random_ops, record, run_both, trimmed_to
from test_gpu_flat import eng  # noqa: F401  (the module's engine; writes PAFFY_FLAT_STATS_OUT when it closes)

pytestmark = pytest.mark.gpu

COPY_MAX = 262_144  # FLAT_COPY_MAX of flat_kernel.h: bytes of cigar text the copy writer takes


def text_ops(rng, nbytes, lens=(1, 5, 30, 60, 110, 1234), indel=(1, 2, 3, 12)):
    """ops whose text is exactly nbytes long, M first and last"""
    ops, total = [], 0
    while total < nbytes - 14:
        op = (rng.choice(lens), "M") if len(ops) % 2 == 0 else (rng.choice(indel), rng.choice("ID"))
        ops.append(op)
        total += len(str(op[0])) + 1
    r = nbytes - total
    while r > 5:
        ops.append((12, "M"))
        r -= 3
    ops.append(({2: 7, 3: 12, 4: 150, 5: 1234}[r], "M"))
    assert sum(len(str(L)) + 1 for L, c in ops) == nbytes
    return ops


def test_window_text_either_side_of_the_copy_limit(eng):
    """Cigar texts of 262 144 bytes, of that less the last op's two bytes and of that plus one op's two bytes, as the whole cigar and as what
    an identity trim leaves of a longer cigar with noisy ends (lengths proven on the oracle's output), both strands. At the limit and below
    it an un-reversed window is copied (k_emit_copy), above it the four-wave writer formats its ops; the reversed windows ('-' records
    behind an invert) never are copied: the sized length must not change with the writer. Every record stays with the flat pass."""
    rng = random.Random(4120)
    base = text_ops(rng, COPY_MAX - 4)
    assert base[-1][1] == "M"
    whole = {COPY_MAX - 2: base + [(3, "M")], COPY_MAX: base + [(3, "M"), (7, "M")], COPY_MAX + 2: base + [(3, "M"), (7, "M"), (5, "M")]}
    recs, lens = [], []
    for n, ops in whole.items():
        for strand in "+-":
            recs.append(record(ops, strand, qs=120_000_000, ts=110_000_000))
            recs.append(record(random_ops(rng, 30), strand))
            lens.append(n)
    data = "".join(recs).encode()
    want, werr = O.run([O.stage(O.INVERT)], data)
    assert werr.code == 0 and [len(cigar_of(l)) for l in want.splitlines()[0::2]] == lens  # the boundary is hit, and to either side
    trimmed, tlens = [], []
    for i, n in enumerate((COPY_MAX - 2, COPY_MAX, COPY_MAX + 2)):
        for strand in "+-":
            # the core's text in steps of one byte; what the trim leaves in front of and behind it stays the same
            line, _ = trimmed_to(4121 + i, n, strand, len, lambda r, k: text_ops(r, k, lens=(40, 99, 150, 1234), indel=(1, 2)), qs=120_000_000, ts=110_000_000)
            trimmed.append(line)
            tlens.append(n)
    tdata = "".join(trimmed).encode()
    want, werr = O.run([O.stage(O.TRIM_IDENTITY)], tdata)
    assert werr.code == 0 and [len(cigar_of(l)) for l in want.splitlines()] == tlens
    both = data + tdata
    pipes = ([O.INVERT], [O.TRIM_IDENTITY], [O.INVERT, O.TRIM_IDENTITY])
    run_both(eng, both, pipes=pipes, kept=True)
    run_both(eng, both, pipes=([O.TRIM_FIXED], [O.INVERT, O.TRIM_FIXED]), params={O.TRIM_FIXED: (0.05, 0.1)}, kept=True)
    O.set_filter(min_identity=0.5)
    eng.set_filter(min_identity=0.5)
    try:
        run_both(eng, both, pipes=([O.FILTER], [O.INVERT, O.FILTER], [O.FILTER, O.TRIM_IDENTITY]), kept=True)
    finally:
        O.set_filter()
        eng.set_filter()


MIDDLES = tuple(m for m in range(18) if m != 1) + (31, 32, 33)  # an op's text is two bytes at least: no middle of one byte exists


def mid_ops(m, letters):
    """ops of m bytes of text; letters: which ops, in turn"""
    sizes = []
    while m:
        take = m if m <= 5 else (5 if m - 5 >= 2 else 4 if m - 4 >= 2 else 3)
        sizes.append(take)
        m -= take
    return [({2: 3, 3: 25, 4: 312, 5: 2048}[b], letters[i % len(letters)]) for i, b in enumerate(sizes)]


def fraction_for(cut, aligned):
    """a `trim -f` fraction under which a record of `aligned` aligned bases loses `cut` of them at either end (impl/paf.c:589-598:
    end = (int64)((float)aligned * fraction / 2), the product in single precision)"""
    import numpy as np

    f = float(np.float32((2 * cut + 1) / aligned))
    assert int(float(np.float32(aligned) * np.float32(f)) / 2.0) == cut
    return f


def test_fixed_trim_copy_with_tiny_middles(eng):
    """`paffy trim -f` on records of one to nine ops: k_emit_copy writes the shortened first and last op anew and copies the text between
    them -- here of 0 and 2 to 17 bytes (its 16-byte loop does not run, or once with a tail) and of 31, 32 and 33 bytes; end ops that lose
    a digit (1000 -> 999, 100 -> 99, 10 -> 9, 1005 -> 5); cuts that fall on an op boundary (the indels behind it go too); a single op cut
    from both ends. Every line is run under every fraction. Un-reversed windows take k_emit_copy, reversed ones ('-' records behind an
    invert) k_emit_line. The middle lengths and the lost digits are read from the oracle's output.
    (A fixed trim always stops in front of an aligned op -- cigar_trim, impl/paf.c:518-545, drops the indels at an end even for a cut of
    nothing -- so no output begins or ends with an I or D op and the letter swap in k_emit_copy's put_op is never asked for; what an invert
    does swap are the indels of the copied middle, next to the rewritten end ops, and that is asserted.)"""
    pairs = ((1000, 1000), (100, 100), (10, 10), (1005, 1005), (1000, 10), (10, 1000), (2345, 100))
    lines, fractions = [], {0.1, 0.3333, 0.5, 0.9}
    k = 0
    for H, T in pairs:
        for cut in sorted({1, min(H, T) - 1, min(H, T), 1000 if H == 1005 else 1}):
            if 2 * cut + 1 < H + T:  # a fraction below 1: something is left of every record
                fractions.add(fraction_for(cut, H + T))
        for m in MIDDLES:
            for letters in ("ID", "DI", "IMD", "MDI"):
                lines.append(record([(H, "M")] + mid_ops(m, letters) + [(T, "M")], "+-"[k & 1], qs=5000 + k, ts=7000 + 2 * k))
                k += 1
    for n in (1000, 100, 10, 1005, 3, 2):  # the record's only op, cut from both ends
        for strand in "+-":
            lines.append(record([(n, "M")], strand, qs=5000, ts=7000))
        if n >= 10:
            fractions.add(fraction_for(1, n))
    fractions.add(fraction_for(496, 1000))
    assert len(lines) > 500
    data = "".join(lines).encode()
    seen_mid, seen_digits, boundary_cuts, swapped_next_to_an_end = set(), set(), 0, 0
    for f in sorted(fractions):
        params = {O.TRIM_FIXED: (0.05, f)}
        want, werr = O.run([O.stage(O.TRIM_FIXED, 0.05, f)], data)
        inv, ierr = O.run([O.stage(O.INVERT), O.stage(O.TRIM_FIXED, 0.05, f)], data)
        assert werr.code == 0 and ierr.code == 0 and len(want.splitlines()) == len(lines) == len(inv.splitlines())
        for src, out, iout in zip(lines, want.splitlines(), inv.splitlines()):
            a = re.findall(rb"(\d+)([MID])", cigar_of(src.encode()))
            b = re.findall(rb"(\d+)([MID])", cigar_of(out))
            c = re.findall(rb"(\d+)([MID])", cigar_of(iout))
            assert b[0][1] == b"M" and b[-1][1] == b"M" and c[0][1] == b"M" and c[-1][1] == b"M"
            if a != b:  # the trim cut something
                seen_mid.add(sum(len(n) + 1 for n, _ in b[1:-1]))
            if len(a) == len(b):
                seen_digits.add((int(a[0][0]), int(b[0][0])))
            elif len(b) <= len(a) - 2 and (b[0] == a[len(a) - len(b)] or b[-1] == a[len(b) - 1]):  # an end op went whole, and the indels behind it
                boundary_cuts += 1
            if "\t+\t" in src and len(c) == len(a) >= 3 and c[0] != a[0] and a[1][1] in b"ID" and c[1] == (a[1][0], b"ID"[a[1][1] == b"I":][:1]):
                swapped_next_to_an_end += 1
        run_both(eng, data, pipes=([O.TRIM_FIXED], [O.INVERT, O.TRIM_FIXED]), params=params, kept=True)
        run_both(eng, data, pipes=([O.TRIM_IDENTITY, O.TRIM_FIXED],), params=params)
    assert set(MIDDLES) <= seen_mid, sorted(set(MIDDLES) - seen_mid)
    assert {(1000, 999), (100, 99), (10, 9), (1005, 5)} <= seen_digits
    assert boundary_cuts > 20 and swapped_next_to_an_end > 20, (boundary_cuts, swapped_next_to_an_end)


def homologous(ops, rng_seed, margin=1000):
    """(target, query, reverse complement of the query) as bytes for a '+' record of these ops at query / target start `margin`: the query
    follows the target along the cigar, with a substitution every 37th base of an M op's columns; built with numpy (a million ops, some
    twenty million bases)"""
    import numpy as np

    rs = np.random.RandomState(rng_seed)
    L = np.array([l for l, _ in ops], dtype=np.int64)
    code = np.array([ord(c) for _, c in ops], dtype=np.uint8)
    is_m, is_i, is_d = code == ord("M"), code == ord("I"), code == ord("D")
    q_off = margin + np.concatenate(([0], np.cumsum(np.where(is_d, 0, L))))
    t_off = margin + np.concatenate(([0], np.cumsum(np.where(is_i, 0, L))))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = acgt[rs.randint(0, 4, size=int(t_off[-1]) + margin)]
    q = acgt[rs.randint(0, 4, size=int(q_off[-1]) + margin)]
    Lm = L[is_m]
    within = np.arange(int(Lm.sum()), dtype=np.int64) - np.repeat(np.concatenate(([0], np.cumsum(Lm)[:-1])), Lm)
    q_idx = np.repeat(q_off[:-1][is_m], Lm) + within
    q[q_idx] = t[np.repeat(t_off[:-1][is_m], Lm) + within]
    sub = q_idx[::37]
    q[sub] = acgt[(np.searchsorted(acgt, q[sub]) + 1) & 3]
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    return t.tobytes(), q.tobytes(), comp[q[::-1]].tobytes()


@pytest.mark.parametrize("n_ops", [100_001, 1_000_001])
def test_add_mismatches_on_very_long_records(n_ops):
    """`add_mismatches` alone on records of 100 001 and 1 000 001 input ops, the '-' record against the reverse complement of the query: the
    flat encoder works piece by piece, k_add_final cuts the lines into segments for k_emit_line (some 1.5 million new ops, a hundred
    segments a line). A fresh engine; no record may leave the flat pass. Preparing the sequences of the million-op case (numpy) takes
    about 2 s of CPU and the oracle's run about 1 s, so they are built per case."""
    import paffy_amd

    rng = random.Random(4130 + n_ops)
    ops = exact_ops(rng, n_ops, lens=(1, 5, 30, 60, 110), indel=(1, 2, 3))
    t0 = time.time()
    t, q, qr = homologous(ops, n_ops)
    print("sequences: %.1f s, %d + %d bases" % (time.time() - t0, len(t), len(q)))
    seqs = {b"tt": t, b"qf": q, b"qr": qr}
    span_q = sum(L for L, c in ops if c in "MI")
    recs = [record(ops, "+", qname="qf", tname="tt", qlen=len(q), tlen=len(t), qs=1000, ts=1000),
            record(random_ops(rng, 40, lens=(1, 5, 30), indel=(1, 2)), "+", qname="qf", tname="tt", qlen=len(q), tlen=len(t), qs=5000, ts=5000),
            record(ops, "-", qname="qr", tname="tt", qlen=len(q), tlen=len(t), qs=len(q) - 1000 - span_q, ts=1000)]
    data = "".join(recs).encode()
    want, werr = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs)
    assert werr.code == 0
    e2 = paffy_amd.Engine()
    try:
        e2.set_sequences(seqs)
        got, info = e2.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], data, raise_on_error=False)
        left, why = e2.flat_stats()
        STATS.append(("test_add_mismatches_on_very_long_records[%d]" % n_ops, (O.ADD_MISMATCHES,), (left, why)))
        print("flat stats", STATS[-1])
        assert info.error.code == 0
        assert len(got) == len(want) and hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest()
        assert left == 0, (left, list(why))
    finally:
        e2.close()
    longest = max(want.splitlines(), key=len)
    assert n_ops_of(cigar_of(longest)) > max(n_ops, 1_000_000 if n_ops > 1_000_000 else 0)
    if n_ops > 1_000_000:
        assert n_ops_of(cigar_of(longest)) > 1_000_000
    assert b"X" in cigar_of(longest) and cigar_of(longest).count(b"X") * 20 < n_ops_of(cigar_of(longest)) * 10  # homologous, not noise


def test_tile_with_very_long_records(eng):
    """`paffy tile` over a batch that holds a record of 100 001 ops and one of 1 000 001 among 300 short ones piled on the same query contig"""
    rng = random.Random(4140)
    qlen = 60_000_000
    recs = []
    for k in range(300):
        ops = random_ops(rng, rng.choice((1, 3, 10, 40)), lens=(1, 5, 30, 200), indel=(1, 2, 9))
        tags = "\t".join(x for x in ("AS:i:%d" % rng.choice((10, 20, 20, 500)) if rng.random() < 0.8 else "", "s1:i:%d" % rng.choice((7, 7, 90)) if rng.random() < 0.5 else "") if x)
        recs.append(record(ops, rng.choice("+-"), qlen=qlen, qs=1_000_000 + rng.randrange(0, 30_000), ts=rng.randrange(0, 10 ** 8), tags=tags or "tp:A:P"))
    recs.insert(100, record(exact_ops(rng, 100_001, lens=(1, 5, 30, 60, 110)), "+", qlen=qlen, qs=1_000_500, ts=50_000, tags="AS:i:20\ts1:i:7"))
    recs.insert(200, record(exact_ops(rng, 1_000_001, lens=(1, 5, 30, 60, 110)), "-", qlen=qlen, qs=1_010_000, ts=90_000, tags="AS:i:500"))
    data = "".join(recs).encode()
    want, werr = O.tile(data)
    got, info = eng.tile(data, raise_on_error=False)
    assert werr.code == 0 and info.error.code == 0
    assert len(got) == len(want) and hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest()
    levels = [int(l.split(b"\ttl:i:")[1].split(b"\t")[0]) for l in want.splitlines()]
    assert max(levels) > 5 and sum(len(l) > 250_000 for l in want.splitlines()) == 2


# ---- the item list of add_mismatches (k_add_final, flat_add_kernel.h; its size: plan_flat_add, paffy_hip.hip) ----
ADD_SEG = 16_384     # ADD_SEG_OPS: a segment closes when the next piece would take it past this many new ops
ROWS_MAX = 32_768    # PAFFY_ROWS_MAX_OPS: a line of at most this many new ops is written whole


def filler(nbytes):
    """nbytes of cigar text that becomes one new op per op (five bytes each): indels, an M op on matching bases first and every 50th op
    (the encoder passes at most 62 ops in a row through)"""
    tail = {0: [], 1: ["10I", "10D"], 2: ["1I"], 3: ["10I"], 4: ["100I"]}[nbytes % 5]
    n5 = (nbytes - sum(len(x) for x in tail)) // 5
    out = ["1000M" if i % 50 == 0 else ("1000I", "1000D")[i & 1] for i in range(n5)] + tail
    assert sum(len(x) for x in out) == nbytes
    return out


def segments_of(line_new_counts):
    """k_add_final's count of segments from the new ops of a line's pieces"""
    if sum(line_new_counts) <= ROWS_MAX:
        return 0
    n_seg = seg = 0
    for c in line_new_counts:
        if seg and seg + c > ADD_SEG:
            n_seg += 1
            seg = 0
        seg += c
    return n_seg + (1 if seg else 0)


def test_add_item_list_overflow_goes_to_the_record_kernels():
    """More segments than the item list holds. The host allots new_words / 8192 + len / 16 384 + 64 items; a line of T new ops has at most
    T / 8192 + 1 segments (two neighbouring segments hold more than 16 384 new ops), and a line uses that "+ 1" with five segments over a
    little more than 32 768 new ops: pieces (1 KiB tiles of the input) of about 5, 16 600, 200, 16 600 and 100 new ops -- two 8191M ops on
    alternating columns in every other tile, indels elsewhere. 1 200 such lines of 4 KiB each: the first try's new_words (len + 2^20) is
    too small, the second has 1.125 x the total, 4.6 items a line, plus 0.25 for the text: 4.86 < 5. The segments are predicted here from
    the oracle's output cut at the tile boundaries of the input, and the prediction must exceed the list. The lines that find no room go to
    the record kernels (k_add_final marks the slots they reserved, the host cuts n_items to the list, the writers skip marked slots):
    some records leave the flat pass, and the bytes are the oracle's."""
    import paffy_amd

    n_lines, period, head = 1200, 4096, 680
    chunks = [["1000I"] * 4 + ["1000M"],            # 25 bytes in the first tile
              ["8191M", "8191M"] + filler(1014),    # a whole tile: 16 382 new ops of the two M ops on alternating columns
              filler(1024),
              ["8191M", "8191M"] + filler(1014),
              filler(period - 1 - head - 25 - 3 * 1024)]
    ops = [(int(x[:-1]), x[-1]) for ch in chunks for x in ch]
    cigar = "".join(x for ch in chunks for x in ch)
    # sequences: all A on both sides, the target columns of the 8191M ops alternate A C
    qspan = sum(L for L, c in ops if c in "MI")
    tspan = sum(L for L, c in ops if c in "MD")
    tseq, tpos = bytearray(b"A" * tspan), 0
    for L, c in ops:
        if c == "M" and L == 8191:
            tseq[tpos:tpos + L] = (b"AC" * L)[:L]
        tpos += L if c in "MD" else 0
    seqs = {b"qa": b"A" * qspan, b"ta": bytes(tseq)}
    bare = record(ops, "+", qname="qa", tname="ta", qlen=qspan, tlen=tspan, qs=0, ts=0, tags="tp:A:P\tzz:Z:", cigar=cigar)
    pad = period - len(bare)
    line = bare.replace("zz:Z:", "zz:Z:" + "p" * pad)
    assert len(line) == period and line.index("cg:Z:") + 5 == head
    first = record([(5, "M")], "+", qname="qa", tname="ta", qlen=qspan, tlen=tspan, qs=0, ts=0, tags="tp:A:P\tzz:Z:")
    first = first.replace("zz:Z:", "zz:Z:" + "p" * (1024 - 25 - head - len(first)))  # the long cigars start 25 bytes in front of a tile boundary
    data = (first + line * n_lines).encode()
    assert (len(first) + head) % 1024 == 1024 - 25
    want, werr = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs)
    assert werr.code == 0
    out_lines = want.splitlines()
    assert len(out_lines) == n_lines + 1 and len(set(out_lines[1:])) == 1
    # the new ops of each input op, from the oracle's line: an M op becomes the = and X ops that add up to it
    new = re.findall(rb"(\d+)([=XID])", cigar_of(out_lines[1]))
    per_tile, at, j = {}, len(first) + head, 0
    for L, c in ops:
        letter_at = at + len(str(L))
        at = letter_at + 1
        n, covered = 0, 0
        while covered < (L if c == "M" else 1):
            covered += int(new[j][0]) if c == "M" else 1
            assert (new[j][1] in b"=X") == (c == "M")
            j += 1
            n += 1
        assert covered == (L if c == "M" else 1)
        per_tile[letter_at >> 10] = per_tile.get(letter_at >> 10, 0) + n
    assert j == len(new)
    counts = [per_tile[k] for k in sorted(per_tile)]
    total_line = sum(counts)
    assert len(counts) == 5 and ROWS_MAX < total_line < 5 * 8192 and segments_of(counts) == 5, counts
    predicted = n_lines * segments_of(counts)
    total = n_lines * total_line + 1
    new_words = len(data) + (1 << 20)          # the first try (a fresh engine)
    assert total > new_words                   # ... does not hold the new ops: the batch is encoded again with
    new_words = total + (total >> 3) + 1024    # the total and an eighth
    items_cap = new_words // 8192 + (len(data) >> 14) + 64
    print("predicted segments %d, item list %d" % (predicted, items_cap))
    assert predicted > items_cap + 50
    e2 = paffy_amd.Engine()
    try:
        e2.set_sequences(seqs)
        got, info = e2.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], data, raise_on_error=False)
        left, why = e2.flat_stats()
        STATS.append(("test_add_item_list_overflow_goes_to_the_record_kernels", (O.ADD_MISMATCHES,), (left, why)))
        print("flat stats", STATS[-1])
        assert info.error.code == 0
        assert len(got) == len(want) and hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest()
        assert 0 < left < n_lines, left  # the lines the list had no room for, and only those
        # the same engine, a batch that fits: nothing of the overflowed list is read
        small = (first + line * 20).encode()
        got, info = e2.run([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], small, raise_on_error=False)
        assert info.error.code == 0 and got == b"\n".join(out_lines[:21]) + b"\n" and e2.flat_stats()[0] == 0
    finally:
        e2.close()

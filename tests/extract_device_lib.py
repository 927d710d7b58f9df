"""Inputs of the `faffy extract` plan tests (the BED text parsed, sorted and merged on the device) and the status a case must end
with. The checker stays tests/faffy_lib.py; `expected` adds what it does not report: the record of a failing plan.

A case is (id, bed, flank, min_size, skip_missing) over GENOME: about a dozen records of at most 5 000 bases and one of 200 000."""
import random

import faffy_lib as F

ASSERT, MISSING = 25, 27  # PAFFY_ERR_FAFFY_ASSERT, PAFFY_ERR_FAFFY_MISSING_SEQ (include/paffy_hip.h)
SLICE, TILE = 256, 65536  # bytes of BED text per thread and per workgroup of the line index

_BASES = bytes(b"ACGTacgtN"[i % 9] for i in range(256))


def _record(rnd, name, n, width=60):
    s = rnd.randbytes(n).translate(_BASES)
    return b">" + name + b"\n" + b"".join(s[i:i + width] + b"\n" for i in range(0, n, width))


def _genome():
    rnd = random.Random(20240)
    recs = [(b"chr1", 3000), (b"chr10", 2500), (b"dup", 900), (b"chr1_random", 1800), (b"chr1|x", 2200), (b"chr\xe9\x80", 1500), (b"chrA", 1400),
            (b"chrz", 1300), (b"has space", 800), (b"big", 200000), (b"dup", 1200), (b"empty", 0), (b"s12", 5000), (b"\xc3\xa9t\xc3\xa9", 700)]
    return b"".join(_record(rnd, name, n) for name, n in recs), recs


GENOME, RECORDS = _genome()
FILES = [GENOME]
LENGTH = {name: n for name, n in RECORDS}  # the last record of a name wins, as in the checker


def expected(files, bed, flank=10, min_size=100, skip_missing=False):
    """(code, record) the plan ends with: (0, None), (ASSERT, line) for a line of fewer than three tokens, (MISSING, line) for a name
    without a record (unless skipped) -- the first such line decides --, then (ASSERT, index in the sorted intervals) for the first
    interval of at least min_size that fails 0 <= i <= start <= end <= j <= len."""
    seqs = dict(F.fasta_read_files(files))
    ivs = []
    for n, line in enumerate(F.bed_lines(bed)):
        toks = line.split()  # bytes.split(): ' ', \t \n \r \v \f, the C locale's isspace
        if len(toks) < 3:
            return ASSERT, n
        if toks[0] not in seqs:
            if skip_missing:
                continue
            return MISSING, n
        ivs.append((toks[0], F.atol(toks[1]), F.atol(toks[2])))
    ivs.sort()
    for k, (name, start, end) in enumerate(ivs):
        if F.wrap(end - start) < min_size:
            continue
        n = len(seqs[name])
        sf, ef = F.wrap(start - flank), F.wrap(end + flank)
        i = sf if sf > 0 else 0
        j = ef if ef <= n else n
        if not 0 <= i <= start <= end <= j <= n:
            return ASSERT, k
    return 0, None


def items(out):
    """the header lines of an output"""
    return [ln for ln in out.split(b"\n") if ln[:1] == b">"]


def filler(n):
    """exactly n bytes (n >= 32) of valid lines over chr10, ending in '\\n'"""
    assert n >= 32
    q, r = divmod(n, 16)
    body = b"chr10 5 300    \n" * (q - 1) if r else b"chr10 5 300    \n" * q
    return body + (b"chr10 5 300" + b" " * (4 + r) + b"\n" if r else b"")


def straddle(at, tok):
    """a BED whose byte `at` lies inside token `tok` of a line over chr1_random, between filler lines"""
    line = b"chr1_random 1000 1500\n"
    inside = (4, 14, 19)[tok]  # an offset inside "chr1_random", "1000", "1500"
    return filler(at - inside) + line + filler(48)


def lines32(n, special):
    """n lines of 32 bytes each (line k starts at byte 32 k); special: {line: text}"""
    out = []
    for k in range(n):
        t = special.get(k, b"chr1 100 400")
        out.append(t + b" " * (31 - len(t)) + b"\n")
    return b"".join(out)


NUMBER_TOKENS = [b"+5", b"-3", b"12abc", b"abc", b"0x10", b"+-5", b"0007", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775809",
                 b"1234567890123456789012345", b"-1234567890123456789012345", b"-9223372036854775808"]

# the atol table: what each token reads as (glibc)
ATOL = {b"+5": 5, b"-3": -3, b"12abc": 12, b"abc": 0, b"0x10": 0, b"+-5": 0, b"0007": 7, b"9223372036854775807": (1 << 63) - 1,
        b"9223372036854775808": (1 << 63) - 1, b"-9223372036854775809": -(1 << 63), b"1234567890123456789012345": (1 << 63) - 1,
        b"-1234567890123456789012345": -(1 << 63), b"-9223372036854775808": -(1 << 63)}


def _cases():
    c = []

    def add(cid, bed, flank=0, min_size=0, skip=False):
        c.append((cid, bed, flank, min_size, skip))

    # ---- tokens
    add("tok-leading-space", b"  \tchr1 10 200\n \x0b chr10 5 300\n")
    add("tok-mixed-runs", b"chr1 \t  10\t\t 200\nchr10\t \t5 \t 300\t\n")
    add("tok-crlf", b"chr1\t10\t200\r\nchr10\t5\t300\r\n")
    add("tok-vt-ff", b"chr1\x0b10\x0c200\nchr10\x0c\x0b5\x0b300\x0c\n")
    add("tok-more-columns", b"chr1\t10\t200\tx\t9\t+\nchr10 5 300 chr1 1 2 3 4 5 6 7\n")
    add("tok-no-final-newline", b"chr1 10 200\nchr10 5 300")
    add("tok-empty-bed", b"")
    add("tok-one-line", b"chr1 10 200\n")
    add("tok-one-line-bare", b"chr1 10 200")
    add("tok-only-newline", b"\n")
    add("tok-space-line", b"chr1 10 200\n \t \nchr10 5 300\n")
    add("tok-two-tokens-at-end", b"chr1 10 200\nchr10 5")
    # ---- numbers: each token as start, as end and as both
    for t in NUMBER_TOKENS:
        add("num-start-" + t.decode(), b"chr10 7 9\nchr1 " + t + b" 100\n")
        add("num-end-" + t.decode(), b"chr10 7 9\nchr1 1 " + t + b"\n")
        add("num-both-" + t.decode(), b"chr10 7 9\nchr1 " + t + b" " + t + b"\n")
        add("num-start-nomin-" + t.decode(), b"chr1 3 4\nchr1 " + t + b" 100\n", 0, -(1 << 63))
    # ---- names
    add("name-prefixes", b"chr1|x 0 50\nchr1_random 0 50\nchr10 0 50\nchr1 0 50\nchr1|x 100 150\nchr1 100 150\n")
    add("name-high-bytes", b"chrz 0 50\nchr\xe9\x80 0 50\nchrA 0 50\n\xc3\xa9t\xc3\xa9 3 40\nchr1 0 50\n")
    add("name-duplicate-last-wins", b"dup 0 50\ndup 1000 1150\n")
    add("name-duplicate-first-length", b"dup 850 950\n")  # inside the second record only
    add("name-space-header", b"chr1 0 50\nhas 0 10\n")
    add("name-space-header-skip", b"chr1 0 50\nhas 0 10\nspace 0 10\n", 0, 0, True)
    add("name-missing", b"chr1 0 50\nnope 0 50\nchr10 0 50\n")
    add("name-missing-skip", b"chr1 0 50\nnope 0 50\nchr10 0 50\n", 0, 0, True)
    add("name-prefix-of-a-name", b"chr 0 50\n")
    add("name-longer-than-a-name", b"chr1_randomx 0 50\n", 0, 0, True)
    add("name-all-missing-skip", b"nope 0 50\nnada 1 2\n", 0, 0, True)
    add("name-empty-record", b"empty 0 0\nchr1 5 9\n")
    # ---- who fails first
    six = [b"chr1 1 90", b"chr10 1 90", b"chr1 200 300", b"chr1 400 500", b"chrA 1 90", b"chrz 1 90", b"chr1 600 700"]
    short_then_missing = list(six)
    short_then_missing[3], short_then_missing[5] = b"chr1 400", b"nope 1 90"
    missing_then_short = list(six)
    missing_then_short[3], missing_then_short[5] = b"nope 1 90", b"chr1 400"
    for skip in (False, True):
        add("first-short3-missing5" + "-skip" * skip, b"\n".join(short_then_missing) + b"\n", 0, 0, skip)
        add("first-missing3-short5" + "-skip" * skip, b"\n".join(missing_then_short) + b"\n", 0, 0, skip)
    add("first-empty-line-in-the-middle", b"chr1 1 2\n\nchr10 1 2\n")
    add("first-line-parse-before-bounds", b"chr1 -5 100\nchr1 1\n")
    add("first-fail-at-slice-start", lines32(20, {8: b"nope 1 2"}))          # line 8 starts at byte 256
    add("first-fail-at-slice-start-short", lines32(20, {8: b"chr1 1", 16: b"nope 1 2"}))
    add("first-fail-before-slice-start", lines32(20, {7: b"chr1", 8: b"nope 1 2"}))
    add("first-fail-in-last-slice", lines32(21, {20: b"nope 1 2"}) + b"chr1 7")
    add("first-fail-last-line-alone-in-its-slice", lines32(24, {}) + b"chr1 7")  # the last slice holds these 6 bytes only
    add("first-fail-at-tile-start", lines32(2050, {2048: b"nope 1 2"}))       # line 2048 starts at byte 65 536
    add("first-fail-lowest-of-many", lines32(2050, {2049: b"nope 1 2", 1030: b"chr1 9", 1031: b"nope 1 2", 8: b"chr1 5 6"}))
    # ---- sweep (chr1: 3000 bases, chr10: 2500)
    add("sweep-min-size-equal-and-below", b"chr1 100 200\nchr10 100 199\n", 0, 100)
    add("sweep-min-size-one-more", b"chr1 100 200\nchr10 100 199\n", 0, 101)
    add("sweep-dropped-between-merging", b"chr1 100 300\nchr1 150 160\nchr1 250 500\n", 0, 50)
    add("sweep-dropped-between-separate", b"chr1 100 200\nchr1 250 260\nchr1 400 500\n", 0, 50)
    add("sweep-touching", b"chr1 100 200\nchr1 210 300\n", 5, 1)       # p_end = 205 = i
    add("sweep-one-apart", b"chr1 100 200\nchr1 211 300\n", 5, 1)      # p_end = 205 = i - 1
    add("sweep-flanks-clipped", b"chr1 3 200\nchr1 2900 2998\nchr10 0 2500\n", 10, 1)
    add("sweep-negative-flank", b"chr1 100 110\nchr1 300 500\n", -5, 50)
    add("sweep-negative-flank-fits", b"chr1 300 300\n", -5, -20)
    add("sweep-negative-start", b"chr1 500 600\nchr10 -5 100\nchr1 10 20\n")
    add("sweep-end-past-length", b"chr10 100 2501\nchr1 1 2000\n")
    add("sweep-end-at-length", b"chr10 100 2500\nchr1 1 3000\n", 10, 1)
    add("sweep-skipped-then-failing", b"nope 1 2\nchr10 100 2501\nchr1 10 20\n", 0, 0, True)
    add("sweep-identical-triples", b"chr1 100 300\nchr1 100 300\nchr10 5 9\nchr1 100 300\n", 3, 1)
    add("sweep-equal-starts", b"chr1 100 300\nchr1 100 200\nchr1 100 400\nchr1 500 600\nchr1 100 250\n", 0, 1)
    add("sweep-same-interval-two-names", b"chr1 100 300\nchr10 100 300\nchr1 200 400\nchr10 200 400\n", 0, 1)
    add("sweep-huge-flank", b"chr1 100 300\nchr10 7 9\n", 1 << 40, 1)
    # ---- prefix maximum (big: 200 000 bases)
    rnd = random.Random(77)
    inside = [b"big %d %d" % (s, s + rnd.randrange(1, 50)) for s in (rnd.randrange(100, 9000) for _ in range(300))]
    cover = [b"big 0 10000"] + inside
    rnd.shuffle(cover)
    add("pmax-covering", b"\n".join(cover) + b"\n", 0, 1)
    add("pmax-covering-joins", b"\n".join(cover + [b"big 10000 10040"]) + b"\n", 0, 1)
    add("pmax-covering-new-item", b"\n".join(cover + [b"big 10001 10040"]) + b"\n", 0, 1)
    add("pmax-covering-flank-joins", b"\n".join(cover + [b"big 10014 10040"]) + b"\n", 7, 1)
    add("pmax-covering-flank-at-flank", b"\n".join(cover + [b"big 10007 10040", b"big 10008 10041"]) + b"\n", 7, 1)
    add("pmax-covering-flank-new-item", b"\n".join(cover + [b"big 10015 10040"]) + b"\n", 7, 1)
    run = [b"big %d %d" % (30 * k, 30 * k + 50) for k in range(5000)] + [b"big 150100 150200", b"chr1 5 50", b"s12 100 4000"]
    rnd.shuffle(run)
    add("pmax-run-of-5000", b"\n".join(run) + b"\n", 0, 1)
    # ---- slice and tile edges
    for at in (SLICE, TILE):
        for tok in range(3):
            add("edge-straddle-%d-token%d" % (at, tok), straddle(at, tok), 0, 1)
    add("edge-exactly-a-tile", filler(TILE), 0, 1)
    add("edge-a-tile-less-one", filler(TILE - 1), 0, 1)
    add("edge-a-tile-and-one", filler(TILE + 1), 0, 1)
    add("edge-a-tile-no-final-newline", filler(TILE + 1)[:-1], 0, 1)
    add("edge-a-tile-then-one-byte", filler(TILE) + b"c", 0, 1)
    add("edge-a-tile-then-a-newline", filler(TILE) + b"\n", 0, 1)
    add("edge-newline-at-slice-end", filler(SLICE) + b"chr1 5 50\n" + filler(SLICE - 10) + b"chrA 5 50\n", 0, 1)
    add("edge-long-first-token-skip", b"x" * 70000 + b" 1 2\nchr1 10 200\n", 0, 1, True)
    add("edge-long-first-token", b"chr1 10 200\n" + b"x" * 70000 + b" 1 2\n", 0, 1)
    return c


CASES = _cases()
ERROR_CASES = [c for c in CASES if expected(FILES, c[1], c[2], c[3], c[4])[0]]


def big_case(n=100001, seed=5):
    """n lines over the genome: mixed names (some missing, to be skipped), seeded; the intervals on `big` overlap into long runs"""
    rnd = random.Random(seed)
    names = [name for name, ln in RECORDS if b" " not in name and ln >= 700]
    lines = []
    for k in range(n):
        r = rnd.random()
        if r < 0.02:
            lines.append(b"nope%d\t%d\t%d\n" % (k % 7, k, k + 200))
            continue
        name = b"big" if r < 0.6 else rnd.choice(names)
        ln = LENGTH[name]
        size = rnd.randrange(20, 400)
        st = rnd.randrange(0, ln - size)
        lines.append(b"%s\t%d\t%d\n" % (name, st, st + size))
    return ("size-%d-lines" % n, b"".join(lines), 10, 100, True)


def longest_run(bed, flank, min_size):
    """the most intervals that one item of the output merges"""
    seqs = dict(F.fasta_read_files(FILES))
    ivs = sorted((t[0], F.atol(t[1]), F.atol(t[2])) for t in (ln.split() for ln in F.bed_lines(bed)) if t[0] in seqs)
    best = cur = 0
    prev = None
    for name, s, e in ivs:
        if e - s < min_size:
            continue
        i, j = max(s - flank, 0), min(e + flank, len(seqs[name]))
        if prev and prev[0] == name and prev[1] >= i:
            prev[1] = max(prev[1], j)
            cur += 1
        else:
            prev, cur = [name, j], 1
        best = max(best, cur)
    return best

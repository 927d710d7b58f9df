"""`paffy add_mismatches -a` (paf_remove_mismatches, impl/paf.c:786-809) on the pieces of the flat pass (paffy_amd/csrc/flat_remove_kernel.h)
against the oracle. A merged run does not stop where a 1 KiB piece of cigar text does, so the cases put the ends of runs on, next to and
across the piece boundaries, runs over many whole pieces, pieces of 512 ops (eight windows of a wave), merged lengths to either side of
every power of ten and of the parser's per-op limit, the 29-bit word limit, what the pass leaves to the record kernels, errors, and the
plan's other consumers. Every case compares error code, error record, length and SHA-256 of the whole output; `left` is what
Engine.flat_stats() reports: -1 for a plan the flat pass did not take (the code before this mode existed), else the records it left."""
import hashlib
import os
import random
import re
import subprocess

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
TILE = 1024          # FLAT_TILE: a piece is a record's cigar text inside one 1 KiB tile of the batch
ROWS_MAX = 32_768    # PAFFY_ROWS_MAX_OPS: a line of more new ops is written as segments
REMOVE = (O.REMOVE_MISMATCHES,)


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def record(cigar, strand="+", qname="hs.chr3", tname="pt.chr9", qlen=250_000_000, tlen=240_000_000, qs=1000, ts=2000, tags="tp:A:P\tAS:i:777\ts1:i:42", dq=0):
    """a record whose coordinates agree with its cigar (dq: bases added to the query end, for a failing check)"""
    ops = [(int(n), c) for n, c in re.findall(r"(\d+)([MIDX=])", cigar)]
    qspan = sum(n for n, c in ops if c in "M=XI")
    tspan = sum(n for n, c in ops if c in "M=XD")
    return f"{qname}\t{qlen}\t{qs}\t{qs + qspan + dq}\t{strand}\t{tname}\t{tlen}\t{ts}\t{ts + tspan}\t{qspan}\t{qspan + tspan}\t60\t{tags}\tcg:Z:{cigar}\n"


def pad_line(n):
    """a small valid record of exactly n bytes (n >= 80)"""
    base = record("5M", qname="p", tname="q", qlen=100, tlen=100, qs=0, ts=0, tags="tp:A:P\tzz:Z:")
    assert n >= len(base), n
    return base.replace("zz:Z:", "zz:Z:" + "p" * (n - len(base)))


def placed(lines_and_offsets, at=0):
    """the lines in order, each behind a padding line that puts the first byte of its cigar at the given offset inside a 1 KiB tile
    (None: no padding line); at: bytes of the batch in front"""
    out = []
    for line, off in lines_and_offsets:
        if off is not None:
            head = line.index("cg:Z:") + 5
            n = (off - at - head) % TILE
            while n < 100:
                n += TILE
            out.append(pad_line(n))
            at += n
            assert (at + head) % TILE == off
        out.append(line)
        at += len(line)
    return "".join(out)


def merged(cigar):
    """paf_remove_mismatches on cigar text, in Python: what the test expects beside the oracle"""
    out = []
    for n, c in re.findall(r"(\d+)([MIDX=])", cigar):
        if c in "M=X" and out and out[-1][1] == "M":
            out[-1][0] += int(n)
        else:
            out.append([int(n), "M" if c in "M=X" else c])
    return "".join(f"{n}{c}" for n, c in out)


def cigars_of(out):
    return [l.split(b"cg:Z:")[1].split(b"\t")[0].decode() for l in out.splitlines() if b"cg:Z:" in l]


def run_both(eng, data, want_left=0, pipe=REMOVE):
    """error code, error record, length and SHA-256 of the whole output against the oracle's; want_left: records the flat pass must have
    left to the record kernels (None: not asserted). Returns (output, left)."""
    import paffy_amd

    if isinstance(data, str):
        data = data.encode()
    want, werr = O.run([O.stage(k) for k in pipe], data)
    got, info = eng.run([paffy_amd.stage(k) for k in pipe], data, raise_on_error=False)
    left = eng.flat_stats()[0]
    print("flat left", left, "records", info.n_records, "bytes", len(got))
    assert info.error.code == werr.code, (info.error.code, werr.code, info.error.record, werr.record)
    if werr.code:
        assert info.error.record == werr.record, (info.error.record, werr.record)
    assert len(got) == len(want) and hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest(), (len(got), len(want))
    if want_left is not None:
        assert left == want_left, left
    return got, left


# ---- 1 ----
KNOWN = [("3=2X1I", "5M1I"), ("5M3M", "8M"), ("2I3D", "2I3D"), ("3I4I", "3I4I"), ("1=", "1M"), ("4M2=1X3M", "10M"),
         ("2I3=1X4D", "2I4M4D"), ("7D1X1=1X2I", "7D3M2I"), ("1I1D1I1D", "1I1D1I1D"), ("1D5=", "1D5M"), ("5X1D", "5M1D"),
         ("10=3I4I2X7M1D1D9=", "10M3I4I9M1D1D9M")]


def test_known_answers(eng):
    lines = [record(c, strand) for strand in "+-" for c, _ in KNOWN]
    got, _ = run_both(eng, "".join(lines))
    assert cigars_of(got) == [w for _ in "+-" for _, w in KNOWN]
    assert [merged(c) for c, _ in KNOWN] == [w for _, w in KNOWN]  # the Python model used below agrees with them


def test_records_without_a_cigar_empty_input_and_an_open_last_line(eng):
    no_cg = record("5M").replace("\tcg:Z:5M", "")
    empty_cg = record("5M").replace("cg:Z:5M", "cg:Z:")
    assert "cg:Z:" not in no_cg and empty_cg.endswith("cg:Z:\n")
    run_both(eng, record("3=2X1I") + no_cg + record("4=") + empty_cg + record("1X1="), want_left=None)  # these two may be left: the bytes only
    got, info = eng.run([__import__("paffy_amd").stage(O.REMOVE_MISMATCHES)], b"")
    assert got == b"" and O.run([O.stage(O.REMOVE_MISMATCHES)], b"")[0] == b""
    got, _ = run_both(eng, (record("3=2X1I") + record("2=2X", "-"))[:-1])  # no newline behind the last line
    assert cigars_of(got) == ["5M1I", "4M"]


# ---- 2 ----
def sweep_cigar():
    """about 3 KiB of text with runs of one to sixty = / X ops, numbers of one to four digits, I and D ops alone, in pairs (I D, D I) and
    doubled (I I). With the cigar's first byte at every offset of a tile, a tile boundary falls behind every byte of the first 2 KiB of
    it: behind the last letter of a run, in front of a run's first digit, inside a run, inside a number, between an I and a D."""
    rng = random.Random(7)
    parts = []
    while sum(len(p) for p in parts) < 3000:
        for _ in range(rng.choice((1, 1, 2, 3, 8, 60))):
            parts.append("%d%s" % (rng.choice((1, 2, 9, 10, 37, 99, 100, 512, 999, 1000, 4096, 8191)), rng.choice("=X=XM")))
        parts.append(rng.choice(("3I", "12D", "2I3D", "4D1I", "3I4I", "1000I", "1D")))
    return "".join(parts)


def test_every_tile_offset(eng):
    cigar = sweep_cigar()
    assert 3000 <= len(cigar) < 3200 and "I3D" in cigar and re.search(r"\d{4}[=X]\d{4}[=X]", cigar) and re.search(r"[ID]\d+[=XM]", cigar)
    line = record(cigar, "-")
    data = placed([(line, off) for off in range(TILE)])
    got, _ = run_both(eng, data)
    cg = cigars_of(got)
    assert len(cg) == 2 * TILE and cg[1::2] == [merged(cigar)] * TILE


# ---- 3 ----
def eqx(n_ops, rng, indel_every=0):
    """n_ops ops of = and X (lengths 1 to 9), with an I or D about every indel_every ops"""
    out = []
    for i in range(n_ops):
        if indel_every and i % indel_every == indel_every - 1 - (i // indel_every) % 3:
            out.append("%d%s" % (rng.choice((1, 2, 30)), "ID"[(i // indel_every) & 1]))
        else:
            out.append("%d%s" % (rng.randrange(1, 10), "=X"[i & 1]))
    return "".join(out)


def long_run_records():
    rng = random.Random(11)
    recs = []
    for whole in (1, 2, 3, 70):  # the run covers this many whole pieces and a part of the two around them
        run = eqx((whole + 1) * TILE // 2 + 50, rng)
        assert len(run) >= (whole + 1) * TILE
        recs.append(record("5I" + run + "3D7=", "+-"[whole & 1]))
    for n in (100_001, 1_000_001):
        recs.append(record(eqx(n, rng), "+"))
        recs.append(record(eqx(n, rng, 40), "-"))
    filler = [record(eqx(rng.choice((1, 5, 40, 300)), rng, rng.choice((0, 3, 7)))) for _ in range(30)]
    out = []
    for k, r in enumerate(recs):
        out += filler[3 * k:3 * k + 3] + [r]
    return out + filler[24:]


@pytest.fixture(scope="module")
def long_runs():
    return "".join(long_run_records()).encode()


def test_runs_over_whole_pieces(eng, long_runs):
    """The 100 001-op record with an I or D every 40 ops becomes about 5 000 ops: a whole line. The 1 000 001-op one becomes about 50 000,
    more than PAFFY_ROWS_MAX_OPS: segments."""
    got, _ = run_both(eng, long_runs)
    cg = cigars_of(got)
    lines = long_runs.decode().splitlines()
    big = sorted(range(len(lines)), key=lambda i: -len(lines[i]))[:4]
    n_new = sorted(len(re.findall(r"[MID]", cg[i])) for i in big)
    assert n_new[:2] == [1, 1] and n_new[2] > 4000 and n_new[3] > ROWS_MAX, n_new
    assert all(re.fullmatch(r"5I\d+M3D7M", cg[i]) for i in (3, 7, 11, 15))


# ---- 4 ----
def test_dense_pieces(eng):
    """1=1X1=1X...: 512 ops in every piece (the cigar starts on a tile boundary). An I in the middle of a piece, at the ends of a wave's
    windows, as a piece's first op, as its last, as both; and the same cigars one byte off the boundary."""
    n = 4 * 512 + 100
    cases = [[], [512 + 256], [512 + 63], [512 + 64], [512 + 65], [512], [511], [1023], [1024], [511, 512], [1023, 1024, 1535, 1536], [0], [n - 1],
             list(range(512, 1024, 2)), list(range(513, 1024, 2))]
    lines = []
    for at in cases:
        ops = ["1=" if i % 2 == 0 else "1X" for i in range(n)]
        for i in at:
            ops[i] = "1I" if i % 3 else "1D"
        for off in (0, 1, TILE - 1):
            lines.append((record("".join(ops), "+-"[len(lines) & 1]), off))
    got, _ = run_both(eng, placed(lines))
    cg = [c for c in cigars_of(got) if c != "5M"]
    assert cg == [merged(re.search(r"cg:Z:(\S+)", l).group(1)) for l, _ in lines]


# ---- 5 ----
SUMS = sorted({10 ** k - d for k in range(1, 9) for d in (0, 1)} | {8191, 8192, 8193})


def split_sum(total, n_ops, rng):
    """n_ops lengths of 1..8191 that add up to total"""
    assert n_ops <= total <= 8191 * n_ops
    lens = [1] * n_ops
    rest = total - n_ops
    for i in rng.sample(range(n_ops), n_ops):
        add = min(rest, 8190)
        lens[i] += add
        rest -= add
    assert rest == 0 and sum(lens) == total
    return lens


def test_digit_counts_of_merged_lengths(eng):
    """Runs whose sums are 9, 10, 99, 100, ... 10^8 - 1, 10^8 and 8 191, 8 192, 8 193 (the merged op may exceed the parser's per-op
    limit): put together inside one piece where 200 ops of at most 8 191 can hold the sum, and from ops spread over two pieces (the small
    sums: the cigar straddles a tile boundary) or many (ops of at most 8 191 over several KiB of text)."""
    rng = random.Random(5)
    lines, want = [], []
    for total in SUMS:
        shapes = []
        if total <= 200 * 8191:  # one piece: the cigar starts on a tile boundary and is shorter than a tile
            shapes.append((split_sum(total, max(min(total, 2), -(-total // 8191)), rng), 0))
        if total >= 3000:        # many pieces
            shapes.append((split_sum(total, max(1500, -(-total // 8191) + 7), rng), rng.randrange(TILE)))
        if total >= 2:           # two pieces: the boundary falls inside the run
            shapes.append((split_sum(total, max(min(total, 4), -(-total // 8191)), rng), TILE - 6))
        for lens, off in shapes:
            cigar = "2I" + "".join("%d%s" % (n, "=X"[i & 1]) for i, n in enumerate(lens)) + "1D3="
            lines.append((record(cigar, "+-"[len(lines) & 1], qlen=1_500_000_000, tlen=1_400_000_000), off))
            want.append("2I%dM1D3M" % total)
    got, _ = run_both(eng, placed(lines))
    assert [c for c in cigars_of(got) if c != "5M"] == want
    assert len({len(w) for w in want}) >= 9  # one to nine digits


# ---- 6 ----
def test_the_word_limit(eng):
    """A run of 2^29 - 1 bases fits the 4-byte op (29 bits of length): kept. One of 2^29 does not: the record kernels' 8-byte ops."""
    assert 65_544 * 8191 + 7 == (1 << 29) - 1
    kw = dict(qlen=600_000_000, tlen=600_000_000, qs=0, ts=0)
    fits = record("8191=" * 65_544 + "7=", "+", **kw)
    wide = record("8191=" * 65_544 + "8=", "-", **kw)
    got, _ = run_both(eng, record("3=1X") + fits + record("2I3="), want_left=0)
    assert cigars_of(got) == ["4M", "%dM" % ((1 << 29) - 1), "2I3M"]
    got, _ = run_both(eng, record("3=1X") + fits + wide + record("2I3="), want_left=1)
    assert cigars_of(got) == ["4M", "%dM" % ((1 << 29) - 1), "%dM" % (1 << 29), "2I3M"]


# ---- 7 ----
def test_mixed_batch(eng):
    rng = random.Random(3)
    recs = [record(eqx(rng.choice((1, 4, 30, 200, 900)), rng, rng.choice((0, 2, 5, 40))), rng.choice("+-")) for _ in range(200)]
    odd = ["3=8192=2X1I4=", "7=10000=1D2X", "4=05=1X", "4=0X2=1I3="]
    for k, c in enumerate(odd):
        recs.insert(30 + 40 * k, record(c))
    got, _ = run_both(eng, "".join(recs), want_left=len(odd))
    cg = cigars_of(got)
    assert [cg[30 + 40 * k] for k in range(4)] == ["8197M1I4M", "10007M1D2M", "10M", "6M1I3M"]


# ---- 8 ----
@pytest.mark.parametrize("bad", ["sums", "letter", "strand"])
def test_errors(eng, bad):
    rng = random.Random(9)
    recs = [record(eqx(rng.choice((1, 4, 30, 700)), rng, rng.choice((0, 5))), rng.choice("+-")) for _ in range(60)]
    if bad == "sums":
        recs[31] = record("30=2X1I4=", dq=3)
    elif bad == "letter":
        recs[31] = record("30=2X1I4=").replace("1I", "1N")
    else:
        recs[31] = record("30=2X1I4=").replace("\t+\t", "\t*\t")
    want, werr = O.run([O.stage(O.REMOVE_MISMATCHES)], "".join(recs).encode())
    assert werr.code != 0 and werr.record == 31 and want.count(b"\n") == 31
    run_both(eng, "".join(recs), want_left=None)


# ---- 9 ----
def test_fixture(eng):
    with open(os.path.join(ROOT, "tests", "golden", "human_chimp.paf"), "rb") as fh:
        data = fh.read()
    _, left = run_both(eng, data, want_left=None)
    _, left_pass = run_both(eng, data, want_left=None, pipe=(O.PASS,))
    assert 0 <= left <= left_pass, (left, left_pass)


# ---- 10, 11 ----
@pytest.fixture(scope="module")
def cfg4():
    """a small cfg4 setup: 4 contig pairs of 2-3 Mb, 2 000 records; the records as generated and as ADD_MISMATCHES writes them"""
    import paffy_amd as P

    e = P.Engine()
    e.synth4_setup(0x5EED0004, 1024, n_contigs=4, tlen_min=2_000_000, tlen_span=1_000_000)
    buf, nbytes = e.synth4(0, 2000)
    plain = bytes(buf[:nbytes].cpu().numpy().tobytes())
    enc, info = e.run([P.stage(P.ADD_MISMATCHES)], plain)
    assert info.error.code == 0 and info.n_records == 2000
    yield e, plain, enc
    e.close()


def test_round_trip_on_encoded_text(cfg4):
    e, plain, enc = cfg4
    got, _ = run_both(e, enc)
    n_eqx = sum(c.count("=") + c.count("X") for c in cigars_of(enc))
    n_m = sum(c.count("M") for c in cigars_of(got))
    print("= / X ops in: %d, M ops out: %d" % (n_eqx, n_m))
    assert n_eqx > 2 * n_m > 0  # the text needed merging
    assert got == O.run([O.stage(O.REMOVE_MISMATCHES)], plain)[0]  # and the merge gives back the cigars the records came with


def test_one_plan_after_another(cfg4):
    """[REMOVE], [INVERT], [ADD], [REMOVE] on one engine, twice: the same bytes each time, no state outlives its plan"""
    import paffy_amd as P

    e, plain, enc = cfg4
    want_rm = O.run([O.stage(O.REMOVE_MISMATCHES)], enc)[0]
    want_inv = O.run([O.stage(O.INVERT)], plain)[0]
    for _ in range(2):
        for st, data, want, left in ((P.REMOVE_MISMATCHES, enc, want_rm, 0), (P.INVERT, plain, want_inv, None), (P.ADD_MISMATCHES, plain, enc, None),
                                     (P.REMOVE_MISMATCHES, enc, want_rm, 0)):
            got, info = e.run([P.stage(st)], data)
            assert info.error.code == 0 and got == want, st
            assert left is None or e.flat_stats()[0] == left


def test_emit_again_and_into_pieces(eng, long_runs):
    """The plan's other consumers. paffy_hip_emit a second time, into another buffer, writes the same bytes (the new ops, the plans and
    the segment list are the plan's, not the emit's). paffy_hip_emit_lines serves line plans (tile, dedupe) only: after this plan it
    reports PAFFY_E_STATE as after every record plan, and leaves the plan usable."""
    import paffy_amd as P

    want = O.run([O.stage(O.REMOVE_MISMATCHES)], long_runs)[0]
    d_in = eng.to_device(long_runs)
    info = eng.plan([P.stage(P.REMOVE_MISMATCHES)], d_in, len(long_runs))
    assert info.error.code == 0 and info.out_bytes == len(want) and eng.flat_stats()[0] == 0
    outs = []
    for k in range(2):
        d_out = eng.alloc_out(info.out_bytes)
        eng.emit(d_out)
        eng.sync()
        outs.append(bytes(d_out[:info.out_bytes].cpu().numpy().tobytes()))
        if k == 0:
            with pytest.raises(Exception):
                eng.emit_lines(0, 1, eng.alloc_out(1 << 20))
    assert outs[0] == want and outs[1] == want


def test_cli(cfg4):
    """`bin/paffy add_mismatches -a` on the = / X text"""
    import paffy_amd

    paffy_amd.build_library()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    _, _, enc = cfg4
    p = subprocess.run([PAFFY, "add_mismatches", "-a"], input=enc, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr[-500:]
    assert p.stdout == O.run([O.stage(O.REMOVE_MISMATCHES)], enc)[0]

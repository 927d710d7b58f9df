"""The base-level rows of `paffy view -a` (k_pretty_size / k_pretty_rows, paffy_amd/csrc/pretty_kernel.h) and the per-record sums of
PAFFY_STATS after every stage list, through the C-ABI (Engine.alignment_sizes / alignment_rows / record_stats) against the oracle: the
same stage list run by O.run, each of its output lines printed by O.pretty_print with the sequences its own names ask for; what follows
the stats line must be the GPU's block byte for byte and as long as alignment_sizes says, and O.cigar_stats of the line's cigar must be
the record's six sums. The kernel reads a record's ops through every form the sizing passes leave them in -- 2-byte words in the mirror,
4-byte words in the mirror (a length of 8 192 or more), 4-byte words in an arena block (add_mismatches: the record kernels' rebuilt array
and the flat add pass's new_ops), 8-byte ops of the arena class -- and through the view a stage list leaves (reversed, I / D exchanged,
query / target exchanged, whole ops cut by an identity trim, the end ops shortened by a fixed trim). Engine.record_layout says which form
each record was really read from, and every form is asserted under a plain, an inverted and a fixed-trimmed view where it can occur.
The record shapes are the smallest at which each mechanism of the kernel can go wrong: op counts round its chunks of 256, column totals
round its windows of 150. SHATTER and FILTER change which records exist (one input line is no longer one block of rows), so they are left
out here; their outputs are pinned elsewhere (test_gpu_parity.py, test_filter.py)."""
import os
import random
import subprocess

import pytest

import oracle_lib as O
from test_gpu_flat import cigar_of, exact_ops, random_ops, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")

STATS = 10                                            # PAFFY_STATS: the oracle has no such stage (it changes no line)
HALF, MIRROR_BITS, IN_ARENA, FLAT_ADD = 0x40000, 0x60000, 0x20000, 0x100000  # RecPlan.flags, record_types.h
KLASS_LDS, KLASS_ARENA = 0, 1
LDS_TOP = 36_864                                      # ops of the largest LDS store (record_kernel.h: the third sizing launch); more go to the arena class
ERR_MISSING_QUERY, ERR_MISSING_TARGET, ERR_SEQ_RANGE = 17, 18, 21
GUARD = 256


def fraction_for(cut, aligned):
    """a `trim -f` fraction under which a record of `aligned` aligned bases loses `cut` of them at either end (impl/paf.c:589-598:
    end = (int64)((float)aligned * fraction / 2), the product in single precision)"""
    import numpy as np

    f = float(np.float32((2 * cut + 1) / aligned))
    assert int(float(np.float32(aligned) * np.float32(f)) / 2.0) == cut
    return f


F10 = fraction_for(10, 260)  # the records of fixed_trim_lines() have 260 aligned bases: ten off each end

# stage lists: (kind, trim -r, trim -t); STATS last wherever the sums are compared with the output line
INV, TRI, FIX, ADD = (O.INVERT, 0.05, 1.0), (O.TRIM_IDENTITY, 0.05, 1.0), (O.TRIM_FIXED, 0.05, 0.1), (O.ADD_MISMATCHES, 0.05, 1.0)
ST = (STATS, 0.0, 0.0)
STAGE_LISTS = {
    "none": [],                                       # the record kernels (no stage: no flat pass)
    "stats": [ST],                                    # what paf_pretty_print of host/paf_api.c plans
    "invert": [INV, ST],
    "invert_invert": [INV, INV, ST],
    "trim_identity": [TRI, ST],
    "trim_fixed": [FIX],                              # the flat pass takes a fixed trim as the last stage only
    "trim_fixed_stats": [FIX, ST],
    "invert_trim_fixed": [INV, FIX],
    "trim_fixed_invert": [FIX, INV, ST],
    "trim_to_nothing": [(O.TRIM_FIXED, 0.05, 1.0), ST],
    "add_flat": [ADD],                                # flat_add_kernel.h sizes `add_mismatches` alone
    "add_records": [ADD, ST],                         # any longer list: the record kernels' encoder
    "add_invert": [ADD, INV, ST],
    "add_trim_fixed": [ADD, FIX, ST],
}
PLAIN, INVERTED, TRIMMED = "plain", "inverted", "fixed-trimmed"


# ---- sequences: mixed case, runs of N / n, a few letters outside ACGT; the rows show them as loaded ----
def make_seq(rng, n):
    s = bytearray(rng.choices(b"ACGTacgt", weights=(6, 6, 6, 6, 2, 2, 2, 2), k=n))
    for _ in range(n // 3000 + 2):
        at, run = rng.randrange(n), rng.randrange(1, 40)
        s[at:at + run] = (b"N" if rng.random() < 0.5 else b"n") * len(s[at:at + run])
    for _ in range(n // 500 + 2):
        s[rng.randrange(n)] = rng.choice(b"RyKmSw")
    return bytes(s)


_SEQS = {}


def sequences():
    if not _SEQS:
        rng = random.Random(0xA11C)
        ta = make_seq(rng, 150_000)
        qa = bytearray(ta)  # the query of the long pair follows its target: half of the columns of an M op agree, case aside
        for i in range(0, len(qa), 2):
            qa[i] = rng.choice(b"ACGTacgt")
        _SEQS.update({"ta": ta, "qa": bytes(qa), "tb": make_seq(rng, 30_000), "qb": make_seq(rng, 30_000)})
    return _SEQS


def place(ops, strand, k, pair="b", tags="tp:A:P\tAS:i:77"):
    """a record of the pair's contigs, far enough from their ends that no column of it lies within 10 000 bases of one"""
    seqs = sequences()
    qn, tn = "q" + pair, "t" + pair
    return record(ops, strand, qname=qn, tname=tn, qlen=len(seqs[qn]), tlen=len(seqs[tn]), qs=10_000 + 37 * k, ts=10_000 + 53 * k, tags=tags).encode()


def with_ends(core):
    return [(5, "M"), (2, "I")] + core + [(1, "D"), (9, "M")]


def noisy_ends(rng):
    """ends of single matches between long indels round a clean core: an identity trim cuts whole ops there"""
    front = [(1, "M") if i % 2 == 0 else (30, "ID"[i // 2 % 2]) for i in range(20)]
    back = [(30, "ID"[i // 2 % 2]) if i % 2 == 0 else (1, "M") for i in range(20)]
    return front + random_ops(rng, 41, lens=(40, 99, 150), indel=(1, 2)) + back


def flat_shapes():
    """[(label, ops)] the flat pass takes: M / I / D ops, every length below 8 192"""
    rng = random.Random(0xA11D)
    out = [("ops%d" % n, exact_ops(rng, n, lens=(1, 2, 3, 7), indel=(1, 2, 3))) for n in (1, 255, 256, 257, 513)]
    a, b = exact_ops(rng, 257, lens=(1, 2, 3), indel=(1, 2)), exact_ops(rng, 257, lens=(1, 2, 3), indel=(1, 2))
    a[255] = (400, a[255][1])  # a long op is the last op of the first chunk of 256 ...
    b[256] = (400, b[256][1])  # ... and the first of the second
    out += [("long_op_ends_chunk", a), ("long_op_starts_chunk", b)]
    for total in (1, 149, 150, 151, 300, 301):  # columns round the windows of 150
        out.append(("cols%d" % total, [(total, "M")] if total < 3 else [(total // 3, "M"), (1, "I"), (total - total // 3 - 1, "M")]))
    out.append(("op_over_three_windows", [(100, "M"), (3, "D"), (350, "M"), (2, "I"), (10, "M")]))
    out.append(("window_ends_on_op_ends", [(150, "M"), (5, "I"), (145, "M"), (7, "D"), (20, "M")]))
    out.append(("noisy_ends", noisy_ends(rng)))
    out.append(("len8191", with_ends([(8191, "M")])))
    return out


def arena_ops():
    rng = random.Random(0xA11E)
    ops = exact_ops(rng, LDS_TOP + 137, lens=(1, 2, 3), indel=(1, 2, 3))
    ops[20_000] = (8192, "M")  # the flat pass leaves the record (it keeps lengths below 8 192)
    return ops


_LINES = {}


def flat_lines():
    if "flat" not in _LINES:
        _LINES["flat"] = [(lab + s, place(ops, s, 2 * k + (s == "-"))) for k, (lab, ops) in enumerate(flat_shapes()) for s in "+-"]
    return _LINES["flat"]


def mixed_lines():
    """every shape in one batch: [(label, line)]"""
    if "mixed" not in _LINES:
        seqs = sequences()
        lines = list(flat_lines())
        eqx = [(1, "X"), (3, "I"), (1, "="), (2, "X"), (2, "D"), (300, "="), (1, "X"), (200, "="), (2, "I"), (1, "X"), (1, "="), (3, "X")]
        extra = [("len8192" + s, place(with_ends([(8192, "M")]), s, 60 + (s == "-"))) for s in "+-"]
        extra += [("eqx" + s, place(eqx, s, 64 + (s == "-"))) for s in "+-"]
        # no aligned base at all (the flat pass leaves such records): one row is all '-'
        extra += [("only_inserts" + s, place([(5, "I"), (200, "I")], s, 68 + (s == "-"))) for s in "+-"]
        extra += [("only_deletes" + s, place([(5, "D"), (200, "D")], s, 72 + (s == "-"))) for s in "+-"]
        nocg = b"qb\t%d\t10100\t10200\t+\ttb\t%d\t10300\t10400\t100\t100\t60\ttp:A:P\n" % (len(seqs["qb"]), len(seqs["tb"]))
        ops = arena_ops()
        qspan = sum(n for n, c in ops if c in "MI")
        # the - strand reads the query backwards from query_end: the record ends 2 000 bases in front of the contig's end
        arena = record(ops, "-", qname="qa", tname="ta", qlen=len(seqs["qa"]), tlen=len(seqs["ta"]), qs=len(seqs["qa"]) - 2000 - qspan, ts=2500, tags="tp:A:P\tAS:i:5").encode()
        half = len(lines) // 2
        _LINES["mixed"] = lines[:half] + extra[:2] + [("no_cigar", nocg)] + extra[2:] + lines[half:] + [("arena", arena)]
    return _LINES["mixed"]


def fixed_trim_lines():
    """260 aligned bases each: under F10 ten go at either end"""
    shapes = [("cut_inside_both_end_ops", [(100, "M"), (5, "I"), (160, "M")]),                         # sub_lo and sub_hi
              ("one_op_cut_twice", [(260, "M")]),                                                    # the window is one op: both cuts hit it
              ("whole_end_ops_go", [(10, "M"), (3, "I"), (240, "M"), (2, "D"), (10, "M")]),          # lo and n move, nothing is subtracted
              ("cut_inside_first_op_only", [(50, "M"), (2, "I"), (200, "M"), (3, "D"), (10, "M")]),  # sub_lo alone
              ("cut_inside_last_op_only", [(10, "M"), (2, "I"), (200, "M"), (3, "D"), (50, "M")])]   # sub_hi alone
    return [(lab + s, place(ops, s, 2 * k + (s == "-"))) for k, (lab, ops) in enumerate(shapes) for s in "+-"]


# ---- the oracle's side, computed once per (batch, stage list) ----
_WANT = {}


def ostages(stages):
    return [O.stage(*s) for s in stages if s[0] != STATS]


def expected(batch, lines, stages):
    """the records of the batch the stage list admits (the oracle runs them without an error), and per record (output line, rows,
    six sums): [(label, input line)], [(line, rows, sums)]"""
    key = (batch, repr(stages))
    if key not in _WANT:
        seqs = sequences()
        lines = list(lines)
        while True:  # a record the reference would stop at under this stage list (a trim of a record without a cigar, say) is left out
            out, err = O.run(ostages(stages), b"".join(l for _, l in lines), seqs)
            if err.code == 0:
                break
            del lines[err.record]
        outs = out.splitlines(keepends=True)
        assert len(outs) == len(lines)
        want = []
        for ln in outs:
            f = ln.split(b"\t")
            rc, text = O.pretty_print(ln, seqs[f[0].decode()], seqs[f[5].decode()])
            assert rc == 0
            sums = O.cigar_stats(cigar_of(ln).decode()) if b"cg:Z:" in ln else [0] * 6
            want.append((ln, text.split(b"\n", 1)[1], sums))
        _WANT[key] = (lines, want)
    return _WANT[key]


class Run:
    pass


def run_case(eng, batch, lines, stages):
    """plan the stage list over the batch's admitted records; sizes, rows (with a guard behind the host buffer) and sums against the
    oracle, record by record. The plan stays current: the Run keeps the device text alive."""
    import paffy_amd

    lines, want = expected(batch, lines, stages)
    n = len(lines)
    data = b"".join(l for _, l in lines)
    r = Run()
    r.labels, r.want, r.n = [lab for lab, _ in lines], want, n
    r.d_in = eng.to_device(data)
    info = eng.plan([paffy_amd.stage(*s) for s in stages], r.d_in, len(data))
    assert info.error.code == 0 and info.n_records == n, (info.error.code, info.error.record, info.n_records, n)
    r.sizes = eng.alignment_sizes(0, n)
    for lab, size, (_, rows, _) in zip(r.labels, r.sizes, want):  # before anything is fetched by these sizes
        assert size == len(rows), (lab, size, len(rows))
    got, err = eng.alignment_rows(0, n, guard=GUARD)
    assert err is None, err
    assert got[-GUARD:] == b"\xa5" * GUARD, "the guard behind the host buffer was written"
    r.rows = got[:-GUARD]
    r.offsets = [0]
    for b in r.sizes:
        r.offsets.append(r.offsets[-1] + b)
    for i, (lab, (ln, rows, _)) in enumerate(zip(r.labels, want)):
        block = r.rows[r.offsets[i]:r.offsets[i + 1]]
        if block != rows:
            at = next(k for k in range(len(rows)) if block[k] != rows[k])
            raise AssertionError("%s: rows differ from byte %d of %d: %r != %r" % (lab, at, len(rows), block[at:at + 40], rows[at:at + 40]))
    assert len(r.rows) == r.offsets[-1]
    if stages and stages[-1][0] == STATS:
        sums = eng.record_stats(n)
        for lab, s, (_, _, w) in zip(r.labels, sums, want):
            assert list(s) == w, (lab, s, w)
    r.flags, r.klass = eng.record_layout(0, n)
    r.left = eng.flat_stats()[0]
    return r


def index_of(r, label):
    return r.labels.index(label) if label in r.labels else None


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    e.keep_raw_sequences(True)
    e.set_sequences(sequences())
    yield e
    e.close()


@pytest.mark.parametrize("name", list(STAGE_LISTS))
def test_rows_and_sums_of_the_mixed_batch(eng, name):
    """every record shape in one plan, a record without cg:Z: (size 0) in the middle: row_off places every block, nothing is written past
    one (the guard), and each representation is the one the stage list should leave"""
    stages = STAGE_LISTS[name]
    r = run_case(eng, "mixed", mixed_lines(), stages)
    if name in ("none", "stats", "invert", "invert_invert"):
        assert r.n == len(mixed_lines()) and r.sizes[index_of(r, "no_cigar")] == 0  # these lists admit every shape
    has_cg = [b"cg:Z:" in ln for ln, _, _ in r.want]
    assert sum(s > 0 for s in r.sizes) > 30 or name == "trim_to_nothing"
    if name == "trim_to_nothing":  # cigar_trim takes every op of a record with an even count of aligned bases: the stats line alone
        assert sum(s == 0 for s in r.sizes) >= 8 and r.n > 30
        return
    for s in "+-":  # both strands of every shape stay in
        assert any(lab.endswith(s) for lab in r.labels)
    add = stages and stages[0][0] == O.ADD_MISMATCHES
    if not add:
        # the flat pass keeps lengths below 8 192: a record with an op of exactly 8 192 is left to the record kernels, which keep 4-byte
        # words in the mirror for it; its twin of 8 191 has 2-byte words whoever sized it
        for s in "+-":
            i, j = index_of(r, "len8192" + s), index_of(r, "len8191" + s)
            assert r.klass[i] == KLASS_LDS and r.flags[i] & MIRROR_BITS == 0, hex(r.flags[i])
            assert r.klass[j] == KLASS_LDS and r.flags[j] & MIRROR_BITS == HALF, hex(r.flags[j])
        assert r.klass[index_of(r, "arena")] == KLASS_ARENA
        assert sum(k == KLASS_ARENA for k in r.klass) == 1
        assert not any(f & (IN_ARENA | FLAT_ADD) for f in r.flags)  # only add_mismatches rebuilds the op array
    elif name == "add_flat":
        mine = [f for f, c in zip(r.flags, has_cg) if c and f & FLAT_ADD]
        assert mine and all(f & IN_ARENA for f in mine) and r.left < r.n, (len(mine), r.left)
    else:
        # FLAT_MODE_ADD is `add_mismatches` alone (classify_stages): behind any other stage the record kernels' encoder rebuilds the ops
        assert r.left == -1 and not any(f & FLAT_ADD for f in r.flags)
        assert any(f & IN_ARENA for f, k in zip(r.flags, r.klass) if k == KLASS_LDS)


def test_each_representation_under_each_view(eng):
    """the five forms the kernel reads ops in, each seen under a plain, an inverted and a fixed-trimmed view (the bytes are compared in
    every run). new_ops of the flat add pass exists under the plain view only: the pass runs for the one-stage list [ADD_MISMATCHES]
    (classify_stages, paffy_hip.hip), so no reversed, exchanged or shortened view is ever laid over it -- asserted as absent."""
    lists = {PLAIN: ("stats", "add_flat", "add_records"), INVERTED: ("invert", "add_invert"), TRIMMED: ("trim_fixed", "invert_trim_fixed", "add_trim_fixed")}
    seen = {}
    for view, names in lists.items():
        for name in names:
            batch, lines = ("flat", flat_lines()) if name in ("stats", "invert", "trim_fixed", "invert_trim_fixed") else ("mixed", mixed_lines())
            runs = [run_case(eng, batch, lines, STAGE_LISTS[name])]
            if batch == "flat":
                assert runs[0].left == 0  # sized by the flat pass: its 2-byte mirror
                runs.append(run_case(eng, "mixed", mixed_lines(), STAGE_LISTS[name]))
            for k, r in enumerate(runs):
                for lab, f, kl, (ln, _, _), size in zip(r.labels, r.flags, r.klass, r.want, r.sizes):
                    if size == 0:
                        continue
                    if view == INVERTED:
                        assert f & 4, (name, lab, hex(f))  # query / target exchanged
                    if kl == KLASS_ARENA:
                        form = "wide"
                    elif f & FLAT_ADD:
                        form = "arena4_flat_add"
                    elif f & IN_ARENA:
                        form = "arena4_records"
                    elif f & MIRROR_BITS == HALF:
                        form = "flat_mirror2" if batch == "flat" and k == 0 else "mirror2"
                    else:
                        form = "mirror4"
                    seen.setdefault((form, view), 0)
                    seen[(form, view)] += 1
    print(sorted(seen.items()))
    for form in ("flat_mirror2", "mirror4", "arena4_records", "wide"):
        for view in (PLAIN, INVERTED, TRIMMED):
            assert seen.get((form, view), 0) > 0, (form, view)
    assert seen.get(("arena4_flat_add", PLAIN), 0) > 0
    assert ("arena4_flat_add", INVERTED) not in seen and ("arena4_flat_add", TRIMMED) not in seen


@pytest.mark.parametrize("name", ["stats", "invert", "invert_invert", "trim_identity", "trim_fixed", "invert_trim_fixed"])
def test_records_the_flat_pass_sizes(eng, name):
    """the lean lists on records the flat pass takes: none is left to the record kernels, every mirror holds 2-byte words"""
    r = run_case(eng, "flat", flat_lines(), STAGE_LISTS[name])
    assert r.left == 0, (r.left, eng.flat_stats()[1])
    assert all(f & MIRROR_BITS == HALF for f, (ln, _, _) in zip(r.flags, r.want) if b"cg:Z:" in ln)
    assert all(k == KLASS_LDS for k in r.klass)
    if name in ("stats", "invert", "invert_invert"):
        assert r.n == len(flat_lines())


def test_lengths_of_8191_and_8192_take_different_paths(eng):
    lines = [("len8191+", place(with_ends([(8191, "M")]), "+", 1)), ("len8192+", place(with_ends([(8192, "M")]), "+", 2))]
    for name in ("stats", "invert", "trim_fixed"):
        r = run_case(eng, "pair8192", lines, STAGE_LISTS[name])
        assert r.left == 1, r.left  # the flat pass kept the first and left the second
        assert r.flags[0] & MIRROR_BITS == HALF and r.flags[1] & MIRROR_BITS == 0 and r.klass == [KLASS_LDS, KLASS_LDS]


def ops_of(cigar):
    import re

    return [(int(n), c.decode()) for n, c in re.findall(rb"(\d+)([MIDX=])", cigar)]


def test_identity_trim_cuts_whole_ops_from_both_ends(eng):
    """what the trim leaves is a stretch of the record's own ops (RecPlan lo > 0, n smaller): proven on the oracle's lines"""
    lines = [(lab, l) for lab, l in mixed_lines() if lab.startswith(("noisy_ends", "eqx"))]
    assert len(lines) == 4
    r = run_case(eng, "noisy", lines, STAGE_LISTS["trim_identity"])
    front = back = 0
    for (lab, src), (ln, _, _) in zip(lines, r.want):
        a, b = ops_of(cigar_of(src)), ops_of(cigar_of(ln))
        starts = [k for k in range(len(a) - len(b) + 1) if a[k:k + len(b)] == b]
        assert len(b) < len(a) and starts, lab  # whole ops went, none was shortened
        front += starts[0] > 0
        back += starts[-1] + len(b) < len(a)
    assert front > 0 and back > 0, (front, back)
    run_case(eng, "noisy", lines, [INV, TRI, ST])
    run_case(eng, "noisy", lines, [TRI, INV, ST])


def test_fixed_trim_cuts_inside_the_end_ops(eng):
    """`trim -f` of ten bases an end: the cut inside the first op, inside the last, inside both, twice inside the only op, and on an op
    boundary (the shapes are proven on the oracle's cigars); alone, in front of and behind an invert -- the reversed view subtracts from
    the raw first and last op, not from the view's"""
    lines = fixed_trim_lines()
    fix = (O.TRIM_FIXED, 0.05, F10)
    r = run_case(eng, "fixed", lines, [fix])
    got = {lab: ops_of(cigar_of(ln)) for lab, (ln, _, _) in zip(r.labels, r.want)}
    for s in "+-":
        assert got["cut_inside_both_end_ops" + s] == [(90, "M"), (5, "I"), (150, "M")]
        assert got["one_op_cut_twice" + s] == [(240, "M")]
        assert got["whole_end_ops_go" + s] == [(240, "M")]
        assert got["cut_inside_first_op_only" + s] == [(40, "M"), (2, "I"), (200, "M")]
        assert got["cut_inside_last_op_only" + s] == [(200, "M"), (3, "D"), (40, "M")]
    assert r.left == 0
    for stages in ([fix, ST], [INV, fix], [INV, fix, ST], [fix, INV, ST], [INV, INV, fix], [ADD, fix, ST], [ADD, INV, fix, ST]):
        r = run_case(eng, "fixed", lines, stages)
        assert r.n == len(lines) and all(s > 0 for s in r.sizes)


def test_first_count_and_fetching_in_pieces(eng):
    r = run_case(eng, "mixed", mixed_lines(), STAGE_LISTS["invert"])
    n, whole = r.n, r.rows
    cuts = [0, n // 3, n // 2 + 1, n]  # the record without a cigar and the arena record lie in different pieces
    pieces = []
    for a, b in zip(cuts, cuts[1:]):
        rows, err = eng.alignment_rows(a, b - a, offsets=r.offsets[a:b + 1], guard=GUARD)  # a slice of the batch's offsets: h_off[0] > 0
        assert err is None and rows[-GUARD:] == b"\xa5" * GUARD
        assert eng.alignment_sizes(a, b - a) == r.sizes[a:b]
        pieces.append(rows[:-GUARD])
    assert b"".join(pieces) == whole
    assert r.offsets[cuts[1]] > 0
    mine, err = eng.alignment_rows(cuts[1], cuts[2] - cuts[1])  # offsets built from the sizes of the piece
    assert err is None and mine == pieces[1]
    shifted, err = eng.alignment_rows(0, n, offsets=[o + 12_345 for o in r.offsets])
    assert err is None and shifted == whole
    assert eng.alignment_rows(5, 0) == (b"", None) and eng.alignment_rows(n, 0) == (b"", None) and eng.alignment_sizes(3, 0) == []
    for first, count in ((0, n + 1), (n, 1), (n - 1, 2), (-1, 1)):
        with pytest.raises(RuntimeError, match=r"\(-2\)"):  # PAFFY_E_ARG
            eng.alignment_rows(first, count, offsets=[0] * (count + 1))
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            eng.alignment_sizes(first, count)
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            eng.record_layout(first, count)


def test_missing_sequences_and_ranges_are_reported_by_batch_index():
    """err.record is the record's index in the planned batch, also where the call starts behind the batch's first record, and of several
    failing records the smallest is named"""
    import paffy_amd

    rng = random.Random(0xA11F)
    seqs = {"q1": make_seq(rng, 1000), "t1": make_seq(rng, 1000), "qshort": make_seq(rng, 300), "tcut": make_seq(rng, 650)}

    def rec(qn, tn, qs, ts, n=100, strand="+", qlen=1000, tlen=1000):
        return record([(n // 2, "M"), (2, "I"), (n - n // 2, "M")], strand, qname=qn, tname=tn, qlen=qlen, tlen=tlen, qs=qs, ts=ts).encode()

    good = rec("q1", "t1", 100, 200)
    e = paffy_amd.Engine()
    try:
        e.keep_raw_sequences(True)
        e.set_sequences(seqs)
        # names that are not among the sequences
        data = good + good + rec("nobody", "t1", 100, 200) + good + rec("q1", "nothing", 100, 200, strand="-")
        d_in = e.to_device(data)
        for stages in ([ST], [INV, ST]):
            assert e.plan([paffy_amd.stage(*s) for s in stages], d_in, len(data)).error.code == 0
            inv = len(stages) == 2  # behind an invert the missing name is the other side's
            assert e.alignment_rows(0, 5)[1] == (ERR_MISSING_TARGET if inv else ERR_MISSING_QUERY, 2)  # records 2 and 4 fail: the smaller
            assert e.alignment_rows(3, 2)[1] == (ERR_MISSING_QUERY if inv else ERR_MISSING_TARGET, 4)  # first > 0: still the batch's index
            assert e.alignment_rows(4, 1)[1] == (ERR_MISSING_QUERY if inv else ERR_MISSING_TARGET, 4)
            assert e.alignment_rows(0, 2)[1] is None and e.alignment_rows(3, 1)[1] is None
        # coordinates beyond the loaded sequence (the lengths in the lines say 1 000)
        crossed = rec("qshort", "t1", 100, 600, qlen=300)  # fits: its query range would not fit the target's place and the other way round
        far_q = rec("qshort", "t1", 250, 200)              # query_end 352 > 300 loaded
        far_t = rec("q1", "tcut", 100, 600, strand="-")    # target_end 700 > 650 loaded
        data = crossed + far_q + good + far_t
        d_in = e.to_device(data)
        for stages in ([ST], [INV, ST], [INV, INV, ST]):
            assert e.plan([paffy_amd.stage(*s) for s in stages], d_in, len(data)).error.code == 0
            assert e.alignment_rows(0, 4)[1] == (ERR_SEQ_RANGE, 1)
            assert e.alignment_rows(2, 2)[1] == (ERR_SEQ_RANGE, 3)
            assert e.alignment_rows(1, 1)[1] == (ERR_SEQ_RANGE, 1) and e.alignment_rows(3, 1)[1] == (ERR_SEQ_RANGE, 3)
            rows, err = e.alignment_rows(0, 1)  # after an invert the range is checked against the exchanged sequence: this one fits
            assert err is None
            ln = O.run(ostages(stages), crossed)[0]
            f = ln.split(b"\t")
            assert rows == O.pretty_print(ln, seqs[f[0].decode()], seqs[f[5].decode()])[1].split(b"\n", 1)[1]
        # a missing name is found before a range (the reference never gets to read the sequence)
        data = good + rec("nobody", "tcut", 100, 600)
        d_in = e.to_device(data)
        assert e.plan([paffy_amd.stage(*ST)], d_in, len(data)).error.code == 0
        assert e.alignment_rows(0, 2)[1] == (ERR_MISSING_QUERY, 1)
    finally:
        e.close()


def test_rows_need_raw_sequences_and_a_current_record_plan():
    import paffy_amd

    seqs = sequences()
    data = b"".join(l for _, l in fixed_trim_lines())
    e = paffy_amd.Engine()
    try:
        e.set_sequences(seqs)  # without keep_raw_sequences: the upper-cased store alone
        d_in = e.to_device(data)
        st = [paffy_amd.stage(*ST)]
        assert e.plan(st, d_in, len(data)).error.code == 0
        for call in (lambda: e.alignment_sizes(0, 1), lambda: e.alignment_rows(0, 1, offsets=[0, 0])):
            with pytest.raises(RuntimeError, match=r"\(-5\)"):  # PAFFY_E_STATE
                call()
        e.keep_raw_sequences(True)
        e.set_sequences(seqs)
        assert e.plan(st, d_in, len(data)).error.code == 0
        assert sum(e.alignment_sizes(0, 10)) > 0 and len(e.record_layout(0, 10)[0]) == 10
        # a tile or dedupe plan since: the record plan's buffers describe nothing any more (test_gpu_to_bed.py, for this entry point)
        for other in (lambda: e.tile(data), lambda: e.dedupe(data)):
            assert e.plan(st, d_in, len(data)).error.code == 0
            assert e.alignment_rows(0, 2)[1] is None
            other()
            for call in (lambda: e.alignment_sizes(0, 1), lambda: e.alignment_rows(0, 1, offsets=[0, 0]), lambda: e.record_layout(0, 1), lambda: e.record_stats(10)):
                with pytest.raises(RuntimeError, match=r"\(-5\)"):
                    call()
    finally:
        e.close()


def test_cli_names_the_failing_record_by_its_input_position(tmp_path):
    """`bin/paffy view -a` on a file whose third record names a query that is in no FASTA file: stderr and exit status are those of the
    same record failing as the first of its batch at the same input position (batches of 1 MiB: the first three lines carry a tag of
    600 KB each, so no two of them share a batch and the third line opens the last one; the two lines printed in full show that).
    The command's own add_mismatches stage looks the names up first, so it is the plan that reports this record; the rows of a batch
    are fetched in pieces of at most 128 MiB, and a record that fails in a second piece cannot be had at test size, so the meaning of
    err->record behind the first piece is pinned through the C-ABI alone (test_missing_sequences_and_ranges_are_reported_by_batch_index)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    seqs = sequences()
    ops = [(40, "M"), (2, "I"), (58, "M")]
    pad = "tp:A:P\tAS:i:9\tzz:Z:" + "p" * 600_000
    kw = dict(qlen=len(seqs["qb"]), tlen=len(seqs["tb"]), qs=12_000, ts=13_000)
    good = record(ops, "+", qname="qb", tname="tb", tags=pad, **kw)
    bad = record(ops, "-", qname="stranger", tname="tb", tags=pad, **kw)  # as long: the batch of the second line has no room for it
    paf, fa = tmp_path / "in.paf", tmp_path / "s.fa"
    paf.write_text(good + good + bad + good.replace(pad, "tp:A:P"))
    with open(fa, "wb") as fh:
        for name in ("qb", "tb"):
            fh.write(b">" + name.encode() + b"\n" + seqs[name] + b"\n")
    runs = [subprocess.run([PAFFY, "view", "-a", "-i", str(paf), str(fa)], capture_output=True, env=dict(os.environ, **env), timeout=120)
            for env in ({}, {"PAFFY_CHUNK_MB": "1"})]
    one_batch, one_record_batches = runs
    assert one_batch.returncode == 1 and one_batch.stderr == b"No query sequence found for record 2\n", (one_batch.returncode, one_batch.stderr[-300:])
    assert (one_record_batches.returncode, one_record_batches.stderr) == (one_batch.returncode, one_batch.stderr)
    # the records in front of it were printed in both runs
    ln = (good.replace(pad, "tp:A:P\tAS:i:9")).encode()
    want = O.pretty_print(O.run([O.stage(O.ADD_MISMATCHES)], ln, seqs)[0], seqs["qb"], seqs["tb"])[1]
    assert one_record_batches.stdout == want + want

"""Inputs of the flat pass's stage lists with a fixed trim (`paffy trim -f`) in front of other stages (paffy_amd/csrc/flat_kernel.h,
FlatCuts). Not a test module: test_flat_fixed_pipe_cpu.py proves on the oracle that the inputs hit their cases,
test_gpu_flat_fixed_pipe.py runs the same bytes on the GPU.

A pipe here is a list of stage kinds; every TRIM_FIXED of it takes the fraction the caller names, every TRIM_IDENTITY the defaults. The
oracle knows neither the stats stage (to it a PASS: `paffy view -s` reads what the pipe wrote) nor dechunk (chunk_lib restates it): expected() applies
the latter to the text first."""
import hashlib
import random
import re

import chunk_lib as K
import float_edges as E
import oracle_lib as O
from test_gpu_flat import random_ops, record

FIX, INV, TRI, PAS, FIL, SHA = O.TRIM_FIXED, O.INVERT, O.TRIM_IDENTITY, O.PASS, O.FILTER, O.SHATTER
STATS, DECHUNK = 10, 12  # PAFFY_STATS, PAFFY_DECHUNK
WHY_IRREG, WHY_EMPTY, WHY_STAGE, WHY_NONPLAIN = 1, 3, 6, 7  # FLAT_WHY_* of flat_kernel.h

PIPES = {
    "fix_invert": [FIX, INV], "fix_pass": [FIX, PAS], "fix_filter": [FIX, FIL], "fix_stats": [FIX, STATS], "fix_trim": [FIX, TRI],
    "fix_fix": [FIX, FIX], "fix_invert_fix": [FIX, INV, FIX], "fix_trim_fix": [FIX, TRI, FIX], "invert_fix_trim_filter": [INV, FIX, TRI, FIL],
    "trim_fix_invert_stats": [TRI, FIX, INV, STATS], "dechunk_fix_invert": [DECHUNK, FIX, INV],
}
SHATTER_PIPES = {"fix_shatter": [FIX, SHA], "fix_invert_shatter": [FIX, INV, SHA]}  # stay with the record kernels
FRACTIONS = (0.0, 0.001, 0.1, 0.5, 0.999)
STRANDS = "+-"


# ---- running a pipe ----
def oracle_stages(pipe, frac):
    """the stats stage is `paffy view -s` behind a pipe of its own: to the oracle a PASS (the record is written and parsed again)"""
    return [O.stage(PAS if k == STATS else k, 0.05, frac if k == FIX else 1.0) for k in pipe if k != DECHUNK]


def gpu_stages(pipe, frac):
    import paffy_amd

    return [paffy_amd.stage_dechunk() if k == DECHUNK else paffy_amd.stage(k, 0.0, 0.0) if k == STATS else paffy_amd.stage(k, 0.05, frac if k == FIX else 1.0)
            for k in pipe]


_WANT = {}


def expected(pipe, frac, data, tag=None):
    """(error code, error record, output) of the oracle; tag keeps runs under different filter thresholds apart"""
    key = (tuple(pipe), frac, hashlib.sha256(data).hexdigest(), tag)
    if key not in _WANT:
        text = data
        if DECHUNK in pipe:
            text, fail = K.dechunk(data)
            assert fail is None
        out, err = O.run(oracle_stages(pipe, frac), text)
        _WANT[key] = (err.code, err.record, out)
    return _WANT[key]


def check(eng, pipe, frac, data, tag=None):
    """the GPU's run against the oracle's: the error code and record, the output's length, its SHA-256; with a stats stage (the pipe's
    last) the six sums of every record that came through. Returns (records left to the record kernels, counts per reason)."""
    wcode, wrec, want = expected(pipe, frac, data, tag)
    got, info = eng.run(gpu_stages(pipe, frac), data, raise_on_error=False)
    left, why = eng.flat_stats()
    print("flat stats", pipe, frac, tag, left, list(why)[:12])
    assert info.error.code == wcode and (wcode == 0 or info.error.record == wrec), (pipe, frac, info.error.code, wcode, info.error.record, wrec)
    assert len(got) == len(want), (pipe, frac, len(got), len(want))
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest(), (pipe, frac)
    if STATS in pipe and wcode == 0:
        assert pipe[-1] == STATS
        n_in = data.count(b"\n")
        sums = eng.record_stats(n_in)
        outs = want.splitlines()
        assert len(outs) == n_in  # no filter in these pipes: a line per record
        for i, (s, ln) in enumerate(zip(sums, outs)):
            assert list(s) == (O.cigar_stats(cigar_of(ln).decode()) if b"cg:Z:" in ln else [0] * 6), (pipe, frac, i)
    return left, why


class Thresholds:
    """filter thresholds for the oracle and the engine alike, reset on the way out"""

    def __init__(self, eng=None, **thr):
        self.eng, self.thr = eng, thr

    def __enter__(self):
        O.set_filter(**self.thr)
        if self.eng is not None:
            self.eng.set_filter(**self.thr)

    def __exit__(self, *exc):
        O.set_filter()
        if self.eng is not None:
            self.eng.set_filter()


# ---- reading lines ----
def cigar_of(line):
    return line.split(b"cg:Z:")[1].split(b"\t")[0].strip()


def ops_of(line):
    if isinstance(line, str):
        line = line.encode()
    return [(int(n), c.decode()) for n, c in re.findall(rb"(\d+)([MID=X])", cigar_of(line))]


def aligned(ops):
    return sum(L for L, c in ops if c in "M=X")


def end_of(ops, frac):
    """bases a fixed trim takes at either end (impl/paf.c:593)"""
    return E.fixed_end(aligned(ops), frac)[0]


def t_bases(ops):
    return sum(L for L, c in ops if c != "I")


def fixed_cuts(in_line, out_line):
    """What a fixed trim did, from its input and output line: (f, s0, b, s1) -- f ops went at the front of the text and b at its back, the
    op the front cut stopped in lost s0 bases and the one the back cut stopped in s1 (the same op when one is left). The target start
    moves over the front's ops and s0."""
    a, t = ops_of(in_line), ops_of(out_line)
    d_ts = int(out_line.split(b"\t")[7]) - int(in_line.split(b"\t")[7])
    found = []
    for f in range(len(a) - len(t) + 1):
        w = a[f:f + len(t)]
        if [c for _, c in w] != [c for _, c in t] or w[1:-1] != t[1:-1]:
            continue
        s0 = d_ts - t_bases(a[:f])
        if len(t) == 1:
            s1 = w[0][0] - t[0][0] - s0
        else:
            s1 = w[-1][0] - t[-1][0]
            if w[0][0] - t[0][0] != s0:
                continue
        if s0 < 0 or s1 < 0 or (s0 and w[0][1] not in "M=X") or (s1 and w[-1][1] not in "M=X"):
            continue
        found.append((f, s0, len(a) - len(t) - f, s1))
    assert len(found) == 1, (found, a[:4], t[:4])
    return found[0]


def stretch_cuts(in_line, out_line):
    """(ops gone at the front of the text, at its back) where the output's cigar is a stretch of whole ops of the input's (identity trim)"""
    a, t = ops_of(in_line), ops_of(out_line)
    d_ts = int(out_line.split(b"\t")[7]) - int(in_line.split(b"\t")[7])
    found = [f for f in range(len(a) - len(t) + 1) if a[f:f + len(t)] == t and t_bases(a[:f]) == d_ts]
    assert len(found) == 1, (found, len(a), len(t))
    return found[0], len(a) - len(t) - found[0]


def run1(kind, line, frac=1.0):
    out, err = O.run([O.stage(kind, 0.05, frac)], line if isinstance(line, bytes) else line.encode())
    assert err.code == 0, err.code
    return out


def with_end_op(line, which, length):
    """the line with its first (which 0) / last (-1) op given another length, the coordinates consistent again"""
    f = line.decode().rstrip("\n").split("\t")
    ops = ops_of(line)
    ops[which] = (length, ops[which][1])
    return record(ops, f[4], qname=f[0], tname=f[5], qs=int(f[2]), ts=int(f[7])).encode()


# ---- case 1: regular records ----
def regular_batch(n=40, seed=7301):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        k = rng.choice([1, 2, 3, 5, 9, 30, 64, 65, 200, 700, 1500])
        recs.append(record(random_ops(rng, k), STRANDS[i & 1], tags="tp:A:P\tAS:i:%d\ts1:i:42" % (100 + i), rng=rng))
    return "".join(recs).encode()


# ---- case 2: where the cuts land (fraction 0.1 of 2 000 aligned bases: 100 at either end, unless said otherwise) ----
def middle_ops(k):
    """indel ops whose text is k bytes (k = 0 or k >= 2)"""
    ops, i = [], 0
    while k:
        n = 3 if k == 3 or k >= 5 else 2
        ops.append((12 if n == 3 else 4, "ID"[i & 1]))
        k -= n
        i += 1
    return ops


LANDINGS = {  # name -> (ops, fraction)
    "inside_first_and_last": ([(300, "M"), (5, "I"), (1400, "M"), (4, "D"), (300, "M")], 0.1),
    "on_boundary_i_d_next": ([(100, "M"), (7, "I"), (1800, "M"), (6, "D"), (100, "M")], 0.1),
    "on_boundary_d_i_next": ([(100, "M"), (7, "D"), (1800, "M"), (6, "I"), (100, "M")], 0.1),
    "one_op_record": ([(2000, "M")], 0.1),
    "both_cuts_in_one_op": ([(40, "M"), (3, "D"), (1920, "M"), (2, "I"), (40, "M")], 0.1),
    "digits_1000_to_999_and_10_to_9": ([(1000, "M"), (3, "D"), (990, "M"), (2, "I"), (10, "M")], 0.001),
    "digits_1099_to_999_and_109_to_9": ([(1099, "M"), (3, "I"), (792, "M"), (2, "D"), (109, "M")], 0.1),
    "digits_10_to_9_twice": ([(10, "M"), (2, "I"), (1980, "M"), (1, "D"), (10, "M")], 0.001),
}
for _k in [0] + list(range(2, 18)):
    LANDINGS["middle_%d_bytes" % _k] = ([(300, "M")] + middle_ops(_k) + [(300, "M")], 0.1)
LANDING_PIPES = ("fix_invert", "fix_filter", "fix_stats", "fix_pass")


def landing_batch(frac):
    names = [n for n in sorted(LANDINGS) if LANDINGS[n][1] == frac]
    lines = [record(LANDINGS[n][0], s, qname="q_" + n) for n in names for s in STRANDS]
    return [(n, s) for n in names for s in STRANDS], lines


# ---- case 3: a second fixed trim (0.1 twice: 100 of 2 000 bases, then 90 of 1 800) ----
SECONDS = {
    "ends_inside_the_shortened_op": [(1000, "M"), (3, "I"), (1000, "M")],            # 900M left, 90 more go
    "consumes_it_exactly": [(190, "M"), (3, "I"), (1620, "M"), (2, "D"), (190, "M")],  # 90M left and 90 go: the indel behind it too
    "stops_in_the_next_match_op": [(150, "M"), (3, "I"), (1700, "M"), (2, "D"), (150, "M")],  # 50M left: 40 more from 1700M
    "consumes_it_exactly_x": [(190, "X"), (3, "D"), (1620, "M"), (2, "I"), (190, "X")],
}
SECOND_PIPES = ("fix_fix", "fix_invert_fix")


def second_batch():
    names = sorted(SECONDS)
    return [(n, s) for n in names for s in STRANDS], [record(SECONDS[n], s, qname="q_" + n) for n in names for s in STRANDS]


# ---- case 4: identity trim behind a fixed trim ----
def noise(n, gap=30):
    """short matches between indels: n pairs of (gap D or I, 1 M)"""
    out = []
    for i in range(n):
        out += [(gap, "DI"[i & 1]), (1, "M")]
    return out


def _mirror(ops):
    return ops[::-1]


# the far end is clean (thousands of M, 2I), so that only the end under test is trimmed; the core in ops the flat pass takes (below 8 192)
_CORE = E.split(18000, "M")
_A = [(1060, "M")] + noise(20) + _CORE + [(2, "I"), (2000, "M")]  # aligned 21 080: 1 054 go, 6M is left in front of the noise
_C = [(1300, "M"), (30, "D"), (1, "M"), (30, "I")] + _CORE + [(2, "I"), (2000, "M")]  # 1 065 go: 235M, 30D is a hit (0.887 < 0.947), 1300M, 30D is none
# 0.01 of 24 000: 120 go. 5X, 300M, 10D is no hit (0.952 > 0.949); 125X, 300M, 10D is one, and no suffix of it is kept
_X = [(125, "X"), (300, "M"), (10, "D")] + _CORE + [(2, "I"), (5575, "M")]
TRIMS = {  # name -> (ops, fraction)
    # the trim removes the shortened op and more
    "removes_the_shortened_op_and_more": (_A, 0.1),
    # the trim removes the shortened op and the noise behind it; with the op's uncut length (1 300M) no prefix is a hit: nothing would go
    "removes_only_because_of_the_cut": (_C, 0.1),
    # the back of the text: what the second (inverted) pass of a '-' record cuts, where the other shortened op is
    "back_removes_the_shortened_op_and_more": (_mirror(_A), 0.1),
    "back_removes_only_because_of_the_cut": (_mirror(_C), 0.1),
    # a shortened X op always goes (its prefix has identity 0); the ops behind it stay only because it is short: see test_flat_fixed_pipe_cpu
    "x_op_stays_short_of_a_second_hit": (_X, 0.01),
    "back_x_op_stays_short_of_a_second_hit": (_mirror(_X), 0.01),
}
TRIM_PIPES = ("fix_trim", "fix_trim_fix", "invert_fix_trim_filter")
TRIM_FRACTIONS = (0.1, 0.01)


def trim_batch(frac):
    names = [n for n in sorted(TRIMS) if TRIMS[n][1] == frac]
    return [(n, s) for n in names for s in STRANDS], [record(TRIMS[n][0], s, qname="q_" + n) for n in names for s in STRANDS]


# ---- case 5: long records ----
def long_record(n_ops, strand, seed):
    rng = random.Random(seed)
    return record(random_ops(rng, n_ops, lens=(1, 2, 7, 12, 40, 99, 150), indel=(1, 2, 3)), strand, rng=rng)


# ---- case 6: who leaves ----
def even_batch():
    """records with an even count of aligned bases: a fixed trim of 1.0 takes everything"""
    rng = random.Random(7306)
    recs = []
    for i in range(8):
        ops = random_ops(rng, rng.choice([1, 3, 9, 41]))
        if aligned(ops) & 1:
            ops[0] = (ops[0][0] + 1, "M")
        recs.append(record(ops, STRANDS[i & 1], rng=rng))
    return "".join(recs).encode()


def irregular_batch():
    rng = random.Random(7307)
    recs = [record(random_ops(rng, 9), STRANDS[i & 1], rng=rng) for i in range(6)]
    recs.insert(3, record([(500, "M"), (3, "I"), (8192, "M"), (2, "D"), (500, "M")], "-", rng=rng))
    return "".join(recs).encode()


def nonplain_batch():
    rng = random.Random(7308)
    recs = [record(random_ops(rng, 9), STRANDS[i & 1], rng=rng) for i in range(6)]
    recs.insert(1, record([(300, "="), (5, "X"), (3, "I"), (900, "="), (2, "D"), (300, "=")], "+", rng=rng))
    recs.insert(4, record([(300, "M"), (5, "X"), (3, "I"), (900, "M"), (2, "D"), (300, "M")], "-", rng=rng))
    return "".join(recs).encode(), 2


# ---- case 7: filter at a tie behind the trim ----
TIES = {
    "first_op_m_last_op_x": [(500, "M"), (30, "X"), (3, "I"), (1400, "M"), (20, "X"), (2, "D"), (700, "M"), (350, "X")],
    "first_op_x_last_op_m": [(400, "X"), (700, "M"), (3, "D"), (1300, "M"), (20, "X"), (2, "I"), (580, "M")],
}


def tie_batch(name):
    return [record(TIES[name], s, qname="q_" + name) for s in STRANDS]


def window_sums(line):
    """(M and = bases, X bases) of a line's cigar: what the filter's identity is made of"""
    ops = ops_of(line)
    return sum(L for L, c in ops if c in "M="), sum(L for L, c in ops if c == "X")


def tie_thresholds(name, frac=0.1):
    """min_identity on the float32 identity of the trimmed window and one float32 step to either side: [(steps, threshold)]"""
    out = run1(FIX, tie_batch(name)[0], frac)
    m, x = window_sums(out)
    t0 = E.quot(m, m + x)
    return [(u, float(E.step(t0, u))) for u in (-1, 0, 1)], (m, x)

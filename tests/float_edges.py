"""Records at the float32 edges of the reference's threshold decisions (not a test module: test_float_edges_cpu.py proves every family
sharp on the oracle, test_gpu_float_edges.py runs them on the GPU).

The reference decides an identity trim, a filter and a chain trim from `(float)a / (a + b)` or `(float)n * fraction`, widened or truncated
afterwards (oracle/paf_oracle.c: trim_scan, trim_prefix, trim_identity, trim_fixed, filter_keeps, po_chain). The expressions are restated
here with numpy float32 -- the only arithmetic this module does -- to FIND operands whose quotient equals a threshold, sits a given number
of float32 steps beside it or a given relative distance from it, and to lay them into records whose totals are fixed: the thresholds of
a record come from its totals, so they do not move when the probe changes. What the oracle then does with the records is not computed
here; the CPU test reads it from the oracle's output."""
from fractions import Fraction

import numpy as np

from test_gpu_flat import record

F = np.float32
TWO24 = 1 << 24
OP_MAX = 8191  # the longest op the flat pass parses (13 bits)


# ---- the reference's expressions ----
def f32(n):
    """(float)n of an integer below 2^53: round to nearest even"""
    return F(n)


def quot(a, d):
    """(float)a / d of the reference: both operands converted, one float32 divide"""
    return F(f32(a) / f32(d))


def step(t, ulps):
    """the float32 `ulps` steps above (below) t"""
    t = F(t)
    for _ in range(abs(ulps)):
        t = np.nextafter(t, F(4.0) if ulps > 0 else F(-4.0))
    return t


def thresholds(m, x, p0, p1):
    """(thr_f, id_f, max_trim) of trim_identity for a record of m match and x other bases"""
    identity = float(quot(m, m + x))
    thr = identity - identity * float(F(p0))
    return F(thr), F(identity), int(F(f32(m + x) * F(p1)))


def fixed_end(aligned, pct):
    """trim_fixed: bases cut at either end; and the two near misses -- the product in double, the conversion truncated"""
    ref = int(float(F(f32(aligned) * F(pct))) / 2.0)
    in_double = int(float(aligned) * float(F(pct)) / 2.0)
    return ref, in_double, int(float(F(trunc32(aligned) * F(pct))) / 2.0)


def trunc32(n):
    """(float)n rounded towards zero: what a truncating conversion would give"""
    f = F(n)
    return f if int(f) <= n else np.nextafter(f, F(0.0))


def chain_trim(length, pct):
    """po_chain: bases taken off either end of an alignment whose query and target spans are both `length`; and the two near misses"""
    ref = int(F(f32(length) * F(pct))) // 2
    return ref, int(float(length) * float(F(pct))) // 2, int(F(trunc32(length) * F(pct))) // 2


def max_trim_of(total, p1):
    """trim_identity's max_trim; and the two near misses"""
    return int(F(f32(total) * F(p1))), int(float(total) * float(F(p1))), int(F(trunc32(total) * F(p1)))


# ---- operands at a distance from a threshold ----
def pairs_at(t, lo_den, hi_den):
    """every (a, d), lo_den <= d < hi_den, 0 < a < d, with (float)a / (float)d == t, by d"""
    t = F(t)
    d = np.arange(lo_den, hi_den, dtype=np.int64)
    a0 = np.floor(np.float64(t) * d.astype(np.float64)).astype(np.int64)
    got = []
    for da in (-2, -1, 0, 1, 2, 3):
        a = a0 + da
        ok = (a > 0) & (a < d) & ((a.astype(F) / d.astype(F)) == t)
        got += list(zip(d[ok].tolist(), a[ok].tolist()))
    return [(a, dd) for dd, a in sorted(set(got))]


def near(thr_f, ulps, lo_den, hi_den, rounds=False, exact=None, ok=None):
    """(a, b) with (float)a / (float)(a + b) exactly `ulps` float32 steps from thr_f, the smallest a + b with lo_den <= a + b < hi_den.
    rounds: a or a + b is above 2^24 and odd (its conversion rounds).
    exact: "below" / "above" -- the exact fraction a / (a + b) is below / not below the exact value of thr_f (where the float quotient and
    the exact fraction disagree about the threshold, a decision taken in higher precision goes wrong).
    ok: a further condition on (a, b)."""
    t = step(thr_f, ulps)
    cand = pairs_at(t, lo_den, hi_den)
    if rounds:
        cand = [(a, d) for a, d in cand if (a > TWO24 and a & 1) or (d > TWO24 and d & 1)]
    if exact:
        ft = Fraction(float(F(thr_f)))
        cand = [(a, d) for a, d in cand if (Fraction(a, d) < ft) == (exact == "below")]
    if ok:
        cand = [(a, d) for a, d in cand if ok(a, d - a)]
    assert cand, (thr_f, ulps, lo_den, hi_den, rounds, exact)
    a, d = cand[0]
    assert quot(a, d) == t
    return a, d - a


def near_rel(thr_f, rel, lo_den, hi_den, ok=None):
    """(a, b) whose float32 quotient is as close as the range allows to thr_f * (1 + rel): the edges of a band round the threshold"""
    want = float(F(thr_f)) * (1.0 + rel)
    d = np.arange(lo_den, hi_den, dtype=np.int64)
    best = None
    for da in (0, 1):
        a = np.floor(want * d.astype(np.float64)).astype(np.int64) + da
        q = (a.astype(F) / d.astype(F)).astype(np.float64)
        err = np.abs(q / float(F(thr_f)) - (1.0 + rel))
        for i in np.argsort(err)[:50]:
            if ok is None or ok(int(a[i]), int(d[i] - a[i])):
                if best is None or err[i] < best[0]:
                    best = (float(err[i]), int(a[i]), int(d[i] - a[i]))
                break
    assert best is not None and best[0] < 2e-7, (thr_f, rel, best)
    return best[1], best[2]


# ---- records ----
def split(n, letter, op=OP_MAX, small_first=False):
    """n bases as ops of at most `op`"""
    ops = [(op, letter)] * (n // op) + ([(n % op, letter)] if n % op else [])
    return ops[::-1] if small_first else ops


EARLY_HIT = [(1, "M"), (30, "D"), (8000, "M")]  # a clear hit at index 1 (1 / 31), then the identity is back above every threshold used


def rest_ops(m_left, x_left, front_m, rest_op=OP_MAX, irregular=None, x_op=OP_MAX):
    """what is left of the totals behind a probe, laid so that no prefix that ends in it is a hit: front_m match bases, every other
    base (as D ops), the remaining match bases. irregular: a length the flat pass does not take, as one op in the anchor."""
    front_m = min(front_m, m_left)
    ops = []
    if irregular:
        ops.append((irregular, "M"))
        front_m -= irregular
        m_left -= irregular
        assert front_m >= 0
    return ops + split(front_m, "M", rest_op) + split(x_left, "D", x_op) + split(m_left - front_m, "M", rest_op)


def lt_prefix(a, b, n_pad=0, pad_m=200, early=False, op_max=OP_MAX, d_run=0):
    """ops with a match and b other bases, the probe's op last: an early clear hit (early), n_pad pairs of pad_m M, 1 D (their prefixes
    are far above the threshold), the rest of a as M ops, the rest of b as D ops, the shortest first -- or, with d_run, as that many D
    ops of two digits: no match base between them, so a bound taken anywhere inside the run IS the probe's quotient"""
    ops = list(EARLY_HIT) if early else []
    ops += [(pad_m, "M"), (1, "D")] * n_pad
    ua = sum(L for L, c in ops if c == "M")
    ub = sum(L for L, c in ops if c != "M")
    assert a > ua and b > ub, (a, b, ua, ub)
    if d_run:
        run = [(10 + i % 8, "D") for i in range(d_run - 1)]
        left = b - ub - sum(L for L, _ in run)
        assert left > 0, (b, ub, left)
        return ops + split(a - ua, "M", op_max) + split(left, "D", op_max) + run
    return ops + split(a - ua, "M", op_max) + split(b - ub, "D", op_max, small_first=True)


def lt_ops(a, b, m, x, n_pad=0, pad_m=200, early=False, front_m=500_000, rest_op=OP_MAX, irregular=None, op_max=OP_MAX, d_run=0):
    """(ops, k): a record of m match and x other bases whose prefix [0..k] has a match and b other bases -- the probe of the scan for
    the last hit (trim_scan: q < thr)"""
    ops = lt_prefix(a, b, n_pad, pad_m, early, op_max, d_run)
    return ops + rest_ops(m - a, x - b, front_m, rest_op, irregular, op_max), len(ops) - 1


def ge_ops(big_a, b, m, x, junk, front_m=500_000, rest_op=OP_MAX, irregular=None, op_max=OP_MAX):
    """(ops, n_probe): junk D, big_a M, b D, anchor. The prefix that ends with the b D ops is a clear hit; of the suffixes that end there
    only [1 ..] = big_a / (big_a + b) can reach the identity (trim_prefix: q >= id): the trim cuts the junk alone, or all n_probe ops."""
    ops = split(junk, "D", op_max) + split(big_a, "M", op_max) + split(b, "D", op_max, small_first=True)
    n = len(ops)
    return ops + rest_ops(m - big_a, x - b - junk, front_m, rest_op, irregular, op_max), n


def text_len(ops):
    return sum(len(str(L)) + 1 for L, _ in ops)


def line_of(ops, strand="+", mirror=False, **kw):
    """the PAF line; mirror: the ops back to front (the probe at the end of the text: what the second pass of a '-' record, or a
    reversed view, scans first). Up to 10^8 bases the names, lengths and starts are such that the one-wave row writer takes the record's
    rows and no coordinate passes a power of ten; beyond, sequences of 4 * 10^18."""
    if sum(L for L, _ in ops) <= 100_000_000:
        kw.setdefault("qs", 120_000_000)
        kw.setdefault("ts", 110_000_000)
    else:
        kw.setdefault("qlen", 4_000_000_000_000_000_000)
        kw.setdefault("tlen", 4_000_000_000_000_000_000)
    return record(ops[::-1] if mirror else ops, strand, **kw)


class Batch:
    """lines one behind the other, with the byte offset of every line's cigar: the flat pass cuts the batch's text into pieces of 1 KiB
    wherever the records lie, so which piece an op falls into depends on everything in front of it"""

    def __init__(self):
        self.lines, self.at, self.where = [], 0, []

    def add(self, line, where=None):
        self.lines.append(line)
        self.where.append(where)
        self.at += len(line)
        return len(self.lines) - 1

    def data(self):
        return "".join(self.lines).encode()


def pads_for(batch, header_len, prefix_of, residue, piece):
    """(n_pad, name pad) that put the letter of the probe's op at byte `residue` of piece `piece` of its record (1023: the next op lies
    wholly in the next piece; 1: its digits straddle the boundary in front of it).
    header_len: bytes of the line in front of its cigar with a name pad of 0 (the totals are fixed: it does not depend on the pads);
    prefix_of(n_pad): bytes of the ops up to the probe."""
    for n_pad in range(0, 1200):
        n = prefix_of(n_pad)
        for shift in range(6):
            start = batch.at + header_len + shift
            end = start + n - 1  # offset of the letter in the batch
            if end % 1024 == residue and (end >> 10) - (start >> 10) == piece:
                return n_pad, shift
    raise AssertionError((residue, piece))


# ---- the case families: (Batch, [expected number of ops the identity trim cuts from a record]) ----
# (kind, distance, exact): "u" float32 steps, "r" relative distance; exact: see near()
ULPS = (("u", -1, None), ("u", 0, None), ("u", 1, None))
BAND = tuple(("r", s * r, None) for r in (3e-6, 4e-6, 5e-6) for s in (-1, 1))
# above 2^24 the conversions round: ties of the float quotient whose exact fraction is on either side, and the same one step below
ULPS_ROUNDED = (("u", -1, "below"), ("u", -1, "above"), ("u", 0, "below"), ("u", 0, "above"), ("u", 1, None))
# where the probe's op lies: (name, piece of its record, byte of the piece, D ops in a run in front of it)
EARLY, LAST1, FIRST2, DRUN1, MID3 = ("early", None, None, 0), ("last1", 1, 1023, 0), ("first2", 2, 1, 0), ("drun1", 1, 760, 100), ("mid3", 3, 300, 0)
POSITIONS = (EARLY, LAST1, FIRST2, DRUN1, MID3)
# strand, mirror: a '+' record is scanned from the front of its text twice, a '-' record from the front and then from the back
VARIANTS = (("+", False), ("-", False), ("-", True))


def probe_pair(thr_f, dist, lo, hi, **kw):
    kind, v, exact = dist
    if kind == "u":
        return near(thr_f, v, lo, hi, exact=exact, **kw)
    return near_rel(thr_f, v, lo, hi, ok=kw.get("ok"))


def lt_batch(m, x, p0, p1, dists=ULPS, positions=POSITIONS, hits=(False, True), variants=VARIANTS, lo=140_000, hi=200_000, pad_m=200,
             front_m=500_000, rest_op=OP_MAX, irregular=None, op_max=OP_MAX, rounds=False, **rec_kw):
    """Probes of `q < thr` (the scan for the last hit) in records of m match and x other bases. Returns (batch, cut): cut[i] ops go
    from the front of record i's view when the probe is below the threshold (the whole prefix up to the probe), 2 when only an early hit
    in front of it counts, 0 when nothing does."""
    thr_f, _, max_trim = thresholds(m, x, p0, p1)
    pairs = {d: probe_pair(thr_f, d, lo, min(hi, max_trim), rounds=rounds, ok=lambda a, b: b < x - 1200 and a < m) for d in dists}
    batch, cut, lens = Batch(), [], {}
    for where, piece, residue, d_run in positions:
        for dist in dists:
            a, b = pairs[dist]
            for early in hits:
                for strand, mirror in variants:
                    def prefix_of(n):
                        key = (a, b, early, d_run, n)
                        if key not in lens:
                            lens[key] = text_len(lt_prefix(a, b, n, pad_m, early, op_max, d_run))
                        return lens[key]
                    n_pad = shift = 0
                    if piece is not None:
                        probe_line = line_of(lt_ops(a, b, m, x, 0, pad_m, early, front_m, rest_op, irregular, op_max, d_run)[0], strand, mirror, **rec_kw)
                        n_pad, shift = pads_for(batch, probe_line.index("cg:Z:") + 5, prefix_of, residue, piece)
                    ops, k = lt_ops(a, b, m, x, n_pad, pad_m, early, front_m, rest_op, irregular, op_max, d_run)
                    batch.add(line_of(ops, strand, mirror, qname="hs.chr3" + "x" * shift, **rec_kw), where)
                    cut.append(k + 1 if dist[1] < 0 else 2 if early else 0)
    return batch, cut


def ge_batch(m, x, p0, p1, lo, hi, variants=VARIANTS, rest_op=OP_MAX, irregular=None, op_max=OP_MAX, rounds=False, front_m=500_000):
    """Probes of `q >= id` (the search for the suffix that is kept): junk D, big_a M, b D with big_a / (big_a + b) at the identity -1,
    0 and +1 step. p1 < 1: the junk is sized so that the cumulative bases pass max_trim inside the anchor's first op -- the scan ends
    there, the probe's last op is the last hit. Returns (batch, cut): the junk ops alone (>= holds), or the whole probe."""
    thr_f, id_f, max_trim = thresholds(m, x, p0, p1)
    batch, cut = Batch(), []
    for u in (-1, 0, 1):
        if p1 < 1.0:
            big_a, b = near(id_f, u, lo, hi, rounds=rounds)
            junk = max_trim - 10 - big_a - b
        else:
            big_a, b = near(id_f, u, lo, hi, rounds=rounds, ok=lambda a, b: a <= op_max)
            junk = int(big_a * (1.0 / float(thr_f) - 1.0) * 1.3) + 10
        assert junk > 0 and quot(big_a, big_a + b + junk) < step(thr_f, -1000) and junk + b <= x, (big_a, b, junk)
        ops, n = ge_ops(big_a, b, m, x, junk, front_m, rest_op, irregular, op_max)
        for strand, mirror in variants:
            batch.add(line_of(ops, strand, mirror))
            cut.append(len(split(junk, "D", op_max)) if u >= 0 else n)
    return batch, cut


def rounding_total(p1, lo=TWO24 + 1, hi=TWO24 + 4000):
    """an odd total above 2^24 whose max_trim differs from the product taken in double and from the one of a truncated conversion"""
    for t in range(lo, hi, 2):
        ref, dbl, trunc = max_trim_of(t, p1)
        if ref != dbl and ref != trunc:
            return t
    raise AssertionError(p1)


def even_ops(m_left, x_left, irregular=None):
    """m_left match and x_left other bases spread evenly, M ops of one size first and last: the identity of every prefix and of every
    suffix is that of the whole"""
    m_left -= irregular or 0
    n = m_left // OP_MAX + 1
    ms = [m_left // n + (1 if i < m_left % n else 0) for i in range(n)]
    xs = [x_left // (n - 1) + (1 if i < x_left % (n - 1) else 0) for i in range(n - 1)]
    ops = []
    for i in range(n):
        ops.append((ms[i], "M"))
        if irregular and i == n // 2:
            ops.append((irregular, "M"))
        if i < n - 1:
            ops.append((xs[i], "D"))
    assert all(0 < L <= OP_MAX or L == irregular for L, _ in ops)
    return ops


def max_trim_batch(totals, p1s=(0.3, 0.1, 0.02), variants=VARIANTS, p0=0.05, irregular=None):
    """A prefix of M ops, then D ops, that falls below the threshold (by 5e-4) with its last op, where its cumulative bases are exactly
    max_trim; and the same one base longer: the scan stops in front of that op (impl/paf.c:829) and nothing is cut. The rest of the
    record has the same identity everywhere, so the scan from the other end finds nothing before it stops. Returns (batch, cut)."""
    batch, cut = Batch(), []
    for total in totals:
        for p1 in p1s:
            x = total // 5
            m = total - x
            thr_f, _, max_trim = thresholds(m, x, p0, p1)
            for extra in (0, 1):
                cum = max_trim + extra
                h_x = int(cum * (1.0 - float(thr_f))) + max(1, cum // 2000)
                h_m = cum - h_x
                last = min(OP_MAX, h_x)
                assert quot(h_m, cum) < step(thr_f, -1000) and quot(h_m, cum - last) > step(thr_f, 1000) and h_x < x
                hit = split(h_m, "M") + split(h_x - last, "D") + [(last, "D")]
                ops = hit + even_ops(m - h_m, x - h_x, irregular)
                for strand, mirror in variants:
                    batch.add(line_of(ops, strand, mirror))
                    cut.append(0 if extra else len(hit))
    return batch, cut


# ---- fixed trim ----
FIXED_ALIGNED = (TWO24 + 1, TWO24 + 3, 2 * TWO24 + 2, 10 ** 8 + 1)
FIXED_FRACTIONS = (0.1, 0.3, 0.7)


def fixed_ops(aligned, op=OP_MAX, irregular=None):
    """`aligned` aligned bases with an insert and a delete in the middle; irregular: one op of that length among them"""
    first = aligned // 2
    head = [(irregular, "M")] + split(first - irregular, "M", op) if irregular else split(first, "M", op)
    return head + [(7, "D"), (3, "I")] + split(aligned - first, "M", op)


# ---- filter ----
def filter_lines(pairs, wide=False):
    """For every (matches, others): the quotient through = and X ops (identity and identity with gaps), and through I, through D and
    through both (identity 1, the quotient with gaps). wide: single ops, the first number with a leading zero (the flat pass leaves
    such a record to the record kernels whatever its lengths); else ops of at most 8 191. Returns [(line, (m, x), gaps only)]."""
    out = []
    for k, (m, x) in enumerate(pairs):
        forms = [([(m, "=")], [(x, "X")], False), ([(m, "M")], [(x, "I")], True), ([(m, "M")], [(x, "D")], True)]
        if x > 1:
            forms.append(([(m, "M")], [(1, "I"), (x - 1, "D")], True))
        for j, (ms, xs, gaps_only) in enumerate(forms):
            ops = [o for L, c in ms + xs if L for o in ([(L, c)] if wide else split(L, c))]
            text = "0" + "".join("%d%s" % o for o in ops) if wide else None
            out.append((record(ops, "+-"[(k + j) & 1], qname="f%d_%d" % (k, j), cigar=text, qlen=10 ** 10, tlen=10 ** 10), (m, x), gaps_only))
    return out


TENTHS = tuple((k, 10 - k) for k in range(1, 10))
FILTER_BIG = ((1, 2), (2, 1), (TWO24 + 1, 2), (TWO24 + 3, TWO24 + 5), (2 * TWO24 + 3, 7), (3, TWO24 + 2))
ONLY_INSERTS = [(5, "I"), (200, "I")]  # 0 / 0: fails every threshold, passes under invert


def filter_keeps(m, x, thr):
    """(double)((float)m / (m + x)) >= thr; 0 / 0 is NaN and fails"""
    if m + x == 0:
        return False
    return float(quot(m, m + x)) >= thr


# ---- chain ----
# 10 is in the list as a small length only: the reference halves the trim, and 10 x 0.7f = 7.0 against 6.99... in double both give 3
CHAIN_LENGTHS = (10, TWO24 + 1, TWO24 + 3, 2 * TWO24 + 2, 10 ** 9 + 1)
CHAIN_TRIMS = (0.1, 0.3, 0.7)


def chain_lines(trim, strand, lengths=CHAIN_LENGTHS):
    """For every length three pairs A, B on a (query, target) of their own: A of that length on both sequences, B one base long, with
    B's start one base inside A's trimmed end, exactly on it, and one base behind it. Only the middle pair chains (s1 150): the first
    overlaps, the last pays a gap of 5 002 against B's score of 50. Returns (data, [(length, offset)] per pair)."""
    out, pairs = [], []
    qlen = 4 * 10 ** 9
    for i, length in enumerate(lengths):
        t_a = chain_trim(length, trim)[0]
        for off in (-1, 0, 1):
            name = "%d_%d" % (i, off + 1)
            a_q, b_q = (1000, 1000 + length), (1000 + length - t_a + off, 1000 + length - t_a + off + 1)
            a_t, b_t = (5000, 5000 + length), (5000 + length - t_a + off, 5000 + length - t_a + off + 1)
            if strand == "-":  # the query runs the other way: mirrored round 3 * 10^9
                a_q, b_q = (3 * 10 ** 9 - a_q[1], 3 * 10 ** 9 - a_q[0]), (3 * 10 ** 9 - b_q[1], 3 * 10 ** 9 - b_q[0])
            for (qs, qe), (ts, te), score in ((a_q, a_t, 100), (b_q, b_t, 50)):
                out.append("q%s\t%d\t%d\t%d\t%s\tt%s\t%d\t%d\t%d\t10\t20\t60\tAS:i:%d\tcg:Z:%dM\n" % (name, qlen, qs, qe, strand, name, qlen, ts, te, score, qe - qs))
            pairs.append((length, off))
    return "".join(out).encode(), pairs


# ---- view ----
# matches and totals both above 2^24 and odd: both conversions round
VIEW_SUMS = ((23438759, 1727068), (46877519, 3454136), (93137257, 6862750), (93137269, 6862752), (3 * TWO24 + 5, TWO24 + 2))
VIEW_SHARP = VIEW_SUMS[:4]  # the six decimals differ from those of the quotient taken in double and of truncated conversions


def view_near_misses(m, d):
    return "%f" % (m / d), "%f" % float(F(trunc32(m) / trunc32(d)))


def view_text_of(m, d):
    return "-nan" if d == 0 else "%f" % float(quot(m, d))


def view_lines():
    """[(line, Identity text, Identity-with-gaps text)]: the sums through = and X ops, and the same quotient with gaps through inserts"""
    out = []
    for k, (m, x) in enumerate(VIEW_SUMS):
        assert m > TWO24 and m & 1 and (m + x) & 1
        t = view_text_of(m, m + x)
        out.append((record([(m, "="), (x, "X")], "+-"[k & 1], qname="v%d" % k, tname="w%d" % k, qlen=10 ** 10, tlen=10 ** 10).encode(), t, t))
        out.append((record([(m, "="), (x, "I")], "-+"[k & 1], qname="vi%d" % k, tname="wi%d" % k, qlen=10 ** 10, tlen=10 ** 10).encode(), "1.000000", t))
        out.append((record(split(m, "=") + split(x, "D"), "+-"[k & 1], qname="vd%d" % k, tname="wd%d" % k, qlen=10 ** 10, tlen=10 ** 10).encode(), "1.000000", t))
    return out


# ---- the identity trim's sets: name -> (builder, (p0, p1), who sizes the records) ----
BIG = (1 << 29) - 1  # the longest op the record kernels keep in four bytes
M0, X0 = 1_000_000, 20_000  # thr_f 0.9313725 under the default parameters
M1, X1 = 999_983, 20_011    # totals whose identity is no simple fraction: float32 neighbours of 50 / 51 are rare among small operands
ABOVE = dict(lo=TWO24 + 1, hi=TWO24 + 20_000, rounds=True)
WIDE = dict(lo=(1 << 32) + 1, hi=(1 << 32) + 20_000, rest_op=BIG, op_max=BIG, front_m=1 << 34, positions=(EARLY,))
PLUS = (("+", False),)
# who: "flat" the flat pass (k_flat_lane or k_flat_size, by the depth of the walk), "lane" at most 12 pieces and a shallow walk,
# "regs" 13 to 64 pieces, "hbm" more than 64, "irreg" one irregular op: the record kernels with 32-bit sums, "wide" 64-bit sums over
# 4-byte ops, "arena" over 8-byte ops
TRIM_SETS = {
    "lt": (lambda: lt_batch(M0, X0, 0.05, 1.0, dists=ULPS + BAND), (0.05, 1.0), "flat"),
    "lt_lane": (lambda: lt_batch(M0, X0, 0.05, 1.0, dists=ULPS + BAND, positions=(EARLY,)), (0.05, 1.0), "lane"),
    "lt_regs": (lambda: lt_batch(M0, X0, 0.05, 1.0, rest_op=99), (0.05, 1.0), "regs"),
    "lt_hbm": (lambda: lt_batch(M0, X0, 0.05, 1.0, rest_op=30, positions=(EARLY, DRUN1)), (0.05, 1.0), "hbm"),
    # the two above with fewer records, for the pipe that ends in SHATTER (a row per M op)
    "lt_regs_rows": (lambda: lt_batch(M0, X0, 0.05, 1.0, rest_op=99, positions=(EARLY, DRUN1), hits=(True,)), (0.05, 1.0), "regs"),
    "lt_hbm_rows": (lambda: lt_batch(M0, X0, 0.05, 1.0, rest_op=30, positions=(DRUN1,), hits=(True,)), (0.05, 1.0), "hbm"),
    "lt_irreg": (lambda: lt_batch(M0, X0, 0.05, 1.0, irregular=8192), (0.05, 1.0), "irreg"),
    "lt_wide": (lambda: lt_batch(1 << 35, 1 << 30, 0.05, 1.0, **WIDE), (0.05, 1.0), "wide"),
    "lt_arena": (lambda: lt_batch(1 << 35, 1 << 30, 0.05, 1.0, irregular=(1 << 29) + 5, **WIDE), (0.05, 1.0), "arena"),
    # p0 = 0: the threshold IS the identity; an early hit could not be told from the probe, and a '-' record is cut from its other end
    "lt_p0": (lambda: lt_batch(M1, X1, 0.0, 1.0, positions=(EARLY, DRUN1), hits=(False,), variants=PLUS, front_m=M1), (0.0, 1.0), "flat"),
    "lt_p3": (lambda: lt_batch(M1, X1, 0.3, 1.0, positions=(EARLY, DRUN1), lo=45_000, hi=59_000, pad_m=100), (0.3, 1.0), "flat"),
    "lt_p5": (lambda: lt_batch(M1, 200_017, 0.5, 0.1, positions=(EARLY, DRUN1), lo=60_000, hi=120_000, pad_m=50), (0.5, 0.1), "flat"),
    # prefix sums above 2^24. 18 M bases in at most 12 pieces: the probe is most of the record, only a '+' record keeps its other end
    "lt_above_small": (lambda: lt_batch(16_750_000, 1_250_000, 0.005, 1.0, dists=ULPS_ROUNDED, positions=(EARLY,), variants=PLUS, front_m=1_000_000, **ABOVE),
                       (0.005, 1.0), "flat"),
    "lt_above": (lambda: lt_batch(40_000_000, 1_500_000, 0.05, 1.0, dists=ULPS_ROUNDED, positions=(EARLY,), front_m=12_000_000, **ABOVE), (0.05, 1.0), "regs"),
    "lt_above_irreg": (lambda: lt_batch(40_000_000, 1_500_000, 0.05, 1.0, dists=ULPS_ROUNDED, positions=(EARLY,), front_m=12_000_000, irregular=8192, **ABOVE),
                       (0.05, 1.0), "irreg"),
    "ge": (lambda: ge_batch(M1, X1, 0.05, 1.0, 3000, 8400), (0.05, 1.0), "lane"),
    "ge_irreg": (lambda: ge_batch(M1, X1, 0.05, 1.0, 3000, 8400, irregular=8192), (0.05, 1.0), "irreg"),
    "ge_bounded": (lambda: ge_batch(M1, 60_013, 0.05, 0.1, 80_000, 90_000), (0.05, 0.1), "lane"),
    "ge_regs": (lambda: ge_batch(M1, 60_013, 0.05, 0.1, 80_000, 90_000, rest_op=99), (0.05, 0.1), "regs"),
    "ge_hbm": (lambda: ge_batch(M1, 60_013, 0.05, 0.1, 80_000, 90_000, rest_op=30), (0.05, 0.1), "hbm"),
    "ge_bounded_irreg": (lambda: ge_batch(M1, 60_013, 0.05, 0.1, 80_000, 90_000, irregular=8192), (0.05, 0.1), "irreg"),
    "ge_wide": (lambda: ge_batch(1 << 35, 1 << 30, 0.05, 1.0, 500_000_000, 500_020_000, rest_op=BIG, op_max=BIG, front_m=1 << 34), (0.05, 1.0), "wide"),
    "ge_arena": (lambda: ge_batch(1 << 35, 1 << 30, 0.05, 1.0, 500_000_000, 500_020_000, rest_op=BIG, op_max=BIG, front_m=1 << 34, irregular=(1 << 29) + 5),
                 (0.05, 1.0), "arena"),
    "ge_above": (lambda: ge_batch(40_000_003, 7_000_001, 0.05, 0.45, TWO24 + 1, TWO24 + 20_000, rounds=True, front_m=12_000_000), (0.05, 0.45), "regs"),
}
for _p1 in (0.3, 0.1, 0.02):
    TRIM_SETS["max_trim_%g" % _p1] = (lambda p1=_p1: max_trim_batch((1_020_011, rounding_total(p1)), (p1,)), (0.05, _p1), "flat")
    TRIM_SETS["max_trim_%g_irreg" % _p1] = (lambda p1=_p1: max_trim_batch((1_020_011, rounding_total(p1)), (p1,), irregular=8192), (0.05, _p1), "irreg")

_BUILT = {}


def trim_set(name):
    """(batch, cut, (p0, p1), who), built once"""
    if name not in _BUILT:
        make, params, who = TRIM_SETS[name]
        _BUILT[name] = make() + (params, who)
    return _BUILT[name]


def pieces_of(batch):
    """1 KiB pieces of the batch's text that each record's cigar touches"""
    out, at = [], 0
    for line in batch.lines:
        lo = at + line.index("cg:Z:") + 5
        hi = at + len(line) - 1  # the newline
        out.append(((hi - 1) >> 10) - (lo >> 10) + 1)
        at += len(line)
    return out


LANE_BIT = 0x200000  # FLAT_F_ROW_PIECES: under a pipe that ends in SHATTER only k_flat_lane sets it, k_flat_size never does


def sized_by_lane(batch, cut):
    """Per record: True where k_flat_lane sizes it (lane_trim_prefix decides its trim), False where it hands it to k_flat_size
    (flat_trim_prefix). A record of more than FLAT_LANE_MAX_PIECES = 12 pieces always goes on. Below that the lane's budget of 1 024 ops
    decides: the suffix search costs one per cut op, the walk of the record's first piece and of the probe's piece comes on top (pieces
    whose bound clears the threshold cost nothing). The records here keep clear of that edge -- cuts of at most 520 ops stay, cuts of 790
    and more go -- and a record in between is an error of the set, not a case."""
    out = []
    for n, c in zip(pieces_of(batch), cut):
        assert n > 12 or c <= 520 or c >= 790, (n, c)
        out.append(n <= 12 and c <= 520)
    return out

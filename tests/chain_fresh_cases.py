"""Inputs of the tests of `paffy chain` under the fresh-iterator switch (paffy_hip_chain_fresh_walk), shared by
tests/test_chain_fresh_cpu.py (which shows on the oracle that every input hits its case) and tests/test_gpu_chain_fresh.py. The
expected output is always the oracle as committed, with its walk on; it is computed once per input and kept."""
import functools
import random

import oracle_lib as O


def line(q, qs, qe, t, ts, te, score, strand="+", ql=10_000_000, tl=10_000_000, extra=b""):
    f = [q, str(ql), str(qs), str(qe), strand, t, str(tl), str(ts), str(te), "10", "20", "60", "AS:i:%d" % score]
    return "\t".join(f).encode() + extra + b"\tcg:Z:%dM\n" % max(1, qe - qs)


def collinear_set(rng, n, n_q=3, n_t=3, span=2_000_000, exact=0.2, score_hi=20000):
    """Runs of roughly collinear alignments on a few (query, target) pairs and both strands, shuffled; a share of them abut exactly."""
    out = []
    while len(out) < n:
        q, t = "q%d" % rng.randrange(n_q), "t%d" % rng.randrange(n_t)
        strand = rng.choice("+-")
        qs, ts = rng.randrange(span), rng.randrange(span)
        for _ in range(rng.randrange(1, 12)):
            ln = rng.randrange(50, 5000)
            tln = ln + rng.randrange(-20, 21)
            if strand == "+":
                out.append(line(q, qs, qs + ln, t, ts, ts + max(1, tln), rng.randrange(1, score_hi), "+"))
                gap = 0 if rng.random() < exact else rng.randrange(0, 30000)
                qs += ln + gap
            else:
                out.append(line(q, max(0, qs - ln), max(1, qs), t, ts, ts + max(1, tln), rng.randrange(1, score_hi), "-"))
                gap = 0 if rng.random() < exact else rng.randrange(0, 30000)
                qs = max(ln + 1, qs - ln - gap)
            ts += max(1, tln) + (0 if gap == 0 else rng.randrange(0, 30000))
    rng.shuffle(out)
    return b"".join(out[:n])


_KEYS = ("gap_open", "gap_extend", "max_gap", "trim")


@functools.lru_cache(maxsize=None)
def _oracle(data, kw, fresh_walk):
    out, err, fresh = O.chain(data, fresh_walk=fresh_walk, **dict(kw))
    return out, err.code, err.record, fresh


def want(data, fresh_walk=True, **kw):
    """(output, error code, error record, fresh_hits) of the oracle, walk on unless said otherwise"""
    assert set(kw) <= set(_KEYS)
    return _oracle(data, tuple(sorted(kw.items())), fresh_walk)


# ---- T1: the pair ----
A, B = line("q", 0, 100, "t", 0, 100, 100), line("q", 100, 200, "t", 100, 200, 100)
T1 = B + A
# '-': the mirrored query start of the second record is the smaller one, so it is processed first, and it stands later in the input
T1_NEG = line("q", 0, 100, "t", 100, 200, 100, "-") + line("q", 100, 200, "t", 0, 100, 100, "-")
T1_KW = dict(trim=0.0)

# ---- T2: removal history ----
T2 = (line("q", 6100, 6200, "t", 1100, 1200, 100) + line("q", 6000, 6100, "t", 1000, 1100, 100) + line("q", 0, 100, "t", 0, 100, 100) +
      line("q", 5000, 5100, "t", 2000, 2100, 100))
T2_KW_REMOVED = dict(gap_open=10, gap_extend=1, max_gap=1000, trim=0.0)
T2_KW_KEPT = dict(gap_open=10, gap_extend=1, max_gap=100000, trim=0.0)

# ---- T3: the end of the leading run ----
T3_THIRD = {"smaller_query": ("p", "t", "+"), "greater_query": ("r", "t", "+"), "other_target": ("q", "u", "+"), "other_strand": ("q", "t", "-")}


def t3(which, first):
    """b + a at q/t 1000-1200 and a third record, processed first (q 0-50) or last (q 5000-5050) in its strand"""
    q, t, strand = T3_THIRD[which]
    at = 0 if first else 5000
    return (line("q", 1100, 1200, "t", 1100, 1200, 100) + line("q", 1000, 1100, "t", 1000, 1100, 100) + line(q, at, at + 50, t, at, at + 50, 70, strand))


def t3_fresh_links(which, first):
    return 1 if (which == "other_strand" or not first) else 0


# ---- T4: two candidates ----
T4 = line("q", 1100, 1200, "t", 1100, 1200, 100) + line("q", 1000, 1100, "t", 1000, 1100, 100) + line("q", 1000, 1100, "t", 1000, 1100, 300)

# ---- T5: lane and window edges ----
T5_PAIRS = (1, 63, 64, 65, 127, 128, 199)
T5_KW = dict(gap_open=10, gap_extend=1, max_gap=1000, trim=0.0)


def run_of_pairs(n, pairs, gap_of, rng=None, score=5000, length=100):
    """One group on one strand: n collinear records; the one at run position k in `pairs` abuts the one before it exactly and stands in
    front of it in the input; gap_of(k) is the gap in front of every other position k. rng: the input is shuffled first (a pair is then
    put right by exchanging its two lines). Returns (text, the records' (qs, input index) in run order)."""
    recs, at = [], 0
    for k in range(n):
        if k:
            at += 0 if k in pairs else gap_of(k)
        recs.append((at, at + length))
        at += length
    place = list(range(n))  # place[k]: where record k stands in the input
    if rng:
        rng.shuffle(place)
    else:  # input order = run order but for the blocks of pairs, which stand reversed
        k = 0
        while k < n:
            e = k
            while e + 1 < n and e + 1 in pairs:
                e += 1
            place[k:e + 1] = list(range(e, k - 1, -1))
            k = e + 1
    if rng:
        for k in sorted(pairs):
            if place[k] > place[k - 1]:
                place[k], place[k - 1] = place[k - 1], place[k]
    rows = [None] * n
    for k, (s, e) in enumerate(recs):
        rows[place[k]] = line("chrA", s, e, "chrB", s, e, score, ql=10**9, tl=10**9)
    return b"".join(rows), [(recs[k][0], place[k]) for k in range(n)]


def t5():
    # the gaps alternate above and below max_gap: every second walk removes everything behind it
    return run_of_pairs(200, T5_PAIRS, lambda k: 1500 if k % 2 == 0 else 500)


# ---- T6: the big-group kernel ----
T6_N = 5000
T6_PAIRS = (1, 16, T6_N - 1)  # inside the first tile of sixteen, across a tile boundary (records 15 / 16), at the end
T6_KW = dict(gap_open=10, gap_extend=1, max_gap=1000, trim=0.0)


@functools.lru_cache(maxsize=None)
def t6(with_pairs=True):
    rng = random.Random(66)
    gaps = [rng.randrange(1, 900) for _ in range(T6_N)]
    pairs = T6_PAIRS if with_pairs else ()
    for k in T6_PAIRS:  # a gap beyond max_gap in front of the record a pair's second abuts: its walk empties the set
        if k >= 2:
            gaps[k - 1] = 5000
    return run_of_pairs(T6_N, pairs, lambda k: gaps[k], rng=rng)


# ---- T7: random sets ----
T7_SEEDS = tuple(range(101, 109))
T7_SIZES = (2, 7, 60, 400, 3000, 6000)


def t7_kw(seed):
    kw = dict(gap_open=50, trim=0.0)
    if seed % 4 < 2:
        kw["max_gap"] = 20000
    return kw


@functools.lru_cache(maxsize=None)
def t7(seed):
    """the six inputs of a seed, drawn one after the other from one generator"""
    rng = random.Random(seed)
    k = 1 if seed % 2 else 3
    return tuple(collinear_set(rng, n, n_q=k, n_t=k, exact=0.5) for n in T7_SIZES)


def t7_takes_the_walk(seed, i):
    data, kw = t7(seed)[i], t7_kw(seed)
    on, off = want(data, **kw), want(data, fresh_walk=False, **kw)
    return on[3] > 0 and on[0] != off[0]


# ---- T9: errors ----
T9_BAD_LINE = T2 + b"q\t10\t0\t5\t*\tt\t10\t0\t5\t5\t5\t60\n" + T1
T9_BROKEN = line("q", 0, 100, "t", 0, 100, 100) + line("q", 110, 200, "t", 120, 200, 80, ql=150) + line("q", 300, 400, "t", 300, 400, 70)

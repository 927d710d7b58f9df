"""The walk from a fresh iterator (impl/chaining.c:71-86) without a GPU.

First: every input of tests/test_gpu_chain_fresh.py hits the case it is there for, shown on the oracle (fresh_hits, the output with the
walk against the output without it, the positions of the pairs).

Second: the decomposition the kernels are built on (paffy_amd/csrc/chain_kernel.h) -- leading single-group run, live bits, breaker,
one flag per record, then today's recurrence with one relaxed candidate test -- gives the links of a literal restatement of
chain_one_strand (sorted set, removal list) on a few thousand small random inputs, a good share of which take the walk."""
import bisect
import random

import pytest

import chain_fresh_cases as K


# ---------------------------------------------------------------- the inputs hit their cases ----------------------------------------------------------------
def test_t1_the_pair():
    out, code, _, fresh = K.want(K.T1, **K.T1_KW)
    assert code == 0 and fresh == 1 and out.count(b"s1:i:200") == 2
    assert K.want(K.T1, fresh_walk=False, **K.T1_KW)[0].count(b"s1:i:100") == 2
    out, code, _, fresh = K.want(K.T1_NEG, **K.T1_KW)
    assert code == 0 and fresh == 1 and out.count(b"s1:i:200") == 2
    out, code, _, fresh = K.want(K.A + K.B, **K.T1_KW)
    assert fresh == 0 and out.count(b"s1:i:200") == 2


def test_t2_removal_history():
    out, code, _, fresh = K.want(K.T2, **K.T2_KW_REMOVED)
    assert code == 0 and fresh == 1 and out.count(b"s1:i:200") == 2
    out, code, _, fresh = K.want(K.T2, **K.T2_KW_KEPT)
    assert code == 0 and fresh == 0 and out.count(b"s1:i:100") == 4 and len({ln.split(b"cn:i:")[1] for ln in out.splitlines()}) == 4


@pytest.mark.parametrize("which", sorted(K.T3_THIRD))
@pytest.mark.parametrize("first", [True, False])
def test_t3_the_end_of_the_leading_run(which, first):
    out, code, _, fresh = K.want(K.t3(which, first), trim=0.0)
    assert code == 0 and fresh == K.t3_fresh_links(which, first)
    assert out.count(b"s1:i:200") == 2 * fresh
    assert (out != K.want(K.t3(which, first), fresh_walk=False, trim=0.0)[0]) == bool(fresh)


def test_t4_two_candidates():
    out, code, _, fresh = K.want(K.T4, trim=0.0)
    assert code == 0 and fresh == 2 and out.count(b"s1:i:400") == 2 and out.count(b"s1:i:100") == 1


def run_positions(data):
    """(qs, input index) of one group's records in processing order"""
    rows = [(int(ln.split(b"\t")[2]), i) for i, ln in enumerate(data.splitlines())]
    return sorted(rows)


def pairs_of(data):
    """run positions whose record abuts the one before it exactly on both sequences and stands in front of it in the input"""
    f = [ln.split(b"\t") for ln in data.splitlines()]
    order = [i for _, i in run_positions(data)]
    return tuple(k for k in range(1, len(order)) if f[order[k]][2] == f[order[k - 1]][3] and f[order[k]][7] == f[order[k - 1]][8] and order[k] < order[k - 1])


def test_t5_pairs_stand_where_the_gpu_test_says():
    data, run = K.t5()
    assert run_positions(data) == run and pairs_of(data) == K.T5_PAIRS
    out, code, _, fresh = K.want(data, **K.T5_KW)
    assert code == 0 and fresh >= 3 and out != K.want(data, fresh_walk=False, **K.T5_KW)[0]
    # what the flag kernel has to process: up to the last position whose search skips a candidate
    recs = parse(data)
    flags, skipped = decomposition_flags(recs, K.T5_KW["max_gap"])
    assert max(skipped) == 199 and sorted(set(skipped)) == list(K.T5_PAIRS)
    assert sum(flags[k] for k in K.T5_PAIRS) == fresh


def test_t6_pairs_stand_where_the_gpu_test_says():
    data, run = K.t6()
    assert len(run) == K.T6_N > 4096 and run_positions(data) == run and pairs_of(data) == K.T6_PAIRS
    out, code, _, fresh = K.want(data, **K.T6_KW)
    assert code == 0 and fresh >= 3 and out != K.want(data, fresh_walk=False, **K.T6_KW)[0]
    data0, _ = K.t6(False)
    assert pairs_of(data0) == () and K.want(data0, **K.T6_KW)[3] == 0


def test_t7_enough_random_sets_take_the_walk():
    taking = 0
    for seed in K.T7_SEEDS:
        for i in range(len(K.T7_SIZES)):
            assert K.want(K.t7(seed)[i], **K.t7_kw(seed))[1] == 0
            taking += K.t7_takes_the_walk(seed, i)
    assert taking >= 20, taking


def test_t9_errors_of_the_oracle():
    import oracle_lib as O

    assert K.want(K.T9_BAD_LINE)[1:3] == (O.ERR_STRAND, 4)
    assert K.want(K.T9_BROKEN)[1:3] == (O.ERR_CHECK_QEND, 1)
    assert K.want(K.T2, trim=1.5)[1] == O.ERR_CHAIN_ASSERT


# ---------------------------------------------------------------- the decomposition against the literal walk ----------------------------------------------------------------
def parse(data):
    """records of ONE strand as (qname, tname, qs, qe, ts, te, score); the input index is the address"""
    out = []
    for ln in data.splitlines():
        f = ln.split(b"\t")
        out.append((f[0], f[5], int(f[2]), int(f[3]), int(f[7]), int(f[8]), int(f[12][5:])))
    return out


def gap_cost(dq, dt, gap_open, gap_extend):
    return 0 if dq + dt == 0 else gap_open + gap_extend * (dq + dt)


def literal_links(recs, gap_open, gap_extend, max_gap):
    """chain_one_strand of oracle/paf_oracle.c (impl/chaining.c:136-205) restated line by line: the sorted set, the search, the walk
    from the found element or from the top, the removal list. Returns (predecessor record or None, chain score) per record and how many
    links were taken from a fresh walk."""
    order = sorted(range(len(recs)), key=lambda i: (recs[i][2], i))
    act = []  # (qname, tname, te, qe, address) of the active chains, sorted
    link, fresh_links = {}, 0
    for r in order:
        q, t, qs, qe, ts, te, sc = recs[r]
        lo = bisect.bisect_right(act, (q, t, ts, qs, r))
        fresh = lo == 0
        it = len(act) - 1 if fresh else lo - 1
        best, prev, to_remove, took_fresh = sc, None, [], False
        while it >= 0:
            pq, pt, pte, pqe, p = act[it]
            it -= 1
            if (pq, pt) != (q, t):
                break
            if qs < pqe:
                continue
            if qs - pqe > max_gap:
                to_remove.append((pq, pt, pte, pqe, p))
                continue
            if ts < pte:
                continue
            if ts - pte > max_gap:
                break
            g = gap_cost(qs - pqe, ts - pte, gap_open, gap_extend)
            cs = sc + link[p][1] - g
            if g < sc and cs > best:
                best, prev = cs, p
                took_fresh = fresh
        if prev is not None and took_fresh:
            fresh_links += 1
        link[r] = (prev, best)
        bisect.insort(act, (q, t, te, qe, r))
        for e in to_remove:
            act.remove(e)
    return link, fresh_links


def decomposition_flags(recs, max_gap):
    """The part that depends on the set's history, from the coordinates alone: over the strand's leading single-group run, which
    searches come out empty. Returns (flag per run position, the run positions whose search skips a candidate of the kind only a fresh
    walk sees)."""
    order = sorted(range(len(recs)), key=lambda i: (recs[i][2], i))
    group = recs[order[0]][:2]
    live, flags, skipped = [], [], []
    for k, r in enumerate(order):
        if recs[r][:2] != group:
            break  # the run ends at the first record of another group
        _, _, qs, qe, ts, te, _ = recs[r]
        key = (ts, qs, r)
        below = [e for e in live if e <= key]
        fresh = not below
        flags.append(1 if fresh else 0)
        if any(e[0] == ts and e[1] == qs and e[2] > r for e in live):
            skipped.append(k)
        if fresh:
            visited = list(live)
        else:
            breakers = [e for e in below if qs >= e[1] and qs - e[1] <= max_gap and ts - e[0] > max_gap]
            b = max(breakers) if breakers else None
            visited = [e for e in below if b is None or e > b]
        dead = [e for e in visited if qs >= e[1] and qs - e[1] > max_gap]
        live.append((te, qe, r))
        for e in dead:
            live.remove(e)
    return flags, skipped


def decomposition_links(recs, gap_open, gap_extend, max_gap):
    """The flags, then today's recurrence per group with "sorts after the search key" reading "... and i is not fresh"."""
    order = sorted(range(len(recs)), key=lambda i: (recs[i][2], i))
    flags, _ = decomposition_flags(recs, max_gap)
    fresh_of = {order[k]: f for k, f in enumerate(flags)}
    link, done = {}, []
    for r in order:
        q, t, qs, qe, ts, te, sc = recs[r]
        choice = None  # (chain score, te, qe, address): the descending scan keeps the first best, the largest key among equal scores
        for p in done:
            pq, pt, _, pqe, _, pte, _ = recs[p]
            if (pq, pt) != (q, t) or qs < pqe or qs - pqe > max_gap or ts < pte or ts - pte > max_gap:
                continue
            if pte == ts and pqe == qs and p > r and not fresh_of.get(r, 0):
                continue
            g = gap_cost(qs - pqe, ts - pte, gap_open, gap_extend)
            if not g < sc:
                continue
            cand = (sc + link[p][1] - g, pte, pqe, p)
            if choice is None or cand > choice:
                choice = cand
        link[r] = (choice[3], choice[0]) if choice and choice[0] > sc else (None, sc)
        done.append(r)
    return link


def small_random_strand(rng):
    """up to thirteen records near one diagonal of a small grid, on one to nine (query, target) pairs: exact abutments, equal keys and
    equal scores all the time"""
    n = rng.randrange(1, 14)
    k = rng.choice((1, 1, 1, 2, 3))
    recs = []
    for _ in range(n):
        q, t = b"q%d" % rng.randrange(k), b"t%d" % rng.randrange(k)
        d = rng.randrange(8)
        qs, ts = 10 * d, max(0, 10 * (d + rng.choice((0, 0, 0, 1, -1, 3))))
        recs.append((q, t, qs, qs + 10 * rng.choice((1, 1, 2)), ts, ts + 10 * rng.choice((1, 1, 2)), rng.choice((5, 30, 30, 100))))
    return recs, rng.choice((0, 1, 20)), rng.choice((0, 1)), rng.choice((0, 10, 30, 60, 1000))


def test_the_decomposition_gives_the_links_of_the_literal_walk():
    rng = random.Random(20240)
    took_walk = 0
    for _ in range(6000):
        recs, gap_open, gap_extend, max_gap = small_random_strand(rng)
        lit, fresh_links = literal_links(recs, gap_open, gap_extend, max_gap)
        assert decomposition_links(recs, gap_open, gap_extend, max_gap) == lit, (recs, gap_open, gap_extend, max_gap)
        took_walk += fresh_links > 0
    assert took_walk >= 400, took_walk


def test_the_literal_restatement_is_the_oracle():
    """the Python restatement above against the committed C oracle, through the text: same chains"""
    rng = random.Random(5)
    for _ in range(300):
        recs, gap_open, gap_extend, max_gap = small_random_strand(rng)
        recs = [(q, t, qs + 1, qe + 1, ts + 1, te + 1, sc) for q, t, qs, qe, ts, te, sc in recs]
        data = b"".join(K.line(q.decode(), qs, qe, t.decode(), ts, te, sc) for q, t, qs, qe, ts, te, sc in recs)
        out = K.want(data, gap_open=gap_open, gap_extend=gap_extend, max_gap=max_gap, trim=0.0)[0]
        lit, _ = literal_links(recs, gap_open, gap_extend, max_gap)
        # records joined by the literal links, cut as the reference cuts (a link into a chain taken earlier is dropped): compare the
        # multiset of chain sizes through the recurrence's scores instead -- every record's best score is s1 of the chain it ends
        ends = set(range(len(recs))) - {p for p, _ in lit.values() if p is not None}
        tags = sorted(int(ln.split(b"s1:i:")[1].split(b"\t")[0]) for ln in out.splitlines())
        assert max(tags) == max(lit[e][1] for e in ends)

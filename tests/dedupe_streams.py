"""Streams for the dedupe-in-parts tests (tests/test_gpu_dedupe_parts.py, tests/test_dedupe_parts_host.py): the generator of
tests/test_dedupe.py::test_gpu_dedupe_random_streams restated -- records drawn from a small pool, so that repeats are common, with swapped
twins, near misses that differ in one coordinate or in the strand, and records whose coordinates paf_check rejects -- and the cut of a
stream into rounds of consecutive shares. Test infrastructure only."""


def swapped(line):
    f = line.rstrip(b"\n").split(b"\t")
    f[0], f[5] = f[5], f[0]
    f[1], f[6] = f[6], f[1]
    f[2], f[7] = f[7], f[2]
    f[3], f[8] = f[8], f[3]
    return b"\t".join(f) + b"\n"


def record(qn, tn, qs, ts, ln, strand=b"+", ql=1000, tl=2000, extra=b""):
    return b"\t".join([qn, b"%d" % ql, b"%d" % qs, b"%d" % (qs + ln), strand, tn, b"%d" % tl, b"%d" % ts, b"%d" % (ts + ln), b"%d" % ln, b"%d" % ln, b"60",
                       b"cg:Z:%dM" % ln]) + extra + b"\n"


def bad_check(k=0):
    """parses; query start >= query length: paf_check fails (PAFFY_ERR_CHECK_QSTART), reached only with -a"""
    return b"qb%d\t50\t60\t64\t+\ttb\t200\t0\t3\t3\t3\t60\tcg:Z:3M\n" % k


def pool_of(rng, size=60):
    return [record(b"q%d" % rng.randrange(6), b"t%d" % rng.randrange(6), rng.randrange(0, 900), rng.randrange(0, 1900), rng.randrange(1, 90), rng.choice([b"+", b"-"]))
            for _ in range(size)]


def stream(rng, n, p_bad=0.0, pool_size=60):
    """n lines: pool records, 35 % of them swapped, 15 % near misses (one coordinate or the strand), p_bad of them failing paf_check"""
    pool, lines = pool_of(rng, pool_size), []
    for _ in range(n):
        ln = rng.choice(pool)
        r = rng.random()
        if r < p_bad:
            ln = bad_check(rng.randrange(3))
        elif r < p_bad + 0.15:
            f = ln.rstrip(b"\n").split(b"\t")
            if rng.random() < 0.5:
                f[3] = b"%d" % (int(f[3]) + 1)
            else:
                f[4] = b"-" if f[4] == b"+" else b"+"
            ln = b"\t".join(f) + b"\n"
        if rng.random() < 0.35:
            ln = swapped(ln)
        lines.append(ln)
    return lines


def cut(rng, lines, n_rounds, n_parts, empty=()):
    """the lines as n_rounds rounds of n_parts consecutive shares, cut at arbitrary record boundaries (shares may be empty; the parts
    listed in `empty` get nothing in any round) -> [[bytes per part] per round]"""
    live = [s for s in range(n_rounds * n_parts) if s % n_parts not in empty]
    marks = sorted(rng.randrange(len(lines) + 1) for _ in range(len(live) - 1))
    bounds = [0] + marks + [len(lines)]
    shares = [b""] * (n_rounds * n_parts)
    for k, s in enumerate(live):
        shares[s] = b"".join(lines[bounds[k]: bounds[k + 1]])
    assert b"".join(shares) == b"".join(lines)
    return [shares[r * n_parts: (r + 1) * n_parts] for r in range(n_rounds)]

"""Checker of `paffy dechunk` and `paffy upconvert` (impl/paf_dechunk.c, impl/paf_upconvert.c), which the oracle lacks.

The header edits are restated here; the bytes still come from the oracle: a rewritten text goes through O.run([PASS]) (dechunk: the
cigar is parsed, tags normalised) or O.dedupe (upconvert: the cigar text verbatim). The integers of a name are read by the C library's
own sscanf("%li") -- what "%" PRIi64 is on x86-64 glibc -- so base prefixes, white space and out-of-range values are the C library's.
"""
import ctypes as C

import oracle_lib as O

_libc = C.CDLL("libc.so.6")
DECHUNK_HEADER, UPCONVERT_ASSERT = 23, 24
CHECK_QSTART, CHECK_QEND, CHECK_TSTART, CHECK_TEND, CHECK_CIGAR_Q, CHECK_CIGAR_T = 5, 6, 7, 8, 9, 10
OP_I, OP_D = 1, 2


def scan_li(tok):
    """sscanf(tok, "%li"): the value, or None when nothing converts (the reference's assert)"""
    v = C.c_long(0)
    return v.value if _libc.sscanf(tok, b"%li", C.byref(v)) == 1 else None


def decode(name):
    """decode_fasta_header (impl/paf.c:716-731): (name, start, length) or None"""
    toks = name.split(b"|")
    if len(toks) < 2:  # one token: the length peeks an empty list
        return None
    start = scan_li(toks[-1])
    if start is None:
        return None
    length = scan_li(toks[-2])
    if length is None:
        return None
    return b"|".join(toks[:-2]), start, length


def wrap(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def cigar_of(fields):
    cg = None
    for f in fields[12:]:
        if f.startswith(b"cg:Z:"):
            cg = f[5:]
    return cg


def paf_check(f, with_cigar):
    """paf_check (impl/paf.c:427-461) on split fields; 0 = fine"""
    ql, qs, qe, tl, ts, te = (int(f[k]) for k in (1, 2, 3, 6, 7, 8))
    if qs < 0 or qs >= ql:
        return CHECK_QSTART
    if qs > qe or qe > ql:
        return CHECK_QEND
    if ts < 0 or ts >= tl:
        return CHECK_TSTART
    if ts > te or te > tl:
        return CHECK_TEND
    cg = cigar_of(f) if with_cigar else None
    if cg:
        ops = O.cigar_parse(cg)
        i = sum(n for op, n in ops if op != OP_D)
        j = sum(n for op, n in ops if op != OP_I)
        if i != qe - qs:
            return CHECK_CIGAR_Q
        if j != te - ts:
            return CHECK_CIGAR_T
    return 0


def _lines(data):
    ls = data.split(b"\n")
    return ls[:-1] if ls and ls[-1] == b"" else ls


def dechunk(data, query=True, target=True, check=True):
    """(expected bytes, (code, record) of the first failure or None)"""
    _, perr = O.run([O.stage(O.PASS)], data)  # parse errors of the text as read (the cigar included) come first
    first_parse = perr.record if perr.code else None
    out, fail = [], None
    for i, line in enumerate(_lines(data)):
        if first_parse is not None and i == first_parse:
            fail = (perr.code, i)
            break
        f = line.split(b"\t")
        bad = False
        for on, (ni, li, si, ei) in ((query, (0, 1, 2, 3)), (target, (5, 6, 7, 8))):
            if not on:
                continue
            d = decode(f[ni])
            if d is None:
                bad = True
                break
            name, cs, cl = d
            f[ni], f[si], f[ei], f[li] = name, b"%d" % wrap(int(f[si]) + cs), b"%d" % wrap(int(f[ei]) + cs), b"%d" % cl
        if bad:
            fail = (DECHUNK_HEADER, i)
            break
        code = paf_check(f, True) if check else 0
        if code:
            fail = (code, i)
            break
        out.append(b"\t".join(f) + b"\n")
    want, err = O.run([O.stage(O.PASS)], b"".join(out))
    assert err.code == 0
    return want, fail


def chunk_encode(data, chunk=1_000_000, styles=(b"%d",)):
    """every name becomes name|length|c, c the start rounded down to `chunk`, the coordinates shifted by -c; c is written in the styles
    in turn (printf formats of one integer, e.g. b"0x%x", b"0%o", b"+%d", b" %d")"""
    out, k = [], 0
    for line in _lines(data):
        f = line.split(b"\t")
        for ni, li, si, ei in ((0, 1, 2, 3), (5, 6, 7, 8)):
            ln, s, e = int(f[li]), int(f[si]), int(f[ei])
            c = s // chunk * chunk
            f[ni] = f[ni] + b"|%d|" % ln + styles[k % len(styles)] % c
            k += 1
            f[li], f[si], f[ei] = b"%d" % (ln - c), b"%d" % (s - c), b"%d" % (e - c)
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def intervals_of(fasta):
    """[(header, sequence length)] -> the sorted table [(name, start, end, length)] (cmp_intervals; the tests keep (name, start) distinct)"""
    tab = []
    for h, n in fasta:
        d = decode(h)
        assert d is not None, h
        name, start, length = d
        tab.append((name, start, start + n, length))
    tab.sort(key=lambda t: (t[0], t[1]))
    assert len({(t[0], t[1]) for t in tab}) == len(tab)
    return tab


def bsearch(tab, name, start, end):
    """glibc bsearch over cmp_overlapping_intervals (impl/paf_upconvert.c:26-44): index, -1 for none, -2 for the assert"""
    lo, hi = 0, len(tab)
    while lo < hi:
        idx = (lo + hi) // 2
        yn, ys, ye, _ = tab[idx]
        k = (name > yn) - (name < yn)
        if k == 0:
            if start < ys:
                k = -1
            elif start <= ye:
                return idx if end <= ye else -2
            else:
                k = 1
        if k < 0:
            hi = idx
        else:
            lo = idx + 1
    return -1


def upconvert(data, fasta):
    """(expected bytes, (code, record) or None) of `paffy upconvert` with FASTA records [(header, sequence length)]"""
    tab = intervals_of(fasta)
    out, fail, keys = [], None, set()
    for i, line in enumerate(_lines(data)):
        f = line.split(b"\t")
        hits = []
        for ni, li, si, ei in ((0, 1, 2, 3), (5, 6, 7, 8)):
            k = bsearch(tab, f[ni], int(f[si]), int(f[ei]))
            hits.append(k)
            if k == -2:
                break
        if -2 in hits:
            fail = (UPCONVERT_ASSERT, i)
            break
        for k, (ni, li, si, ei) in zip(hits, ((0, 1, 2, 3), (5, 6, 7, 8))):
            if k >= 0:
                yn, ys, _, yl = tab[k]
                f[ni], f[si], f[ei], f[li] = b"%s|%d|%d" % (yn, yl, ys), b"%d" % (int(f[si]) - ys), b"%d" % (int(f[ei]) - ys), b"%d" % yl
        code = paf_check(f, False)
        if code:
            fail = (code, i)
            break
        key = (f[0], f[5], f[4], f[2], f[3], f[7], f[8])
        assert key not in keys, "dedupe would drop a record: build the input without duplicate keys"
        keys.add(key)
        out.append(b"\t".join(f) + b"\n")
    want, err = O.dedupe(b"".join(out))
    assert err.code == 0
    return want, fail

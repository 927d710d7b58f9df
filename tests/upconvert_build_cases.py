"""Inputs of the device build of upconvert's interval table (paffy_amd/csrc/upconvert_build_kernel.h) and its CPU predictor.

A case is a list of FASTA files, each a list of (header, sequence length). The predictor decodes every header up to its first NUL byte
with chunk_lib.decode -- the C library's own sscanf("%li") reads the integers --, orders the records by (name, start, input index) and
prints the output name as the reference does: the table paffy_hip_set_intervals builds (glibc's qsort is a merge sort: equal keys keep
input order).
"""
import random

import chunk_lib as K
import faffy_lib as F
import oracle_lib as O

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
PREFIX = b"shared_prefix_20bytes"[:20]
BAD_HEADERS = (b"nobar", b"a|x|5", b"a|5|")
STYLES = {b"st|0x1f|017": (b"st", 15, 31), b"st|+5| 7": (b"st", 7, 5), b"st|12abc|-3": (b"st", -3, 12), b"st| 7|+5": (b"st", 5, 7),
          b"st|017|0x1f": (b"st", 31, 15)}  # header -> (name, start, length)
SATURATING = {b"big|5|99999999999999999999": (b"big", I64_MAX, 5), b"big|5|-9223372036854775809": (b"big", I64_MIN, 5),
              b"big|99999999999999999999|1": (b"big", 1, I64_MAX), b"big|-9223372036854775809|2": (b"big", 2, I64_MIN)}


def fasta_text(recs):
    """one FASTA file of (header, sequence length) records, the bases on one line"""
    return b"".join(b">" + h + b"\n" + b"A" * n + b"\n" for h, n in recs)


def texts(case):
    return [fasta_text(f) for f in case]


def iv_records(files):
    """[(header, sequence length)] of FASTA texts, as the loaders read them"""
    return [(h, len(s)) for h, s in F.fasta_read_files(files)]


def key_of(header):
    return header.split(b"\0", 1)[0]


def expected(recs):
    """(header, sequence length) in input order -> [(name, start, end, length, out_name)] in table order; None when a header fails"""
    rows = []
    for i, (h, n) in enumerate(recs):
        d = K.decode(key_of(h))
        if d is None:
            return None
        name, start, length = d
        rows.append((name, start, i, K.wrap(start + n), length))
    rows.sort(key=lambda t: t[:3])
    return [(name, start, end, length, b"%s|%d|%d" % (name, length, start)) for name, start, _, end, length in rows]


def names_of(recs):
    """the decoded names in input order: the keys of the build's name sort"""
    return [K.decode(key_of(h))[0] for h, _ in recs]


def expected_upconvert(data, table):
    """(bytes, (code, record) or None) of `paffy upconvert` over the predictor's table: chunk_lib.upconvert with the table given"""
    tab = [t[:4] for t in table]
    out, fail = [], None
    for i, line in enumerate(data.split(b"\n")[:-1]):
        f = line.split(b"\t")
        hits = []
        for ni, li, si, ei in ((0, 1, 2, 3), (5, 6, 7, 8)):
            hits.append(K.bsearch(tab, f[ni], int(f[si]), int(f[ei])))
            if hits[-1] == -2:
                break
        if -2 in hits:
            fail = (K.UPCONVERT_ASSERT, i)
            break
        for k, (ni, li, si, ei) in zip(hits, ((0, 1, 2, 3), (5, 6, 7, 8))):
            if k >= 0:
                _, ys, _, yl, out_name = table[k]
                f[ni], f[si], f[ei], f[li] = out_name, b"%d" % (int(f[si]) - ys), b"%d" % (int(f[ei]) - ys), b"%d" % yl
        code = K.paf_check(f, False)
        if code:
            fail = (code, i)
            break
        out.append(b"\t".join(f) + b"\n")
    want, err = O.dedupe(b"".join(out))
    assert err.code == 0
    return want, fail


# ---- the cases ----

TIE_SMALL_FIRST = [[(b"c|1000|0", 10), (b"c|1000|0", 100)]]
TIE_LARGE_FIRST = [[(b"c|1000|0", 100), (b"c|1000|0", 10)]]
TIE_PROBE = b"c\t1000\t5\t50\t+\tother\t70\t1\t2\t5\t9\t60\ttp:A:P\n"  # start 5, end 50 on the tied name


def one_name(n, seed):
    """n records of one name, the starts shuffled: negative ones, ones above 2^32, the rest small"""
    rnd = random.Random(seed)
    starts = [-(k + 1) * 1000 for k in range(5)] + [(1 << 32) + 7 * k for k in range(5)] + [(1 << 40) + 1, I64_MIN + 5, I64_MAX - 9]
    starts += [10 * k for k in range(n - len(starts))]
    rnd.shuffle(starts)
    return [[(b"chrQ|123456|%d" % s, 1 + k % 3) for k, s in enumerate(starts)]]


def shared_prefix():
    """300 names behind a 20-byte prefix, two starts each. 30 groups differ in the 8 bytes behind the prefix, each group's two halves in
    one byte with 9 common bytes behind it, the names of a half in their last byte: three rounds, the later ones over many runs"""
    recs = []
    for i in range(300):
        name = PREFIX + b"g%02d_blk_" % (i // 10) + b"sub%d_xyz_pad" % (i % 10 // 5) + b"%d" % (i % 5)
        recs += [(name + b"|5000|%d" % (700 - i), 3), (name + b"|5000|%d" % (i - 100), 2)]
    random.Random(11).shuffle(recs)
    return [recs]


GOOD_256 = [(b"g%03d|900|%d" % (k % 50, 1000 - k), 2) for k in range(256)]


def good_cases():
    return {
        "empty": [[]],
        "one": [[(b"chr1|100|0", 5)]],
        "tie_small_first": TIE_SMALL_FIRST,
        "tie_large_first": TIE_LARGE_FIRST,
        "one_name_65": one_name(65, 1),
        "one_name_257": one_name(257, 2),
        "shared_prefix": shared_prefix(),
        "name_prefix": [[(b"a|b|5|0", 3), (b"a|5|0", 4), (b"a|b|c|5|1", 2), (b"a|5|-1", 1)]],
        "empty_name": [[(b"z|9|1", 2), (b"7|3", 4), (b"|8|2", 1), (b"5|-4", 6)]],
        "styles": [[(h, 3 + k) for k, h in enumerate(STYLES)]],
        "saturating": [[(h, 2 + k) for k, h in enumerate(SATURATING)]],
        "nul": [[(b"n|4|2\0|9|9", 3), (b"n|4|1", 2), (b"m|3|3\0x", 1), (b"n|4|0\0", 5)]],
        "two_files": [[(b"chrB|50000|20000", 50), (b"chrA|100000|2000", 10)], [(b"chrA|100000|0", 7), (b"chrB|50000|100", 20), (b"chrA|100000|1000", 9)]],
        "block_256": [GOOD_256],
    }


def bad_cases():
    cases = {}
    for k, bad in enumerate(BAD_HEADERS):
        good = [(b"ok|10|%d" % j, 2) for j in range(3)]
        cases["bad%d_first" % k] = [[(bad, 4)] + good]
        cases["bad%d_last" % k] = [good + [(bad, 4)]]
        cases["bad%d_among_256" % k] = [GOOD_256[:200] + [(bad, 4)] + GOOD_256[200:]]
    return cases


def flat(case):
    return [r for f in case for r in f]

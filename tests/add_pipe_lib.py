"""Inputs of the flat pass's `add_mismatches | trim | filter` mode (paffy_amd/csrc/flat_add_pipe_kernel.h). Not a test module:
test_flat_add_pipe_cpu.py proves on the oracle that the inputs are sharp, test_gpu_flat_add_pipe.py runs the same bytes on the GPU.

A record here comes with sequences of its own (target `t<i>`, query `q<i>`, reverse complement of the query `r<i>` for the '-' form), so
which columns of its M ops match is chosen per column: the new ops of the encoder -- and with them what the identity trim cuts and what
a filter sees -- are laid by hand. The pieces of the flat pass are 1 KiB tiles of the BATCH text: which piece an input op falls into
depends on where its letter lies in the batch, and a new op belongs to the piece of the input op it comes from."""
import re

import numpy as np

from test_gpu_flat import record

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
TILE = 1024


def sequences(ops, seed, mism, margin=40):
    """(target, query, reverse complement of the query) for a '+' record of these ops (M, I, D) at query / target start `margin`: the
    query follows the target along the cigar; mism: bool per column of the M ops, in cigar order -- True: the two bases differ"""
    rs = np.random.RandomState(seed)
    L = np.array([l for l, _ in ops], dtype=np.int64)
    code = np.array([ord(c) for _, c in ops], dtype=np.uint8)
    is_m, is_i, is_d = code == ord("M"), code == ord("I"), code == ord("D")
    q_off = margin + np.concatenate(([0], np.cumsum(np.where(is_d, 0, L))))
    t_off = margin + np.concatenate(([0], np.cumsum(np.where(is_i, 0, L))))
    t = ACGT[rs.randint(0, 4, size=int(t_off[-1]) + margin)]
    q = ACGT[rs.randint(0, 4, size=int(q_off[-1]) + margin)]
    Lm = L[is_m]
    within = np.arange(int(Lm.sum()), dtype=np.int64) - np.repeat(np.concatenate(([0], np.cumsum(Lm)[:-1])), Lm)
    q_idx = np.repeat(q_off[:-1][is_m], Lm) + within
    q[q_idx] = t[np.repeat(t_off[:-1][is_m], Lm) + within]
    mism = np.asarray(mism, dtype=bool)
    assert mism.shape == q_idx.shape
    sub = q_idx[mism]
    q[sub] = ACGT[(np.searchsorted(ACGT, q[sub]) + 1) & 3]
    return t.tobytes(), q.tobytes(), COMP[q[::-1]].tobytes()


def m_columns(ops):
    return sum(L for L, c in ops if c == "M")


class Batch:
    """lines with their sequences; `at` is where the next line starts in the batch text"""

    def __init__(self, prefix=""):
        self.lines, self.seqs, self.ops, self.at, self.prefix = [], {}, [], 0, prefix

    def add(self, ops, mism, strand, margin=40, pad=0, tags="tp:A:P\tAS:i:777\ts1:i:42", seqs=None):
        """seqs: the (target, query, reverse complement) of an earlier call with the same ops, to put the same alignment on the other strand"""
        i = len(self.lines)
        t, q, qr = seqs or sequences(ops, 9000 + i, mism, margin)
        self.last_seqs = (t, q, qr)
        tn, qn = "%st%d" % (self.prefix, i), "%s%s%d" % (self.prefix, "q" if strand == "+" else "r", i)
        self.seqs[tn.encode()] = t
        self.seqs[qn.encode()] = q if strand == "+" else qr
        span_q = sum(L for L, c in ops if c in "MI")
        qs = margin if strand == "+" else len(q) - margin - span_q
        if pad:
            tags = tags + "\tzz:Z:" + "p" * pad
        line = record(ops, strand, qname=qn, tname=tn, qlen=len(q), tlen=len(t), qs=qs, ts=margin, tags=tags)
        self.lines.append(line)
        self.ops.append(list(ops))
        self.at += len(line)
        return i

    def cigar_start(self, i):
        return sum(len(l) for l in self.lines[:i]) + self.lines[i].index("cg:Z:") + 5

    def data(self):
        return "".join(self.lines).encode()


# ---- reading the oracle's lines ----
def cigar_of(line):
    return line.split(b"cg:Z:")[1].split(b"\t")[0].strip()


def ops_of(line):
    return [(int(n), c.decode()) for n, c in re.findall(rb"(\d+)([MID=X])", cigar_of(line))]


def new_per_input_op(in_ops, new_ops):
    """how many of the encoder's ops each input op became (an M op: the = and X runs that add up to it)"""
    out, j = [], 0
    for L, c in in_ops:
        n, covered = 0, 0
        while covered < (L if c == "M" else 1):
            covered += new_ops[j][0] if c == "M" else 1
            assert (new_ops[j][1] in "=X") == (c == "M")
            j += 1
            n += 1
        assert covered == (L if c == "M" else 1)
        out.append(n)
    assert j == len(new_ops)
    return out


def piece_of_input_ops(cigar_start, in_ops):
    """the 1 KiB tile of the batch that holds each input op's letter"""
    out, at = [], cigar_start
    for L, c in in_ops:
        at += len(str(L)) + 1
        out.append((at - 1) // TILE)
    return out


def new_ops_by_piece(cigar_start, in_ops, new_ops):
    """[new ops of the record's piece 0, of piece 1, ...]"""
    per = new_per_input_op(in_ops, new_ops)
    tiles = piece_of_input_ops(cigar_start, in_ops)
    out = [0] * (tiles[-1] - cigar_start // TILE + 1)
    for n, t in zip(per, tiles):
        out[t - cigar_start // TILE] += n
    return out


def cuts(add_line, trim_line):
    """(ops cut from the front, from the back) of the encoded cigar by the trim: what is left is a stretch of it, and the target start
    has moved over the target bases of the front's ops"""
    a, t = ops_of(add_line), ops_of(trim_line)
    d_ts = int(trim_line.split(b"\t")[7]) - int(add_line.split(b"\t")[7])
    found = []
    tb = 0
    for f in range(len(a) - len(t) + 1):
        if tb == d_ts and a[f:f + len(t)] == t:
            found.append(f)
        if f < len(a):
            tb += a[f][0] if a[f][1] != "I" else 0
    assert len(found) == 1, (found, len(a), len(t))
    return found[0], len(a) - len(t) - found[0]


# ---- T1: plain records with noisy ends ----
def noisy_ends_mask(n_cols, head, tail, every=37):
    """a substitution every `every`-th column, and every other column of the first `head` and the last `tail`"""
    m = np.zeros(n_cols, dtype=bool)
    m[every // 2::every] = True
    m[0:head:2] = True
    if tail:
        m[n_cols - 1:n_cols - 1 - tail:-2] = True
    return m


def plain_ops(rng, n):
    ops = []
    for k in range(n):
        ops.append((rng.choice((1, 5, 30, 60, 110)), "M") if k % 2 == 0 else (rng.choice((1, 2, 3)), rng.choice("ID")))
    if ops[-1][1] != "M":
        ops.append((30, "M"))
    return ops


_T1 = []


def t1_batch():
    """some 200 plain records, both strands, 40 to 3 000 ops, homologous sequences with noisy ends"""
    if not _T1:
        import random

        rng = random.Random(5101)
        b = Batch("a")
        for k in range(200):
            n = rng.choice((40, 41, 90, 300, 333, 700, 1400, 3000)) if k % 25 else 3000
            ops = plain_ops(rng, n)
            cols = m_columns(ops)
            head, tail = rng.choice((0, 0, 30, 60, 120)), rng.choice((0, 0, 20, 40, 90))
            b.add(ops, noisy_ends_mask(cols, min(head, cols // 3), min(tail, cols // 3)), "+-"[k & 1], pad=rng.randrange(0, 40))
        _T1.append(b)
    return _T1[0]


# ---- T2: cuts at piece boundaries ----
PAIR = [(2, "M"), (1, "D")]  # four bytes of text, two new ops when both columns differ: 2X 1D
BIG = 2000                   # a clean op this long behind a noisy end of at most 45 bases lifts the prefix identity over every threshold


def t2_ops(h_front, odd_front, h_back, odd_back, n6, n5):
    """Noise, body, noise. Front: h pairs `2M1D` whose columns all differ (2X 1D: identity 0), then the body's first op, 2000M, with its
    first column differing when odd: the trim's last hit is the last noisy op and no suffix that ends there reaches the record's
    identity, so it cuts 2 h + odd new ops. The back is the mirror image. Between the two 2000M ops: 1I, n6 x 200M1I, n5 x 20M1I
    (2 + 6 n6 + 5 n5 bytes of text, clean columns)."""
    ops = PAIR * h_front + [(BIG, "M"), (1, "I")] + [(200, "M"), (1, "I")] * n6 + [(20, "M"), (1, "I")] * n5 + [(BIG, "M")] + [(1, "D"), (2, "M")] * h_back
    cols = m_columns(ops)
    mism = np.zeros(cols, dtype=bool)
    mism[:2 * h_front + odd_front] = True
    mism[cols - 2 * h_back - odd_back:] = True
    return ops, mism


RELS = (-2, -1, 0, 1)  # the cut's last op against the boundary: the op before the piece's last, its last, the next piece's first, the one behind


def t2_search(rel_front, rel_back):
    """(h_front, odd_front, L_front, h_back, odd_back, mid_bytes): a record whose front cut ends `rel_front` new ops from the first op of
    its piece 1 (-1: on the last new op of piece 0, 0: on the first of piece 1) when its cigar starts L_front bytes in front of a tile
    boundary, and whose back cut, counted from the end, ends rel_back from the last op of the piece before the last"""
    front = back = None
    for L in range(24, 80):
        for h in range(4, 15):
            for odd in (0, 1):
                # letters of the front's ops: pair k at bytes 4k + 1 and 4k + 3, the body's first op at 4h + 4
                in_piece0 = sum(1 for k in range(h) for o in (1, 3) if 4 * k + o < L) + ((1 + odd) if 4 * h + 4 < L else 0)
                # the body's first op must be the last op of piece 0 or lie in piece 1: the op behind it (1I, letter at 4h + 6) is in piece 1
                if 4 * h + 6 < L:
                    continue
                if front is None and (2 * h + odd - 1) - in_piece0 == rel_front:
                    front = (h, odd, L)
                # mirror image: the text ends L bytes behind a boundary. From the end: pair k has letters at 4k (M) and 4k + 2 (D), the body's
                # last op at 4h, the op in front of it (1I) at 4h + 5
                in_last = sum(1 for k in range(h) for o in (0, 2) if 4 * k + o < L) + ((1 + odd) if 4 * h < L else 0)
                if 4 * h + 5 < L:
                    continue
                if back is None and (2 * h + odd - 1) - in_last == rel_back:
                    back = (h, odd, L)
    assert front and back, (rel_front, rel_back, front, back)
    return front, back


_T2 = []


def t2_batch():
    """Per strand four records: record k's front cut ends RELS[k] from the first boundary of its cigar, its back cut RELS[k] from the
    last one. Returns (batch, [(ops cut in front, ops cut behind, rel front, rel back)] as built)."""
    if not _T2:
        b, want = Batch("b"), []
        for strand in "+-":
            for rel in RELS:
                (hf, of, lf), (hb, ob, lb) = t2_search(rel, rel)
                fixed = 4 * hf + 5 + 2 + 5 + 4 * hb
                # the cigar's first byte lf bytes in front of a boundary, its end lb bytes behind one
                mid = next(m for m in range(1400, 1400 + TILE) if (fixed + m - lf) % TILE == lb)
                n5 = (-mid) % 6
                ops, mism = t2_ops(hf, of, hb, ob, (mid - 5 * n5) // 6, n5)
                text_len = sum(len(str(L)) + 1 for L, _ in ops)
                assert text_len == fixed + mid
                i = b.add(ops, mism, strand, pad=_pad_for(b, ops, mism, strand, lf))
                assert (b.cigar_start(i) + lf) % TILE == 0 and (b.cigar_start(i) + text_len) % TILE == lb
                want.append((2 * hf + of, 2 * hb + ob, rel, rel))
        _T2.append((b, want))
    return _T2[0]


def _pad_for(b, ops, mism, strand, lf):
    """the tag pad that puts the cigar of the next line lf bytes in front of a tile boundary (the pad's own tag takes 6 bytes more)"""
    probe = Batch(b.prefix)
    probe.lines, probe.at, probe.ops = list(b.lines), b.at, list(b.ops)
    probe.add(ops, mism, strand, pad=1)
    start = probe.cigar_start(len(probe.lines) - 1)
    return 1 + (-lf - start) % TILE


def t2_seen(batch, add_out, trim_out):
    """per record (strand, rel front, rel back) as the oracle's two outputs show them; rel back is None where the back was not cut (the
    second pass of paf_trim_unreliable_tails works on the inverted record, and paf_invert reverses the cigar of a '-' record only,
    impl/paf.c:469-490: a '+' record's back is never trimmed)"""
    seen = []
    as_lines = lambda x: x.splitlines() if isinstance(x, bytes) else x  # noqa: E731
    for i, (a, t) in enumerate(zip(as_lines(add_out), as_lines(trim_out))):
        f, k = cuts(a, t)
        per_piece = new_ops_by_piece(batch.cigar_start(i), batch.ops[i], ops_of(a))
        assert len(per_piece) >= 3 and f > 0
        seen.append((batch.lines[i].split("\t")[4], (f - 1) - per_piece[0], (k - 1) - per_piece[-1] if k else None))
    return seen


# ---- T4: filter ties ----
F32 = np.float32
TIE = float(F32(7) / F32(10))  # (double)((float)7 / 10): a threshold of 0.7 itself lies ABOVE it


def sums_record(b, eq, xx, ins=0, dele=0, strand="+", tags="tp:A:P\tAS:i:777\ts1:i:42"):
    """a record whose encoded cigar has eq bases in = ops, xx in X ops (every other column of its first M op, from the second on), and an
    I / a D op of `ins` / `dele` bases, each with a clean 3M behind it"""
    rest = ([(ins, "I"), (3, "M")] if ins else []) + ([(dele, "D"), (3, "M")] if dele else [])
    first = eq + xx - sum(L for L, c in rest if c == "M")
    assert first >= 2 * xx + 1
    ops = [(first, "M")] + rest
    mism = np.zeros(m_columns(ops), dtype=bool)
    mism[1:2 * xx:2] = True
    assert int(mism.sum()) == xx
    return b.add(ops, mism, strand, tags=tags)


def t4_identity_batch():
    """identity = eq / (eq + xx) at 0.7f exactly, with one = base more and one less; both strands; gaps that do not count"""
    b, want = Batch("c"), []
    for strand in "+-":
        for eq in (69, 70, 71):
            sums_record(b, eq, 30, ins=4, dele=5, strand=strand)
            want.append((eq, 30))
    return b, want


def t4_gaps_batch():
    """identity with gaps = eq / (eq + xx + ins + del) at 0.7f exactly, one = base more, one less"""
    b, want = Batch("d"), []
    for strand in "+-":
        for eq in (69, 70, 71):
            sums_record(b, eq, 21, ins=4, dele=5, strand=strand)
            want.append((eq, 30))
    return b, want


def quot(a, d):
    return float(F32(F32(a) / F32(d)))


def t4_tags_batch():
    """three records that differ in alignment score, chain score and tile level"""
    b = Batch("t")
    for tags in ("tp:A:P\tAS:i:900\ttl:i:1\ts1:i:50", "tp:A:S\tAS:i:100\ttl:i:2\ts1:i:45", "tp:A:P\tAS:i:100\ttl:i:1\ts1:i:30"):
        sums_record(b, 90, 10, ins=2, dele=2, tags=tags)
    return b


T4_TRIM_THRESHOLDS = dict(min_identity=0.9345)


def t4_trim_batch():
    """Two '+' records under min_identity 0.9345 (matches over matches and mismatches: gaps do not count; the trim's own identity counts
    them). The first has a head of 10M20D pairs on matching columns -- identity 1 for the filter, a third for the trim, which cuts it --
    in front of a clean 5000M and a body with every tenth column differing: 0.9355 untrimmed, 0.9333 trimmed. The second has a head of
    1 200 columns of which every other differs, a clean 5000M and a body with every twentieth column differing: 0.932 untrimmed,
    0.967 trimmed."""
    b = Batch("u")
    ops = [(10, "M"), (20, "D")] * 50 + [(5000, "M"), (1, "I"), (5000, "M"), (1, "D"), (5000, "M")]
    m = np.zeros(m_columns(ops), dtype=bool)
    m[5505::10] = True
    b.add(ops, m, "+")
    ops = [(1200, "M"), (5000, "M"), (1, "I"), (5000, "M"), (1, "D"), (5000, "M")]
    m = np.zeros(m_columns(ops), dtype=bool)
    m[0:1200:2] = True
    m[6210::20] = True
    b.add(ops, m, "+")
    return b


def t9_batch():
    """one record whose cigar starts on a tile boundary: 200 clean columns, ten 8191M ops on alternating columns (fifty bytes of text,
    81 910 new ops, all in the record's first piece), then 150 clean 8191M ops"""
    ops = [(200, "M"), (1, "I")] + [(8191, "M")] * 10 + [(1, "I")] + [(8191, "M"), (1, "I")] * 150 + [(30, "M")]
    m = np.zeros(m_columns(ops), dtype=bool)
    m[200:200 + 81910:2] = True
    b = Batch("w")
    b.add(ops, m, "+", pad=_pad_for(b, ops, m, "+", 0))
    assert b.cigar_start(0) % TILE == 0
    return b


def t6_batch():
    """Lines of more than 32 768 new ops, a clean 2000M at either end of the cigar: two without noise ('+', '-'), two with a noisy head
    and tail of a few hundred columns, two with a noisy head of 44 000 columns (and, '-', a tail of 36 000): more than a segment's worth"""
    import random

    from test_gpu_flat import exact_ops

    rng = random.Random(5107)
    ops = [(2000, "M"), (1, "I")] + exact_ops(rng, 40_001, lens=(1, 5, 30, 60, 110), indel=(1, 2, 3)) + [(1, "I"), (2000, "M")]
    cols = m_columns(ops)
    b = Batch("g")
    b.add(ops, noisy_ends_mask(cols, 0, 0), "+")
    b.add(ops, None, "-", seqs=b.last_seqs)
    b.add(ops, noisy_ends_mask(cols, 400, 300), "+")
    b.add(ops, None, "-", seqs=b.last_seqs)
    b.add(ops, noisy_ends_mask(cols, 44_000, 0), "+")
    b.add(ops, noisy_ends_mask(cols, 44_000, 36_000), "-")
    return b

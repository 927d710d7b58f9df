"""Adversarial FASTA files for the device loaders (paffy_hip_set_sequences_fasta and friends) and PAF records over their sequences.

Each corpus is a list of files (bytes each). faffy_lib.fasta_read_files gives the records the reference's reader makes of them;
`clean` writes the same records one file per file again in the plainest layout, which any reader reads the same way."""
import random

import faffy_lib as F


def _bases(rnd, n):
    return bytes(rnd.choice(b"ACGTacgtNNn") for _ in range(n))


def _wrap(rnd, s, width, eol=b"\n"):
    """s in lines of `width`, with blanks and tabs sprinkled inside the lines"""
    out = []
    for i in range(0, len(s), width):
        line = bytearray(s[i:i + width])
        if rnd.random() < 0.3 and line:
            at = rnd.randrange(len(line) + 1)
            line[at:at] = rnd.choice([b" ", b"\t", b"  \t", b"\r", b"\r\r"])
        out.append(bytes(line) + eol)
    return b"".join(out)


def adversarial(seed=1):
    """every layout case of the issue in four files, one of them empty"""
    rnd = random.Random(seed)
    a = [b"stray line before any header\n", b">chr1 first record, name with spaces\r\n", _wrap(rnd, _bases(rnd, 300), 60, b"\r\n"),
         b">empty\n", b">len0\n\n", b">len1\nA\n", b">len15\n" + _bases(rnd, 15) + b"\n", b">len16\n" + _bases(rnd, 16) + b"\r\r\n",
         b">len17\n" + _bases(rnd, 10) + b"\r" + _bases(rnd, 7) + b"\n", b">\n", b"ACGT\n", b">dup\n" + _bases(rnd, 40) + b"\n",
         b">nrun\n" + b"N" * 70 + b"n" * 33 + b"\n", b">lower\n" + _bases(rnd, 90).lower() + b"\n", b">dup\n" + _bases(rnd, 55) + b"\n",
         b">tail no newline"]
    b = [b"\n\nlines before the first header of a later file\n", b">dup\n", _wrap(rnd, _bases(rnd, 130), 80),
         b">chr2\t tabbed name\n", _wrap(rnd, _bases(rnd, 517), 61), b">cr run \r\r\n", _bases(rnd, 33), b"\r\r\r\n",
         b">last\n" + _bases(rnd, 20)]
    c = []
    d = [b">only\r\n", _bases(rnd, 64), b"\r"]
    return [b"".join(a), b"".join(b), b"".join(c), b"".join(d)]


def scaffolds(n=200_000, seed=2):
    """a fragmented assembly: n one-line scaffolds of 1..40 bases"""
    rnd = random.Random(seed)
    return [b"".join(b">scaf%d\n%s\n" % (i, _bases(rnd, rnd.randrange(1, 41))) for i in range(n))]


def clean(files):
    """the same records, one file per file, '>' + header + '\\n' + the bases on one line"""
    return [b"".join(F.write_record(h, s) for h, s in F.fasta_read(f)) for f in files]


def records(files):
    return F.fasta_read_files(files)


def paf(files, n, seed=3, strands=b"+-"):
    """n records between sequences of the files (names without NUL bytes or tabs, at least one base), with M-only cigars"""
    rnd = random.Random(seed)
    shortest = {}  # a duplicate name stays inside its shortest record (which record the lookup finds is not pinned)
    for h, s in records(files):
        shortest[h] = min(shortest.get(h, len(s)), len(s))
    recs = [(h, n) for h, n in shortest.items() if n and h and b"\t" not in h and b"\0" not in h]
    out = []
    for _ in range(n):
        (qn, ql), (tn, tl) = rnd.choice(recs), rnd.choice(recs)
        m = rnd.randrange(1, min(ql, tl) + 1)
        qs, ts = rnd.randrange(0, ql - m + 1), rnd.randrange(0, tl - m + 1)
        out.append(b"%s\t%d\t%d\t%d\t%c\t%s\t%d\t%d\t%d\t%d\t%d\t60\tcg:Z:%dM\n" % (qn, ql, qs, qs + m, rnd.choice(strands), tn, tl, ts, ts + m, m, m, m))
    return b"".join(out)

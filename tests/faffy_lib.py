"""Checker of `faffy chunk | extract | merge` (impl/fasta_chunk.c, impl/fasta_extract.c, impl/fasta_merge.c): a Python restatement
of the FASTA reader (host/paffy_cmds.c:fasta_read) and of the three commands, byte for byte. Numbers go through the C library's own
atol (ctypes), as the reference's do.

Outcomes are (output, status): status 0, 1 (exit(1) / st_errAbort) or 134 (assert). After a 134 the output is not part of the
contract: the checker returns None for it.
"""
import ctypes as C

_libc = C.CDLL("libc.so.6")
_libc.atol.restype = C.c_long
_libc.atol.argtypes = [C.c_char_p]

I64 = 1 << 64


def atol(tok):
    return _libc.atol(bytes(tok))


def wrap(x):
    return (x + (1 << 63)) % I64 - (1 << 63)


def fasta_read(text):
    """One FASTA file -> [(header, bases)]: lines end at '\\n' (the last may not); each loses its trailing run of '\\r' / '\\n'; a line
    starting with '>' starts a record named by the rest of the line; other lines add their bytes but ' ' and '\\t' to the current
    record; lines before the file's first header are dropped."""
    recs = []
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # the text ended with '\n'
    for line in lines:
        line = line.rstrip(b"\r\n")
        if line[:1] == b">":
            recs.append([line[1:], bytearray()])
        elif recs:
            recs[-1][1] += line.replace(b" ", b"").replace(b"\t", b"")
    return [(h, bytes(s)) for h, s in recs]


def fasta_read_files(files):
    out = []
    for f in files:
        out += fasta_read(f)
    return out


def write_record(header, bases):
    """The one layout of a written record (fastaWrite is unpinned): '>' + header + '\\n' + all bases on one line + '\\n'."""
    return b">" + header + b"\n" + bases + b"\n"


def bases_ok(s):
    """tolower(c) in {a, c, g, t, n} for every byte"""
    return not bytes(s).translate(None, b"acgtnACGTN")


def chunk(files, c=10000000, o=100000, d="./temp_fastas"):
    """faffy chunk: ([(path, bytes)], status). The up-front rejection (c > o but c <= 0 or c + o < 0 or overflowing) is status 1."""
    if c > o and (c <= 0 or c + o < 0 or c + o >= 1 << 63):
        return None, 1
    out, cur, remaining, k = [], None, c, 0
    for name, seq in fasta_read_files(files):
        if not c > o:
            return None, 134
        n = len(seq)
        i = 0
        while i < n:
            if cur is None:
                cur = [f"{d}/{k}.fa", bytearray()]
                k += 1
                remaining = c
            j = min(i + c + o, n)
            piece = seq[i:j]
            if not bases_ok(piece):
                return None, 134
            cur[1] += write_record(b"%s|%d|%d" % (name, n, i), piece)
            remaining -= j - i
            if remaining <= 0:
                out.append((cur[0], bytes(cur[1])))
                cur = None
            i += c
    if cur is not None:
        out.append((cur[0], bytes(cur[1])))
    return out, 0


def bed_lines(bed):
    lines = bed.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def extract(files, bed, flank=10, min_size=100, skip_missing=False):
    """faffy extract: (bytes, status, message)"""
    seqs = {}
    for name, seq in fasta_read_files(files):
        seqs[name] = seq  # duplicate names: the last one wins
    ivs = []
    for line in bed_lines(bed):
        toks = line.split()
        if len(toks) < 3:
            return None, 134, None
        if toks[0] not in seqs:
            if skip_missing:
                continue
            return b"", 1, b"Missing sequence: %s\n" % toks[0]
        ivs.append((toks[0], atol(toks[1]), atol(toks[2])))
    ivs.sort()
    out = bytearray()
    prev = None  # [name, start, end]

    def report(name, s, e):
        seq = seqs[name]
        piece = seq[s:e]
        if not bases_ok(piece):
            return False
        out.extend(write_record(b"%s|%d|%d" % (name, len(seq), s), piece))
        return True

    for name, start, end in ivs:
        if wrap(end - start) < min_size:
            continue
        n = len(seqs[name])
        sf, ef = wrap(start - flank), wrap(end + flank)
        i = sf if sf > 0 else 0
        j = ef if ef <= n else n
        if not (0 <= i <= start <= end <= j <= n):
            return None, 134, None
        if prev is not None:
            if prev[0] == name and prev[2] >= i:
                prev[2] = max(prev[2], j)
                continue
            if not report(*prev):
                return None, 134, None
        prev = [name, i, j]
    if prev is not None and not report(*prev):
        return None, 134, None
    return bytes(out), 0, None


def merge(files):
    """faffy merge over chunk files (bytes each, in list order): (bytes, status)"""
    out = bytearray()
    pending = None  # (coordinate, bases)
    for header, seq in fasta_read_files(files):
        toks = header.split(b"|")
        off = atol(toks[-1])
        if off < 0:
            return None, 134
        if off == 0:
            if pending is not None:
                out += pending[1] + b"\n"
            if len(toks) < 2:
                return None, 134
            out += b">" + b"|".join(toks[:-2]) + b"\n"
            pending = (0, seq)
        else:
            if pending is None:
                return None, 134
            pc, pseq = pending
            if not (pc <= off and pc + len(pseq) >= off):
                return None, 134
            sp = (pc + len(pseq) + off) // 2
            out += pseq[: sp - pc] + b"\n"
            if sp - off > len(seq):
                return None, 134
            pending = (sp, seq[sp - off:])
    if pending is not None:
        out += pending[1] + b"\n"
    return bytes(out), 0

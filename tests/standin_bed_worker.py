#!/usr/bin/env python3
"""Stand-in for `bin/paffy_gpu to_bed` in the CPU tests of the N-GPU launcher (tests/test_launcher_to_bed.py). It honours the part-mode
contract of host/paffy_launch.c -- PAFFY_BED_PART=<prefix> (reads <prefix>.idx and <prefix>.sides, writes <prefix>.bkeys and, under -f -q,
<prefix>.seen; the one worker that is asked reads <prefix>.seen_all and writes <prefix>.tail), PAFFY_BED_FDS=<from_launcher>,<to_launcher>
(a report of eight int64, one int64 verdict back: 0 go on, 1 you are the failure, 2 end) -- and computes the coverage in plain Python:
a side of a line is counted where its mask says so (bit 0 the query side, bit 1 the target side, as the inverted record would count).
Without PAFFY_BED_PART it is the one-worker command over the whole input (every side, the -q tail its own).

A line with strand '*' does not parse (exit status 1); a sequence seen with two lengths, or a cigar that does not end at the range's end,
fails that side (SIGABRT, as an assert would). The message names the global record.

Switches (environment): STANDIN_BED_LOG=path -- every worker appends "<rank>/<world> <its arguments>"; STANDIN_BED_DUMP=dir -- every part
worker writes <dir>/<rank>.json, its [global record, mask] pairs; STANDIN_BED_EXIT_RANK=r -- worker r exits with status 7 before it
reports; STANDIN_BED_LONG_OUT=r -- worker r writes one byte more than its block keys say. Test infrastructure only."""
import getopt
import json
import os
import re
import signal
import struct
import sys

GO_ON, YOU_FAILED, END = 0, 1, 2
LONG = ["logLevel=", "inputFile=", "outputFile=", "binary", "excludeUnaligned", "excludeAligned", "minSize=", "includeInverted", "queryFastaFile=", "help"]


class Failure(Exception):
    def __init__(self, record, kind, what):
        super().__init__(what)
        self.record, self.kind, self.what = record, kind, what

    def message(self):
        return f"stand-in to_bed: {self.what} in record {self.record}"


def walk(ops, start, end, length, counts, skip):
    """increase_alignment_level_counts over one side: M = X bump, `skip` (I on the query side, D on the target side) moves on"""
    i = start
    for n, op in ops:
        if op in "M=X":
            for pos in range(i, i + n):
                if not (0 <= pos < end and pos < length):
                    return False
                counts[pos] = min(counts[pos] + 1, 32766)
            i += n
        elif op == skip:
            i += n
    return i == end


def cover(lines, numbers, masks, with_target):
    """-> [(2 * global record + side, name, counters)] in order of first appearance, or raises the first Failure"""
    seqs, order = {}, []
    for ln, g, mask in zip(lines, numbers, masks):
        f = ln.split(b"\t")
        if len(f) < 12 or f[4] not in (b"+", b"-"):
            raise Failure(g, 0, "a line that does not parse")
        cg = [t[5:].decode() for t in f[12:] if t.startswith(b"cg:Z:")]
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDX=])", cg[-1])] if cg else []
        sides = [(0, f[0], int(f[1]), int(f[2]), int(f[3]), ops, "I")]
        if with_target:
            sides.append((1, f[5], int(f[6]), int(f[7]), int(f[8]), ops[::-1] if f[4] == b"-" else ops, "D"))
        for side, name, length, start, end, side_ops, skip in sides:
            if not mask & (1 << side):
                continue
            if name not in seqs:
                seqs[name] = (length, [0] * length)
                order.append((2 * g + side, name))
            if seqs[name][0] != length:
                raise Failure(g, side + 1, "another length of %s" % name.decode())
            if not walk(side_ops, start, end, length, seqs[name][1], skip):
                raise Failure(g, side + 1, "a walk that leaves its range on %s" % name.decode())
    return [(key, name, seqs[name][1]) for key, name in order]


def block(name, counts, binary, no_unaligned, no_aligned, min_size):
    """write_bed of one sequence"""
    out, i, n = [], 0, len(counts)
    while i < n:
        j = i + 1
        while j < n and ((counts[i] > 0) == (counts[j] > 0) if binary else counts[i] == counts[j]):
            j += 1
        if j - i >= min_size and not (no_unaligned if counts[i] == 0 else no_aligned):
            out.append(name + b" %d %d %d\n" % (i, j, (counts[i] > 0) if binary else counts[i]))
        i = j
    return b"".join(out)


def fasta_records(path):
    """[(header, bases)] of a small FASTA file; None when it cannot be opened"""
    try:
        with open(path, "rb") as fh:
            text = fh.read()
    except OSError:
        return None
    recs = []
    for ln in text.splitlines():
        if ln.startswith(b">"):
            recs.append([ln[1:], 0])
        elif recs:
            recs[-1][1] += len(ln.strip())
    return recs


def names_used(lines, with_target):
    used = set()
    for ln in lines:
        f = ln.split(b"\t")
        used.add(f[0])
        if with_target and len(f) >= 6:
            used.add(f[5])
    return used


def tail_lines(recs, seen):
    return b"".join(b"%s 0 %d\t0\n" % (h, n) for (h, n), s in zip(recs, seen) if not s)


def die(failure):
    sys.stderr.write(failure.message() + "\n")
    sys.stderr.flush()
    if failure.kind == 0:
        sys.exit(1)
    os.kill(os.getpid(), signal.SIGABRT)


def main():
    args = sys.argv[1:]
    assert args[0] == "to_bed", args
    rank, world = os.environ.get("PAFFY_RANK", ""), os.environ.get("PAFFY_WORLD", "")
    if os.environ.get("STANDIN_BED_LOG"):
        with open(os.environ["STANDIN_BED_LOG"], "a") as fh:
            fh.write(f"{rank}/{world} {' '.join(args)}\n")
    opts, rest = getopt.gnu_getopt([a for a in args[1:] if a != "--"], "l:i:o:hbefm:nq:", LONG)
    o = {}
    for k, v in opts:
        o[{"--" + name.rstrip("="): "-" + short for name, short in zip(LONG, "liobefmnqh")}.get(k, k)] = v
    with_target, tail = "-n" in o, "-f" in o and "-q" in o
    style = ("-b" in o, "-e" in o, "-f" in o, int(o.get("-m", "1")))
    with (open(o["-i"], "rb") if "-i" in o else sys.stdin.buffer) as fh:
        lines = fh.read().splitlines()
    out = open(o["-o"], "wb") if "-o" in o else sys.stdout.buffer
    part = os.environ.get("PAFFY_BED_PART")
    if not part:  # the one-worker command
        try:
            seqs = cover(lines, range(len(lines)), [3] * len(lines), with_target)
        except Failure as failure:
            die(failure)
        out.write(b"".join(block(name, counts, *style) for _, name, counts in seqs))
        recs = fasta_records(o["-q"]) if tail else None
        if recs:
            used = names_used(lines, with_target)
            out.write(tail_lines(recs, [h in used for h, _ in recs]))
        out.flush()
        return

    from_fd, to_fd = (int(x) for x in os.environ["PAFFY_BED_FDS"].split(","))
    assert "PAFFY_CHAIN_PART" not in os.environ and "PAFFY_CHAIN_FDS" not in os.environ
    if os.environ.get("STANDIN_BED_EXIT_RANK") == rank:
        sys.exit(7)

    def verdict():
        got = os.read(from_fd, 8)
        if len(got) < 8:
            sys.exit(1)  # end-of-file in place of a verdict
        return struct.unpack("<q", got)[0]

    def report(phase, failed, record, kind, count):
        os.write(to_fd, struct.pack("<8q", phase, 1 if failed else 0, record, kind, 0, count, 0, 0))
        return verdict()

    with open(part + ".idx", "rb") as fh:
        raw = fh.read()
    numbers = list(struct.unpack(f"<{len(raw) // 8}q", raw))
    with open(part + ".sides", "rb") as fh:
        masks = list(fh.read())
    assert len(numbers) == len(lines) == len(masks), (len(numbers), len(lines), len(masks))
    assert all(a < b for a, b in zip(numbers, numbers[1:])), "a line reached this part twice, or out of order"
    assert all(m in (1, 2, 3) if with_target else m == 1 for m in masks), masks
    assert all(m == 1 for ln, m in zip(lines, masks) if ln.count(b"\t") < 5), "a line without a target name has a query side only"
    if os.environ.get("STANDIN_BED_DUMP"):
        with open(os.path.join(os.environ["STANDIN_BED_DUMP"], rank + ".json"), "w") as fh:
            json.dump(list(zip(numbers, masks)), fh)
    try:
        seqs = cover(lines, numbers, masks, with_target)
    except Failure as failure:
        v = report(1, True, failure.record, failure.kind, 0)
        if v == YOU_FAILED:
            die(failure)
        sys.exit(0 if v == END else 1)
    blocks = [block(name, counts, *style) for _, name, counts in seqs]
    with open(part + ".bkeys", "wb") as fh:
        for (key, _, _), b in zip(seqs, blocks):
            fh.write(struct.pack("<3q", key, len(b), b.count(b"\n")))
    recs = None
    if tail:
        recs = fasta_records(o["-q"]) or []
        used = names_used(lines, with_target)
        with open(part + ".seen", "wb") as fh:
            fh.write(bytes(1 if h in used else 0 for h, _ in recs))
    v = report(1, False, 0, 0, len(seqs))
    if v != GO_ON:
        sys.exit(0 if v == END else 1)
    out.write(b"".join(blocks) + (b"!" if os.environ.get("STANDIN_BED_LONG_OUT") == rank else b""))
    out.flush()
    if tail:
        if verdict() != GO_ON:
            sys.exit(0)
        with open(part + ".seen_all", "rb") as fh:
            seen_all = list(fh.read())
        assert len(seen_all) == len(recs)
        with open(part + ".tail", "wb") as fh:
            fh.write(tail_lines(recs, seen_all))
        if report(2, False, 0, 0, 0) != GO_ON:
            sys.exit(1)


if __name__ == "__main__":
    main()

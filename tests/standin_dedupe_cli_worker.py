#!/usr/bin/env python3
"""Stand-in for `bin/paffy_gpu dedupe` in the CPU tests of the N-GPU launcher (tests/test_launcher_dedupe.py). It honours the part-mode
contract of host/paffy_launch.c and host/paffy_stream.c in plain Python:

  PAFFY_DEDUPE_PART=<spooldir>/<rank>, PAFFY_DEDUPE_FDS=<from_launcher>,<to_launcher>, PAFFY_RANK, PAFFY_WORLD = N,
  PAFFY_DEDUPE_SHARE_BYTES = C; cut(j) = the first line end at or after j * C (cut(0) = 0, the last cut the file's size); in round k
  this worker takes share k * N + rank = [cut(j), cut(j + 1)); a record's number is cut(j) + its index in the share;
  per round four phases, after each a report of eight int64 {phase, 0, a, 0, 0, count, 0, 0} and one int64 back, code in the two low
  bits (0 go on, 1 speak, 2 end), a number above them:
    1 keys      <rank>.ent (32-byte entries grouped by owner), <rank>.cnt (N int64); count = records of the share
    2 decide    the owner reads its stretch of every <s>.ent, writes <rank>.ver (one byte per entry)
    3 verdicts  the worker reads its stretch of every <p>.ver; a = its lowest failing number or -1; the answer carries the run's + 1
    4 write     the lines in front of the run's failing record appended to the -o spool; count = bytes, a = 1: the record is here;
                on "speak" the number is the count of records in front of the share.

A key is 128 bits of BLAKE2 over the seven fields (the contract asks only that equal records have equal keys); the owner is
shard.dedupe_owner of the class key. The CPU oracle is asked about single lines only. Without PAFFY_DEDUPE_PART it is the one-worker
run: the oracle's dedupe over the whole input, the same message and status.

Switches (environment): STANDIN_DEDUPE_LOG=path -- every worker appends "<rank>/<world> <part or -> <its arguments>";
STANDIN_DEDUPE_EXIT="rank:phase:round" -- that worker exits with status 7 in place of that report. Test infrastructure only."""
import hashlib
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import oracle_lib as O  # noqa: E402
from paffy_amd.shard import dedupe_owner  # noqa: E402

GO_ON, SPEAK, END = 0, 1, 2
MASK = (1 << 64) - 1


def key128(qn, tn, strand, qs, qe, ts, te):
    d = hashlib.blake2b(b"\0".join([qn, tn, strand, qs, qe, ts, te]), digest_size=16).digest()
    return int.from_bytes(d[:8], "little"), int.from_bytes(d[8:], "little")


def die(err, record):
    sys.stdout.flush()
    sys.stderr.write(f"stand-in dedupe: error {err.code} (stage {err.stage}, aux {err.aux}) in record {record}\n")
    sys.exit(O.exit_status(err.code) or 1)


def options(args):
    assert args[0] == "dedupe", args
    inv, inp, out, k = False, None, None, 1
    while k < len(args):
        if args[k] == "-a":
            inv = True
        elif args[k] in ("-i", "-o", "-l"):
            if args[k] == "-i":
                inp = args[k + 1]
            if args[k] == "-o":
                out = args[k + 1]
            k += 1
        else:
            sys.stderr.write("stand-in dedupe: usage\n")
            sys.exit(0 if args[k] == "-h" else 1)
        k += 1
    return inv, inp, out


def plain(inv, inp, out):
    if inp is None:
        data = sys.stdin.buffer.read()
    else:
        try:
            with open(inp, "rb") as fh:
                data = fh.read()
        except OSError:
            sys.stderr.write(f"stand-in dedupe: cannot open {inp}\n")
            sys.exit(1)
    fh = open(out, "wb") if out else sys.stdout.buffer
    text, err = O.dedupe(data, inv)
    fh.write(text)
    fh.flush()
    if err.code:
        die(err, err.record)


class Part:
    def __init__(self, inv, inp, out):
        self.inv, self.out = inv, open(out, "wb")
        self.dir = os.path.dirname(os.environ["PAFFY_DEDUPE_PART"])
        self.from_fd, self.to_fd = (int(x) for x in os.environ["PAFFY_DEDUPE_FDS"].split(","))
        self.rank, self.n = int(os.environ["PAFFY_RANK"]), int(os.environ["PAFFY_WORLD"])
        self.share = int(os.environ["PAFFY_DEDUPE_SHARE_BYTES"])
        self.fd = os.open(inp, os.O_RDONLY)
        self.size = os.fstat(self.fd).st_size
        self.memory = {}  # class key -> orientation bit of the record written for it
        self.exit_at = tuple(int(x) for x in os.environ.get("STANDIN_DEDUPE_EXIT", "-1:0:0").split(":"))
        self.round = 0

    def path(self, rank, ext):
        return os.path.join(self.dir, f"{rank}.{ext}")

    def cut(self, j):
        if j <= 0:
            return 0
        at = j * self.share
        while at < self.size:
            blk = os.pread(self.fd, 65536, at)
            if not blk:
                break
            nl = blk.find(b"\n")
            if nl >= 0:
                return at + nl + 1
            at += len(blk)
        return self.size

    def settle(self, phase, a, count):
        if self.exit_at == (self.rank, phase, self.round):
            sys.exit(7)
        os.write(self.to_fd, struct.pack("<8q", phase, 0, a, 0, 0, count, 0, 0))
        got = os.read(self.from_fd, 8)
        if len(got) < 8:
            sys.exit(1)  # end-of-file in place of an answer
        v = struct.unpack("<q", got)[0]
        if v & 3 == END:
            sys.exit(0)
        if v & 3 == 3 or (v & 3 == SPEAK and phase != 4):
            sys.exit(1)
        return v

    def keys(self, lines, base):
        """-> (segments of (class hi, class lo, number, flags) per owner, their records, written forms, failures per record)"""
        seg, rec = [[] for _ in range(self.n)], [[] for _ in range(self.n)]
        written, failure = [], {}
        for i, ln in enumerate(lines):
            text, err = O.dedupe(ln)  # one line, no -a: it is written unless it does not parse
            written.append(text)
            if err.code:
                failure[i] = err
                continue
            f = ln.rstrip(b"\n").split(b"\t")
            own, swap = key128(f[0], f[5], f[4], f[2], f[3], f[7], f[8]), key128(f[5], f[0], f[4], f[7], f[8], f[2], f[3])
            cls = min(own, swap) if self.inv else own
            chk = O.dedupe(ln, True)[1]  # alone with -a: its own key is not found, so paf_check runs
            if chk.code:
                failure[i] = chk
            p = dedupe_owner(cls[0], cls[1], self.n)
            seg[p].append((cls[0], cls[1], base + i, (1 if cls == own else 0) | (2 if chk.code else 0)))
            rec[p].append(i)
        for p in range(self.n):  # the order inside a segment is free: backwards here
            seg[p].reverse()
            rec[p].reverse()
        return seg, rec, written, failure

    def decide(self, rows):
        order = sorted(range(len(rows)), key=lambda j: rows[j][:3])
        verdict, head, new = bytearray(len(rows)), None, {}
        for j in order:
            cls, bit = rows[j][:2], rows[j][3] & 1
            is_head = head is None or head[0] != cls
            if is_head:
                head = (cls, bit)
            found = self.memory[cls] == bit if cls in self.memory else (not is_head and head[1] == bit)
            if is_head and cls not in self.memory:
                verdict[j] |= 1
                new[cls] = bit
            if self.inv and not found and rows[j][3] & 2:
                verdict[j] |= 2
        self.memory.update(new)
        return bytes(verdict)

    def run(self):
        n, me = self.n, self.rank
        shares = -(-self.size // self.share)
        for self.round in range(-(-shares // n)):
            a, b = self.cut(self.round * n + me), self.cut(self.round * n + me + 1)
            lines = os.pread(self.fd, b - a, a).splitlines(keepends=True) if b > a else []
            seg, rec, written, failure = self.keys(lines, a)
            with open(self.path(me, "ent"), "wb") as fh:
                for s in seg:
                    for row in s:
                        fh.write(struct.pack("<QQqQ", *row))
            with open(self.path(me, "cnt"), "wb") as fh:
                fh.write(struct.pack(f"<{n}q", *[len(s) for s in seg]))
            self.settle(1, 0, len(lines))
            cnt = []
            for s in range(n):
                with open(self.path(s, "cnt"), "rb") as fh:
                    cnt.append(struct.unpack(f"<{n}q", fh.read()))
            rows = []
            for s in range(n):
                with open(self.path(s, "ent"), "rb") as fh:
                    fh.seek(32 * sum(cnt[s][:me]))
                    raw = fh.read(32 * cnt[s][me])
                rows += [struct.unpack_from("<QQqQ", raw, 32 * k) for k in range(cnt[s][me])]
            with open(self.path(me, "ver"), "wb") as fh:
                fh.write(self.decide(rows))
            self.settle(2, 0, len(rows))
            verdict, bad = {}, [i for i, e in failure.items() if e.stage < 0]
            for p in range(n):
                with open(self.path(p, "ver"), "rb") as fh:
                    fh.seek(sum(cnt[s][p] for s in range(me)))
                    raw = fh.read(cnt[me][p])
                assert len(raw) == len(rec[p]), (len(raw), len(rec[p]))
                for i, v in zip(rec[p], raw):
                    verdict[i] = v
                    if v & 2:
                        bad.append(i)
            run_bad = (self.settle(3, a + min(bad) if bad else -1, 0) >> 2) - 1
            below = len(lines) if run_bad < 0 else max(0, min(len(lines), run_bad - a))
            text = b"".join(written[i] for i in range(below) if verdict.get(i, 0) & 1)
            self.out.write(text)
            self.out.flush()
            here = run_bad >= 0 and 0 <= run_bad - a < len(lines)
            v = self.settle(4, 1 if here else 0, len(text))
            if v & 3 == SPEAK:
                if not here:
                    sys.exit(1)
                die(failure[run_bad - a], (v >> 2) + run_bad - a)


def main():
    args = sys.argv[1:]
    part = os.environ.get("PAFFY_DEDUPE_PART")
    if os.environ.get("STANDIN_DEDUPE_LOG"):
        with open(os.environ["STANDIN_DEDUPE_LOG"], "a") as fh:
            fh.write(f"{os.environ.get('PAFFY_RANK', '')}/{os.environ.get('PAFFY_WORLD', '')} {part or '-'} {' '.join(args)}\n")
    inv, inp, out = options(args)
    if part:
        Part(inv, inp, out).run()
    else:
        plain(inv, inp, out)


if __name__ == "__main__":
    main()

"""CPU stand-in for shard.GpuDedupeWorker in the gloo tests of dedupe in parts (tests/test_dedupe_parts_host.py): the same interface --
reset, count_records, keys, decide, verdicts, plan, emit -- with the keys and the owner's decision restated in plain Python. The CPU
oracle is asked only about single lines: whether a line parses (and with which failure), whether its coordinates pass paf_check, and
what its written form is. The exchange code under test (shard.dedupe_sharded and everything it calls) is what the GPU ranks run.

A key here is 128 bits of BLAKE2 over (query name, target name, strand, four coordinates), not the device's hash: the contract only asks
that equal records have equal keys and that the owner is shard.dedupe_owner of the class key. Test infrastructure only."""
import hashlib
from types import SimpleNamespace

import torch

import oracle_lib as O
from paffy_amd import shard

MASK = (1 << 64) - 1


def signed(x):
    return x - (1 << 64) if x >= (1 << 63) else x


def key128(qn, tn, strand, qs, qe, ts, te):
    d = hashlib.blake2b(b"\0".join([qn, tn, strand] + [b"%d" % int(x) for x in (qs, qe, ts, te)]), digest_size=16).digest()
    return int.from_bytes(d[:8], "little"), int.from_bytes(d[8:], "little")


class StandinDedupeWorker:
    def __init__(self):
        self.memory = {}  # class key -> orientation bit of the record written for it

    def reset(self):
        self.memory = {}

    @staticmethod
    def _lines(batch):
        buf, n = batch
        data = bytes(buf[:n].numpy().tobytes())
        lines = data.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        return [ln + b"\n" for ln in lines]

    def count_records(self, batch):
        return len(self._lines(batch))

    def keys(self, batch, check_inverse, rec_base, n_parts):
        lines = self._lines(batch)
        self.rec_base, self.written, self.failure, self.entry_rec = rec_base, [], {}, []
        segments = [[] for _ in range(n_parts)]
        for i, ln in enumerate(lines):
            out, err = O.dedupe(ln)  # one line, no -a: it is written unless it does not parse
            self.written.append(out)
            if err.code:
                self.failure[i] = (err.code, err.stage, err.aux)
                continue
            f = ln.rstrip(b"\n").split(b"\t")
            own = key128(f[0], f[5], f[4], f[2], f[3], f[7], f[8])
            swap = key128(f[5], f[0], f[4], f[7], f[8], f[2], f[3])
            cls = min(own, swap) if check_inverse else own
            chk = O.dedupe(ln, True)[1]  # alone with -a: its own key is not found, so paf_check runs
            flags = (1 if cls == own else 0) | (2 if chk.code else 0)
            if chk.code:
                self.failure[i] = (chk.code, chk.stage, chk.aux)
            segments[shard.dedupe_owner(cls[0], cls[1], n_parts)].append((i, [signed(cls[0]), signed(cls[1]), rec_base + i, flags]))
        rows = []
        for seg in segments:  # the order inside a segment is free: backwards here
            for i, row in reversed(seg):
                self.entry_rec.append(i)
                rows.append(row)
        self.parse_bad = min([i for i, (c, s, a) in self.failure.items() if s < 0], default=None)
        return torch.tensor(rows, dtype=torch.int64).reshape(-1, 4), [len(s) for s in segments], len(lines)

    def decide(self, entries, check_inverse):
        rows = entries.reshape(-1, 4).tolist()
        order = sorted(range(len(rows)), key=lambda j: (rows[j][0] & MASK, rows[j][1] & MASK, rows[j][2]))
        verdict, head, new = [0] * len(rows), None, {}
        for j in order:
            cls, bit = (rows[j][0], rows[j][1]), rows[j][3] & 1
            if head is None or head[0] != cls:
                head = (cls, bit, cls not in self.memory)  # class, the head's orientation, whether the head is written
                is_head = True
            else:
                is_head = False
            if cls in self.memory:
                found = self.memory[cls] == bit
            else:
                found = (not is_head) and head[1] == bit
            if is_head and head[2]:
                verdict[j] |= 1
                new[cls] = bit
            if check_inverse and not found and rows[j][3] & 2:
                verdict[j] |= 2
        self.memory.update(new)
        return torch.tensor(verdict, dtype=torch.uint8)

    def verdicts(self, v):
        self.verdict = {}
        bad = [] if self.parse_bad is None else [self.parse_bad]
        for i, x in zip(self.entry_rec, v.tolist()):
            self.verdict[i] = x
            if x & 2:
                bad.append(i)
        return self.rec_base + min(bad) if bad else -1

    def plan(self, first_bad_global):
        n_below = len(self.written) if first_bad_global < 0 else max(0, min(len(self.written), first_bad_global - self.rec_base))
        self.out = b"".join(self.written[i] for i in range(n_below) if self.verdict.get(i, 0) & 1)
        err = SimpleNamespace(code=0, stage=0, record=0, aux=0)
        r = first_bad_global - self.rec_base
        if first_bad_global >= 0 and 0 <= r < len(self.written):
            code, stage, aux = self.failure[r]
            err = SimpleNamespace(code=code, stage=stage, record=first_bad_global, aux=aux)
        self.info = SimpleNamespace(error=err, out_bytes=len(self.out), n_rows=self.out.count(b"\n"))
        return self.info

    def emit(self):
        return torch.frombuffer(bytearray(self.out), dtype=torch.uint8) if self.out else torch.zeros(0, dtype=torch.uint8)

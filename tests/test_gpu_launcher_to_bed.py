"""`PAFFY_GPUS=N bin/paffy to_bed` with the real worker (bin/paffy_gpu in its to_bed-part mode) on one GPU (PAFFY_ONE_DEVICE=1): the bytes,
the stderr text and the status of the run with PAFFY_GPUS unset, which in turn writes what the oracle writes. That the command really was
sharded is shown by the logging wrapper of tests/test_gpu_launcher_chain.py in PAFFY_WORKER's place. The launcher's own logic is covered
without a GPU in tests/test_launcher_to_bed.py, whose record generator and failing lines are used here."""
import os
import random
import subprocess

import pytest

import oracle_lib as O
import synth_lib
from paffy_amd import shard
from test_gpu_to_bed import OPTS
from test_launcher_to_bed import LENGTH, block_names, first_appearance, records, unparsable, walk_fails

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
FLAG = {"binary": "-b", "exclude_unaligned": "-e", "exclude_aligned": "-f", "include_inverted": "-n"}


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def args_of(kw):
    return [a for k, v in kw.items() for a in ([FLAG[k]] if k in FLAG else ["-m", str(v)])]


def deal(data, n, inv):
    """{name: part}: the launcher's rule (bytes of the lines that count on a name; heaviest name to the lightest worker) restated"""
    weights, names = {}, {}
    for ln in data.splitlines(keepends=True):
        f = ln.rstrip(b"\n").split(b"\t")
        for name in [f[0]] + ([f[5]] if inv and len(f) >= 6 else []):
            h = shard.name_hash(name)
            names[name] = h
            weights[h] = weights.get(h, 0) + len(ln)
    owner = shard.contig_partition(weights, n)
    return {name: owner[h] for name, h in names.items()}


class Runner:
    """bin/paffy to_bed with the logging wrapper as its worker, spools under a directory of its own"""

    def __init__(self, tmp):
        self.tmp, self.log, self.spool = tmp, tmp / "workers.log", tmp / "spool"
        self.spool.mkdir()
        self.wrapper = tmp / "worker.sh"
        self.wrapper.write_text(f'#!/bin/sh\necho "$PAFFY_RANK/$PAFFY_WORLD" >> "{self.log}"\nexec "{os.path.join(ROOT, "bin", "paffy_gpu")}" "$@"\n')
        self.wrapper.chmod(0o755)

    def __call__(self, args, gpus, data=None, **extra):
        assert gpus <= 5
        env = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_BED_PART", "PAFFY_BED_FDS", "PAFFY_CHUNK_MB")}
        env.update(PAFFY_WORKER=str(self.wrapper), PAFFY_TMPDIR=str(self.spool), **extra)
        if gpus > 1:
            env.update(PAFFY_GPUS=str(gpus), PAFFY_ONE_DEVICE="1")
        if self.log.exists():
            self.log.unlink()
        p = subprocess.run([PAFFY, "to_bed"] + args, input=data, env=env, capture_output=True, timeout=120)
        self.workers = sorted(self.log.read_text().split()) if self.log.exists() else []
        assert os.listdir(self.spool) == []  # nothing is left of the spools, however the run ended
        return p

    def sharded(self, args, n, data=None, started=None, **extra):
        """the run over n workers; the log proves that `started` (default n) workers ran, each told the world is n"""
        p = self(args, n, data, **extra)
        assert self.workers == sorted(f"{r}/{n}" for r in range(n if started is None else started)), self.workers
        return p

    def one(self, args, data=None, **extra):
        p = self(args, 1, data, **extra)
        assert self.workers == ["/"]  # one worker, no rank, no world
        return p


@pytest.fixture
def paffy(tmp_path):
    return Runner(tmp_path)


@pytest.fixture(scope="module")
def piles(tmp_path_factory):
    """the synthetic piles of tests/test_gpu_to_bed_parts.py; per option set what one worker writes, which is what the oracle writes"""
    data = synth_lib.Synth4(0x5EED0004, 512, n_contigs=5, tlen_min=1_500_000, tlen_span=1_000_000).records(0, 3000)
    one = Runner(tmp_path_factory.mktemp("one"))
    wants = []
    for kw in OPTS:
        want, err = O.to_bed(data, **kw)
        p = one.one(args_of(kw), data)
        assert err.code == 0 and p.returncode == 0 and p.stdout == want, p.stderr[-2000:]
        wants.append(want)
    return data, wants


@pytest.mark.parametrize("k", range(len(OPTS)))
@pytest.mark.parametrize("n", [2, 3, 5])
def test_piles_over_workers_equal_one_worker_and_the_oracle(paffy, tmp_path, piles, n, k):
    data, wants = piles
    inv = bool(OPTS[k].get("include_inverted"))
    started = min(n, len(set(deal(data, n, inv).values())))
    src, dst = tmp_path / "in.paf", tmp_path / "out.bed"
    src.write_bytes(data)
    p = paffy.sharded(args_of(OPTS[k]) + ["-i", str(src), "-o", str(dst)], n, started=started)
    assert p.returncode == 0, p.stderr[-2000:]
    assert dst.read_bytes() == wants[k] and p.stdout == b""


def test_several_batches_per_worker(paffy, human_chimp, tmp_path):
    """PAFFY_CHUNK_MB=1: the fixture (one query name, a little over 1 MiB) three times under three query names gives every one of three
    workers a part of two batches, each with its slice of the record numbers and the side masks"""
    assert (1 << 20) < len(human_chimp) < (2 << 20)
    lines = []
    for suffix in (b"", b"_b", b"_c"):
        for ln in human_chimp.splitlines(keepends=True):
            q, rest = ln.split(b"\t", 1)
            lines.append(q + suffix + b"\t" + rest)
    random.Random(5).shuffle(lines)
    data = b"".join(lines)
    assert len({ln.split(b"\t", 1)[0] for ln in lines}) == 3
    src = tmp_path / "in.paf"
    src.write_bytes(data)
    one = paffy.one(["-i", str(src)], PAFFY_CHUNK_MB="1")
    assert one.returncode == 0 and one.stdout == O.to_bed(data)[0]
    p = paffy.sharded(["-i", str(src)], 3, PAFFY_CHUNK_MB="1")
    assert p.returncode == 0 and p.stdout == one.stdout, p.stderr[-2000:]


@pytest.fixture(scope="module")
def shuffled():
    lines = records(300)
    return lines, b"".join(lines)


def test_roles_and_block_order_with_inverted(paffy, shuffled):
    """sequences that are a query here and a target there, lines whose names have one owner and two, a first appearance as a target side,
    stdin without its last newline: one block per sequence, in the whole input's order of first appearance"""
    lines, data = shuffled
    want = O.to_bed(data, include_inverted=True)[0]
    part_of = deal(data, 3, True)
    pairs = {(part_of[ln.split(b"\t")[0]] == part_of[ln.split(b"\t")[5]]) for ln in lines}
    assert pairs == {True, False}
    one = paffy.one(["-n"], data[:-1])
    assert one.returncode == 0 and one.stdout == want
    for n in (3, 5):
        p = paffy.sharded(["--includeInverted"], n, data[:-1])
        assert p.returncode == 0 and p.stdout == want, p.stderr[-2000:]
    order = block_names(want)
    assert order == first_appearance(lines, True) and len(set(order)) == 10 and order[1] == lines[0].split(b"\t")[5]
    owners = [part_of[name] for name in order]
    assert any(owners[i] != owners[i + 1] and owners[i] in owners[i + 2:] for i in range(len(owners) - 2))  # interleaved across parts
    bare = b"lonely\t500\t4\t4\t+\tt0\t%d\t5\t5\t0\t0\t60\n" % LENGTH["t0"]  # a block without bytes under -e
    edge = b"".join(lines[:20] + [bare] + lines[20:60])
    want = O.to_bed(edge, include_inverted=True, exclude_unaligned=True)[0]
    p = paffy.sharded(["-n", "-e"], 3, edge)
    assert p.returncode == 0 and p.stdout == want and b"lonely" not in want
    few = b"".join(records(50, seed=2, queries=["q0"], targets=["t0"]))  # two names for five workers
    p = paffy.sharded(["-n"], 5, few, started=2)
    assert p.returncode == 0 and p.stdout == O.to_bed(few, include_inverted=True)[0]


def test_the_tail_of_sequences_without_alignments(paffy, shuffled, tmp_path):
    lines, data = shuffled
    fasta = [("q3", 50), ("never seen", 90), ("t1", 130), ("q1", 61), ("nobody", 1), ("t2", 60)]
    fa = tmp_path / "seqs.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (h.encode(), b"\n".join(b"ACGTN" * 12 for _ in range(n // 60)) + b"\n" + b"A" * (n % 60)) for h, n in fasta))
    for inv in (False, True):
        args = ["-f", "-q", str(fa)] + (["-n"] if inv else [])
        named = set(first_appearance(lines, inv))
        tail = b"".join(b"%s 0 %d\t0\n" % (h.encode(), n) for h, n in fasta if h.encode() not in named)
        want = O.to_bed(data, exclude_aligned=True, include_inverted=inv)[0] + tail
        one = paffy.one(args, data)
        assert one.returncode == 0 and one.stdout == want, one.stderr[-2000:]
        for n in (3, 5):
            p = paffy.sharded(args, n, data)
            assert p.returncode == 0 and p.stdout == want, p.stderr[-2000:]
    for args, kw in ((["-f", "-q", str(tmp_path / "missing.fa")], dict(exclude_aligned=True)), (["-q", str(fa)], {})):
        p = paffy.sharded(args, 3, data)  # a file that cannot be opened adds nothing; without -f there is no tail
        assert p.returncode == 0 and p.stdout == O.to_bed(data, **kw)[0], p.stderr[-2000:]
    empty = paffy.one(["-f", "-q", str(fa)], b"")
    p = paffy(["-f", "-q", str(fa)], 3, b"")  # no line: one plain worker lists every record
    assert paffy.workers == ["/"] and (p.returncode, p.stdout) == (empty.returncode, empty.stdout) and p.stdout.count(b"\n") == len(fasta)


@pytest.mark.parametrize("kinds", ["parse,query", "query,parse", "target,target", "query,target", "target,parse"])
@pytest.mark.parametrize("first", [40, 47])
def test_failures_equal_the_one_worker_run(paffy, shuffled, kinds, first):
    """failing lines in two different parts of three: stdout, the text on stderr and the status are one worker's"""
    lines, data = shuffled
    part_of = deal(data, 3, True)
    make = {"parse": unparsable, "query": lambda ln: walk_fails(ln, 0), "target": lambda ln: walk_fails(ln, 1)}
    column = {"parse": 0, "query": 0, "target": 5}  # the name whose owner finds the failure
    k1, k2 = kinds.split(",")
    name_of = lambda g, kind: lines[g].split(b"\t")[column[kind]]  # noqa: E731
    second = next(g for g in range(first + 30, len(lines)) if part_of[name_of(g, k2)] != part_of[name_of(first, k1)])
    bad = list(lines)
    bad[first], bad[second] = make[k1](lines[first]), make[k2](lines[second])
    bad = b"".join(bad)
    now = deal(bad, 3, True)
    assert now[name_of(first, k1)] != now[name_of(second, k2)]
    one = paffy.one(["-n"], bad)
    assert one.returncode != 0 and one.stdout == b"" and one.stderr != b""
    p = paffy.sharded(["-n"], 3, bad)
    assert (p.returncode, p.stdout, p.stderr) == (one.returncode, one.stdout, one.stderr)

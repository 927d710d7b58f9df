"""`PAFFY_GPUS=N bin/paffy view` with the real worker (bin/paffy_gpu) on one GPU (PAFFY_ONE_DEVICE=1): stdout, the end of stderr and the
status of the run with PAFFY_GPUS unset, which in turn writes the oracle's text. That the command really was sharded is shown by the
wrapper of tests/test_gpu_launcher_chain.py in PAFFY_WORKER's place: a shell script that notes $PAFFY_RANK/$PAFFY_WORLD and then replaces
itself by bin/paffy_gpu (a shell has not touched a GPU). The launcher's own logic is covered without a GPU in tests/test_launcher_view.py."""
import os
import subprocess

import pytest

import oracle_lib as O
import synth_lib
from paffy_amd import shard
from test_gpu_flat import cigar_of, record
from test_gpu_view_text import oracle_text, total_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
ASSERTION = b"paffy view: Assertion failed (average identity or aligned bases below the requested minimum)\n"


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


class Runner:
    """bin/paffy view with the logging wrapper as its worker, spools under a directory of its own"""

    def __init__(self, tmp):
        self.tmp, self.log, self.spool = tmp, tmp / "workers.log", tmp / "spool"
        self.spool.mkdir()
        self.wrapper = tmp / "worker.sh"
        self.wrapper.write_text(f'#!/bin/sh\necho "$PAFFY_RANK/$PAFFY_WORLD" >> "{self.log}"\nexec "{os.path.join(ROOT, "bin", "paffy_gpu")}" "$@"\n')
        self.wrapper.chmod(0o755)

    def __call__(self, args, gpus, data=None):
        assert gpus <= 5  # at most six processes with the GPU open
        env = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_RANGE", "PAFFY_VIEW_SUMS", "PAFFY_CHUNK_MB")}
        env.update(PAFFY_WORKER=str(self.wrapper), PAFFY_TMPDIR=str(self.spool))
        if gpus > 1:
            env.update(PAFFY_GPUS=str(gpus), PAFFY_ONE_DEVICE="1")
        if self.log.exists():
            self.log.unlink()
        p = subprocess.run([PAFFY, "view"] + args, input=data, env=env, capture_output=True, timeout=120)
        self.workers = sorted(self.log.read_text().split()) if self.log.exists() else []
        assert os.listdir(self.spool) == []  # nothing is left of the spools, however the run ended
        return p

    def same(self, args, want, data=None, ns=(2, 3, 5)):
        """one worker gives `want` = (status, stdout, the end of stderr); n workers -- the log shows n of them -- give the same"""
        one = self(args, 1, data)
        assert self.workers == ["/"]  # one worker, no rank, no world
        assert (one.returncode, one.stdout) == want[:2], (one.returncode, one.stderr[-1000:])
        assert one.stderr.endswith(want[2]), one.stderr[-1000:]
        for n in ns:
            p = self(args, n, data)
            assert self.workers == sorted(f"{r}/{n}" for r in range(n)), (n, self.workers)
            assert (p.returncode, p.stdout) == want[:2], (n, p.returncode, p.stderr[-1000:])
            assert p.stderr[-200:] == one.stderr[-200:], (n, p.stderr[-1000:])


@pytest.fixture
def paffy(tmp_path):
    return Runner(tmp_path)


_CASE = {}


def case():
    """300 cfg4-style records on their genomes: (data, seqs, the encoded lines, the oracle's stats lines, its blocks, its sums)"""
    if not _CASE:
        host = synth_lib.Synth4(0x5EED0004, 2048, n_contigs=6, tlen_min=200_000, tlen_span=200_000)
        data, seqs = host.records(0, 300), host.genomes()
        enc, err = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs)
        assert err.code == 0
        enc = enc.splitlines(keepends=True)
        tot = [0] * 6
        for ln in enc:
            tot = O.cigar_stats(cigar_of(ln).decode(), tot, zero=False)
        _CASE["c"] = (data, seqs, enc, oracle_text(enc), oracle_text(enc, seqs, True), tot)
    return _CASE["c"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("view")
    data, seqs = case()[:2]
    (d / "in.paf").write_bytes(data)
    with open(d / "g.fa", "wb") as fh:
        for name, s in seqs.items():
            fh.write(b">" + (name if isinstance(name, bytes) else name.encode()) + b"\n" + s + b"\n")
    return str(d / "in.paf"), str(d / "g.fa")


@pytest.mark.parametrize("flags", [("-s",), ("-a", "-s"), ("-s", "-t")], ids=["s", "a_s", "s_t"])
def test_n_workers_write_what_one_writes(paffy, files, flags):
    paf, fa = files
    data, seqs, enc, lines, blocks, tot = case()
    want = (b"" if "-t" in flags else b"".join(blocks if "-a" in flags else lines)) + total_line(300, tot)
    paffy.same(list(flags) + ["-i", paf, fa], (0, want, b""))


def test_the_closing_assert_runs_on_the_sums_of_all_workers(paffy, files):
    paf, fa = files
    data, seqs, enc, lines, blocks, tot = case()
    text = b"".join(lines) + total_line(300, tot)
    identity = tot[0] / (tot[0] + tot[1])
    paffy.same(["-s", "-u", "%.6f" % (identity + 0.001), "-i", paf, fa], (-6, text, ASSERTION))  # above the true identity: abort
    paffy.same(["-s", "-u", "%.6f" % (identity - 0.001), "-v", str(tot[0] + tot[1]), "-i", paf, fa], (0, text, b""), ns=(3,))


def test_stdin_and_two_lines_for_five_workers(paffy, files):
    paf, fa = files
    data, seqs, enc, lines, blocks, tot = case()
    paffy.same(["-s", fa], (0, b"".join(lines) + total_line(300, tot), b""), data=data)
    two = b"".join(data.splitlines(keepends=True)[:2])
    t2 = [0] * 6
    for ln in enc[:2]:
        t2 = O.cigar_stats(cigar_of(ln).decode(), t2, zero=False)
    paffy.same(["-a", "-s", fa], (0, b"".join(blocks[:2]) + total_line(2, t2), b""), data=two, ns=(5,))


def test_a_failing_record_in_the_second_workers_range(paffy, files, tmp_path):
    """each worker reads its range as one chunk, and a chunk with a failing record writes nothing: what is out is the first worker's text,
    and the record is counted from the failing worker's first record, as under every stream command of the launcher. One worker, whose one
    chunk is the whole input, writes nothing and counts from the input's first record (tests/test_gpu_view_cli_stream.py), so stdout and
    the record number are the oracle's for the launcher's cut (shard.stream_cuts restates it); the status and the message are one worker's"""
    paf, fa = files
    data, seqs, enc, lines, blocks, tot = case()
    recs = data.splitlines(keepends=True)
    for n in (2, 3, 5):
        c = shard.stream_cuts(data, n)
        at = data[:(c[1] + c[2]) // 2].count(b"\n")  # a record in the middle of the second range
        lost = b"\t".join([b"nobody"] + recs[at].split(b"\t")[1:])
        text = b"".join(recs[:at]) + lost + b"".join(recs[at:])
        broken = tmp_path / ("broken%d.paf" % n)
        broken.write_bytes(text)
        cuts = shard.stream_cuts(text, n)
        held = text[:cuts[1]].count(b"\n")
        assert 0 < held <= at < text[:cuts[2]].count(b"\n")
        one = paffy(["-s", "-i", str(broken), fa], 1)
        assert (one.returncode, one.stdout, one.stderr) == (1, b"", b"No query sequence found for record %d\n" % at)
        p = paffy(["-s", "-i", str(broken), fa], n)
        assert paffy.workers == sorted(f"{r}/{n}" for r in range(n))
        assert (p.returncode, p.stdout) == (one.returncode, b"".join(lines[:held])), (n, p.returncode, p.stderr[-1000:])
        assert p.stderr == b"No query sequence found for record %d\n" % (at - held), (n, p.stderr[-1000:])


def test_a_rows_failure_in_the_last_workers_range(paffy, files, tmp_path):
    paf, fa = files
    data, seqs, enc, lines, blocks, tot = case()
    recs = data.splitlines(keepends=True)
    f = recs[0].split(b"\t")
    qname, tname = f[0].decode(), f[5].decode()
    qlen = len(seqs[qname])
    # = ops alone, the query range 50 bases past the loaded sequence (the line says more): the plan passes, the rows do not
    far = record([(100, "=")], "+", qname=qname, tname=tname, qlen=qlen + 1000, tlen=int(f[6]), qs=qlen - 50, ts=1000).encode()
    at = 290
    text = b"".join(recs[:at]) + far + b"".join(recs[at:])
    spoiled = tmp_path / "spoiled.paf"
    spoiled.write_bytes(text)
    want = b"".join(blocks[:at]) + oracle_text([far])[0]  # every block in front of the record and its stats line
    one = paffy(["-a", "-s", "-i", str(spoiled), fa], 1)
    assert (one.returncode, one.stdout, one.stderr) == (-11, want, b"alignment reaches outside a sequence (record %d)\n" % at)
    for n in (2, 3, 5):
        base = text[:shard.stream_cuts(text, n)[n - 1]].count(b"\n")  # the last worker's first record
        assert base <= at
        p = paffy(["-a", "-s", "-i", str(spoiled), fa], n)
        assert paffy.workers == sorted(f"{r}/{n}" for r in range(n))
        assert (p.returncode, p.stdout) == (one.returncode, one.stdout), (n, p.returncode, p.stderr[-1000:])
        assert p.stderr == b"alignment reaches outside a sequence (record %d)\n" % (at - base), (n, p.stderr[-1000:])

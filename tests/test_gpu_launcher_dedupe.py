"""`PAFFY_GPUS=N bin/paffy dedupe [-a]` with the real worker (bin/paffy_gpu in its dedupe-part mode) on one GPU (PAFFY_ONE_DEVICE=1), N = 2, 3
and 5: the bytes, the stderr text and the status of the run with PAFFY_GPUS unset, which in turn writes what the oracle writes. That the
command really was sharded is shown by a wrapper in PAFFY_WORKER's place: a three-line shell script that notes $PAFFY_RANK/$PAFFY_WORLD and
then replaces itself by bin/paffy_gpu (a shell has not touched a GPU; the inherited pipe descriptors survive). The launcher's own logic --
dead workers, what does not shard -- is covered without a GPU in tests/test_launcher_dedupe.py, whose helpers restate the cut."""
import os
import random
import subprocess

import pytest

import dedupe_streams as S
import oracle_lib as O
from test_launcher_dedupe import cuts, fixed, rounds_of, share_of_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


class Runner:
    """bin/paffy with the logging wrapper as its worker, spools under a directory of its own"""

    def __init__(self, tmp):
        self.tmp, self.log, self.spool = tmp, tmp / "workers.log", tmp / "spool"
        self.spool.mkdir()
        self.wrapper = tmp / "worker.sh"
        self.wrapper.write_text(f'#!/bin/sh\necho "$PAFFY_RANK/$PAFFY_WORLD" >> "{self.log}"\nexec "{os.path.join(ROOT, "bin", "paffy_gpu")}" "$@"\n')
        self.wrapper.chmod(0o755)

    def __call__(self, args, gpus, data=None, share=None):
        assert gpus <= 5  # never more than five workers with the GPU open
        env = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_CHUNK_MB") and not k.startswith("PAFFY_DEDUPE")}
        env.update(PAFFY_WORKER=str(self.wrapper), PAFFY_TMPDIR=str(self.spool))
        if gpus > 1:
            env.update(PAFFY_GPUS=str(gpus), PAFFY_ONE_DEVICE="1")
            if share:
                env["PAFFY_DEDUPE_SHARE_BYTES"] = str(share)
        if self.log.exists():
            self.log.unlink()
        p = subprocess.run([PAFFY, "dedupe"] + args, input=data, env=env, capture_output=True, timeout=120)
        self.workers = sorted(self.log.read_text().split()) if self.log.exists() else []
        assert os.listdir(self.spool) == []  # nothing is left of the spools, however the run ended
        return p

    def sharded(self, args, n, data=None, share=None):
        """the run over n workers; the log proves that n workers ran, each told the world is n"""
        p = self(args, n, data, share)
        assert self.workers == sorted(f"{r}/{n}" for r in range(n)), self.workers
        return p

    def one(self, args, data=None):
        p = self(args, 1, data)
        assert self.workers == ["/"]  # one worker, no rank, no world
        return p


@pytest.fixture
def paffy(tmp_path):
    return Runner(tmp_path)


def same(p, q):
    assert (p.returncode, p.stdout, p.stderr) == (q.returncode, q.stdout, q.stderr), (p.returncode, q.returncode, p.stderr[-500:], q.stderr[-500:])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """300 records from a pool of 60; what one worker writes for them with and without -a is what the oracle writes (computed once)"""
    lines = S.stream(random.Random(300), 300)
    data, one = b"".join(lines), {}
    run = Runner(tmp_path_factory.mktemp("one"))
    for flags in ((), ("-a",)):
        want, err = O.dedupe(data, bool(flags))
        p = run.one(list(flags), data)
        assert err.code == 0 and (p.returncode, p.stdout, p.stderr) == (0, want, b"") and 0 < want.count(b"\n") < 300
        one[flags] = p
    return data, one


@pytest.mark.parametrize("n", [2, 3, 5])
def test_plain_runs(paffy, plain, n):
    data, one = plain
    share = len(data) // (6 * n)
    assert rounds_of(len(data), share, n) >= 6
    for flags in ((), ("-a",)):
        same(paffy.sharded(list(flags), n, data, share), one[flags])


def test_the_ordering_trap(paffy):
    """one input with both arrangements: an exact twin from worker 1's share of round 0 to worker 0's share of round 1, and a swapped twin
    from worker 0's share of round 0 to worker 1's share of round 1: the first copy in input order is the one written"""
    lines = [fixed(i) for i in range(12)]
    share = len(lines[0]) * 2
    where = share_of_line(lines, share)
    a1, a2 = where.index(1), len(where) - 1 - where[::-1].index(2)
    b1, b2 = where.index(0), len(where) - 1 - where[::-1].index(3)
    lines[a2], lines[b2] = lines[a1], S.swapped(lines[b1])
    assert share_of_line(lines, share) == where and len({a1, a2, b1, b2}) == 4
    data = b"".join(lines)
    for flags, dropped in (([], {a2}), (["-a"], {a2, b2})):
        want = O.dedupe(data, bool(flags))[0]
        assert want == b"".join(O.dedupe(ln)[0] for k, ln in enumerate(lines) if k not in dropped)
        p = paffy.sharded(flags, 2, data, share)
        assert (p.returncode, p.stdout, p.stderr) == (0, want, b"")
        same(p, paffy.one(flags, data))


def test_odd_inputs(paffy, tmp_path):
    some = S.stream(random.Random(8), 40)
    long_name = S.record(b"L" * 5000, b"t", 3, 4, 5)
    long_lines = some[:10] + [long_name] + some[10:] + [S.swapped(long_name)]
    assert len(long_name) > 3 * 1500
    for lines, share, n in ((some, 1, 3),                                   # shares of one line
                            (long_lines, 1500, 3),                           # a line longer than three shares: empty shares
                            (some[:2], 1, 5),                                # fewer lines than workers
                            (some[:30] + [some[3].rstrip(b"\n")], 200, 2)):  # an unterminated last line
        data = b"".join(lines)
        want, err = O.dedupe(data, True)
        p = paffy.sharded(["-a"], n, data, share)  # stdin -> stdout
        assert err.code == 0 and (p.returncode, p.stdout, p.stderr) == (0, want, b""), (share, n)
        same(p, paffy.one(["-a"], data))
    src, dst = tmp_path / "in.paf", tmp_path / "out.paf"
    src.write_bytes(b"".join(some))
    dst.write_bytes(b"what was here before")
    p = paffy.sharded(["-i", str(src), "-o", str(dst)], 3, share=300)
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"") and dst.read_bytes() == O.dedupe(b"".join(some))[0]


def test_a_failing_record_in_the_middle(paffy):
    """stdout is the bytes before the record; stderr, with the true global record number, and the status are the one-worker run's"""
    lines = [fixed(i % 150) for i in range(400)]
    star = fixed(900).replace(b"\t+\t", b"\t*\t")
    for bad_line, flags, n, share in ((S.bad_check(7), ["-a"], 3, 700), (star, [], 5, 1900)):
        bad = list(lines)
        bad[237] = bad_line
        data = b"".join(bad)
        one = paffy.one(flags, data)
        assert one.returncode != 0 and one.stdout == O.dedupe(b"".join(bad[:237]), bool(flags))[0] and one.stderr
        if flags:
            assert b"(record 237)" in one.stderr
        same(paffy.sharded(flags, n, data, share), one)


def test_of_two_failures_in_one_round_the_lower_record_speaks(paffy):
    n, lines = 3, [fixed(i % 150) for i in range(400)]
    share = 5 * len(lines[0])
    where = share_of_line(lines, share)
    lo, hi = where.index(2 * n + 1) + 2, where.index(2 * n + 2) + 2  # round 2: workers 1 and 2
    lines[lo], lines[hi] = S.bad_check(1), fixed(901).replace(b"\t+\t", b"\t*\t")
    where = share_of_line(lines, share)
    assert where[lo] // n == where[hi] // n == 2 and (where[lo] % n, where[hi] % n) == (1, 2) and lo < hi
    data = b"".join(lines)
    one = paffy.one(["-a"], data)
    assert one.returncode != 0 and f"(record {lo})".encode() in one.stderr and one.stdout == O.dedupe(b"".join(lines[:lo]), True)[0]
    same(paffy.sharded(["-a"], n, data, share), one)
    assert cuts(data, share)[2 * n] > 0

"""`PAFFY_GPUS=N bin/paffy chain` with the real worker (bin/paffy_gpu in its chain-part mode) on one GPU (PAFFY_ONE_DEVICE=1): the bytes, the
stderr text and the status of the run with PAFFY_GPUS unset, which in turn writes what the oracle writes with the fresh-iterator walk
switched off. That the command really was sharded is shown by a wrapper in PAFFY_WORKER's place: a three-line shell script that
notes $PAFFY_RANK/$PAFFY_WORLD and then replaces itself by bin/paffy_gpu (a shell has not touched a GPU; the inherited pipe descriptors
survive). The launcher's own logic is covered without a GPU in tests/test_launcher_chain.py."""
import os
import random
import subprocess

import pytest

import oracle_lib as O
from test_gpu_chain import collinear_set, line
from test_gpu_chain_parts import deal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
# the random set's gaps go up to 30000 and its scores to 20000: with a gap cost that does not grow with the gap the runs chain, and
# -g 20000 cuts about a third of the links (600 records: 82 chains without -g, 438 with it, 599 with the command's default costs)
OPTS = ["-g", "20000", "-d", "100", "-e", "0"]
OPTS_KW = dict(max_gap=20000, gap_open=100, gap_extend=0)


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

    def __call__(self, args, gpus, data=None, **extra):
        assert gpus <= 5
        env = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_CHAIN_PART", "PAFFY_CHAIN_FDS", "PAFFY_CHUNK_MB")}
        env.update(PAFFY_WORKER=str(self.wrapper), PAFFY_TMPDIR=str(self.spool), **extra)
        if gpus > 1:
            env.update(PAFFY_GPUS=str(gpus), PAFFY_ONE_DEVICE="1")
        if self.log.exists():
            self.log.unlink()
        p = subprocess.run([PAFFY, "chain"] + args, input=data, env=env, capture_output=True, timeout=120)
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
def random_set(tmp_path_factory):
    """about 600 records, 7 query names x 3 targets, both strands; what one worker and the oracle write for it (computed once)"""
    data = collinear_set(random.Random(1), 600, n_q=7, n_t=3, exact=0.0)
    assert b"\t+\t" in data and b"\t-\t" in data
    want, err, _ = O.chain(data, fresh_walk=False, **OPTS_KW)
    chains = lambda out: len({tag(ln, b"cn") for ln in out.splitlines()})  # noqa: E731
    unlimited = O.chain(data, fresh_walk=False, gap_open=100, gap_extend=0)[0]
    assert err.code == 0 and chains(unlimited) < chains(want) < 500  # gaps that chain, and gaps beyond -g
    p = Runner(tmp_path_factory.mktemp("one")).one(OPTS, data)
    assert p.returncode == 0 and p.stdout == want, p.stderr[-2000:]
    return data, want


def same_as_one_worker(paffy, args, data, ns, started=None, **extra):
    one = paffy.one(args, data, **extra)
    assert one.returncode == 0, one.stderr[-2000:]
    for n in ns:
        p = paffy.sharded(args, n, data, started=started, **extra)
        assert p.returncode == 0, p.stderr[-2000:]
        assert p.stdout == one.stdout, n
    return one.stdout


def tag(ln, name):
    return int(ln.split(b"\t" + name + b":i:")[1].split(b"\t")[0])


@pytest.mark.parametrize("n", [2, 3, 5])
def test_random_set_over_workers_equals_one_worker_and_the_oracle(paffy, tmp_path, random_set, n):
    data, want = random_set
    src, dst = tmp_path / "in.paf", tmp_path / "out.paf"
    src.write_bytes(data)
    p = paffy.sharded(OPTS + ["-i", str(src), "-o", str(dst)], n)
    assert p.returncode == 0, p.stderr[-2000:]
    assert dst.read_bytes() == want and p.stdout == b""


def test_chain_ends_of_different_parts_tie_on_score(paffy):
    """the input of tests/test_gpu_chain_parts.py's test of the same name: the same records under eight query names, so that every chain
    has twins in other parts with the same end score and the same processing key"""
    rng = random.Random(9)
    base = []
    for strand in "+-":
        qs = ts = 1000
        for _ in range(12):
            ln = rng.randrange(100, 900)
            base.append((qs, qs + ln, ts, ts + ln, rng.choice([300, 300, 7000]), strand))
            step = rng.choice([0, 50, 2_000_000])
            qs, ts = qs + ln + step, ts + ln + step
    rows = [line("q%d" % q, qs, qe, "t", ts, te, sc, st) for q in range(8) for qs, qe, ts, te, sc, st in base]
    rng.shuffle(rows)
    data = b"".join(rows)
    args = ["-d", "10", "-g", "100000", "-t", "0.0"]
    got = same_as_one_worker(paffy, args, data, (3,))
    assert got == O.chain(data, gap_open=10, max_gap=100000, trim=0.0, fresh_walk=False)[0]
    by_score = {}
    for ln in got.splitlines():
        by_score.setdefault((tag(ln, b"s1"), ln.split(b"\t")[4]), set()).add(tag(ln, b"cn"))
    assert max(len(v) for v in by_score.values()) >= 8


@pytest.mark.parametrize("n_chains", [14, 130])
def test_chain_numbers_change_their_digit_count_between_parts(paffy, n_chains):
    """the construction of tests/test_gpu_chain_parts.py's test of the same name: cn goes from 9 to 10 (and from 99 to 100) across parts"""
    rng = random.Random(3)
    rows = [line("q%d" % (c % 9), 10_000 * c, 10_000 * c + 500, "t%d" % c, 5, 505, rng.randrange(10, 9000), rng.choice("+-")) for c in range(n_chains)]
    rows += [line("q%d" % (c % 9), 10_000 * c + 600, 10_000 * c + 900, "t%d" % c, 610, 910, 40, "+") for c in range(0, n_chains, 3)]
    rng.shuffle(rows)
    data = b"".join(rows)
    got = same_as_one_worker(paffy, ["-d", "5", "-t", "0.0"], data, (3,))
    assert got == O.chain(data, gap_open=5, trim=0.0, fresh_walk=False)[0]
    assert max(tag(ln, b"cn") for ln in got.splitlines()) >= n_chains - 1


def test_options_reach_the_workers(paffy, random_set):
    """-g -t -d -e change cn and s1 on this input, and change them the same way over three workers"""
    data, other_opts = random_set
    args = ["--maxGapLength", "40000", "-t", "0.5", "-d50", "--chainGapExtend=0"]
    got = same_as_one_worker(paffy, args, data, (3,))
    assert got == O.chain(data, gap_open=50, gap_extend=0, max_gap=40000, trim=0.5, fresh_walk=False)[0]
    plain = paffy.one([], data).stdout
    tags = lambda out: sorted((ln.split(b"\tAS:")[0], tag(ln, b"cn"), tag(ln, b"s1")) for ln in out.splitlines())  # noqa: E731
    assert tags(got) != tags(plain) and tags(got) != tags(other_opts)
    assert [t[0] for t in tags(got)] == [t[0] for t in tags(plain)]


def test_several_batches_per_worker(paffy, human_chimp, tmp_path):
    """PAFFY_CHUNK_MB=1: the fixture (one query name, a little over 1 MiB) three times under three query names gives every one of three
    workers a part of two batches, each with its slice of the record numbers"""
    assert (1 << 20) < len(human_chimp) < (2 << 20)
    lines = []
    for suffix in (b"", b"_b", b"_c"):
        for ln in human_chimp.splitlines(keepends=True):
            q, rest = ln.split(b"\t", 1)
            lines.append(q + suffix + b"\t" + rest)
    rng = random.Random(5)
    rng.shuffle(lines)
    data = b"".join(lines)
    assert len({ln.split(b"\t", 1)[0] for ln in lines}) == 3
    src = tmp_path / "in.paf"
    src.write_bytes(data)
    got = same_as_one_worker(paffy, ["-i", str(src)], None, (3,), PAFFY_CHUNK_MB="1")
    assert got == O.chain(data, fresh_walk=False)[0]


def test_one_query_name_the_empty_input_and_no_last_newline(paffy, tmp_path):
    data = collinear_set(random.Random(21), 300, n_q=1)
    got = same_as_one_worker(paffy, [], data[:-1], (3,), started=1)  # one name: one worker of three is started; stdin without a last newline
    assert got == O.chain(data[:-1], fresh_walk=False)[0]
    empty = tmp_path / "empty.paf"
    empty.write_bytes(b"")
    same_as_one_worker(paffy, ["-i", str(empty)], None, (3,), started=0)
    one = line("q", 0, 100, "t", 0, 100, 100)[:-1]
    assert same_as_one_worker(paffy, [], one, (2,), started=1) == O.chain(one, fresh_walk=False)[0]


NAMES = ["qa", "qb", "qc", "qd", "qe", "qf"]
ROWS_OF = {q: 20 + 4 * i for i, q in enumerate(NAMES)}


def failing_input(extra):
    """the input of tests/test_gpu_chain_parts.py::test_errors_equal_the_one_context_run: the rows of six names interleaved"""
    good = lambda q, k: line(q, 1000 * k, 1000 * k + 900, "t", 1000 * k, 1000 * k + 900, 100 + k)  # noqa: E731
    return b"".join(extra.get((q, k), good(q, k)) for k in range(max(ROWS_OF.values())) for q in NAMES if k < ROWS_OF[q])


def unparsable(q, k):
    return (q + "\t10\t0\t5\t*\tt\t10\t0\t5\t5\t5\t60\n").encode()


def unchecked(q, k):
    return line(q, 1000 * k, 1000 * k + 900, "t", 1000 * k, 1000 * k + 900, 100 + k, ql=150)  # paf_check fails: the query ends beyond its length


@pytest.mark.parametrize("kinds", ["parse,parse", "check,check", "check,parse"])
@pytest.mark.parametrize("rows", [(3, 9), (9, 3)])
def test_failures_equal_the_one_worker_run(paffy, kinds, rows):
    """failing lines in two different parts of three: stdout, the text on stderr and the status are one worker's"""
    part_of = deal(failing_input({}), 3)
    p1 = [q for q in NAMES if part_of[q] == 1][0]
    p2 = [q for q in NAMES if part_of[q] != 1][0]
    make = {"parse": unparsable, "check": unchecked}
    k1, k2 = kinds.split(",")
    data = failing_input({(p1, rows[0]): make[k1](p1, rows[0]), (p2, rows[1]): make[k2](p2, rows[1])})
    now = deal(data, 3)
    assert now[p1] == 1 and now[p2] != 1
    args = ["-d", "10", "-g", "100000"]
    one = paffy.one(args, data)
    assert one.returncode != 0 and one.stdout == b"" and one.stderr != b""
    p = paffy.sharded(args, 3, data)
    assert (p.returncode, p.stdout, p.stderr) == (one.returncode, one.stdout, one.stderr)

"""`PAFFY_GPUS=N bin/paffy dedupe [-a]` (host/paffy_launch.c, run_dedupe) without a GPU: the worker is tests/standin_dedupe_cli_worker.py,
which honours the part-mode contract -- the cuts, the numbers, the exchange files, the reports and the answers -- in plain Python, so that
what is tested is the launcher's own work: N workers per run, four barriers per round, the minimum of the failing numbers, the true record
number handed to the one worker that speaks, the round's segments copied in rank order, and that nothing waits for ever on a worker that
is gone. The expected bytes are the oracle's dedupe over the whole input. tests/test_gpu_launcher_dedupe.py runs the real worker."""
import os
import random
import subprocess

import pytest

import dedupe_streams as S
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.environ.get("PAFFY_LAUNCHER") or os.path.join(ROOT, "bin", "paffy")  # the ASan + UBSan build goes here
STANDIN = os.path.join(ROOT, "tests", "standin_dedupe_cli_worker.py")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s", "../bin/paffy"])
    O.lib()


def run(args, n, data=None, tmp=None, **env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PAFFY_DEDUPE", "STANDIN_DEDUPE"))}
    env.update(PAFFY_WORKER=STANDIN, PAFFY_ONE_DEVICE="1", **{k: str(v) for k, v in env_extra.items()})
    env.pop("PAFFY_GPUS", None)
    if n:
        env["PAFFY_GPUS"] = str(n)
    if tmp:
        env["PAFFY_TMPDIR"] = str(tmp)
        env["STANDIN_DEDUPE_LOG"] = str(tmp / "log.txt")
        if (tmp / "log.txt").exists():
            (tmp / "log.txt").unlink()
    return subprocess.run([PAFFY] + args, input=data, env=env, capture_output=True, timeout=60)


def log_of(tmp):
    p = tmp / "log.txt"
    return p.read_text().splitlines() if p.exists() else []


def parts_started(tmp, n):
    """n workers, ranks 0 .. n - 1 of n, each told its part"""
    log = log_of(tmp)
    return sorted(l.split()[0] for l in log) == sorted(f"{r}/{n}" for r in range(n)) and all(l.split()[1].endswith("/" + l.split("/")[0]) for l in log)


def no_spool(tmp):
    return [f for f in os.listdir(tmp) if f.startswith("paffy.")] == []


def cuts(data, share):
    """the launcher's rule: cut(j) = the first line end at or after j * share, cut(0) = 0, the last cut the size"""
    out, j = [0], 1
    while out[-1] < len(data) or j * share < len(data):
        nl = data.find(b"\n", j * share) if j * share < len(data) else -1
        out.append(nl + 1 if nl >= 0 else len(data))
        j += 1
    return out


def share_of_line(lines, share):
    """the share every line lies in"""
    c, at, where = cuts(b"".join(lines), share), 0, []
    for ln in lines:
        where.append(max(j for j in range(len(c) - 1) if c[j] <= at))
        at += len(ln)
    return where


def rounds_of(size, share, n):
    return -(-(-(-size // share)) // n)


def fixed(i, strand=b"+"):
    """lines of one length, all different"""
    return S.record(b"q%03d" % (i % 1000), b"t%03d" % (i % 7), 100 + i % 800, 1000 + i % 800, 10 + i % 80, strand)


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_plain_runs(tmp_path, n):
    """600 records from a pool of 60, at least 6 rounds, with and without -a: the bytes of the oracle, n workers started"""
    lines = S.stream(random.Random(600 + n), 600)
    data = b"".join(lines)
    share = len(data) // (6 * n)
    assert rounds_of(len(data), share, n) >= 6
    for flags in ([], ["-a"]):
        want, err = O.dedupe(data, bool(flags))
        assert err.code == 0 and 0 < want.count(b"\n") < 600
        p = run(["dedupe"] + flags, n, data=data, tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=share)
        assert (p.returncode, p.stderr) == (0, b"")
        assert p.stdout == want
        assert parts_started(tmp_path, n) and no_spool(tmp_path)
        one = run(["dedupe"] + flags, 0, data=data)
        assert (one.returncode, one.stdout, one.stderr) == (0, want, b"")


def test_the_ordering_trap(tmp_path):
    """a twin whose first copy lies in worker 1's share of round 0 and whose second lies in worker 0's share of round 1: the first copy in
    input order is the one written, though worker 0 holds the other. And the reverse: worker 0 of round 0, worker 1 of round 1."""
    n, base = 2, [fixed(i) for i in range(12)]
    share = len(base[0]) * 2
    where = share_of_line(base, share)
    assert sorted(set(where)) == list(range(max(where) + 1)) and max(where) >= 3
    for first_share, second_share in ((1, 2), (0, 3)):
        first, second = where.index(first_share), len(where) - 1 - where[::-1].index(second_share)
        assert first < second
        for twin, flags in ((base[first], []), (S.swapped(base[first]), ["-a"])):
            lines = list(base)
            lines[second] = twin
            assert len(twin) == len(base[second]) and share_of_line(lines, share) == where
            data = b"".join(lines)
            want = O.dedupe(data, bool(flags))[0]
            assert want == b"".join(O.dedupe(ln)[0] for k, ln in enumerate(lines) if k != second)
            p = run(["dedupe"] + flags, n, data=data, tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=share)
            assert (p.returncode, p.stdout, p.stderr) == (0, want, b"")
            assert parts_started(tmp_path, n)


def test_odd_inputs(tmp_path):
    some = S.stream(random.Random(8), 40)
    long_name = S.record(b"L" * 5000, b"t", 3, 4, 5)
    cases = [
        (some, 1, 3),                                                          # shares of one line
        (some[:10] + [long_name] + some[10:] + [long_name], 1500, 3),          # a line longer than three shares: empty shares
        (some[:2], 1, 5), (some[:2], 1 << 20, 5), (some[:1], 7, 8),            # fewer lines than workers
        (some[:30] + [some[3].rstrip(b"\n")], 200, 4),                         # an unterminated last line
        (some[:30] + [long_name.rstrip(b"\n")], 64, 2),
    ]
    for lines, share, n in cases:
        data = b"".join(lines)
        for flags in ([], ["-a"]):
            want, err = O.dedupe(data, bool(flags))
            assert err.code == 0
            p = run(["dedupe"] + flags, n, data=data, tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=share)  # stdin -> stdout
            assert (p.returncode, p.stdout, p.stderr) == (0, want, b""), (share, n, flags)
            assert parts_started(tmp_path, n) and no_spool(tmp_path)
    assert max(len(c) for c in cases[1][0]) > 3 * 1500
    # -i and -o; without the knob one share of PAFFY_CHUNK_MB holds everything: one round
    data = b"".join(some)
    src, dst = tmp_path / "in.paf", tmp_path / "out.paf"
    src.write_bytes(data)
    dst.write_bytes(b"what was here before")
    for extra in ({"PAFFY_DEDUPE_SHARE_BYTES": 300}, {}):
        p = run(["dedupe", "-a", "-i", str(src), "--outputFile", str(dst)], 3, tmp=tmp_path, **extra)
        assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"")
        assert dst.read_bytes() == O.dedupe(data, True)[0]
        assert parts_started(tmp_path, 3) and no_spool(tmp_path)
    p = run(["dedupe", "-i", str(src), "-o", str(tmp_path / "no" / "such" / "out.paf")], 3, tmp=tmp_path)
    assert p.returncode == 1 and p.stderr.decode() == f"paffy dedupe: cannot open {tmp_path / 'no' / 'such' / 'out.paf'}\n" and log_of(tmp_path) == []


def bad_check_like(line):
    """the line with a query length of 0001: it parses, paf_check fails; the same bytes long"""
    f = line.split(b"\t")
    assert f[1] == b"1000"
    f[1] = b"0001"
    return b"\t".join(f)


def bad_strand_like(line):
    f = line.split(b"\t")
    f[4] = b"*"
    return b"\t".join(f)


def test_a_failing_record_in_the_middle(tmp_path):
    """stdout is the bytes before the record; stderr and status are the one-stand-in run's, with the true global record number"""
    lines = [fixed(i % 150) for i in range(400)]
    for n, share in ((3, 700), (5, 1)):
        for make, flags in ((bad_check_like, ["-a"]), (bad_strand_like, ["-a"]), (bad_strand_like, [])):
            bad = list(lines)
            bad[237] = make(fixed(900))
            data = b"".join(bad)
            one = run(["dedupe"] + flags, 0, data=data)
            assert one.returncode != 0 and one.stdout == O.dedupe(b"".join(bad[:237]), bool(flags))[0]
            assert one.stderr.decode().endswith("in record 237\n") and one.stderr.count(b"\n") == 1
            p = run(["dedupe"] + flags, n, data=data, tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=share)
            assert (p.returncode, p.stdout, p.stderr) == (one.returncode, one.stdout, one.stderr)
            assert parts_started(tmp_path, n) and no_spool(tmp_path)
    # without -a the record that fails paf_check is written like any other
    bad = list(lines)
    bad[237] = bad_check_like(fixed(900))
    p = run(["dedupe"], 3, data=b"".join(bad), tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=700)
    assert (p.returncode, p.stderr) == (0, b"") and p.stdout == O.dedupe(b"".join(bad))[0]
    # -o: the file holds the bytes before the record
    dst = tmp_path / "out.paf"
    bad[237] = bad_strand_like(fixed(900))
    p = run(["dedupe", "-o", str(dst)], 3, data=b"".join(bad), tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=700)
    assert p.returncode != 0 and dst.read_bytes() == O.dedupe(b"".join(bad[:237]))[0] and p.stderr.decode().endswith("in record 237\n")


def test_of_two_failures_in_one_round_the_lower_record_speaks(tmp_path):
    n, lines = 3, [fixed(i % 150) for i in range(400)]
    share = 5 * len(lines[0])
    where = share_of_line(lines, share)
    lo, hi = where.index(2 * n + 1) + 2, where.index(2 * n + 2) + 1  # round 2: workers 1 and 2
    assert where[lo] // n == where[hi] // n == 2 and (where[lo] % n, where[hi] % n) == (1, 2) and lo < hi
    for make_lo, make_hi in ((bad_check_like, bad_strand_like), (bad_strand_like, bad_check_like)):
        bad = list(lines)
        bad[lo], bad[hi] = make_lo(fixed(900)), make_hi(fixed(901))
        assert share_of_line(bad, share) == where
        data = b"".join(bad)
        one = run(["dedupe", "-a"], 0, data=data)
        p = run(["dedupe", "-a"], n, data=data, tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=share)
        assert (p.returncode, p.stdout, p.stderr) == (one.returncode, one.stdout, one.stderr)
        assert p.returncode != 0 and p.stderr.decode().endswith(f"in record {lo}\n") and p.stderr.count(b"\n") == 1
        assert p.stdout == O.dedupe(b"".join(bad[:lo]), True)[0] and no_spool(tmp_path)


@pytest.mark.parametrize("phase", [1, 2, 3, 4])
def test_a_worker_that_dies_ends_the_run(tmp_path, phase):
    """the stand-in exits in place of a report of round 1: the launcher returns its status, what round 0 wrote stays, the spool is gone"""
    lines = S.stream(random.Random(77), 300)
    data = b"".join(lines)
    share = len(data) // 20
    want = O.dedupe(data, True)[0]
    for rank in (0, 2):
        p = run(["dedupe", "-a"], 4, data=data, tmp=tmp_path, PAFFY_DEDUPE_SHARE_BYTES=share, STANDIN_DEDUPE_EXIT=f"{rank}:{phase}:1")
        assert p.returncode == 7 and p.stderr == b""
        assert p.stdout == O.dedupe(data[: cuts(data, share)[4]], True)[0] and want.startswith(p.stdout) and 0 < len(p.stdout) < len(want)
        assert parts_started(tmp_path, 4) and no_spool(tmp_path)


def test_what_does_not_shard_becomes_one_plain_worker(tmp_path):
    env = dict(os.environ, PAFFY_WORKER="/bin/echo", PAFFY_GPUS="4", PAFFY_TMPDIR=str(tmp_path))
    missing, empty = str(tmp_path / "missing.paf"), tmp_path / "empty.paf"
    empty.write_bytes(b"")
    for args in (["dedupe", "-h"], ["dedupe", "-Z", "-a"], ["dedupe", "-a", "-i", missing], ["dedupe", "-i", str(empty), "-a"], ["dedupe", "--checkInverse"]):
        p = subprocess.run([PAFFY] + args, env=env, input=b"", capture_output=True, timeout=30)
        assert p.stdout == (" ".join(args) + "\n").encode() and p.returncode == 0  # the one worker says what the reference says about it
        assert no_spool(tmp_path)
    # and the stand-in as that one worker: no part, the world is not set
    for args, data in ((["dedupe", "-i", str(empty)], None), (["dedupe", "-a"], b"")):
        p = run(args, 4, data=data, tmp=tmp_path)
        assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"")
        assert [l.split()[:2] for l in log_of(tmp_path)] == [["/", "-"]]


def test_the_part_variables_reach_no_other_command(tmp_path):
    """a stream command started by the launcher sees neither of dedupe's names, whatever the caller's environment holds"""
    script = tmp_path / "env_worker.sh"
    script.write_text('#!/bin/sh\necho "$PAFFY_RANK part=[$PAFFY_DEDUPE_PART] fds=[$PAFFY_DEDUPE_FDS]" >> "$ENV_WORKER_LOG"\n')
    script.chmod(0o755)
    env = dict(os.environ, PAFFY_WORKER=str(script), PAFFY_GPUS="2", PAFFY_TMPDIR=str(tmp_path), ENV_WORKER_LOG=str(tmp_path / "env.txt"),
               PAFFY_DEDUPE_PART="/nowhere/0", PAFFY_DEDUPE_FDS="3,4")
    subprocess.run([PAFFY, "invert"], env=env, input=b"".join(S.stream(random.Random(1), 10)), capture_output=True, timeout=30)
    assert sorted((tmp_path / "env.txt").read_text().splitlines()) == ["0 part=[] fds=[]", "1 part=[] fds=[]"]

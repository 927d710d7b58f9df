"""`PAFFY_GPUS=N bin/paffy chain` (host/paffy_launch.c, run_chain) without a GPU: the worker is tests/standin_chain_worker.py, which honours
the part-mode contract (files, pipes, report layout, verdicts) with a trivial chaining -- every record a chain of its own -- so that what is
tested is the launcher's own work: the partition by query name, the global chain numbers from the workers' tail keys, the merge of the
workers' lines by their line keys, the one failure that ends the run, and that nothing can wait for ever on a worker that is gone. The
expected bytes are computed here by brute force from the stand-in's rule. tests/test_gpu_launcher_chain.py runs the real worker."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.environ.get("PAFFY_LAUNCHER") or os.path.join(ROOT, "bin", "paffy")  # the ASan + UBSan build goes here
STANDIN = os.path.join(ROOT, "tests", "standin_chain_worker.py")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s", "../bin/paffy"])


def run(args, n, data=None, tmp=None, **env_extra):
    env = dict(os.environ, PAFFY_GPUS=str(n), PAFFY_WORKER=STANDIN, PAFFY_ONE_DEVICE="1", **env_extra)
    if tmp:
        env["PAFFY_TMPDIR"] = str(tmp)
        env["STANDIN_CHAIN_LOG"] = str(tmp / "log.txt")
        if (tmp / "log.txt").exists():
            (tmp / "log.txt").unlink()
    return subprocess.run([PAFFY] + args, input=data, env=env, capture_output=True, timeout=60)


def log_of(tmp):
    p = tmp / "log.txt"
    return p.read_text().splitlines() if p.exists() else []


def no_spool(tmp):
    return [f for f in os.listdir(tmp) if f.startswith("paffy.")] == []


def rec(q, qs, score, strand="+"):
    return f"{q}\t100000\t{qs}\t{qs + 50}\t{strand}\tt\t100000\t{qs}\t{qs + 50}\t50\t50\t60\tAS:i:{score}\tcg:Z:50M\n".encode()


def records(n, names=7, seed=11, scores=(5, 5, 80, 900)):
    rng = random.Random(seed)
    return [rec("c%d" % rng.randrange(names), rng.randrange(0, 90000), rng.choice(scores), rng.choice("+-")) for _ in range(n)]


def brute_force(lines):
    """the stand-in's rule over the whole input: ids = rank by (class asc, AS desc, query start desc, number desc); lines by (AS desc, id)"""
    keys = []
    for g, ln in enumerate(lines):
        f = ln.rstrip(b"\n").split(b"\t")
        keys.append((0 if f[4] == b"+" else 1, int(f[12][5:]), int(f[2]), g))
    order = sorted(range(len(lines)), key=lambda g: (keys[g][0], -keys[g][1], -keys[g][2], -keys[g][3]))
    ids = [0] * len(lines)
    for k, g in enumerate(order):
        ids[g] = k
    out = sorted(range(len(lines)), key=lambda g: (-keys[g][1], ids[g]))
    return b"".join(lines[g].rstrip(b"\n") + b"\tcn:i:%d\n" % ids[g] for g in out), ids


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_chain_over_workers_is_the_brute_force_output(tmp_path, n):
    """600 records over 7 query names, four distinct scores, both strands: scores tie across parts all the time. Seven names start at most
    seven workers (a worker without a line is not started), each of them told the world is n."""
    lines = records(600)
    assert any(b"\t+\t" in ln for ln in lines) and any(b"\t-\t" in ln for ln in lines)
    data = b"".join(lines)
    want, _ = brute_force(lines)
    src, dst = tmp_path / "in.paf", tmp_path / "out.paf"
    src.write_bytes(data)
    p = run(["chain", "-i", str(src), "-o", str(dst)], n, tmp=tmp_path)
    assert p.returncode == 0, p.stderr
    assert dst.read_bytes() == want and p.stdout == b""
    log = log_of(tmp_path)
    assert len(log) == min(n, 7) and sorted(l.split()[0] for l in log) == sorted(f"{r}/{n}" for r in range(min(n, 7)))
    assert no_spool(tmp_path)
    p = run(["chain"], n, data=data[:-1], tmp=tmp_path)  # stdin -> stdout, the last line without its newline
    assert p.returncode == 0, p.stderr
    assert p.stdout == want
    assert len(log_of(tmp_path)) == min(n, 7) and no_spool(tmp_path)


@pytest.mark.parametrize("n_chains", [14, 130])
def test_chain_numbers_change_their_digit_count_between_parts(tmp_path, n_chains):
    """more than 10 and more than 100 chains: the appended id has one, two or three digits, differently in every part, so a line's length
    is what the line keys say and nothing the input could tell"""
    lines = records(n_chains, names=5, seed=n_chains)
    want, ids = brute_force(lines)
    assert len({len(str(i)) for i in ids}) == (2 if n_chains < 100 else 3)
    for n in (2, 3):
        p = run(["chain"], n, data=b"".join(lines), tmp=tmp_path)
        assert p.returncode == 0 and p.stdout == want, p.stderr
        assert len(log_of(tmp_path)) == n


def test_fewer_names_than_workers_one_name_and_the_empty_input(tmp_path):
    for names, n, started in ((2, 5, 2), (1, 3, 1), (1, 8, 1)):
        lines = records(120, names=names, seed=names)
        p = run(["chain"], n, data=b"".join(lines), tmp=tmp_path)
        assert p.returncode == 0 and p.stdout == brute_force(lines)[0], p.stderr
        assert [l.split()[0].split("/")[1] for l in log_of(tmp_path)] == [str(n)] * started
    p = run(["chain"], 4, data=b"", tmp=tmp_path)
    assert p.returncode == 0 and p.stdout == b"" and log_of(tmp_path) == []
    src, dst = tmp_path / "empty.paf", tmp_path / "out.paf"
    src.write_bytes(b"")
    dst.write_bytes(b"what was here before")
    p = run(["chain", "-i", str(src), "-o", str(dst)], 3, tmp=tmp_path)
    assert p.returncode == 0 and dst.read_bytes() == b"" and log_of(tmp_path) == []
    assert no_spool(tmp_path)
    p = run(["chain", "-i", str(src), "-o", str(tmp_path / "no" / "such" / "out.paf")], 3, tmp=tmp_path)
    assert p.returncode == 1 and p.stderr.decode() == f"paffy chain: cannot open {tmp_path / 'no' / 'such' / 'out.paf'}\n"


def test_of_two_parse_failures_the_lower_record_reports(tmp_path):
    """seven workers for seven names: c1 and c4 are in different parts, and either part may hold the lower record"""
    lines = records(300)
    star = lambda q, qs: rec(q, qs, 7).replace(b"\t+\t", b"\t*\t")  # noqa: E731
    for lo, hi in ((40, 200), (90, 91)):
        for q_lo, q_hi in (("c1", "c4"), ("c4", "c1")):
            bad = list(lines)
            bad[lo], bad[hi] = star(q_lo, 10), star(q_hi, 20)
            dst = tmp_path / "out.paf"
            dst.write_bytes(b"old")
            p = run(["chain", "-o", str(dst)], 7, data=b"".join(bad), tmp=tmp_path)
            assert p.returncode == 1 and p.stdout == b"" and dst.read_bytes() == b""
            assert p.stderr.decode() == f"stand-in chain: unexpected strand in record {lo}\n"  # exactly one message
            assert len(log_of(tmp_path)) == 7 and no_spool(tmp_path)
    # a parse failure in one part, a failed check in another: the parse failure ends the run before anything is numbered
    bad = list(lines)
    bad[250] = star("c2", 10)
    other = next(g for g, ln in enumerate(bad) if ln.startswith(b"c5\t"))
    p = run(["chain"], 7, data=b"".join(bad), tmp=tmp_path, STANDIN_CHAIN_FAIL2=str(other))
    assert p.returncode == 1 and p.stdout == b"" and p.stderr.decode() == "stand-in chain: unexpected strand in record 250\n"


def test_of_two_failed_checks_the_smaller_chain_id_reports(tmp_path):
    lines = records(300)
    _, ids = brute_force(lines)
    of_name = lambda q: [g for g, ln in enumerate(lines) if ln.startswith(q + b"\t")]  # noqa: E731
    by_id = lambda q: sorted(of_name(q), key=lambda g: ids[g])  # noqa: E731
    c1, c4, c2 = by_id(b"c1"), by_id(b"c4"), by_id(b"c2")
    # in different parts (seven workers for seven names), each of the two the one to report once; then both in ONE part of three: that
    # worker reports its own least
    for a, b, n, first in ((c1[0], c4[-1], 7, c1[0]), (c1[-1], c4[0], 7, c4[0]), (c2[5], c2[1], 3, c2[1])):
        p = run(["chain"], n, data=b"".join(lines), tmp=tmp_path, STANDIN_CHAIN_FAIL2=f"{a},{b}")
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr.decode() == f"stand-in chain: check failed in record {first} (chain {ids[first]})\n"
        assert no_spool(tmp_path)


@pytest.mark.parametrize("rank", [0, 2])
def test_a_worker_that_exits_before_it_reports_ends_the_run(tmp_path, rank):
    """end-of-file on that worker's pipe is its failure: the others are told to end, nothing is written, the status is the dead worker's"""
    lines = records(300)
    dst = tmp_path / "out.paf"
    p = run(["chain", "-o", str(dst)], 4, data=b"".join(lines), tmp=tmp_path, STANDIN_CHAIN_EXIT_RANK=str(rank))
    assert p.returncode == 7 and p.stdout == b"" and dst.read_bytes() == b""
    assert len(log_of(tmp_path)) == 4 and no_spool(tmp_path)
    # and with a reported failure elsewhere: the worker that is gone still decides, nobody else speaks
    bad = list(lines)
    bad[5] = rec("c3", 10, 7).replace(b"\t+\t", b"\t*\t")
    p = run(["chain"], 4, data=b"".join(bad), tmp=tmp_path, STANDIN_CHAIN_EXIT_RANK=str(rank))
    assert p.returncode == 7 and p.stdout == b"" and p.stderr == b"" and no_spool(tmp_path)


def test_what_does_not_shard_becomes_one_worker(tmp_path):
    env = dict(os.environ, PAFFY_WORKER="/bin/echo", PAFFY_GPUS="4", PAFFY_TMPDIR=str(tmp_path))
    missing = str(tmp_path / "missing.paf")
    p = subprocess.run([PAFFY, "chain", "-i", missing], env=env, capture_output=True, timeout=30)
    assert p.stdout == f"chain -i {missing}\n".encode()  # the one worker says what the reference says about it
    p = subprocess.run([PAFFY, "chain", "-h"], env=env, capture_output=True, timeout=30)
    assert p.stdout == b"chain -h\n"
    p = subprocess.run([PAFFY, "chain", "-Z", "-g", "5"], env=env, capture_output=True, timeout=30)
    assert p.stdout == b"chain -Z -g 5\n"
    assert no_spool(tmp_path)


def test_options_are_forwarded_to_every_worker(tmp_path):
    lines = records(100)
    src, dst = tmp_path / "in.paf", tmp_path / "out.paf"
    src.write_bytes(b"".join(lines))
    p = run(["chain", "-g7", "--trimFraction", "0.5", "-i", str(src), "-d", "3", "--chainGapExtend=2", "-o", str(dst), "--logLevel", "INFO"], 3, tmp=tmp_path)
    assert p.returncode == 0, p.stderr
    assert dst.read_bytes() == brute_force(lines)[0]
    log = log_of(tmp_path)
    assert len(log) == 3
    for entry in log:
        who, _, argv = entry.partition(" ")
        r = who.split("/")[0]
        assert argv.startswith("chain -g 7 -t 0.5 -d 3 -e 2 -l INFO -i ") and argv.endswith(f"/{r}.in -o " + argv.split(" -o ")[1])
        assert argv.split(" -o ")[1].endswith(f"/{r}.out")
    assert b"launcher: partition" in p.stderr  # -l INFO: the launcher's own steps are timed on stderr
    p = run(["chain", "-i", str(src)], 3, tmp=tmp_path)
    assert p.returncode == 0 and p.stderr == b""

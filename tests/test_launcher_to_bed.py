"""`PAFFY_GPUS=N bin/paffy to_bed` (host/paffy_launch.c, run_to_bed) without a GPU: the worker is tests/standin_bed_worker.py, which honours
the part-mode contract (files, pipes, report layout, verdicts) and counts the coverage in plain Python, so that what is tested is the
launcher's own work: the partition by the names of both sides with its side masks, the one failure that ends the run, the order of the
sequence blocks, the -q tail, and that nothing can wait for ever on a worker that is gone. The expected bytes are the oracle's
(oracle_lib.to_bed) on the whole input; the -q tail is computed here. tests/test_gpu_launcher_to_bed.py runs the real worker."""
import json
import os
import random
import subprocess

import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.environ.get("PAFFY_LAUNCHER") or os.path.join(ROOT, "bin", "paffy")  # the ASan + UBSan build goes here
STANDIN = os.path.join(ROOT, "tests", "standin_bed_worker.py")
QUERIES = ["q%d" % i for i in range(7)]
TARGETS = ["t0", "t1", "t2", "q1", "q4"]  # two sequences are queries of some lines and targets of others
LENGTH = {name: 2000 + 371 * k for k, name in enumerate(QUERIES + TARGETS[:3])}


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s", "../bin/paffy"])


def run(args, n, data=None, tmp=None, timeout=60, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_BED_PART", "PAFFY_BED_FDS")}
    env.update(PAFFY_WORKER=STANDIN, PAFFY_ONE_DEVICE="1", **env_extra)
    if n > 1:
        env["PAFFY_GPUS"] = str(n)
    if tmp:
        dump = tmp / "dump"
        dump.mkdir(exist_ok=True)
        for f in list(dump.iterdir()) + [tmp / "log.txt"]:
            if f.exists():
                f.unlink()
        env.update(PAFFY_TMPDIR=str(tmp), STANDIN_BED_LOG=str(tmp / "log.txt"), STANDIN_BED_DUMP=str(dump))
    p = subprocess.run([PAFFY, "to_bed"] + args, input=data, env=env, capture_output=True, timeout=timeout)
    if tmp:
        assert [f for f in os.listdir(tmp) if f.startswith("paffy.")] == []  # nothing is left of the spools, however the run ended
    return p


def log_of(tmp):
    p = tmp / "log.txt"
    return p.read_text().splitlines() if p.exists() else []


def ranks_of(tmp):
    return sorted(l.split()[0] for l in log_of(tmp))


def parts_of(tmp):
    """{rank: {global record: mask}} as the part workers got them"""
    return {int(f.name.split(".")[0]): {g: m for g, m in json.loads(f.read_text())} for f in (tmp / "dump").iterdir()}


def rec(q, t, qs, ts, ops, strand="+", qe_off=0, te_off=0, qlen=None, tlen=None):
    qe = qs + sum(n for n, op in ops if op in "MI") + qe_off
    te = ts + sum(n for n, op in ops if op in "MD") + te_off
    cg = "".join("%d%s" % o for o in ops)
    return f"{q}\t{qlen or LENGTH[q]}\t{qs}\t{qe}\t{strand}\t{t}\t{tlen or LENGTH[t]}\t{ts}\t{te}\t10\t10\t60\tcg:Z:{cg}\n".encode()


def records(n, seed=7, queries=QUERIES, targets=TARGETS):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        q, t = rng.choice(queries), rng.choice(targets)
        if q == t:
            continue
        ops = [(rng.randrange(1, 40), "M")]
        for _ in range(rng.randrange(0, 4)):
            ops += [(rng.randrange(1, 9), rng.choice("ID")), (rng.randrange(1, 40), "M")]
        out.append(rec(q, t, rng.randrange(0, 1500), rng.randrange(0, 1500), ops, rng.choice("+-")))
    return out


def first_appearance(lines, with_target):
    seen = []
    for ln in lines:
        f = ln.split(b"\t")
        for name in [f[0]] + ([f[5]] if with_target else []):
            if name not in seen:
                seen.append(name)
    return seen


def block_names(out):
    names = []
    for ln in out.splitlines():
        if not names or names[-1] != ln.split(b" ")[0]:
            names.append(ln.split(b" ")[0])
    return names


OPTION_SETS = [([], {}), (["-n"], dict(include_inverted=True)), (["--binary"], dict(binary=True)), (["-e"], dict(exclude_unaligned=True)),
               (["--excludeAligned"], dict(exclude_aligned=True)), (["-m", "50"], dict(min_size=50)),
               (["-nfm3"], dict(include_inverted=True, exclude_aligned=True, min_size=3)),
               (["--includeInverted", "-f", "--minSize=3"], dict(include_inverted=True, exclude_aligned=True, min_size=3))]


@pytest.fixture(scope="module")
def shuffled():
    """300 records, 7 query names, 5 target names (two of them query names too), both strands; what the oracle writes per option set"""
    lines = records(300)
    data = b"".join(lines)
    want = []
    for _, kw in OPTION_SETS:
        out, err = O.to_bed(data, **kw)
        assert err.code == 0 and out
        want.append(out)
    return lines, data, want


@pytest.mark.parametrize("n", [2, 3, 5])
def test_option_sets_over_workers_are_the_oracle_output(tmp_path, shuffled, n):
    lines, data, wants = shuffled
    src, dst = tmp_path / "in.paf", tmp_path / "out.bed"
    src.write_bytes(data)
    for (args, kw), want in zip(OPTION_SETS, wants):
        p = run(args + ["-i", str(src), "--outputFile", str(dst)], n, tmp=tmp_path)
        assert p.returncode == 0 and p.stdout == b"" and p.stderr == b"", p.stderr
        assert dst.read_bytes() == want, args
        assert ranks_of(tmp_path) == sorted(f"{r}/{n}" for r in range(n))  # at least seven names: every worker has lines
        short = [{"binary": "-b", "exclude_unaligned": "-e", "exclude_aligned": "-f", "include_inverted": "-n"}.get(k, "-m " + str(v)) for k, v in kw.items()]
        for entry in log_of(tmp_path):  # the options as the launcher parsed them, then its own -i / -o
            who, _, argv = entry.partition(" ")
            r = who.split("/")[0]
            assert sorted(argv.split(" -i ")[0].replace("-m ", "-m_").split()[1:]) == sorted(s.replace("-m ", "-m_") for s in short), argv
            assert argv.split(" -i ")[1].split(" -o ")[0].endswith(f"/{r}.in") and argv.endswith(f"/{r}.out")
    p = run(["-n"], n, data=data[:-1], tmp=tmp_path)  # stdin -> stdout, the last line without its newline
    assert p.returncode == 0 and p.stdout == wants[1], p.stderr


def test_roles_masks_and_block_order_with_inverted(tmp_path, shuffled):
    lines, data, wants = shuffled
    p = run(["-n"], 3, data=data, tmp=tmp_path)
    assert p.returncode == 0 and p.stdout == wants[1]
    parts = parts_of(tmp_path)
    owner = {}
    for r, got in parts.items():
        for g, m in got.items():
            f = lines[g].split(b"\t")
            for bit, name in ((1, f[0]), (2, f[5])):
                if m & bit:
                    assert owner.setdefault(name, r) == r  # a sequence is counted in one part only
    copies = {g: sorted(parts[r][g] for r in parts if g in parts[r]) for g in range(len(lines))}
    assert [3] in copies.values() and [1, 2] in copies.values()  # both names with one owner: once, mask 3; with two owners: a side each
    for g, masks in copies.items():
        f = lines[g].split(b"\t")
        assert masks == ([3] if owner[f[0]] == owner[f[5]] else [1, 2]), g
    order = block_names(p.stdout)
    assert order == first_appearance(lines, True) and len(order) == len(set(order)) == 10  # q1, q4: query here, target there, one block each
    assert order[1] == lines[0].split(b"\t")[5]  # the second block's sequence first appeared as a target side
    owners = [owner[name] for name in order]
    assert any(owners[i] != owners[i + 1] and owners[i] in owners[i + 2:] for i in range(len(owners) - 2))  # interleaved across parts
    p = run([], 3, data=data, tmp=tmp_path)  # without -n: every line once, mask 1
    assert p.returncode == 0 and p.stdout == wants[0]
    parts = parts_of(tmp_path)
    assert sorted(g for got in parts.values() for g in got) == list(range(len(lines))) and {m for got in parts.values() for m in got.values()} == {1}


def test_fewer_names_than_workers_one_name_and_the_empty_input(tmp_path):
    for names, n, started in ((2, 5, 2), (1, 3, 1)):
        lines = records(80, seed=names, queries=QUERIES[:names], targets=["t0"])
        p = run([], n, data=b"".join(lines), tmp=tmp_path)
        assert p.returncode == 0 and p.stdout == O.to_bed(b"".join(lines))[0], p.stderr
        assert ranks_of(tmp_path) == [f"{r}/{n}" for r in range(started)]
    lines = records(80, seed=5, queries=QUERIES[:1], targets=["t0"])
    p = run(["-n"], 5, data=b"".join(lines), tmp=tmp_path)  # with -n the target name is a second name: two workers
    assert p.returncode == 0 and p.stdout == O.to_bed(b"".join(lines), include_inverted=True)[0] and len(log_of(tmp_path)) == 2
    fa = tmp_path / "q.fa"
    fa.write_bytes(b">q0\nACGT\n>nobody\nACGTA\nCG\n")
    for args, want in (([], b""), (["-f", "-q", str(fa)], b"q0 0 4\t0\nnobody 0 7\t0\n")):
        p = run(args, 4, data=b"", tmp=tmp_path)  # no line at all: one plain worker, which under -f -q still lists every FASTA record
        assert p.returncode == 0 and p.stdout == want and ranks_of(tmp_path) == ["/"]
    src, dst = tmp_path / "empty.paf", tmp_path / "out.bed"
    src.write_bytes(b"")
    dst.write_bytes(b"what was here before")
    p = run(["-i", str(src), "-o", str(dst)], 3, tmp=tmp_path)
    assert p.returncode == 0 and dst.read_bytes() == b"" and ranks_of(tmp_path) == ["/"]
    p = run(["-i", str(src), "-o", str(tmp_path / "no" / "such" / "out.bed")], 3, data=None, tmp=tmp_path)
    assert p.returncode != 0
    src.write_bytes(b"".join(lines))
    p = run(["-i", str(src), "-o", str(tmp_path / "no" / "such" / "out.bed")], 3, tmp=tmp_path)
    assert p.returncode == 1 and p.stderr.decode() == f"paffy to_bed: cannot open {tmp_path / 'no' / 'such' / 'out.bed'}\n"


def test_a_block_without_bytes_and_a_short_line(tmp_path):
    lines = records(60, seed=9)
    bare = b"lonely\t500\t4\t4\t+\tt0\t%d\t5\t5\t0\t0\t60\n" % LENGTH["t0"]  # no cigar, empty ranges: a sequence no base of which is covered
    data = b"".join(lines[:20] + [bare] + lines[20:])
    for args, kw in ((["-e"], dict(exclude_unaligned=True)), (["-e", "-n"], dict(exclude_unaligned=True, include_inverted=True))):
        want = O.to_bed(data, **kw)[0]
        assert b"lonely" not in want and b"lonely" in O.to_bed(data)[0]
        for n in (2, 5):
            p = run(args, n, data=data, tmp=tmp_path)
            assert p.returncode == 0 and p.stdout == want, p.stderr
    short = b"q0\t%d\t1\t2\t+\n" % LENGTH["q0"]  # fewer than six columns: a query side only, and no worker can parse it
    data = b"".join(lines[:30] + [short] + lines[30:])
    one = run(["-n"], 1, data=data, tmp=tmp_path)
    assert one.returncode == 1 and one.stderr.decode() == "stand-in to_bed: a line that does not parse in record 30\n"
    p = run(["-n"], 3, data=data, tmp=tmp_path)
    assert (p.returncode, p.stdout, p.stderr) == (one.returncode, b"", one.stderr)
    assert [r for r, got in parts_of(tmp_path).items() if 30 in got and got[30] == 1] and sum(30 in got for got in parts_of(tmp_path).values()) == 1


def test_the_tail_of_sequences_without_alignments(tmp_path, shuffled):
    lines, data, _ = shuffled
    fasta = [("q3", 5), ("never", 9), ("t1", 3), ("q1", 4), ("also never", 2), ("t2", 6)]
    fa = tmp_path / "seqs.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (h.encode(), b"A" * n) for h, n in fasta))
    for inv in (False, True):
        named = set(first_appearance(lines, inv))
        tail = b"".join(b"%s 0 %d\t0\n" % (h.encode(), n) for h, n in fasta if h.encode() not in named)
        assert tail.count(b"\n") == (2 if inv else 4)  # without -n the target names t1, t2 are not seen (q1 is a query name too)
        want = O.to_bed(data, exclude_aligned=True, include_inverted=inv)[0]
        for n in (2, 3, 5):  # every query name lies in one part only: a flag seen in another part must not be listed
            p = run(["-f", "-q", str(fa)] + (["-n"] if inv else []), n, data=data, tmp=tmp_path)
            assert p.returncode == 0 and p.stdout == want + tail, (n, inv, p.stderr)
            assert len(log_of(tmp_path)) == n
    p = run(["-f", "--queryFastaFile", str(tmp_path / "missing.fa")], 3, data=data, tmp=tmp_path)  # cannot be opened: adds nothing
    assert p.returncode == 0 and p.stdout == O.to_bed(data, exclude_aligned=True)[0]
    p = run(["-q", str(fa)], 3, data=data, tmp=tmp_path, timeout=20)  # without -f there is no tail and no second phase to wait for
    assert p.returncode == 0 and p.stdout == O.to_bed(data)[0]


def walk_fails(line, side):
    """the same record with a range one base longer than its cigar on the query (0) or the target (1) side"""
    f = line.split(b"\t")
    f[3 if side == 0 else 8] = b"%d" % (int(f[3 if side == 0 else 8]) + 1)
    return b"\t".join(f)


def unparsable(line):
    f = line.split(b"\t")
    f[4] = b"*"
    return b"\t".join(f)


def test_of_failures_in_two_parts_the_lower_record_speaks(tmp_path, shuffled):
    lines, _, _ = shuffled
    make = {"parse": unparsable, "query": lambda ln: walk_fails(ln, 0), "target": lambda ln: walk_fails(ln, 1)}
    of_query = lambda q: [g for g, ln in enumerate(lines) if ln.startswith(q + b"\t")]  # noqa: E731
    a, b = of_query(b"q0"), of_query(b"q5")
    seen_apart = 0
    for lo, hi in ((a[3], b[-2]), (b[2], a[-1])):
        for k_lo, k_hi in (("parse", "query"), ("query", "parse"), ("target", "target"), ("query", "target")):
            bad = list(lines)
            bad[lo], bad[hi] = make[k_lo](lines[lo]), make[k_hi](lines[hi])
            data = b"".join(bad)
            one = run(["-n"], 1, data=data, tmp=tmp_path)
            assert one.returncode in (1, -6) and one.stdout == b"" and one.stderr.decode().endswith(f"in record {lo}\n")
            dst = tmp_path / "out.bed"
            dst.write_bytes(b"old")
            p = run(["-n", "-o", str(dst)], 7, data=data, tmp=tmp_path)
            assert (p.returncode, p.stdout, p.stderr) == (one.returncode, b"", one.stderr)  # exactly one message, that worker's status
            assert dst.read_bytes() == b""
            parts = parts_of(tmp_path)
            seen_apart += not any(lo in got and hi in got for got in parts.values())
    assert seen_apart  # the two failing lines did lie in different parts
    # one record whose two sides fail in different parts: the query side is checked first
    g = next(g for g in a if lines[g].split(b"\t")[5] in (b"t0", b"t1", b"t2"))
    bad = list(lines)
    bad[g] = walk_fails(walk_fails(lines[g], 0), 1)
    for n in (3, 5, 7):
        one = run(["-n"], 1, data=b"".join(bad), tmp=tmp_path)
        p = run(["-n"], n, data=b"".join(bad), tmp=tmp_path)
        assert one.returncode == -6 and b"q0 in record %d\n" % g in one.stderr
        assert (p.returncode, p.stdout, p.stderr) == (one.returncode, b"", one.stderr)
    # a line that does not parse reaches both of its owners, and one of them speaks
    bad = list(lines)
    bad[g] = unparsable(lines[g])
    p = run(["-n"], 7, data=b"".join(bad), tmp=tmp_path)
    assert p.returncode == 1 and p.stderr.decode() == f"stand-in to_bed: a line that does not parse in record {g}\n"
    assert sum(g in got for got in parts_of(tmp_path).values()) == 2


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_a_worker_that_exits_before_it_reports_ends_the_run(tmp_path, shuffled, rank):
    _, data, _ = shuffled
    dst = tmp_path / "out.bed"
    for args in (["-n"], ["-f", "-q", str(tmp_path / "missing.fa")]):
        p = run(args + ["-o", str(dst)], 3, data=data, tmp=tmp_path, timeout=20, STANDIN_BED_EXIT_RANK=str(rank))
        assert p.returncode == 7 and p.stdout == b"" and dst.read_bytes() == b""
        assert len(log_of(tmp_path)) == 3


def test_an_output_that_disagrees_with_its_block_keys(tmp_path, shuffled):
    _, data, _ = shuffled
    p = run([], 3, data=data, tmp=tmp_path, STANDIN_BED_LONG_OUT="1")
    assert p.returncode == 1 and p.stderr.decode() == "paffy to_bed: the output of worker 1 is not what its block keys say\n"


def test_what_does_not_shard_becomes_one_worker(tmp_path):
    env = dict(os.environ, PAFFY_WORKER="/bin/echo", PAFFY_GPUS="4", PAFFY_TMPDIR=str(tmp_path))
    missing = str(tmp_path / "missing.paf")
    for args in (["-i", missing], ["-h"], ["-n", "--help"], ["-Z", "-m", "5"], ["-m"]):
        p = subprocess.run([PAFFY, "to_bed"] + args, env=env, capture_output=True, timeout=30)
        assert p.stdout == ("to_bed " + " ".join(args) + "\n").encode()  # the one worker says what the reference says about it
    assert os.listdir(tmp_path) == []

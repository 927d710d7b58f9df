"""`PAFFY_GPUS=N bin/paffy view` (host/paffy_launch.c) without a GPU: the worker is tests/standin_view_worker.py (PAFFY_WORKER), which
honours PAFFY_RANGE and PAFFY_VIEW_SUMS with the CPU oracle, so what is tested is the launcher's own work -- the cut at line ends, the
rank-ordered concatenation, the aggregate line from the workers' sums files in the reference's float arithmetic, the two closing
asserts, the statuses, the spool directory. Expected bytes are the oracle's. Every case runs through bin/paffy and through the
AddressSanitizer + UBSan build of the launcher (bin/paffy_asan, a stand-alone program); PAFFY_LAUNCHER replaces the former, as in
tests/test_launcher.py. tests/test_gpu_launcher_view.py runs the real worker on one GPU."""
import math
import os
import struct
import subprocess

import pytest

import oracle_lib as O
import synth_lib
from paffy_amd import shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "standin_view_worker.py")
SAN = dict(ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
ASSERTION = b"paffy view: Assertion failed (average identity or aligned bases below the requested minimum)\n"


@pytest.fixture(scope="module", params=["plain", "asan"])
def launcher(request):
    if request.param == "asan":
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s", "asan"])
        return os.path.join(ROOT, "bin", "paffy_asan")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s", "../bin/paffy"])
    return os.environ.get("PAFFY_LAUNCHER") or os.path.join(ROOT, "bin", "paffy")


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def fmt(a, b):  # (float)a / b as %f prints it
    return "%f" % f32(f32(a) / f32(b)) if b else "-nan"


def total_line(n, tot):
    m, x, qi, qd, qib, qdb = tot
    return ("Total-alignments:%d\tAvg-Identity:%s\tAvg-Identity-with-gaps:%s\tAligned-bases:%d\tAligned-bases-with-gaps:%d\tQuery-inserts:%d\tQuery-deletes:%d\n"
            % (n, fmt(m, m + x), fmt(m, m + x + qib + qdb), m + x, m + x + qib + qdb, qi, qd)).encode()


_CASE = {}


def case():
    """120 cfg4-style records on their genomes: (data, seqs, the oracle's stats lines, its blocks with rows, its sums)"""
    if not _CASE:
        host = synth_lib.Synth4(0x5EED0004, 2048, n_contigs=6, tlen_min=200_000, tlen_span=200_000)
        data, seqs = host.records(0, 120), host.genomes()
        enc, err = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs)
        assert err.code == 0
        lines, blocks, tot = [], [], [0] * 6
        for ln in enc.splitlines(keepends=True):
            f = ln.split(b"\t")
            lines.append(O.pretty_print(ln, b"", b"", False)[1])
            blocks.append(O.pretty_print(ln, seqs[f[0].decode()], seqs[f[5].decode()], True)[1])
            tot = O.cigar_stats(ln.split(b"cg:Z:")[1].split(b"\t")[0].strip().decode(), tot, zero=False)
        _CASE["c"] = (data, seqs, lines, blocks, tot)
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


def run(launcher, args, n, tmp, data=None, **extra):
    env = dict(os.environ, PAFFY_GPUS=str(n), PAFFY_WORKER=STANDIN, PAFFY_ONE_DEVICE="1", PAFFY_TMPDIR=str(tmp), **SAN, **extra)
    p = subprocess.run([launcher, "view"] + args, input=data, env=env, capture_output=True, timeout=300)
    assert [f for f in os.listdir(tmp) if f.startswith("paffy.")] == [], "a spool directory was left behind"
    return p


@pytest.mark.parametrize("flags", [("-s",), ("-a", "-s"), ("-s", "-t"), ()], ids=["s", "a_s", "s_t", "plain"])
def test_n_workers_write_what_one_writes(launcher, files, tmp_path, flags):
    paf, fa = files
    data, seqs, lines, blocks, tot = case()
    want = b"" if "-t" in flags else b"".join(blocks if "-a" in flags else lines)
    if "-s" in flags:
        want += total_line(120, tot)
    status = 0 if "-s" in flags else -6  # without -s the reference adds nothing up, and its first closing assert fails on the NaN of 0 / 0
    one = run(launcher, list(flags) + ["-i", paf, fa], 1, tmp_path)
    assert (one.returncode, one.stdout) == (status, want), one.stderr[-2000:]
    for n in (2, 3, 5):
        p = run(launcher, list(flags) + ["-i", paf, fa], n, tmp_path)
        assert (p.returncode, p.stdout, p.stderr) == (status, want, one.stderr), (n, p.stderr[-2000:])
    # -o, long options, an option value that looks like an option
    out = tmp_path / "out.txt"
    p = run(launcher, list(flags) + ["--inputFile", paf, "--outputFile=" + str(out), "-l", "-i", fa], 3, tmp_path)
    assert p.returncode == status and out.read_bytes() == want and p.stdout == b""


def test_stdin_and_fewer_lines_than_workers(launcher, files, tmp_path):
    paf, fa = files
    data, seqs, lines, blocks, tot = case()
    p = run(launcher, ["-s", fa], 3, tmp_path, data=data)
    assert (p.returncode, p.stdout) == (0, b"".join(lines) + total_line(120, tot)), p.stderr[-2000:]
    two = b"".join(data.splitlines(keepends=True)[:2])
    enc = O.run([O.stage(O.ADD_MISMATCHES)], two, seqs)[0].splitlines(keepends=True)
    t2 = [0] * 6
    for ln in enc:
        t2 = O.cigar_stats(ln.split(b"cg:Z:")[1].split(b"\t")[0].strip().decode(), t2, zero=False)
    p = run(launcher, ["-s", fa], 5, tmp_path, data=two)
    assert (p.returncode, p.stdout) == (0, b"".join(lines[:2]) + total_line(2, t2)), p.stderr[-2000:]
    p = run(launcher, ["-s", fa], 2, tmp_path, data=two[:-1])  # no line end behind the last record
    assert (p.returncode, p.stdout) == (0, b"".join(lines[:2]) + total_line(2, t2)), p.stderr[-2000:]


def test_the_aggregate_line_of_records_without_aligned_bases_and_of_no_record(launcher, files, tmp_path):
    """totals of 0: both ratios print as -nan, and the first closing assert fails as in the reference (NaN >= 0 is false): abort"""
    paf, fa = files
    data, seqs, lines, blocks, tot = case()
    bare = b"".join(ln[:ln.index(b"\tcg:Z:")] + b"\n" for ln in data.splitlines(keepends=True)[:7])
    want = b"".join(O.pretty_print(ln, b"", b"", False)[1] for ln in bare.splitlines(keepends=True)) + total_line(7, [0] * 6)
    assert b"Avg-Identity:-nan\tAvg-Identity-with-gaps:-nan\t" in want
    for n in (1, 3):
        p = run(launcher, ["-s", fa], n, tmp_path, data=bare)
        assert (p.returncode, p.stdout) == (-6, want), (n, p.returncode, p.stderr[-2000:])
        assert p.stderr.endswith(ASSERTION)
    for n in (1, 4):  # no record at all
        p = run(launcher, ["-s", fa], n, tmp_path, data=b"")
        assert (p.returncode, p.stdout) == (-6, total_line(0, [0] * 6)), (n, p.returncode, p.stderr[-2000:])
        assert p.stderr.endswith(ASSERTION)
        p = run(launcher, [fa], n, tmp_path, data=b"")  # without -s too
        assert (p.returncode, p.stdout) == (-6, b"") and p.stderr.endswith(ASSERTION)


def test_the_two_closing_asserts_run_on_the_sums_of_all_parts(launcher, files, tmp_path):
    paf, fa = files
    data, seqs, lines, blocks, tot = case()
    m, x = tot[0], tot[1]
    identity = f32(f32(m) / f32(m + x))
    assert 0.0 < identity < 1.0 and not math.isnan(identity)
    text = b"".join(lines) + total_line(120, tot)
    below, above = "%.6f" % (identity - 0.001), "%.6f" % (identity + 0.001)
    for args, fails in ((["-u", below], False), (["-u", above], True), (["-v", str(m + x)], False), (["-v", str(m + x + 1)], True),
                        (["-u", below, "-v", str(m + x + 1)], True), (["-u", above, "-u", below], False)):
        for n in (1, 3):
            p = run(launcher, ["-s"] + args + ["-i", paf, fa], n, tmp_path)
            assert (p.returncode, p.stdout) == (-6 if fails else 0, text), (args, n, p.returncode, p.stderr[-2000:])
            assert p.stderr.endswith(ASSERTION) == fails
    # without -s the reference adds nothing up: sums of 0, and the first assert fails whatever -u says
    p = run(launcher, ["-u", below, "-i", paf, fa], 3, tmp_path)
    assert (p.returncode, p.stdout) == (-6, b"".join(lines)) and p.stderr.endswith(ASSERTION)


def test_a_worker_that_fails_in_the_middle_ends_the_run(launcher, files, tmp_path):
    paf, fa = files
    data, seqs, lines, blocks, tot = case()
    recs = data.splitlines(keepends=True)
    bad = b"q\t10\t0\t5\t*\tt\t10\t0\t5\t5\t5\t60\n"  # strand '*': exit 1 (impl/paf.c:154-158)
    broken = b"".join(recs[:70]) + bad + b"".join(recs[70:])
    one = run(launcher, ["-s", fa], 1, tmp_path, data=broken)
    assert (one.returncode, one.stdout) == (1, b"".join(lines[:70]))
    for n in (2, 4):
        p = run(launcher, ["-s", fa], n, tmp_path, data=broken)
        assert (p.returncode, p.stdout) == (1, b"".join(lines[:70])), (n, p.stderr[-2000:])  # no later worker's text, no aggregate line
        assert b"Total-alignments" not in p.stdout


def test_a_worker_that_leaves_no_sums(launcher, files, tmp_path):
    paf, fa = files
    data, seqs, lines, blocks, tot = case()
    cuts = shard.stream_cuts(data, 3)  # the launcher's cut, restated: which records worker 0 and 1 hold
    held = data[:cuts[2]].count(b"\n")
    assert 0 < data[:cuts[1]].count(b"\n") < held < 120
    # killed once its output is written: the outputs of the lower ranks and its own are out, nothing behind them, its signal is ours
    p = run(launcher, ["-s", "-i", paf, fa], 3, tmp_path, STANDIN_VIEW_DIE_RANK="1")
    assert (p.returncode, p.stdout) == (-9, b"".join(lines[:held])), p.stderr[-2000:]
    # ends well without a sums file: no aggregate line can be right
    p = run(launcher, ["-s", "-i", paf, fa], 3, tmp_path, STANDIN_VIEW_NO_SUMS_RANK="1")
    assert (p.returncode, p.stdout) == (1, b"".join(lines[:held])) and b"left no sums" in p.stderr


def test_without_a_sequence_file_one_worker_speaks(launcher, files, tmp_path):
    p = run(launcher, ["-s", "-i", files[0]], 3, tmp_path)
    assert (p.returncode, p.stdout, p.stderr) == (1, b"", b"Expected at least one sequence file\n")

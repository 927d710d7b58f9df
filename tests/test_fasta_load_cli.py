"""`bin/paffy add_mismatches | view | upconvert | to_bed -q` on FASTA files read by the device index: the adversarial files give the
bytes, statuses and -l INFO lines their clean rewrite gives, add_mismatches matches the oracle, and to_bed -q scales with the lines."""
import os
import random
import re
import subprocess

import pytest

import chunk_lib as K
import fasta_corpus as FC
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
FASTA_CMDS = (["add_mismatches"], ["view", "-s"], ["upconvert"])


@pytest.fixture(scope="module", autouse=True)
def built():
    import paffy_amd

    paffy_amd.build_library()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def run(args, data=b"", env=None, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in ("PAFFY_WORKER", "PAFFY_GPUS", "PAFFY_ONE_DEVICE")}
    e.update(env or {})
    p = subprocess.run([PAFFY] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def write(tmp_path, tag, files):
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / ("%s%d.fa" % (tag, k))
        p.write_bytes(f)
        paths.append(str(p))
    return paths


# ---- without a GPU: files are read, and fail, before the GPU is touched ----

@pytest.mark.parametrize("cmd", FASTA_CMDS)
def test_cannot_open(cmd, tmp_path):
    ok = write(tmp_path, "ok", [b">a\nAC\n"])[0]
    missing = str(tmp_path / "no" / "such.fa")
    rc, out, err = run(cmd + ["-l", "INFO", ok, missing])
    assert rc == 1 and out == b""
    assert err == b"Parsing sequence file : %s\nParsing sequence file : %s\npaffy %s: cannot open %s\n" % (ok.encode(), missing.encode(), cmd[0].encode(),
                                                                                                         missing.encode())
    if os.geteuid() != 0:  # root reads any file
        locked = tmp_path / "locked.fa"
        locked.write_bytes(b">a\nAC\n")
        locked.chmod(0)
        rc, out, err = run(cmd + [str(locked)])
        assert rc == 1 and err == b"paffy %s: cannot open %s\n" % (cmd[0].encode(), str(locked).encode())


def test_view_needs_a_file():
    rc, out, err = run(["view"])
    assert rc == 1 and out == b"" and err == b"Expected at least one sequence file\n"


# ---- on the GPU ----

def both(tmp_path, args, files, paf, env=None, stdin=True):
    """(status, stdout, stderr) with the adversarial files and with their clean rewrite"""
    res = []
    for tag, fs in (("adv", files), ("clean", FC.clean(files))):
        paths = write(tmp_path, tag, fs)
        rc, out, err = run(args + paths, paf if stdin else b"", env)
        res.append((rc, out, re.sub(rb"\d+ seconds have elapsed", b"N seconds have elapsed", err.replace(b"/clean", b"/adv"))))
    return res


@pytest.mark.gpu
def test_add_mismatches_and_view(tmp_path):
    files = FC.adversarial()
    paf = FC.paf(files, 2000)
    for args in (["add_mismatches"], ["add_mismatches", "-l", "INFO"], ["view", "-s"], ["view", "-a"], ["view", "-t", "-s"], ["view"]):
        adv, clean = both(tmp_path, args, files, paf)
        assert adv == clean and adv[1], args
        assert adv[0] == 0 or "-s" not in args, args  # without -s the reference's identity assert fails on its zeroed sums
    # -l INFO: every file announced, then the count, before anything else
    rc, out, err = both(tmp_path, ["add_mismatches", "-l", "INFO"], files, paf)[0]
    lines = err.split(b"\n")
    assert [ln.startswith(b"Parsing sequence file : ") for ln in lines[:4]] == [True] * 4
    assert lines[4:7] == [b"Read %d sequences from sequence files" % len(FC.records(files)), b"Input file string : (stdin)",
                          b"Output file string : (stdout)"]
    # the oracle on the records of unique names
    recs = FC.records(files)
    names = [h for h, _ in recs]
    uniq = {h: s for h, s in recs if names.count(h) == 1}
    sub = b"".join(ln + b"\n" for ln in paf.splitlines() if ln.split(b"\t")[0] in uniq and ln.split(b"\t")[5] in uniq)
    want, werr = O.run([O.stage(O.ADD_MISMATCHES)], sub, uniq)
    rc, out, _ = run(["add_mismatches"] + write(tmp_path, "adv", files), sub)
    assert werr.code == 0 and rc == 0 and out == want
    # a record naming no sequence: same status and message
    bad = paf[:2000].rsplit(b"\n", 1)[0] + b"\nnosuch\t10\t0\t5\t+\tlen16\t16\t0\t5\t5\t5\t60\tcg:Z:5M\n"
    adv, clean = both(tmp_path, ["add_mismatches"], files, bad)
    assert adv == clean and adv[0] == 1 and b"No query sequence found" in adv[2]


@pytest.mark.gpu
def test_scaffolds_cli(tmp_path):
    files = FC.scaffolds(200_000)
    paf = FC.paf(files, 5000, seed=5)
    adv, clean = both(tmp_path, ["add_mismatches"], files, paf)
    assert adv == clean and adv[0] == 0


IV = [b">chrA|100000|0\r\n" + b"A" * 600 + b"\n\t" + b"C" * 400 + b"\n>chrA|100000|1000\n" + b"G" * 1000 + b"\n", b"",
      b"x\n>chrA|100000|2000\n" + b"T" * 1000 + b"\n>chrB|50000|10000\n" + b"N" * 10000]


@pytest.mark.gpu
def test_upconvert(tmp_path):
    fasta = [(h, len(s)) for h, s in FC.records(IV)]
    data = b"".join(b"chrA\t100000\t%d\t%d\t+\tchrB\t50000\t%d\t%d\t5\t9\t60\n" % (s, s + 3, t, t + 7) for s, t in ((0, 10000), (1000, 15000), (2500, 3), (1997, 19000)))
    want, fail = K.upconvert(data, fasta)
    assert fail is None
    for args in (["upconvert"], ["upconvert", "-l", "INFO"]):
        adv, clean = both(tmp_path, args, IV, data)
        assert adv == clean and adv[0] == 0 and adv[1] == want
    assert b"Read 4 sequences from sequence files\nInput file string : (stdin)\n" in adv[2]
    # a header that does not decode: the reference's abort, after the count
    bad = IV + [b">plain name\nACGT\n"]
    adv, clean = both(tmp_path, ["upconvert", "-l", "INFO"], bad, data)
    assert adv == clean and adv[0] in (134, -6) and adv[1] == b""
    assert b"Read 5 sequences from sequence files\nInput file string : (stdin)\nOutput file string : (stdout)\nupconvert: " in adv[2]
    # the N-GPU launcher: every worker loads its own copy
    env = {"PAFFY_GPUS": "2", "PAFFY_ONE_DEVICE": "1"}
    assert run(["upconvert"] + write(tmp_path, "adv", IV), data, env)[:2] == (0, want)
    files = FC.adversarial()
    paf = FC.paf(files, 3000, seed=8)
    one = run(["add_mismatches"] + write(tmp_path, "adv", files), paf)
    assert one[0] == 0 and run(["add_mismatches"] + write(tmp_path, "adv", files), paf, env)[:2] == one[:2]


def missing_lines(recs, paf, with_target):
    named = set()
    for ln in paf.split(b"\n"):
        f = ln.split(b"\t")
        if len(f) > 1:
            named.add(f[0])
        if with_target and len(f) > 6:
            named.add(f[5])
    return b"".join(b"%s 0 %d\t0\n" % (h, len(s)) for h, s in recs if h not in named)


@pytest.mark.gpu
def test_to_bed_query_fasta(tmp_path):
    files = [b"".join(FC.adversarial()[:2])]
    paf = FC.paf(files, 40, seed=6, strands=b"+")
    fa = write(tmp_path, "q", files)[0]
    p = tmp_path / "in.paf"
    p.write_bytes(paf)
    beds = []
    for extra in ([], ["-n"]):
        rc0, bed, _ = run(["to_bed", "-f", "-i", str(p)] + extra)
        rc, out, err = run(["to_bed", "-f", "-q", fa, "-i", str(p)] + extra)
        assert rc0 == 0 and rc == 0 and out == bed + missing_lines(FC.records(files), paf, bool(extra))
        assert missing_lines(FC.records(files), paf, bool(extra))
        beds.append(bed)
    # a -q file that cannot be opened adds nothing
    rc, out, _ = run(["to_bed", "-f", "-q", str(tmp_path / "none.fa"), "-i", str(p)])
    assert rc == 0 and out == beds[0]


@pytest.mark.gpu
def test_to_bed_query_fasta_at_scale(tmp_path):
    """50 000 names, 200 000 lines: one lookup per line (the former scan was names x bytes)"""
    rnd = random.Random(12)
    names = [b"seq%d" % i for i in range(50_000)]
    fa = tmp_path / "q.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (n, b"A" * (1 + i % 50)) for i, n in enumerate(names)))
    lines = []
    for _ in range(200_000):
        q, t = rnd.randrange(0, 60_000), rnd.randrange(0, 60_000)
        lines.append(b"seq%d\t100\t0\t10\t+\tseq%d\t100\t0\t10\t10\t10\t60\tcg:Z:10M\n" % (q, t))
    paf = b"".join(lines)
    p = tmp_path / "in.paf"
    p.write_bytes(paf)
    recs = [(n, b"A" * (1 + i % 50)) for i, n in enumerate(names)]
    for extra in ([], ["-n"]):
        rc0, bed, _ = run(["to_bed", "-f", "-i", str(p)] + extra)
        rc, out, _ = run(["to_bed", "-f", "-q", str(fa), "-i", str(p)] + extra, timeout=120)
        assert rc0 == 0 and rc == 0 and out == bed + missing_lines(recs, paf, bool(extra))

"""bin/faffy extract over the device plan: a 3 000-line BED from a file and from stdin, and the two ways a BED line ends the run."""
import os
import random
import subprocess

import pytest

import extract_device_lib as X
import faffy_lib as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAFFY = os.path.join(ROOT, "bin", "faffy")


def faffy(args, stdin=b""):
    p = subprocess.run([FAFFY] + args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout, p.stderr


def bed_lines(n=3000, seed=31):
    rnd = random.Random(seed)
    names = [name for name, ln in X.RECORDS if b" " not in name and ln >= 700]
    lines = []
    for _ in range(n):
        name = rnd.choice(names)
        size = rnd.randrange(20, 400)
        st = rnd.randrange(0, X.LENGTH[name] - size)
        lines.append(b"%s\t%d\t%d\n" % (name, st, st + size))
    return lines


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    p = tmp_path_factory.mktemp("extract") / "g.fa"
    p.write_bytes(X.GENOME)
    return str(p)


def test_bed_from_a_file_and_from_stdin(fasta, tmp_path):
    bed = b"".join(bed_lines())
    want, status, _ = F.extract(X.FILES, bed, 10, 100)
    assert status == 0 and len(X.items(want)) > 20
    (tmp_path / "x.bed").write_bytes(bed)
    rc, out, err = faffy(["extract", fasta, "-i", str(tmp_path / "x.bed")])
    assert rc == 0, err
    assert out == want
    rc, out, err = faffy(["extract", fasta, "-o", str(tmp_path / "o.fa")], stdin=bed)
    assert rc == 0, err
    assert out == b"" and (tmp_path / "o.fa").read_bytes() == want


def test_a_missing_name_on_line_1500(fasta, tmp_path):
    lines = bed_lines()
    lines[1500] = b"chr1_randomly\t5\t500\n"
    bed = b"".join(lines)
    assert F.extract(X.FILES, bed, 10, 100)[1:] == (1, b"Missing sequence: chr1_randomly\n")
    assert X.expected(X.FILES, bed, 10, 100) == (X.MISSING, 1500)
    rc, out, err = faffy(["extract", fasta, "-o", str(tmp_path / "o.fa")], stdin=bed)
    assert rc == 1 and err.endswith(b"Missing sequence: chr1_randomly\n")
    assert out == b"" and (tmp_path / "o.fa").read_bytes() == b""
    want, status, _ = F.extract(X.FILES, bed, 10, 100, skip_missing=True)
    rc, out, err = faffy(["extract", fasta, "-n"], stdin=bed)
    assert rc == 0 and status == 0 and out == want


def test_a_line_of_two_tokens(fasta, tmp_path):
    lines = bed_lines()
    lines[2999] = b"chr1\t5\n"
    bed = b"".join(lines)
    assert F.extract(X.FILES, bed, 10, 100)[1] == 134
    rc, out, err = faffy(["extract", fasta, "-o", str(tmp_path / "o.fa")], stdin=bed)
    assert rc in (134, -6)
    assert out == b"" and (tmp_path / "o.fa").read_bytes() == b""

"""`paffy dechunk` / `paffy upconvert` without a GPU: their option tables (impl/paf_dechunk.c:55-95, impl/paf_upconvert.c:84-111) and the
test-side checker's name decode (decode_fasta_header, impl/paf.c:716-731) against the C library's sscanf."""
import os
import subprocess

import pytest

import chunk_lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")


@pytest.fixture(scope="module", autouse=True)
def built():
    import paffy_amd

    paffy_amd.build_library()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def run(args):
    p = subprocess.run([PAFFY] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("flag", ["-h", "--help"])
def test_dechunk_help(flag):
    rc, out, err = run(["dechunk", flag])
    assert rc == 0 and out == b""
    for opt in (b"--inputFile", b"--query", b"--target"):
        assert opt in err


def test_upconvert_help():
    rc, out, err = run(["upconvert", "-h"])
    assert rc == 0 and out == b"" and b"--inFile" in err


@pytest.mark.parametrize("cmd", ["dechunk", "upconvert"])
def test_bad_flag(cmd):
    rc, out, _ = run([cmd, "-Z"])
    assert rc == 1 and out == b""


def test_upconvert_missing_fasta():
    rc, out, err = run(["upconvert", "/nonexistent/x.fa"])
    assert rc == 1 and out == b"" and b"cannot open" in err


def test_usage_lists_both():
    rc, _, err = run([])
    assert rc == 0
    assert b"not in this build" not in err
    assert b"dechunk" in err and b"upconvert" in err


def test_decode_reference_vector():
    assert K.decode(b"seqname|100|0") == (b"seqname", 0, 100)  # tests/paf_unit_test.c:607-616


@pytest.mark.parametrize("name,want", [
    (b"a|b|100|0", (b"a|b", 0, 100)),
    (b"x|0x10|010", (b"x", 8, 16)),  # %li is base 0: 0x10 = 16, 010 = 8
    (b"x| +5|-3", (b"x", -3, 5)),  # white space and a sign
    (b"100|0", (b"", 0, 100)),  # two tokens: the name is the join of none
    (b"x|12345678901234567890|0", (b"x", 0, 2**63 - 1)),  # out of range: saturates
    (b"x|-99999999999999999999|0", (b"x", 0, -2**63)),
    (b"x|08|0x", (b"x", 0, 0)),  # octal stops at 8; a bare 0x is 0
])
def test_decode_hand_worked(name, want):
    assert K.decode(name) == want


@pytest.mark.parametrize("name", [b"abc", b"5", b"a|5", b"a||5", b"a|x|5", b"a|5|", b"a|5| ", b"a|5|+", b"a|5|x1"])
def test_decode_malformed(name):
    assert K.decode(name) is None


def test_bsearch_probe_order():
    # adjacent extracted intervals share an endpoint (ends are inclusive): the probe order decides which one a start of 100 meets
    tab = K.intervals_of([(b"c|1000|0", 100), (b"c|1000|100", 100), (b"c|1000|200", 100)])
    assert K.bsearch(tab, b"c", 100, 150) == 1  # the middle one is probed first
    assert K.bsearch(tab, b"c", 100, 100) == 1
    tab2 = K.intervals_of([(b"c|1000|0", 100), (b"c|1000|100", 100)])
    assert K.bsearch(tab2, b"c", 100, 150) == 1  # probe 1 first: [100, 200]
    assert K.bsearch(tab2, b"c", 50, 150) == -2  # starts in [0, 100], ends beyond: the assert
    assert K.bsearch(tab2, b"d", 0, 10) == -1
    assert K.bsearch(tab2, b"c", 201, 210) == -1

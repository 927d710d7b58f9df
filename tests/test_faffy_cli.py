"""`faffy` without a GPU: the dispatcher, the option tables, the checks made before the GPU is touched (impl/fasta_chunk.c's directory
checks, the up-front rejection of chunk sizes that give no chunks), and known answers of the checker (tests/faffy_lib.py) worked by
hand from impl/fasta_chunk.c, impl/fasta_extract.c and impl/fasta_merge.c."""
import os
import subprocess

import pytest

import faffy_lib as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAFFY = os.path.join(ROOT, "bin", "faffy")


@pytest.fixture(scope="module", autouse=True)
def built():
    import paffy_amd

    paffy_amd.build_library()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def run(args, cwd=None):
    p = subprocess.run([FAFFY] + args, input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=cwd)
    return p.returncode, p.stdout, p.stderr


def test_no_arguments_is_usage():
    rc, out, err = run([])
    assert rc == 0 and out == b""
    for cmd in (b"chunk", b"merge", b"extract"):
        assert cmd in err


def test_unknown_command():
    rc, out, err = run(["chunky"])
    assert rc == 1 and out == b""
    assert err.startswith(b"chunky is not a valid faffy command\n") and b"extract" in err


@pytest.mark.parametrize("cmd,opts", [("chunk", [b"--chunkSize", b"--overlap", b"--dir", b"--logLevel"]),
                                      ("extract", [b"--bedFile", b"--outputFile", b"--flank", b"--minSize", b"--skipMissing"]),
                                      ("merge", [b"--inputFile", b"--outputFile", b"--logLevel"])])
@pytest.mark.parametrize("flag", ["-h", "--help"])
def test_help(cmd, opts, flag):
    rc, out, err = run([cmd, flag])
    assert rc == 0 and out == b""
    for o in opts:
        assert o in err


@pytest.mark.parametrize("cmd", ["chunk", "extract", "merge"])
def test_bad_flag(cmd):
    rc, out, _ = run([cmd, "-Z"])
    assert rc == 1 and out == b""


def test_chunk_dir_is_a_file(tmp_path):
    f = tmp_path / "plain"
    f.write_bytes(b"x")
    rc, out, err = run(["chunk", "-d", str(f)])
    assert rc == 1 and out == b""
    assert err == b"Output directory is not a directory: " + str(f).encode()  # no newline, as the reference


def test_chunk_dir_not_empty(tmp_path):
    (tmp_path / "old.fa").write_bytes(b">a\nACGT\n")
    rc, out, err = run(["chunk", "-d", str(tmp_path)])
    assert rc == 1 and out == b""
    assert err == b"Output directory is not empty, please specify an empty directory "


@pytest.mark.parametrize("c,o", [("0", "-5"), ("-3", "-10"), ("10", "-11"), ("9223372036854775807", "1")])
def test_chunk_sizes_rejected_up_front(tmp_path, c, o):
    d = tmp_path / "out"
    rc, out, err = run(["chunk", "-c", c, "-o", o, "-d", str(d)])
    assert rc == 1 and out == b"" and b"give no chunks" in err
    assert not d.exists()  # rejected before the directory is made
    assert F.chunk([b">a\nACGT\n"], int(c), int(o))[1] == 1


def test_missing_fasta_is_status_1(tmp_path):
    rc, out, err = run(["extract", "-i", "/dev/null", str(tmp_path / "nope.fa")])
    assert rc == 1 and b"cannot open" in err
    rc, out, err = run(["chunk", "-d", str(tmp_path / "d"), str(tmp_path / "nope.fa")])
    assert rc == 1 and b"cannot open" in err


# ---------------------------------------------------------------- checker known answers


def test_reader_rules():
    text = b"junk\n>r1 x\tz\r\nAC GT\r\r\n\nA\rC\r\n>r2\n>r3\r\nTT"
    assert F.fasta_read(text) == [(b"r1 x\tz", b"ACGTA\rC"), (b"r2", b""), (b"r3", b"TT")]
    # text before the second file's first header does not join the first file's last record
    assert F.fasta_read_files([b">a\nAC", b"GG\n>b\nT\n"]) == [(b"a", b"AC"), (b"b", b"T")]


def test_chunk_packs_short_records():
    # c = 10: "a" (4) and "b" (3) share file 0 (remaining 10 - 4 - 3 = 3 > 0), "c" (5) closes it (3 - 5 <= 0)
    got, st = F.chunk([b">a\nACGT\n>b\nGGG\n>c\nTTTTT\n>d\nA\n"], 10, 2)
    assert st == 0
    assert got == [("./temp_fastas/0.fa", b">a|4|0\nACGT\n>b|3|0\nGGG\n>c|5|0\nTTTTT\n"), ("./temp_fastas/1.fa", b">d|1|0\nA\n")]


def test_chunk_remaining_exactly_zero():
    got, _ = F.chunk([b">a\nACGTA\n>b\nCCCCC\n>c\nG\n"], 10, 0, d="d/")
    assert got == [("d//0.fa", b">a|5|0\nACGTA\n>b|5|0\nCCCCC\n"), ("d//1.fa", b">c|1|0\nG\n")]


@pytest.mark.parametrize("n,want", [
    (4, [b">s|4|0\nACGT\n"]),                              # c
    (3, [b">s|3|0\nACG\n"]),                               # c - 1
    (5, [b">s|5|0\nACGTA\n", b">s|5|4\nA\n"]),             # c + 1: a chunk of c + o = 5, then the last base again from 4
    (0, []),                                                # an empty record writes nothing and opens no file
])
def test_chunk_lengths(n, want):
    seq = b"ACGTA"[:n]
    got, st = F.chunk([b">s\n" + seq + b"\n"], 4, 1)
    assert st == 0
    assert b"".join(b for _, b in got) == b"".join(want)


def test_chunk_overlap_not_below_size_asserts_per_record():
    assert F.chunk([b">a\n\n"], 5, 5)[1] == 134  # fires for an empty record too
    assert F.chunk([b"no header\n"], 5, 5) == ([], 0)  # no record: the run succeeds


def test_chunk_bad_base():
    assert F.chunk([b">a\nACGU\n"], 10, 0)[1] == 134
    assert F.chunk([b">a\nacgtnNTGCA\n"], 10, 0)[1] == 0


def test_merge_split_points():
    # chunks of "AAAACCCCGG" with c = 4, o = 2: [0,6) [4,10) [8,10)
    files = [b">s|10|0\nAAAACC\n>s|10|4\nCCCCGG\n", b">s|10|8\nGG\n"]
    out, st = F.merge(files)
    # split (0 + 6 + 4) / 2 = 5, then (5 + 5 + 8) / 2 = 9
    assert st == 0 and out == b">s\nAAAAC\nCCCG\nG\n"


def test_merge_odd_sum_rounds_down():
    # pending (0, 5 bases), next offset 2: (0 + 5 + 2) / 2 = 3
    out, st = F.merge([b">q|5|0\nABCDE\n>q|6|2\nCDEFGH\n"])
    assert st == 0 and out == b">q\nABC\nDEFGH\n"


def test_merge_headers():
    assert F.merge([b">a|b|0\nAC\n"]) == (b">a\nAC\n", 0)   # name "a|b|0": pop "0" and "b"
    assert F.merge([b">x|0\nAC\n"]) == (b">\nAC\n", 0)      # two tokens: an empty name
    assert F.merge([b">0\nAC\n"])[1] == 134                 # one token: stList_pop of an empty list


def test_merge_errors():
    assert F.merge([b">s|10|4\nAC\n"])[1] == 134                    # no pending sequence
    assert F.merge([b">s|10|0\nAC\n>s|10|5\nAC\n"])[1] == 134       # a gap: 0 + 2 < 5
    assert F.merge([b">s|10|0\nACGTAC\n>s|10|-1\nAC\n"])[1] == 134  # a negative offset
    assert F.merge([b">s|9|0\nACGTACGT\n>s|9|1\nA\n"])[1] == 134    # split 4 lies 3 past the end of a 1-base record


def test_extract_abutting_overlapping_flanks_and_min_size():
    seq = b"ACGT" * 25  # 100 bases
    fa = [b">c\n" + seq + b"\n"]
    # f = 3: [0,10) -> [0,13) clipped at 0; [13,20) -> [10,23) overlaps (13 >= 10): [0,23); [50,60) -> [47,63) new;
    # [95,100) -> [92,100) clipped at 100; [70,72) is under m = 3
    bed = b"c 13 20\nc 0 10\nc\t50\t60\nc 95 100\nc 70 72\n"
    out, st, _ = F.extract(fa, bed, flank=3, min_size=3)
    assert st == 0
    assert out == (b">c|100|0\n" + seq[0:23] + b"\n" + b">c|100|47\n" + seq[47:63] + b"\n" + b">c|100|92\n" + seq[92:100] + b"\n")
    # abutting after the flanks: [20,30) -> [17,33), [36,40) -> [33,43): 33 >= 33 joins them
    out, _, _ = F.extract(fa, b"c 20 30\nc 36 40\n", flank=3, min_size=1)
    assert out == b">c|100|17\n" + seq[17:43] + b"\n"


def test_extract_missing_and_duplicates():
    fa = [b">a\nAAAA\n", b">a\nCCCCCC\n"]
    assert F.extract(fa, b"a 0 2\n", flank=0, min_size=1)[0] == b">a|6|0\nCC\n"  # the last record of a name wins
    assert F.extract(fa, b"a 0 2\nb 0 1\nzz\n", flank=0, min_size=1)[1:] == (1, b"Missing sequence: b\n")
    assert F.extract(fa, b"b 0 1\na 0 2\n", flank=0, min_size=1, skip_missing=True)[:2] == (b">a|6|0\nCC\n", 0)
    assert F.extract(fa, b"a 3 2\n", flank=0, min_size=-5)[1] == 134  # start > end passes m, then the asserts fire

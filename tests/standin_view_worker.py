#!/usr/bin/env python3
"""Stand-in for `bin/paffy_gpu view` in the CPU tests of the N-GPU launcher (tests/test_launcher_view.py): the worker's command line
(`view [options] [-i input] [-o output] fasta...`, parsed with getopt as the worker parses it) and its environment contract --
PAFFY_RANGE="first:end" (it reads only its byte range), PAFFY_VIEW_SUMS=<file> (it leaves seven int64 there when it ends well, the six
sums and its record count, prints no Total-alignments line and runs neither closing assert) -- with the CPU oracle doing the work:
paf_encode_mismatches, paf_pretty_print and paf_stats_calc per record, the reference's float arithmetic for the last line.
Two knobs for the tests: STANDIN_VIEW_DIE_RANK=r (worker r is killed once its output is written, before its sums) and
STANDIN_VIEW_NO_SUMS_RANK=r (worker r ends well without sums). Test infrastructure only."""
import getopt
import math
import os
import signal
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O  # noqa: E402


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def ratio(a, b):  # (float)a / b
    return f32(f32(a) / f32(b)) if b else math.nan


def fmt(x):  # %f as x86-64 glibc prints the NaN of 0.0f / 0.0f
    return "-nan" if math.isnan(x) else "%f" % x


def read_fasta(paths):
    seqs = {}
    for p in paths:
        name, parts = None, []
        with open(p, "rb") as fh:
            for ln in fh.read().splitlines():
                if ln.startswith(b">"):
                    if name is not None:
                        seqs[name] = b"".join(parts)
                    name, parts = ln[1:].split()[0].decode(), []
                else:
                    parts.append(ln.strip())
        if name is not None:
            seqs[name] = b"".join(parts)
    return seqs


def main():
    assert sys.argv[1] == "view", sys.argv
    opts, fasta = getopt.gnu_getopt(sys.argv[2:], "l:i:o:hastu:v:",
                                    ["logLevel=", "inputFile=", "outputFile=", "includeAlignment", "printAggregateStats", "noPerAlignmentStats",
                                     "errorIfIdentityLowerThanX=", "errorIfAlignedBasesLowerThanX=", "help"])
    o = {}
    for k, v in opts:
        o[{"--inputFile": "-i", "--outputFile": "-o", "--includeAlignment": "-a", "--printAggregateStats": "-s", "--noPerAlignmentStats": "-t",
           "--errorIfIdentityLowerThanX": "-u", "--errorIfAlignedBasesLowerThanX": "-v", "--logLevel": "-l"}.get(k, k)] = v
    if not fasta:
        sys.stderr.write("Expected at least one sequence file\n")
        sys.exit(1)
    seqs = read_fasta(fasta)
    data = open(o["-i"], "rb").read() if "-i" in o else sys.stdin.buffer.read()
    rg = os.environ.get("PAFFY_RANGE")
    if rg:
        a, b = (int(x) for x in rg.split(":"))
        data = data[a:b]
    rank = os.environ.get("PAFFY_RANK", "0")
    enc, err = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs)  # everything in front of a failing record
    out = open(o["-o"], "wb") if "-o" in o else sys.stdout.buffer
    tot, n = [0] * 6, 0
    for ln in enc.splitlines(keepends=True):
        f = ln.split(b"\t")
        if "-t" not in o:
            rc, text = O.pretty_print(ln, seqs[f[0].decode()] if "-a" in o else b"", seqs[f[5].decode()] if "-a" in o else b"", "-a" in o)
            assert rc == 0
            out.write(text)
        if b"cg:Z:" in ln:
            tot = O.cigar_stats(ln.split(b"cg:Z:")[1].split(b"\t")[0].strip().decode(), tot, zero=False)
        n += 1
    out.flush()
    if err.code:
        sys.stderr.write("standin view: record %d fails with code %d\n" % (err.record, err.code))
        status = O.lib().po_error_exit_status(err.code)
        if status == 134:
            os.kill(os.getpid(), signal.SIGABRT)
        sys.exit(status or 1)
    if os.environ.get("STANDIN_VIEW_DIE_RANK") == rank:
        os.kill(os.getpid(), signal.SIGKILL)
    sums_path = os.environ.get("PAFFY_VIEW_SUMS")
    if sums_path:
        if os.environ.get("STANDIN_VIEW_NO_SUMS_RANK") != rank:
            with open(sums_path, "wb") as fh:
                fh.write(struct.pack("<7q", *tot, n))
        return
    if "-s" not in o:
        tot = [0] * 6
    m, x, qi, qd, qib, qdb = tot
    if "-s" in o:
        out.write(("Total-alignments:%d\tAvg-Identity:%s\tAvg-Identity-with-gaps:%s\tAligned-bases:%d\tAligned-bases-with-gaps:%d\tQuery-inserts:%d\tQuery-deletes:%d\n"
                   % (n, fmt(ratio(m, m + x)), fmt(ratio(m, m + x + qib + qdb)), m + x, m + x + qib + qdb, qi, qd)).encode())
        out.flush()
    if not (ratio(m, m + x) >= f32(float(o.get("-u", 0)))) or not (m + x >= int(o.get("-v", 0))):
        sys.stderr.write("paffy view: Assertion failed (average identity or aligned bases below the requested minimum)\n")
        sys.stderr.flush()
        os.kill(os.getpid(), signal.SIGABRT)


if __name__ == "__main__":
    main()

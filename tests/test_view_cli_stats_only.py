"""`paffy view` switches the sums-only plan on (paffy_hip_stats_only, paffy_amd/csrc/flat_view_kernel.h) whenever it prints no
base-level rows. Its output may not show it: every form gives the bytes and the status it gives with the flat pass switched off
(PAFFY_NO_FLAT=1: the record kernels' encoder), and both are the oracle's lines in the reference's formats."""
import os
import struct
import subprocess

import pytest

import oracle_lib as O
import synth_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the input files and the oracle's lines: (paf path, fasta path, per-record lines, total line)"""
    d = tmp_path_factory.mktemp("view_cli")
    host = synth_lib.Synth4(0x5EED0004, 2048, n_contigs=6, tlen_min=200_000, tlen_span=200_000)
    data, seqs = host.records(0, 1500), host.genomes()
    paf, fa = d / "in.paf", d / "g.fa"
    paf.write_bytes(data)
    with open(fa, "wb") as fh:
        for name, s in seqs.items():
            fh.write(b">" + name.encode() + b"\n" + s + b"\n")
    enc, err = O.run([O.stage(O.ADD_MISMATCHES)], data, seqs)
    assert err.code == 0
    per, tot = [], [0] * 6
    for ln in enc.splitlines():
        f = ln.split(b"\t")
        m1, x1, i1, d1, ib1, db1 = st = O.cigar_stats(ln.split(b"cg:Z:")[1].split(b"\t")[0].decode())
        tot = [a + b for a, b in zip(tot, st)]
        per.append("Query:%s\tQ-start:%d\tQ-length:%d\tTarget:%s\tT-start:%d\tT-length:%d\tSame-strand:%d\tScore:%d\tIdentity:%f\tIdentity-with-gaps%f"
                   "\tAligned-bases:%d\tQuery-inserts:%d\tQuery-deletes:%d\n"
                   % (f[0].decode(), int(f[2]), int(f[3]) - int(f[2]), f[5].decode(), int(f[7]), int(f[8]) - int(f[7]), 1 if f[4] == b"+" else 0,
                      int([t for t in f if t.startswith(b"AS:i:")][0][5:]), f32(f32(m1) / f32(m1 + x1)), f32(f32(m1) / f32(m1 + x1 + ib1 + db1)), m1 + x1, i1, d1))
    m, x, qi, qd, qib, qdb = tot
    line = ("Total-alignments:%d\tAvg-Identity:%f\tAvg-Identity-with-gaps:%f\tAligned-bases:%d\tAligned-bases-with-gaps:%d\tQuery-inserts:%d\tQuery-deletes:%d\n"
            % (1500, f32(f32(m) / f32(m + x)), f32(f32(m) / f32(m + x + qib + qdb)), m + x, m + x + qib + qdb, qi, qd))
    return str(paf), str(fa), "".join(per), line


def view(case, *flags, no_flat=False, chunk_mb=None):
    env = dict(os.environ)
    env.pop("PAFFY_NO_FLAT", None)
    if no_flat:
        env["PAFFY_NO_FLAT"] = "1"
    if chunk_mb:
        env["PAFFY_CHUNK_MB"] = str(chunk_mb)
    r = subprocess.run([PAFFY, "view", *flags, "-i", case[0], case[1]], capture_output=True, env=env)
    return r.returncode, r.stdout.decode()


# (flags, stdout as (per-record lines?, total line?), exit status): without -s the totals stay zero and the reference's closing assert
# (NaN >= 0) ends the process with SIGABRT after everything is printed
FORMS = [(("-s", "-t"), (False, True), 0), (("-s",), (True, True), 0), ((), (True, False), -6), (("-a", "-t", "-s"), (False, True), 0)]


@pytest.mark.parametrize("flags,shape,status", FORMS, ids=["s_t", "s", "plain", "a_t_s"])
def test_view_prints_the_same_with_and_without_the_flat_pass(case, flags, shape, status):
    want = (case[2] if shape[0] else "") + (case[3] if shape[1] else "")
    got = view(case, *flags)
    ref = view(case, *flags, no_flat=True)
    assert got[0] == ref[0] == status, (got[0], ref[0])
    assert got[1] == ref[1]
    assert got[1] == want


def test_view_in_many_batches(case):
    assert view(case, "-s", chunk_mb=1) == (0, case[2] + case[3])


def test_identity_below_the_minimum_still_aborts_behind_the_total_line(case):
    for no_flat in (False, True):
        assert view(case, "-s", "-t", "-u", "0.995", no_flat=no_flat) == (-6, case[3])

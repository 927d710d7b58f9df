"""`bin/paffy view` prints what it always printed now that its per-record text is written on the GPU (paffy_hip_plan_view_text) and
no longer formatted by the host: the batches of test_gpu_view_text.py -- every rounding case of the two %f fields with the "-nan" records,
every decimal width, names up to 5 000 bytes -- through the CLI in one chunk and in chunks of 1 MiB, against the oracle's
paf_pretty_print of every line and the aggregate line in the reference's float arithmetic."""
import os
import subprocess

import pytest

import oracle_lib as O
from test_gpu_alignment_rows import sequences
from test_gpu_flat import cigar_of
from test_gpu_view_text import name_lines, name_sequences, oracle_text, ratio_lines, row_case, total_line, width_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def write_case(d, lines, seqs):
    paf, fa = d / "in.paf", d / "g.fa"
    paf.write_bytes(b"".join(lines))
    with open(fa, "wb") as fh:
        for name, s in seqs.items():
            fh.write(b">" + name.encode() + b"\n" + s + b"\n")
    return str(paf), str(fa)


def sums_of(lines):
    tot = [0] * 6
    for ln in lines:
        if b"cg:Z:" in ln:
            tot = O.cigar_stats(cigar_of(ln).decode(), tot, zero=False)
    return tot


def view(paf, fa, *flags, chunk_mb=None):
    env = dict(os.environ)
    env.pop("PAFFY_CHUNK_MB", None)
    if chunk_mb:
        env["PAFFY_CHUNK_MB"] = str(chunk_mb)
    r = subprocess.run([PAFFY, "view", *flags, "-i", paf, fa], capture_output=True, env=env, timeout=120)
    return r.returncode, r.stdout, r.stderr[-500:]


def test_view_s_prints_the_oracles_lines(built, tmp_path):
    # no record here has an M op, so add_mismatches reads no base and the sums are those of the cigars as written; the long names
    # make the batch, repeated, pass 1 MiB twice
    lines = ([c[0] for c in ratio_lines()] + width_lines() + name_lines()) * 24
    paf, fa = write_case(tmp_path, lines, name_sequences(lines))
    assert len(b"".join(lines)) > 2 << 20
    want = b"".join(oracle_text(lines)) + total_line(len(lines), sums_of(lines))
    assert want.count(b"Identity:-nan\tIdentity-with-gaps-nan\t") == 24 * (len(width_lines()) + 1)
    for chunk_mb in (None, 1):
        status, out, err = view(paf, fa, "-s", chunk_mb=chunk_mb)
        assert status == 0, err
        assert out == want, chunk_mb


def test_view_a_s_prints_the_oracles_blocks(built, tmp_path):
    lines, blocks, _ = row_case()
    seqs = sequences()
    paf, fa = write_case(tmp_path, lines, seqs)
    enc = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines), seqs)[0].splitlines(keepends=True)
    want = b"".join(blocks) + total_line(len(lines), sums_of(enc))
    for chunk_mb in (None, 1):
        status, out, err = view(paf, fa, "-a", "-s", chunk_mb=chunk_mb)
        assert status == 0, err
        assert out == want, chunk_mb

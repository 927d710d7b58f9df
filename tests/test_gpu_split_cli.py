"""`bin/paffy split_file` over the library's group table (one fwrite per group and chunk): many interleaved names over several chunks
against the oracle's directory, and a failing record in a later chunk."""
import os
import subprocess

import pytest

import oracle_lib as O
from test_cli import PAFFY

pytestmark = pytest.mark.gpu

CIGAR = "1M1X" * 130  # 520 bytes: 2 400 lines make about 1.4 MiB, two chunks under PAFFY_CHUNK_MB=1
N_NAMES, ROUNDS = 300, 8


@pytest.fixture(scope="module", autouse=True)
def built():
    import paffy_amd

    paffy_amd.build_library()
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "host"), "-s"])


def line(i):
    """Line i: query q<i % 300> and target t<(7 i) % 300>, so that neither side's groups are contiguous; lengths from 50 to 349."""
    q, t = i % N_NAMES, (7 * i) % N_NAMES
    return f"q{q}\t{50 + q}\t0\t260\t+\tctg/{t}\t{50 + t}\t0\t260\t130\t260\t60\tAS:i:{i}\tcg:Z:{CIGAR}\n".encode()


LINES = [line(i) for i in range(N_NAMES * ROUNDS)]


def read_dir(d):
    out = {}
    for n in sorted(os.listdir(d)):
        with open(os.path.join(d, n), "rb") as fh:
            out[n] = fh.read()
    return out


def run_split(args, data, prefix):
    env = dict(os.environ)
    env["PAFFY_CHUNK_MB"] = "1"
    return subprocess.run([PAFFY, "split_file", "-p", prefix] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


@pytest.mark.parametrize("args,kw", [([], dict()), (["-q"], dict(by_query=True)), (["-m", "200"], dict(min_length=200)), (["-q", "-m", "123"], dict(by_query=True, min_length=123))],
                         ids=["default", "q", "m", "q_m"])
def test_many_interleaved_names_over_chunks(tmp_path, args, kw):
    data = b"".join(LINES)
    assert len(data) > (1 << 20) + 100000
    want_dir, got_dir = tmp_path / "want", tmp_path / "got"
    want_dir.mkdir()
    got_dir.mkdir()
    assert O.split_file(data, str(want_dir) + "/s_", **kw).code == 0
    p = run_split(args, data, str(got_dir) + "/s_")
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    want = read_dir(want_dir)
    assert len(want) >= 150 and read_dir(got_dir) == want


def test_opened_lines_come_in_opening_order(tmp_path):
    """-l INFO: one "Opened output file" line per file, in the order of the files' first lines."""
    data = b"".join(LINES[:40])
    p = run_split(["-l", "INFO"], data, str(tmp_path) + "/s_")
    assert p.returncode == 0, p.stderr
    opened = [ln.split(b"Opened output file: ", 1)[1] for ln in p.stderr.splitlines() if b"Opened output file: " in ln]
    assert opened == [f"{tmp_path}/s_ctg_{(7 * i) % N_NAMES}.paf".encode() for i in range(40)]


def test_a_failing_record_in_the_second_chunk(tmp_path):
    from paffy_amd.engine import lib

    bad_at = 2000  # about 1.2 MB in: the second chunk
    assert len(b"".join(LINES[:bad_at])) > (1 << 20) + 50000
    data = b"".join(LINES[:bad_at]) + b"q\t100\t0\t5\t+\tt\t100\t0\t5\t5\n" + b"".join(LINES[bad_at:])
    want_dir, got_dir = tmp_path / "want", tmp_path / "got"
    want_dir.mkdir()
    got_dir.mkdir()
    err = O.split_file(data, str(want_dir) + "/s_")
    assert err.code != 0 and err.record == bad_at
    p = run_split([], data, str(got_dir) + "/s_")
    L = lib()
    status = L.paffy_hip_error_exit_status(err.code)
    assert p.returncode == {134: -6, 139: -11}.get(status, status or 1), p.stderr
    assert p.stdout == b""
    assert p.stderr == b"%s (record %d)\n" % (L.paffy_hip_error_string(err.code), bad_at)
    assert read_dir(got_dir) == read_dir(want_dir)

"""Shatter records with short names (chr1, 2L, q) on the one-wave row writer: a first constant row piece `qname \\t qlen \\t` (piece A) of 4
to 15 bytes is written by k_emit_rows_short (RecPlan flag bit 23 in place of bit 6), which composes the first 16 bytes of every row
from A, `q0 \\t`, `q1`, B and `t0 \\t`. Every test compares error code, length and SHA-256 of the whole output with the oracle's, pipe by
pipe; tests/test_short_names_cpu.py proves on the oracle alone that the inputs (tests/short_name_cases.py) reach every head shape."""
import hashlib
import os
import subprocess
import sys

import pytest

import oracle_lib as O
import short_name_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
PIPES = ([O.SHATTER], [O.INVERT, O.SHATTER], [O.INVERT, O.TRIM_IDENTITY, O.SHATTER], [O.INVERT, O.INVERT, O.SHATTER])
ROWS, ROWS_SHORT, SEGMENTS = 1 << 6, 1 << 23, 1 << 19  # RecPlan.flags, record_types.h: k_emit_rows, k_emit_rows_short, EmitItem segments
WHY_ROW_SHAPE = 8  # FLAT_WHY_ROW_SHAPE of flat_kernel.h


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def run_both(eng, lines, pipes=PIPES, kept=False):
    """every pipe against the oracle; returns per pipe (records the flat pass left, reasons, RecPlan flags of the records)"""
    import paffy_amd

    data = "".join(lines).encode()
    res = []
    for pipe in pipes:
        want, werr = O.run([O.stage(k) for k in pipe], data)
        got, info = eng.run([paffy_amd.stage(k) for k in pipe], data, raise_on_error=False)
        left, why = eng.flat_stats()
        flags, _ = eng.record_layout(0, len(lines))
        print("pipe", pipe, "left", left, "why", list(why), "short", sum(1 for f in flags if f & ROWS_SHORT), "of", len(lines))
        assert info.error.code == werr.code == 0, (pipe, info.error.code, werr.code, info.error.record, werr.record)
        assert len(got) == len(want) and hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest(), (pipe, len(got), len(want), first_difference(got, want))
        if kept:
            assert left == 0, (pipe, left, list(why))
        res.append((left, why, flags))
    return res


def first_difference(got, want):
    for k, (a, b) in enumerate(zip(got.splitlines(), want.splitlines())):
        if a != b:
            return k, a[:80], b[:80]
    return None


def check_bits(lines, pipe, flags):
    """bit 23 exactly where the piece A the writer sees (the target side behind an odd number of inverts) is shorter than 16 bytes, bit 6 elsewhere"""
    inverted = sum(1 for k in pipe if k == O.INVERT) % 2 == 1
    for line, f in zip(lines, flags):
        want = ROWS_SHORT if S.piece_a_len(line, inverted) < 16 else ROWS
        assert f & (ROWS | ROWS_SHORT) == want, (pipe, line[:60], hex(f))


def test_every_piece_a_length_on_both_sides(eng):
    """piece A of 4 to 17 bytes on the query and on the target side, chosen independently, both strands, 1 to 300 ops (a window is 128 ops):
    the flat pass keeps every record, and the records go to the two row kernels by the piece A the writer sees"""
    lines = S.len_a_grid()
    for pipe, (left, why, flags) in zip(PIPES, run_both(eng, lines, kept=True)):
        check_bits(lines, pipe, flags)


def test_heads_that_reach_into_b_and_t0(eng):
    """one- and two-character names with one-digit lengths, coordinates from 0 and ranges that gain a digit inside a window, far windows
    (M ops of 4 000 to 8 191) and M lengths of 100 and more; whoever sized a record (many powers of ten inside a range leave the flat
    pass for the record kernels), the short row kernel writes it"""
    lines = S.deep_heads()
    for pipe, (left, why, flags) in zip(PIPES, run_both(eng, lines)):
        check_bits(lines, pipe, flags)


def test_two_rows_in_one_lane(eng):
    lines = S.two_rows_in_a_lane()
    for pipe, (left, why, flags) in zip(PIPES, run_both(eng, lines)):
        check_bits(lines, pipe, flags)


def test_the_record_kernels_sizing(eng):
    """a short-named record the flat pass leaves (one op of 8 192 bases) gets bit 23 from the record kernels; and the whole batch under
    PAFFY_NO_FLAT=1 (read once per process: a fresh child process), where the record kernels size everything"""
    lines = S.one_long_op() + S.named_checked()
    (left, why, flags), = run_both(eng, lines, pipes=([O.SHATTER],))
    assert left == 2 and all(f & ROWS_SHORT and not f & ROWS for f in flags[:3]), (left, [hex(f) for f in flags[:3]])
    check_bits(lines, [O.SHATTER], flags)
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r); import paffy_amd; e = paffy_amd.Engine();"
            "d = sys.stdin.buffer.read(); n = d.count(b'\\n');"
            "got, _ = e.run([paffy_amd.stage(paffy_amd.INVERT), paffy_amd.stage(paffy_amd.TRIM_IDENTITY), paffy_amd.stage(paffy_amd.SHATTER)], d);"
            "print(hashlib.sha256(got).hexdigest(), e.flat_stats()[0], ' '.join('%%x' %% f for f in e.record_layout(0, n)[0]))") % (ROOT, here)
    data = "".join(lines).encode()
    out = subprocess.run([sys.executable, "-c", code], input=data, env=dict(os.environ, PAFFY_NO_FLAT="1"), capture_output=True, check=True).stdout.split()
    want, werr = O.run([O.stage(O.INVERT), O.stage(O.TRIM_IDENTITY), O.stage(O.SHATTER)], data)
    assert werr.code == 0 and out[0].decode() == hashlib.sha256(want).hexdigest()
    assert int(out[1]) != 0  # no flat pass ran (-1), or it kept nothing
    check_bits(lines, [O.INVERT, O.TRIM_IDENTITY, O.SHATTER], [int(x, 16) for x in out[2:]])


def test_neighbours_of_the_other_kernel(eng):
    lines = S.neighbours()
    for pipe, (left, why, flags) in zip(PIPES, run_both(eng, lines, kept=True)):
        check_bits(lines, pipe, flags)
        assert 0 < sum(1 for f in flags if f & ROWS_SHORT) < len(lines)


def test_the_short_kernel_is_launched_only_when_needed(eng):
    import paffy_amd

    long_named = [S.record([(5, "M"), (1, "I"), (7, "M")], "+-"[k & 1], "hs.chr3", "pt.chr9", qs=1000 + k, ts=2000 + k) for k in range(40)]
    try:
        for lines, launches in ((long_named, 0), (long_named[:20] + [S.record([(5, "M"), (1, "D"), (7, "M")])] + long_named[20:], 1)):
            eng.profile(True)
            got, _ = eng.run([paffy_amd.stage(paffy_amd.SHATTER)], "".join(lines).encode())
            prof = eng.profile_read()
            assert got == O.run([O.stage(O.SHATTER)], "".join(lines).encode())[0]
            assert prof["k_emit_rows"][1] == 1, prof
            assert prof.get("k_emit_rows_short", (0, 0))[1] == launches, prof
    finally:
        eng.profile(False)


def test_segmented_records_keep_the_gate(eng):
    """the stated limit: a chr1 record of 32 768 ops (PAFFY_ROWS_MAX_OPS) stays with the flat pass and the short kernel, one of 32 769 ops
    would be written as segments and leaves with FLAT_WHY_ROW_SHAPE"""
    import random

    rng = random.Random(2307)
    for n, stays in ((32_768, True), (32_769, False)):
        ops = S.alternating_ops(rng, n, (1, 5, 30, 60), indel=(1, 2))
        ops[-1] = (3, "M")
        assert len(ops) == n
        lines = [S.record(ops, "+", qs=120_000_000, ts=110_000_000), S.record([(5, "M")], "-")]
        for pipe, (left, why, flags) in zip(PIPES[:2], run_both(eng, lines, pipes=PIPES[:2])):
            if stays:
                assert left == 0 and flags[0] & ROWS_SHORT and not flags[0] & (ROWS | SEGMENTS), (n, pipe, left, hex(flags[0]))
            else:
                assert left == 1 and why[WHY_ROW_SHAPE] == 1 and not flags[0] & (ROWS | ROWS_SHORT | SEGMENTS), (n, pipe, left, list(why), hex(flags[0]))


def test_command_line(tmp_path, human_chimp):
    """tests/golden/human_chimp.paf with chr10 renamed to chr1 (a 15-byte piece A) through bin/paffy shatter, on one GPU and as two parts"""
    data = human_chimp.replace(b"chr10", b"chr1")
    assert data != human_chimp
    want, werr = O.run([O.stage(O.SHATTER)], data)
    assert werr.code == 0 and any(S.head_pieces(r)[0] == 15 for r in want.splitlines())
    src = tmp_path / "in.paf"
    src.write_bytes(data)
    for k, env in enumerate((dict(os.environ), dict(os.environ, PAFFY_GPUS="2", PAFFY_ONE_DEVICE="1"))):
        env.pop("PAFFY_GPUS", None) if k == 0 else None
        dst = tmp_path / ("out%d.paf" % k)
        p = subprocess.run([PAFFY, "shatter", "-i", str(src), "-o", str(dst)], env=env, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert dst.read_bytes() == want

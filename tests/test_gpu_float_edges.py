"""The float32 threshold decisions of the port at ties, one float32 step to either side, near the edges of the 4e-6 band of
flat_ratio_lt / flat_ratio_ge, and with sums above 2^24 where the conversions round: error code, length and SHA-256 of the whole output
against the oracle (run_both of test_gpu_flat.py). The records are float_edges.py's; test_float_edges_cpu.py proves on the oracle alone
that every family is sharp -- the record one step on the wrong side comes out differently -- so none of this passes vacuously.

Every identity-trim set is built to reach one of the five implementations, and every record asserts which one took it. The flat pass
keeps every record (flat_stats left 0); under [TRIM_IDENTITY, SHATTER] RecPlan flag bit 21 (FLAT_F_ROW_PIECES) is set by k_flat_lane
alone, so record_layout tells lane_trim_prefix (at most 12 pieces and a cut within the lane's walk budget) from k_flat_size's
flat_trim_prefix, whose summaries are in registers up to 64 pieces and in HBM above (piece counts from the batch's offsets). One op of
8 192 sends every record to the record kernels with 32-bit sums (left = all, FLAT_WHY_IRREG, 4-byte words); ops just under 2^29 with
sums of 2^35 take the 64-bit trim over 4-byte ops, one op above 2^29 the arena's 8-byte ops.
Above 2^24 the lane kernel decides only ties and misses: a hit there lies behind 2 049 ops at least (8 191 bases an op), the suffix
search alone is beyond the lane's budget, and the record goes to k_flat_size (lt_above_small asserts exactly that)."""
import hashlib
import re

import numpy as np
import pytest

import float_edges as E
import oracle_lib as O
from test_gpu_flat import STATS, run_both
from test_gpu_flat import eng  # noqa: F401  (the module's engine)

pytestmark = pytest.mark.gpu

WHY_IRREG = 1  # FLAT_WHY_IRREG of flat_kernel.h
MIRROR_BITS, HALF = 0x60000, 0x40000  # RecPlan.flags, record_types.h: how the ops are kept (HALF: 2-byte words)
KLASS_LDS, KLASS_ARENA = 0, 1
STATS_STAGE = 10  # PAFFY_STATS
TRIM_PIPES = ([O.TRIM_IDENTITY], [O.INVERT, O.TRIM_IDENTITY], [O.TRIM_IDENTITY, O.SHATTER])
NO_SHATTER = {"lt_regs", "lt_hbm"}  # a million rows and more: lt_regs_rows and lt_hbm_rows are their subsets for the row writer


def layout(eng, pipe, params, data, n):
    """(flags, classes) of the records under this pipe"""
    import paffy_amd

    d_in = eng.to_device(data)
    info = eng.plan([paffy_amd.stage(k, *params.get(k, ())) for k in pipe], d_in, len(data))
    assert info.error.code == 0 and info.n_records == n
    return eng.record_layout(0, n)


@pytest.mark.parametrize("name", sorted(E.TRIM_SETS))
def test_identity_trim_at_the_thresholds(eng, name):
    """q < thr (the last hit wins: probes alone and behind an early hit, early in the record, last op of a piece, first op of the next,
    behind a run of a hundred D ops that spans a 64-op step of the wave's walk and the lane's blocks of eight, in a later piece),
    q >= id (the suffix search) and max_trim, on both strands, the probe at the front and at the back of the text"""
    batch, cut, params, who = E.trim_set(name)
    data, n = batch.data(), len(batch.lines)
    p = {O.TRIM_IDENTITY: params}
    pipes = tuple(pp for pp in TRIM_PIPES if O.SHATTER not in pp or name not in NO_SHATTER)
    if who in ("flat", "lane", "regs", "hbm"):
        run_both(eng, data, pipes=pipes, params=p, kept=True)
        pieces = E.pieces_of(batch)
        lo, hi = {"lane": (1, 12), "regs": (13, 64), "hbm": (65, 1 << 20)}.get(who, (1, 1 << 20))
        assert lo <= min(pieces) and max(pieces) <= hi
        flags, klass = layout(eng, TRIM_PIPES[0], p, data, n)
        assert all(k == KLASS_LDS for k in klass) and all(f & MIRROR_BITS == HALF for f in flags), [hex(f) for f in flags[:4]]
        # which of the two flat kernels decided each record's trim (the plan alone: no row is written)
        flags, _ = layout(eng, TRIM_PIPES[2], p, data, n)
        want = E.sized_by_lane(batch, cut)
        assert eng.flat_stats()[0] == 0 and [bool(f & E.LANE_BIT) for f in flags] == want
        assert who != "lane" or all(want)
        assert who not in ("regs", "hbm") or not any(want)
    elif who == "irreg":
        run_both(eng, data, pipes=pipes, params=p, want_left=(n, WHY_IRREG))
        flags, klass = layout(eng, TRIM_PIPES[0], p, data, n)
        assert all(k == KLASS_LDS for k in klass) and all(f & MIRROR_BITS == 0 for f in flags), [hex(f) for f in flags[:4]]
    else:
        run_both(eng, data, pipes=pipes, params=p)
        assert all(left == n for _, _, (left, _) in STATS[-len(pipes):])
        flags, klass = layout(eng, TRIM_PIPES[0], p, data, n)
        if who == "wide":
            assert all(k == KLASS_LDS for k in klass) and all(f & MIRROR_BITS == 0 for f in flags), [hex(f) for f in flags[:4]]
        else:
            assert all(k == KLASS_ARENA for k in klass)


def test_fixed_trim_above_2_24(eng):
    """end = (int64)((double)((float)aligned * fraction) / 2) with aligned above 2^24: odd values whose conversion rounds, both strands,
    records the wave kernel sizes from summaries in registers and in HBM, and the same through the record kernels (one op of 8 192;
    single ops of millions of bases)"""
    flat, irreg, wide = E.Batch(), E.Batch(), E.Batch()
    for aligned in E.FIXED_ALIGNED:
        for strand in "+-":
            flat.add(E.line_of(E.fixed_ops(aligned, 6000 if aligned > 50_000_000 else E.OP_MAX), strand))
            irreg.add(E.line_of(E.fixed_ops(aligned, irregular=8192), strand))
            wide.add(E.line_of(E.fixed_ops(aligned, E.BIG), strand))
    pieces = E.pieces_of(flat)
    assert min(pieces) <= 12 < 64 < max(pieces)
    pipes = ([O.TRIM_FIXED], [O.INVERT, O.TRIM_FIXED])
    for frac in E.FIXED_FRACTIONS:
        p = {O.TRIM_FIXED: (0.05, frac)}
        run_both(eng, flat.data(), pipes=pipes, params=p, kept=True)
        run_both(eng, irreg.data(), pipes=pipes, params=p, want_left=(len(irreg.lines), WHY_IRREG))
        run_both(eng, wide.data(), pipes=pipes, params=p, want_left=(len(wide.lines), WHY_IRREG))


def filtered(eng, data, n_left, tag, **thresholds):
    """the filter pipes under these thresholds; tag keeps the oracle's cached digests of run_both apart (the thresholds are no stage
    parameters); n_left: records the flat pass leaves (0: it keeps every one)"""
    O.set_filter(**thresholds)
    eng.set_filter(**thresholds)
    try:
        pipes = ([O.FILTER], [O.INVERT, O.FILTER])
        if n_left:
            run_both(eng, data, pipes=pipes, params={"filter": tag}, want_left=(n_left, WHY_IRREG))
        else:
            run_both(eng, data, pipes=pipes, params={"filter": tag}, kept=True)
        # behind the filter a record of I ops alone fails the trim's own assert (0 / 0): whoever sizes it, the error is the oracle's
        run_both(eng, data, pipes=([O.FILTER, O.TRIM_IDENTITY],), params={"filter": tag})
    finally:
        O.set_filter()
        eng.set_filter()


@pytest.mark.parametrize("wide", [False, True])
def test_filter_at_the_thresholds(eng, wide):
    """k = (10 - k) X against min_identity k / 10 and the same quotients through I and D bases against min_identity_with_gaps: the
    float32 quotient widened lies above the double for some k and below it for others; thresholds on the float32 quotient itself and
    one double above it, sums above 2^24; a record of I ops alone; with and without invert. Sized by the flat pass, and (wide: single
    ops, a leading zero) by the record kernels."""
    cases = E.filter_lines(E.TENTHS, wide)
    data = "".join(c[0] for c in cases).encode() + E.record(E.ONLY_INSERTS, qname="only_i").encode()
    for k in range(1, 10):
        for inv in (False, True):
            filtered(eng, data, len(cases) if wide else 0, ("tenth", k, inv), min_identity=k / 10, min_identity_with_gaps=k / 10, invert=inv)
    big = E.filter_lines(E.FILTER_BIG, wide)
    bdata = "".join(c[0] for c in big).encode()
    for m, x in E.FILTER_BIG:
        t0 = float(E.quot(m, m + x))
        for thr in (t0, float(np.nextafter(t0, 2.0))):
            for inv in (False, True):
                filtered(eng, bdata, len(big) if wide else 0, ("big", thr, inv), min_identity=thr, min_identity_with_gaps=thr, invert=inv)
            filtered(eng, bdata, len(big) if wide else 0, ("gaps", thr), min_identity_with_gaps=thr)


@pytest.mark.parametrize("trim", E.CHAIN_TRIMS)
def test_chain_trim_decides_by_one_base(eng, trim):
    """(int64)((float)length * trim) / 2 with lengths whose conversion rounds: of three pairs per length only the one whose B starts
    exactly on A's trimmed end chains; A stands in front of B in the input (no candidate is seen through a fresh iterator)"""
    for strand in "+-":
        data, pairs = E.chain_lines(trim, strand)
        want, err, fresh = O.chain(data, trim=trim)
        assert err.code == 0 and fresh == 0
        got, info = eng.chain(data, trim=trim)
        assert got == want, (trim, strand)
        assert got.count(b"s1:i:150") == 2 * len(E.CHAIN_LENGTHS)


def test_view_ratios_above_2_24(eng):
    """the view's two %f fields for match and total sums above 2^24 and odd (both conversions round): the GPU's lines are the oracle's"""
    import paffy_amd

    cases = E.view_lines()
    lines = [c[0] for c in cases]
    want = []
    for ln in lines:
        rc, text = O.pretty_print(ln, b"", b"", False)
        assert rc == 0
        want.append(text)
    data = b"".join(lines)
    d_in = eng.to_device(data)
    info = eng.plan([paffy_amd.stage(STATS_STAGE, 0.0, 0.0)], d_in, len(data))
    assert info.error.code == 0 and info.n_records == len(lines)
    sizes = eng.view_sizes(0, len(lines))
    assert sizes == [len(w) for w in want]
    whole = eng.view_text(0, len(lines), guard=256)
    assert hashlib.sha256(whole).hexdigest() == hashlib.sha256(b"".join(want)).hexdigest()
    for g, (ln, ident, gaps) in zip(whole.splitlines(), cases):
        m = re.search(rb"\tIdentity:([^\t]+)\tIdentity-with-gaps([^\t]+)\t", g)
        assert (m.group(1).decode(), m.group(2).decode()) == (ident, gaps), (ln[:60], g)

"""Stage lists with a fixed trim (`paffy trim -f`) at any place, sized by the flat pass (k_flat_size<2>, FlatCuts of flat_kernel.h):
pipe by pipe against the oracle -- the error code and record, the output's length, its SHA-256 -- and then who sized the records
(Engine.flat_stats). The inputs are fixed_pipe_lib's; test_flat_fixed_pipe_cpu.py shows on the oracle that they hit their cases."""
import pytest

import chunk_lib as K
import fixed_pipe_lib as L
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def regular():
    data = L.regular_batch()
    return data, K.chunk_encode(data)


def test_who_sized_it(eng, regular):
    """every pipe of the table on a batch of regular records, both strands, every fraction: the flat pass keeps every record (at the
    parent commit flat_stats gives -1 for each of them). With a shatter behind the trim the record kernels size the batch as before.
    Then pipes without a fixed trim, and with it last, on the same engine: nothing of a plan is left over."""
    data, chunked = regular
    with L.Thresholds(eng, min_identity_with_gaps=0.95):
        for frac in L.FRACTIONS:
            for name, pipe in L.PIPES.items():
                left, why = L.check(eng, pipe, frac, chunked if L.DECHUNK in pipe else data, tag="gaps95")
                assert left == 0, (name, frac, left, list(why))
        for name, pipe in L.SHATTER_PIPES.items():
            left, why = L.check(eng, pipe, 0.1, data, tag="gaps95")
            assert left == -1, (name, left)
        for pipe in ([L.INV], [L.FIX], [L.FIX, L.INV], [L.TRI, L.SHA], [L.FIX, L.TRI]):
            left, why = L.check(eng, pipe, 0.1, data, tag="gaps95")
            assert left == 0, (pipe, left, list(why))


@pytest.mark.parametrize("frac", sorted({f for _, f in L.LANDINGS.values()}))
def test_where_the_cuts_land(eng, frac):
    """a cut inside the first and the last op, on an op boundary with an indel next, both cuts in one op, shortened ops that lose a
    digit, and 0 to 17 bytes of text between the two rewritten end ops: in front of an invert, a filter, the stats stage and a pass"""
    _, lines = L.landing_batch(frac)
    data = "".join(lines).encode()
    for name in L.LANDING_PIPES:
        left, why = L.check(eng, L.PIPES[name], frac, data)
        assert left == 0, (name, left, list(why))


def test_a_second_fixed_trim(eng):
    """the second cut ends inside the op the first one shortened, consumes it exactly, consumes it and stops in the next match op;
    the same with an invert between the two trims"""
    _, lines = L.second_batch()
    data = "".join(lines).encode()
    for name in L.SECOND_PIPES + ("fix_trim_fix",):
        left, why = L.check(eng, L.PIPES[name], 0.1, data)
        assert left == 0, (name, left, list(why))


@pytest.mark.parametrize("frac", L.TRIM_FRACTIONS)
def test_identity_trim_behind_a_fixed_trim(eng, frac):
    """noisy-ended records whose identity trim removes the shortened op and more, removes it only because it is shortened, at the
    front and (the second pass of a '-' record) at the back; a shortened X op"""
    _, lines = L.trim_batch(frac)
    data = "".join(lines).encode()
    plain = b"X" not in b"".join(L.cigar_of(ln.encode()) for ln in lines)  # (the stats stage leaves a record with X ops to the record kernels)
    for name in L.TRIM_PIPES + (("trim_fix_invert_stats",) if plain else ()):
        left, why = L.check(eng, L.PIPES[name], frac, data)
        assert left == 0, (name, left, list(why))


@pytest.mark.parametrize("n_ops,what", [(30_001, "pieces"), (50_001, "segments")])
def test_long_records(eng, n_ops, what):
    """a record of more than 64 pieces (its summaries are scanned in HBM), and one with more than 32 768 ops left in the window (written
    as segments), both strands"""
    lines = [L.long_record(n_ops, s, 7305 + i) for i, s in enumerate(L.STRANDS)]
    data = "".join(lines).encode()
    if what == "pieces":
        assert all(len(L.cigar_of(ln.encode())) > 64 * 1024 for ln in lines)
    for name in ("fix_invert", "fix_trim", "fix_fix"):
        left, why = L.check(eng, L.PIPES[name], 0.1, data)
        assert left == 0, (name, left, list(why))
        if what == "segments":
            _, _, want = L.expected(L.PIPES[name], 0.1, data)
            assert all(len(L.ops_of(ln)) > 32768 for ln in want.splitlines())


def test_who_leaves(eng):
    """what the flat pass hands to the record kernels, counted exactly; bytes and errors are the oracle's"""
    even = L.even_batch()
    n = even.count(b"\n")
    for name in ("fix_invert", "fix_trim", "fix_stats"):
        left, why = L.check(eng, L.PIPES[name], 1.0, even)
        assert left == n and why[L.WHY_EMPTY] == n and sum(why) == n, (name, left, list(why))
    left, why = L.check(eng, L.PIPES["fix_invert"], 1.5, even)
    assert left == n and why[L.WHY_STAGE] == n and sum(why) == n, (left, list(why))
    left, why = L.check(eng, L.PIPES["fix_invert_fix"], 0.1, L.irregular_batch())
    assert left == 1 and why[L.WHY_IRREG] == 1 and sum(why) == 1, (left, list(why))
    data, n_np = L.nonplain_batch()
    left, why = L.check(eng, L.PIPES["fix_stats"], 0.1, data)
    assert left == n_np and why[L.WHY_NONPLAIN] == n_np and sum(why) == n_np, (left, list(why))


@pytest.mark.parametrize("name", sorted(L.TIES))
def test_filter_at_a_tie_behind_the_trim(eng, name):
    """min_identity on the float32 identity of the trimmed window and one float32 step to either side; records with X ops, one of
    them shortened; plain and inverted"""
    thr, _ = L.tie_thresholds(name)
    data = "".join(L.tie_batch(name)).encode()
    for u, t in thr:
        for inv in (False, True):
            with L.Thresholds(eng, min_identity=t, invert=inv):
                left, why = L.check(eng, L.PIPES["fix_filter"], 0.1, data, tag=("tie", u, inv))
                assert left == 0, (u, inv, left, list(why))
                wcode, _, want = L.expected(L.PIPES["fix_filter"], 0.1, data, tag=("tie", u, inv))
                assert wcode == 0 and want.count(b"\n") == (2 if (u <= 0) != inv else 0)

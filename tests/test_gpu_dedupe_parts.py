"""Dedupe in parts (include/paffy_hip.h): `paffy dedupe [-a]` sharded by key owner. For any number of parts and any cut of the input into
rounds of consecutive shares, the parts' outputs in part order, round by round, are byte for byte what one context writes for the whole
input (Engine.dedupe), which in turn is what the oracle's po_dedupe writes; the same failing record is reported."""
import ctypes as C
import random

import pytest
import torch

import dedupe_streams as S
import oracle_lib as O
from paffy_amd import engine, shard

pytestmark = pytest.mark.gpu
PARTS = (1, 2, 3, 5)
E_CAPACITY, E_STATE = -4, -5
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def engines():
    import paffy_amd

    es = [paffy_amd.Engine() for _ in range(max(PARTS) + 1)]  # the last one runs the whole input
    yield es
    for e in es:
        e.close()


def tobytes(t):
    return bytes(t.cpu().numpy().tobytes())


_whole = {}


def whole_run(engines, data, inv):
    """one context on the whole input == the oracle (computed once per input and mode)"""
    if (data, inv) not in _whole:
        got, info = engines[-1].dedupe(data, inv, raise_on_error=False)
        want, werr = O.dedupe(data, inv)
        assert got == want and info.error.code == werr.code
        err = None
        if werr.code:
            assert info.error.record == werr.record
            err = {"code": info.error.code, "stage": info.error.stage, "record": info.error.record, "aux": info.error.aux}
        _whole[data, inv] = (got, err)
    return _whole[data, inv]


def parts_run(engines, rounds, inv):
    """rounds: [[bytes per part] per round] -> (output bytes, error, result)"""
    k = len(rounds[0])
    workers = [shard.GpuDedupeWorker(e) for e in engines[:k]]
    res = shard.dedupe_in_parts(workers, [[(engines[p].to_device(b), len(b)) for p, b in enumerate(rnd)] for rnd in rounds], inv)
    return tobytes(res["out"]), res["error"], res


def check(engines, lines, ks=PARTS, n_rounds=(1,), modes=(False, True), seed=1):
    data = b"".join(lines)
    for inv in modes:
        want, werr = whole_run(engines, data, inv)
        for k in ks:
            for r in n_rounds:
                out, err, res = parts_run(engines, S.cut(random.Random(seed * 100 + k * 10 + r), lines, r, k), inv)
                assert out == want, (k, r, inv)
                assert err == werr, (k, r, inv)
                if not werr:
                    assert res["records"] == len(lines)


@pytest.mark.parametrize("n", [0, 1, 4, 7, 300, 5000])
def test_random_streams_from_small_pools(engines, n):
    """fewer records than parts, more than one workgroup (256 records each), more than one wave per owner; runs of duplicates straddle
    the parts"""
    lines = S.stream(random.Random(500 + n), n, pool_size=60 if n < 1000 else 400)
    check(engines, lines, seed=n)
    if n >= 300:
        want, _ = whole_run(engines, b"".join(lines), True)
        assert 0 < want.count(b"\n") < n


def test_a_record_and_its_swapped_twin_in_the_first_and_the_last_part(engines):
    """without -a both are written, with -a only the first"""
    a, b, c = S.record(b"qa", b"ta", 10, 20, 30), S.record(b"qb", b"tb", 1, 2, 3), S.record(b"qc", b"tc", 5, 6, 7, b"-")
    twin = S.swapped(a)
    for k in (2, 3, 5):
        shares = [a + b] + [c] * (k - 2) + [b + twin]
        lines = b"".join(shares).splitlines(keepends=True)
        for inv in (False, True):
            want, werr = whole_run(engines, b"".join(lines), inv)
            out, err, _ = parts_run(engines, [shares], inv)
            assert out == want and err is None and werr is None
            assert out.count(O.dedupe(twin)[0]) == (0 if inv else 1) and out.count(O.dedupe(a)[0]) == 1
        # the twin first: it is the one that stays
        shares = [twin + b] + [c] * (k - 2) + [a]
        out, err, _ = parts_run(engines, [shares], True)
        assert out == whole_run(engines, b"".join(shares), True)[0] and out.count(O.dedupe(a)[0]) == 0


def test_a_record_that_is_its_own_swap_twice_in_different_parts(engines):
    own = S.record(b"s", b"s", 40, 40, 25, ql=1000, tl=1000)
    assert S.swapped(own) == own
    bad_own = b"s\t50\t60\t64\t+\ts\t50\t60\t64\t3\t3\t60\tcg:Z:3M\n"  # its own swap, and paf_check fails
    other = S.record(b"qa", b"ta", 10, 20, 30)
    for k in (2, 3, 5):
        shares = [own + other] + [other] * (k - 2) + [other + own]
        for inv in (False, True):
            out, err, _ = parts_run(engines, [shares], inv)
            assert (out, err) == whole_run(engines, b"".join(shares), inv)
            assert out.count(b"\n") == 2
        shares = [other + bad_own] + [other] * (k - 2) + [bad_own]
        out, err, _ = parts_run(engines, [shares], True)  # nothing of its class came earlier: the run ends at record 1
        assert (out, err) == whole_run(engines, b"".join(shares), True) and err["record"] == 1
        out, err, _ = parts_run(engines, [shares], False)
        assert (out, err) == whole_run(engines, b"".join(shares), False) and err is None


GOOD = b"qb\t1000\t60\t64\t+\ttb\t200\t0\t3\t3\t3\t60\tcg:Z:3M\n"
BAD = b"qb\t50\t60\t64\t+\ttb\t200\t0\t3\t3\t3\t60\tcg:Z:3M\n"  # GOOD's key (the lengths are no part of it); query start >= query length
CHECK_QSTART = 5  # PAFFY_ERR_CHECK_QSTART
FILL = [S.record(b"q%d" % i, b"t", i, 2 * i, 9) for i in range(8)]


def test_paf_check_under_a(engines):
    for k in (2, 3, 5):
        mid = [FILL[2 + (i % 3)] for i in range(k - 2)]
        # its exact duplicate was written earlier in another part: no failure, dropped
        shares = [GOOD + FILL[0]] + mid + [FILL[1] + BAD + FILL[5]]
        for inv in (False, True):
            out, err, _ = parts_run(engines, [shares], inv)
            assert (out, err) == whole_run(engines, b"".join(shares), inv) and err is None
            assert O.dedupe(BAD)[0] not in out and out.endswith(O.dedupe(FILL[5])[0])
        # only its swapped twin was written earlier / nothing of its class came earlier: the run ends there
        for first in ([S.swapped(GOOD) + FILL[0]], [FILL[6] + FILL[0]]):
            shares = first + mid + [FILL[1] + BAD + FILL[5]]
            data = b"".join(shares)
            at = data.count(b"\n") - 2
            out, err, _ = parts_run(engines, [shares], True)
            assert (out, err) == whole_run(engines, data, True)
            assert err == {"code": CHECK_QSTART, "stage": 0, "record": at, "aux": 0}
            assert out == O.dedupe(b"".join(data.splitlines(keepends=True)[:at]), True)[0] and out.endswith(O.dedupe(FILL[1])[0])
            out, err, _ = parts_run(engines, [shares], False)  # without -a it passes and is written
            assert (out, err) == whole_run(engines, data, False) and err is None and O.dedupe(BAD)[0] in out


def test_two_failures_in_different_parts(engines):
    """the lowest global number is reported; parts behind it write only their records in front of it"""
    broken = b"q\t1\t2\n"
    for k in (2, 3, 5):
        mid = [FILL[2 + (i % 3)] + FILL[0] for i in range(k - 2)]
        for early, late in ((BAD, broken), (broken, BAD)):
            shares = [FILL[0] + FILL[1] + early + FILL[6]] + mid + [FILL[7] + late + FILL[5]]
            data = b"".join(shares)
            out, err, _ = parts_run(engines, [shares], True)
            assert (out, err) == whole_run(engines, data, True)
            assert err["record"] == 2 and out == O.dedupe(FILL[0] + FILL[1])[0]
        # the parse error is the later one's only failure without -a; with the failing record in the middle of a later part
        shares = [FILL[0] + FILL[1]] + mid + [FILL[7] + FILL[1] + broken + FILL[5]]
        data = b"".join(shares)
        for inv in (False, True):
            out, err, _ = parts_run(engines, [shares], inv)
            assert (out, err) == whole_run(engines, data, inv)
            assert err["record"] == data.count(b"\n") - 2 and err["stage"] == -1 and out.endswith(O.dedupe(FILL[7])[0])


def test_rounds(engines):
    """the same input as 1, 2 and 4 rounds; a duplicate whose original was written in an earlier round by another part"""
    lines = S.stream(random.Random(31), 600)
    check(engines, lines, ks=(2, 3, 5), n_rounds=(1, 2, 4), seed=3)
    for k in (2, 3, 5):
        pad = [FILL[2]] * (k - 2)
        # round 0: part 0 writes GOOD (or its twin); round 1: the last part brings the duplicate / the check-failing record
        for first, fails in ((GOOD, False), (S.swapped(GOOD), True)):
            rounds = [[first + FILL[0]] + pad + [FILL[1]], [FILL[6]] + pad + [FILL[7] + BAD + FILL[5]]]
            data = b"".join(b"".join(r) for r in rounds)
            out, err, _ = parts_run(engines, rounds, True)
            assert (out, err) == whole_run(engines, data, True) and (err is not None) == fails
            out, err, _ = parts_run(engines, rounds, False)
            assert (out, err) == whole_run(engines, data, False) and err is None
    # after a reset the same input writes its first records again; without one it writes nothing
    k, inv = 3, True
    workers = [shard.GpuDedupeWorker(e) for e in engines[:k]]
    rounds = S.cut(random.Random(5), lines[:200], 1, k)
    dev = [[(engines[p].to_device(b), len(b)) for p, b in enumerate(rnd)] for rnd in rounds]
    first = tobytes(shard.dedupe_in_parts(workers, dev, inv)["out"])
    assert first == whole_run(engines, b"".join(lines[:200]), inv)[0] and first
    twice = tobytes(shard.dedupe_in_parts(workers, dev + dev, inv)["out"])  # one run, the input twice: the second round is all duplicates
    assert twice == first
    assert tobytes(shard.dedupe_in_parts(workers, dev, inv)["out"]) == first  # dedupe_in_parts resets


def test_one_class_empty_parts_and_odd_lines(engines):
    one = S.record(b"qa", b"ta", 10, 20, 30)
    lines = [one if i % 3 else S.swapped(one) for i in range(700)]  # with -a one class: one owner gets every entry
    check(engines, lines, seed=9)
    for inv in (False, True):
        workers = [shard.GpuDedupeWorker(e) for e in engines[:5]]
        for w in workers:
            w.reset()
        data = b"".join(lines)
        entries, counts, n_rec = workers[0].keys((engines[0].to_device(data), len(data)), inv, 0, 5)
        assert n_rec == 700 and sum(counts) == 700 and sorted(counts)[:3] == [0, 0, 0] and (max(counts) == 700 or not inv)
    # empty parts in every place, an empty input
    some = S.stream(random.Random(8), 40)
    for k in (2, 3, 5):
        for empty in ((0,), (k - 1,), tuple(range(1, k))):
            for inv in (False, True):
                out, err, _ = parts_run(engines, S.cut(random.Random(k), some, 2, k, empty), inv)
                assert (out, err) == whole_run(engines, b"".join(some), inv)
        out, err, res = parts_run(engines, [[b""] * k], True)
        assert out == b"" and err is None and res["records"] == 0
    # an unterminated last line (the last part's, and a middle part's: the cut is then inside no line), a 5 000-byte name
    long_name = S.record(b"L" * 5000, b"t", 3, 4, 5)
    odd = some[:10] + [long_name] + some[10:20] + [long_name, S.swapped(long_name)] + [some[3].rstrip(b"\n")]
    data = b"".join(odd)
    for inv in (False, True):
        want, werr = whole_run(engines, data, inv)
        assert werr is None and want.endswith(b"\n")
        for k in PARTS:
            out, err, _ = parts_run(engines, S.cut(random.Random(k), odd, 1, k), inv)
            assert (out, err) == (want, None)


def test_routing(engines):
    """after part_keys: the counts sum to the records that parsed, every entry lies in the segment of shard.dedupe_owner of its class
    key, the global numbers are a permutation of the parsed records'"""
    lines = S.stream(random.Random(77), 3000)
    for at in (5, 1500, 2999):
        lines[at] = b"q\t1\t2\n"
    data, base = b"".join(lines), 1 << 33
    d_in = engines[0].to_device(data)
    for inv in (False, True):
        for k in (1, 2, 3, 5, 8, 1500):  # 1500: more owners than one pass of the LDS counters takes
            engines[0].dedupe_reset()
            entries, counts, n_rec = engines[0].dedupe_part_keys(d_in, len(data), inv, base, k)
            assert n_rec == 3000 and len(counts) == k and sum(counts) == 2997 == entries.shape[0]
            rows, p, end = entries.cpu().tolist(), 0, counts[0]
            for j, (hi, lo, g, flags) in enumerate(rows):
                while j >= end:
                    p += 1
                    end += counts[p]
                assert shard.dedupe_owner(hi & MASK, lo & MASK, k) == p and flags in ((0, 1) if inv else (1,))
            assert sorted(r[2] for r in rows) == [base + i for i in range(3000) if i not in (5, 1500, 2999)]
            if not inv:
                keys = {r[2] - base: (r[0], r[1]) for r in rows}
                assert all((keys[i] == keys[j]) == (lines[i] == lines[j]) for i, j in zip(range(6, 600), range(7, 601)))


def test_states_and_capacity(engines):
    L, eng = engine.lib(), engines[0]
    lines = S.stream(random.Random(3), 50)
    data = b"".join(lines)
    d_in = eng.to_device(data)
    info, bad = engine.PlanInfo(), C.c_int64()
    counts, n_rec = (C.c_int64 * 2)(), C.c_int64()
    verdicts = torch.zeros(64, dtype=torch.uint8, device=eng.device)
    entries = torch.full((50, 4), -7, dtype=torch.int64, device=eng.device)

    def keys(cap=50):
        return L.paffy_hip_dedupe_part_keys(eng._ctx, C.c_void_p(d_in.data_ptr()), len(data), 1, 0, 2, C.c_void_p(entries.data_ptr()), cap, counts, C.byref(n_rec))

    def verd():
        return L.paffy_hip_dedupe_part_verdicts(eng._ctx, C.c_void_p(verdicts.data_ptr()), 50, C.byref(bad))

    def plan(first_bad=-1):
        return L.paffy_hip_dedupe_part_plan(eng._ctx, first_bad, C.byref(info))

    out = torch.full((1 << 16,), 7, dtype=torch.uint8, device=eng.device)

    def nothing_written():
        rc = L.paffy_hip_emit(eng._ctx, C.c_void_p(out.data_ptr()), out.numel())
        eng.sync()
        return rc == E_STATE and bool((out == 7).all().item())

    eng.dedupe_reset()
    eng.dedupe_plan(d_in, 0, False)  # an empty plan: no round is under way
    assert verd() == E_STATE and plan() == E_STATE  # without part_keys
    assert keys() == 0 and plan() == E_STATE         # part_plan before part_verdicts
    assert nothing_written()
    assert verd() == 0 and verd() == E_STATE         # the verdicts are in: not twice
    assert plan() == 0 and plan() == E_STATE and info.n_rows == 0  # all-zero verdicts: nothing is written
    # another plan in between drops the round
    assert keys() == 0
    eng.dedupe_plan(d_in, len(data), True)
    assert verd() == E_STATE and plan() == E_STATE
    assert keys() == 0 and verd() == 0
    eng.query_names(d_in, len(data))
    eng.drop_index()
    assert plan() == E_STATE
    # a round that reported a failure: every call refuses until the reset
    assert keys() == 0 and verd() == 0 and plan(17) == 0 and info.error.code == 0 and info.n_rows == 0
    assert keys() == E_STATE and verd() == E_STATE and plan() == E_STATE
    assert L.paffy_hip_dedupe_part_decide(eng._ctx, C.c_void_p(entries.data_ptr()), 50, 1, C.c_void_p(verdicts.data_ptr())) == E_STATE
    eng.dedupe_reset()
    # an entry buffer one entry short: found before anything is written, and the round is not begun
    entries.fill_(-7)
    assert keys(49) == E_CAPACITY
    eng.sync()
    assert bool((entries == -7).all().item()) and verd() == E_STATE and nothing_written()
    assert keys(50) == 0 and n_rec.value == 50 and sum(counts) == 50
    # n_parts = 1: the four calls write what paffy_hip_dedupe_plan writes
    for inv in (False, True):
        out1, err, _ = parts_run(engines, [[data]], inv)
        assert (out1, err) == whole_run(engines, data, inv)

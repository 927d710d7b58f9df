"""The owner's memory of dedupe in parts (paffy_amd/csrc/dedupe_parts_kernel.h): every round's new classes are merged into the sorted
memory of the classes written before (k_dd_merge), and the next round's entries are looked up in it. One part through the four part calls,
eight rounds that add 1, 1, 254, 1, 1, 300, 5 000 and 1 new classes -- the memory holds 1, 2, 256, 257, 258, 558, 5 558 and 5 559 classes
after them: just below, at and just above one workgroup's width, and far above it. Every round also repeats records of every earlier
round; under -a it repeats them with lengths that fail paf_check (the lengths are no part of the key: a record whose own key was written
is dropped without a failure, so an orientation word that lost its key shows as a failure bit that should not be there) and as swapped
twins. The 300 new classes of round 5 all lie below the memory and the one of round 7 above it, by the device's own keys: the keys are read
from the entries of a part_keys call over the pool (the stand-in's key128 is another hash and says nothing about the device's order).

The verdicts are compared with the plain-Python decision of tests/standin_dedupe_worker.py over the same entries, the lines with one
context's paffy_hip_dedupe_plan over the same batches and with the oracle over the whole input. A 3-part, 6-round run on
dedupe_streams.cut follows. These pass with the memory sorted again after every round too: they pin the kernel, not a feature."""
import random

import pytest
import torch

import dedupe_streams as S
import oracle_lib as O
from paffy_amd import shard
from standin_dedupe_worker import StandinDedupeWorker

pytestmark = pytest.mark.gpu
NEW = (1, 1, 254, 1, 1, 300, 5000, 1)
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def engines():
    import paffy_amd

    es = [paffy_amd.Engine() for _ in range(4)]
    yield es
    for e in es:
        e.close()


def tobytes(t):
    return bytes(t.cpu().numpy().tobytes())


def pool_record(i, ql=1000, tl=2000):
    return S.record(b"q%d" % (i % 97), b"t%d" % (i % 89), i % 900, (i * 7) % 1900, 1 + i // 900 % 90, b"+" if i % 3 else b"-", ql=ql, tl=tl)


def device_keys(eng, lines, inv):
    """the class key (hi, lo) of every line, as the device hashes it"""
    data = b"".join(lines)
    eng.dedupe_reset()
    entries, counts, n_rec = eng.dedupe_part_keys(eng.to_device(data), len(data), inv, 0, 1)
    assert n_rec == len(lines) == counts[0]
    keys = [None] * len(lines)
    for hi, lo, g, _ in entries.cpu().tolist():
        keys[g] = (hi & MASK, lo & MASK)
    eng.dedupe_reset()
    return keys


def rounds_for(eng, inv, seed):
    """[lines per round]: NEW[r] new classes and repeats of every earlier round; the new classes of round 5 lie below everything in the
    memory and that of round 7 above everything"""
    rng = random.Random(seed)
    pool = [pool_record(i) for i in range(7000)]
    keys = device_keys(eng, pool, inv)
    assert len(set(keys)) == len(pool)
    by_key = sorted(range(len(pool)), key=lambda i: keys[i])
    low, top, middle = by_key[:300], by_key[-1:], by_key[300:-1]
    rng.shuffle(middle)
    rounds, fresh_of, at = [], [], 0
    for r, n_new in enumerate(NEW):
        fresh = low if r == 5 else top if r == 7 else middle[at: at + n_new]
        at += 0 if r in (5, 7) else n_new
        assert len(fresh) == n_new
        lines = [pool[i] for i in fresh]
        for earlier in fresh_of:  # repeats of every earlier round
            for i in rng.sample(earlier, min(40, len(earlier))):
                if inv:
                    lines.append(pool_record(i, ql=0, tl=0))   # the written record's own key, lengths that fail paf_check: dropped, no failure
                    lines.append(S.swapped(pool[i]))           # its swapped twin: dropped
                else:
                    lines.append(pool[i])
        rng.shuffle(lines)
        rounds.append(lines)
        fresh_of.append(fresh)
        if r in (4, 6):  # what the memory holds before rounds 5 and 7
            held = [keys[i] for f in fresh_of for i in f]
            nxt = low if r == 4 else top
            assert (max(keys[i] for i in nxt) < min(held)) if r == 4 else (min(keys[i] for i in nxt) > max(held))
    return rounds


@pytest.mark.parametrize("inv", [False, True])
def test_eight_rounds_grow_one_owners_memory_past_a_workgroup(engines, inv):
    part, whole = engines[0], engines[1]
    rounds = rounds_for(engines[2], inv, 11 + inv)
    model = StandinDedupeWorker()
    part.dedupe_reset()
    whole.dedupe_reset()
    base, outs, held = 0, [], 0
    for r, lines in enumerate(rounds):
        data = b"".join(lines)
        d_in = part.to_device(data)
        entries, counts, n_rec = part.dedupe_part_keys(d_in, len(data), inv, base, 1)
        assert n_rec == len(lines) == counts[0]
        v = part.dedupe_part_decide(entries, inv)
        want_v = model.decide(entries.cpu(), inv)
        assert torch.equal(v.cpu(), want_v), (r, inv)
        held += NEW[r]
        assert int((v & 1).sum().item()) == NEW[r] and len(model.memory) == held and not bool((v & 2).any().item())
        assert part.dedupe_part_verdicts(v) == -1
        info = part.dedupe_part_plan(-1)
        out = part.alloc_out(info.out_bytes)
        part.emit(out)
        part.sync()
        got = tobytes(out[: info.out_bytes])
        one, one_info = whole.dedupe(data, inv, reset=False)
        assert one_info.error.code == 0 and got == one, (r, inv)
        assert got.count(b"\n") == NEW[r]
        outs.append(got)
        base += n_rec
    assert held == 5559
    want, err = O.dedupe(b"".join(b"".join(lines) for lines in rounds), inv)
    assert err.code == 0 and b"".join(outs) == want


def test_a_swapped_twin_with_failing_lengths_fails_in_a_late_round(engines):
    """the failure bit that should be there: after the eight rounds, the swapped twin of a record of round 2, with lengths that fail
    paf_check -- its own key was never written, its class was -- ends the run at its number"""
    part, inv = engines[0], True
    rounds = rounds_for(engines[2], inv, 12)
    model, base = StandinDedupeWorker(), 0
    part.dedupe_reset()
    fresh = next(ln for ln in rounds[2] if ln.startswith(b"q") and ln.split(b"\t")[1] == b"1000")  # under -a the repeats are twins or have length 0
    twin = S.swapped(fresh).split(b"\t")
    twin[1], twin[6] = b"0", b"0"
    last = [rounds[0][0], b"\t".join(twin), rounds[1][0]]
    for lines in rounds + [last]:
        data = b"".join(lines)
        d_in = part.to_device(data)
        entries, counts, n_rec = part.dedupe_part_keys(d_in, len(data), inv, base, 1)
        v = part.dedupe_part_decide(entries, inv)
        assert torch.equal(v.cpu(), model.decide(entries.cpu(), inv))
        bad = part.dedupe_part_verdicts(v)
        info = part.dedupe_part_plan(bad)
        if lines is last:
            assert bad == base + 1 and info.error.code != 0 and info.error.record == base + 1 and info.out_bytes == 0
            want, err = O.dedupe(b"".join(b"".join(x) for x in rounds + [last]), inv)
            assert err.code == info.error.code and err.record == base + 1
        else:
            assert bad == -1 and info.error.code == 0
        base += n_rec


def test_three_parts_six_rounds(engines):
    """every owner's memory grows over six rounds, from a pool large enough that it passes a workgroup's width"""
    lines = S.stream(random.Random(41), 4000, pool_size=1500)
    data = b"".join(lines)
    for inv in (False, True):
        want, err = O.dedupe(data, inv)
        assert err.code == 0 and want.count(b"\n") > 3 * 300
        one, info = engines[3].dedupe(data, inv)
        assert one == want and info.error.code == 0
        rounds = S.cut(random.Random(6 + inv), lines, 6, 3)
        workers = [shard.GpuDedupeWorker(e) for e in engines[:3]]
        res = shard.dedupe_in_parts(workers, [[(engines[p].to_device(b), len(b)) for p, b in enumerate(rnd)] for rnd in rounds], inv)
        assert res["error"] is None and tobytes(res["out"]) == want and res["records"] == len(lines)

"""Dedupe in parts, the host side: the four calls are exported and declared, shard.dedupe_owner is a pure function that spreads keys
evenly, and shard.dedupe_sharded over gloo ranks -- with a Python stand-in for the device (tests/standin_dedupe_worker.py) -- writes what
the oracle's po_dedupe writes for the whole stream and reports the same failure."""
import json
import os
import random
import re
import socket
import subprocess

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dedupe_streams as S
import oracle_lib as O
from paffy_amd import engine, shard
from standin_dedupe_worker import StandinDedupeWorker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["paffy_hip_dedupe_part_keys", "paffy_hip_dedupe_part_decide", "paffy_hip_dedupe_part_verdicts", "paffy_hip_dedupe_part_plan"]


def test_the_four_calls_are_exported_and_declared():
    lib = engine.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        header = fh.read()
    for name in CALLS:
        assert name in exported, name
        assert re.search(r"\bint %s\(paffy_hip_ctx \*ctx," % name, header), name
    for name in ("paffy_hip_dedupe_plan", "paffy_hip_dedupe_reset"):  # kept as they were
        assert name in exported


def test_owner_is_a_pure_function_that_spreads_keys():
    """10 000 uniform keys over k parts: a part's count is Binomial(10 000, 1 / k), standard deviation sqrt(n p (1 - p)) <= 47 (k = 2: 50).
    The bound is the mean +- 6 standard deviations: a uniform hash misses it with probability below 2e-9 per part (normal tail; the
    binomial is close to normal at these sizes), about 1e-7 over the 35 parts of all seven cases -- and the keys are fixed by the seed,
    so the test is deterministic either way."""
    rng = random.Random(2024)
    keys = [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(10000)]
    for k in range(2, 9):
        owners = [shard.dedupe_owner(hi, lo, k) for hi, lo in keys]
        assert owners == [shard.dedupe_owner(hi, lo, k) for hi, lo in keys] and all(0 <= o < k for o in owners)
        p = 1.0 / k
        slack = 6 * (10000 * p * (1 - p)) ** 0.5
        for part in range(k):
            assert abs(owners.count(part) - 10000 * p) <= slack, (k, part, owners.count(part))
    assert {shard.dedupe_owner(hi, lo, 1) for hi, lo in keys} == {0}
    # the device's arithmetic, by hand for one key: x = hi ^ lo, the 64-bit finalizer, the high half of x * n_parts
    x = 0x0123456789abcdef ^ 0xfedcba9876543210
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) % (1 << 64)
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) % (1 << 64)
    x ^= x >> 33
    assert shard.dedupe_owner(0x0123456789abcdef, 0xfedcba9876543210, 5) == (x * 5) >> 64
    # keys that differ in one bit do not share an owner more often than chance allows (a key and its near miss are such a pair)
    same = sum(shard.dedupe_owner(hi, lo, 8) == shard.dedupe_owner(hi ^ 1, lo, 8) for hi, lo in keys)
    assert abs(same - 1250) <= 6 * (10000 * 0.125 * 0.875) ** 0.5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, tmpdir, rounds_by_rank, inv):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    batches = [(torch.frombuffer(bytearray(b), dtype=torch.uint8) if b else torch.zeros(0, dtype=torch.uint8), len(b)) for b in rounds_by_rank[rank]]
    chunks = []
    res = shard.dedupe_sharded(StandinDedupeWorker(), dist, rank, world, batches, inv, write=lambda b, t: chunks.append((b, bytes(t.numpy().tobytes()))))
    with open(os.path.join(tmpdir, f"res{rank}.json"), "w") as fh:
        json.dump({"error": res["error"], "total": res["total"], "order": [b for b, _ in chunks]}, fh)
    if rank == 0:
        with open(os.path.join(tmpdir, "out.paf"), "wb") as fh:
            fh.write(b"".join(c for _, c in chunks))
    dist.barrier()
    dist.destroy_process_group()


def sharded(tmp_path, rounds, world, inv):
    """rounds: [[bytes per rank] per round] -> (output at rank 0, the error every rank reported)"""
    by_rank = [[rnd[r] for rnd in rounds] for r in range(world)]
    d = tmp_path / f"w{world}_{int(inv)}_{len(list(tmp_path.iterdir()))}"
    d.mkdir()
    mp.spawn(_rank, args=(world, _free_port(), str(d), by_rank, inv), nprocs=world, join=True)
    res = [json.loads((d / f"res{r}.json").read_text()) for r in range(world)]
    out = (d / "out.paf").read_bytes()
    assert all(r["error"] == res[0]["error"] and r["total"] == len(out) for r in res)
    assert res[0]["order"] == sorted(res[0]["order"])
    return out, res[0]["error"]


def against_oracle(tmp_path, lines, world, inv, n_rounds, seed, empty=()):
    data = b"".join(lines)
    want, werr = O.dedupe(data, inv)
    out, err = sharded(tmp_path, S.cut(random.Random(seed), lines, n_rounds, world, empty), world, inv)
    assert out == want, (world, inv, n_rounds)
    if werr.code:
        assert err == {"code": werr.code, "stage": werr.stage, "record": werr.record, "aux": werr.aux}
    else:
        assert err is None
    return want, werr


@pytest.mark.parametrize("world", [2, 3])
def test_dedupe_sharded_over_gloo_ranks(tmp_path, world):
    rng = random.Random(40 + world)
    lines = S.stream(rng, 400)
    for inv in (False, True):
        want, werr = against_oracle(tmp_path, lines, world, inv, 3, 7)
        assert werr.code == 0 and 0 < want.count(b"\n") < len(lines)
    # records that fail paf_check: the run ends at the first one whose own key was not written before it (-a only)
    bad = S.stream(rng, 300, p_bad=0.02)
    want, werr = against_oracle(tmp_path, bad, world, True, 2, 8)
    assert werr.code != 0 and want
    against_oracle(tmp_path, bad, world, False, 2, 8)
    # a line that does not parse
    broken = lines[:150] + [b"q\t1\t2\n"] + lines[150:]
    want, werr = against_oracle(tmp_path, broken, world, False, 2, 9)
    assert werr.code != 0 and werr.record == 150


def test_dedupe_sharded_with_a_rank_that_holds_no_record(tmp_path):
    rng = random.Random(77)
    lines = S.stream(rng, 200)
    for inv in (False, True):
        against_oracle(tmp_path, lines, 3, inv, 2, 3, empty=(1,))
    against_oracle(tmp_path, [], 2, True, 1, 1)

"""Chain in parts, the host side: the five calls are exported and declared, and the two pure-torch helpers that settle what is global in
a `paffy chain` sharded by query sequence -- the chain numbers and the place of every line -- agree with brute-force sorts."""
import functools
import os
import random
import re
import subprocess

import torch

from paffy_amd import engine, shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["paffy_hip_chain_add_indexed", "paffy_hip_chain_run_part", "paffy_hip_chain_tail_keys", "paffy_hip_chain_renumber", "paffy_hip_chain_line_keys"]


def test_the_five_calls_are_exported_and_declared():
    lib = engine.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        header = fh.read()
    for name in CALLS:
        assert name in exported, name
        assert re.search(r"\b(int|int64_t) %s\(paffy_hip_ctx \*ctx," % name, header), name
    for name in ("paffy_hip_chain_run", "paffy_hip_chain_add", "paffy_hip_chain_tags"):  # kept as they were
        assert name in exported


def tail_cmp(a, b):
    """one process: '+' chains first, each strand by chain-end score desc, processing key desc, input number desc"""
    if a[0] != b[0]:
        return -1 if a[0] < b[0] else 1
    for k in (1, 2, 3):
        if a[k] != b[k]:
            return -1 if a[k] > b[k] else 1
    return 0


def test_global_chain_ids_against_a_brute_force_sort():
    rng = random.Random(11)
    for n in (0, 1, 2, 17, 400, 3000):
        # few distinct scores and keys: equal end scores in different parts, equal processing keys, both strand classes; the
        # global input numbers are distinct (a record ends one chain at most) and come in no order
        gidx = rng.sample(range(10 * n + 5), n)
        rows = [(rng.randrange(2), rng.choice([5, 5, 80, 900, -3]), rng.choice([-70000, -1, 0, 12, 12, 10**12]), g) for g in gidx]
        ids = shard.global_chain_ids(torch.tensor(rows, dtype=torch.int64).reshape(n, 4))
        want = sorted(range(n), key=functools.cmp_to_key(lambda i, j: tail_cmp(rows[i], rows[j])))
        got = [0] * n
        for i, c in enumerate(ids.tolist()):
            got[c] = i
        assert got == want, n
        assert sorted(ids.tolist()) == list(range(n))
    # parts one after the other: a chain's number does not depend on the part it stands in
    a = [(0, 100, 7, 3), (1, 100, 7, 9), (0, 50, 2, 4)]
    b = [(0, 100, 7, 8), (0, 100, 9, 1), (1, 200, 0, 2)]
    ids = shard.global_chain_ids(torch.tensor(a + b, dtype=torch.int64)).tolist()
    assert ids == [2, 5, 3, 1, 0, 4]
    assert shard.global_chain_ids(torch.tensor(b + a, dtype=torch.int64)).tolist() == ids[3:] + ids[:3]


def test_chain_line_offsets_against_a_brute_force_merge():
    rng = random.Random(5)
    for world in (1, 2, 3, 5):
        # lines of `world` parts, each part in its own output order (own score desc, chain id, link); chains belong to one part
        n_chains = rng.randrange(1, 40)
        lines = []
        for c in range(n_chains):
            part = rng.randrange(world)
            for link in range(rng.randrange(1, 6)):
                lines.append((part, rng.choice([10, 10, 10, 500, 7]), c, link, rng.randrange(60, 4000)))  # equal own scores across parts
        order = lambda ln: (-ln[1], ln[2], ln[3])  # noqa: E731
        parts = [sorted((ln for ln in lines if ln[0] == p), key=order) for p in range(world)]
        keys = torch.tensor([ln[1:] for p in parts for ln in p], dtype=torch.int64).reshape(-1, 4)
        owner = torch.tensor([ln[0] for p in parts for ln in p], dtype=torch.int64)
        merged, at, place = sorted(lines, key=order), 0, {}
        for ln in merged:
            place[ln[2], ln[3]] = at
            at += ln[4]
        for p in range(world):
            offs, total = shard.chain_line_offsets(keys, owner, p)
            assert total == at and offs.tolist() == [place[ln[2], ln[3]] for ln in parts[p]]
    offs, total = shard.chain_line_offsets(torch.zeros(0, 4, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 0)
    assert total == 0 and offs.numel() == 0


def test_the_failure_that_ends_the_run():
    """any part's parse error before any assert of the trim, the lowest global record first; failed checks by (chain id, link)"""
    E = engine

    def info(code, stage, record):
        i = E.PlanInfo()
        i.error.code, i.error.stage, i.error.record = code, stage, record
        return i

    parse_late, parse_early, trim = info(2, -1, 900), info(1, -1, 40), info(22, 0, 3)
    f = [shard.part_failure(x) for x in (trim, parse_late, parse_early, info(0, 0, 0))]
    assert f[3] is None
    assert shard.least_failure([x for x in f if x]) == {"code": 1, "stage": -1, "record": 40, "aux": 0}
    chk = [shard.part_failure(info(6, 0, 5), (100, 7, 2)), shard.part_failure(info(5, 0, 900), (3, 7, 1)), shard.part_failure(info(8, 0, 1), (9000, 8, 0))]
    assert shard.least_failure(chk)["record"] == 900
    assert shard.first_failure(None, None) is None and shard.first_failure(None, f[1])["record"] == 900

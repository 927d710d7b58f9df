"""to_bed in parts, the host side (paffy_amd/shard.py): where the blocks of BED lines of all parts go in the one-process output, and
which of several parts' failures is the one a single process reports. Pure torch on the CPU: no GPU, no library."""
from types import SimpleNamespace

import torch

from paffy_amd import shard


def keys(rows):
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


def offsets(parts):
    """parts: per part its [(global key, bytes)] in its own order -> ([offsets of part p], total)"""
    all_keys = torch.cat([keys(p) for p in parts])
    owner = torch.cat([torch.full((len(p),), i, dtype=torch.int64) for i, p in enumerate(parts)])
    outs = [shard.bed_block_offsets(all_keys, owner, i) for i in range(len(parts))]
    assert len({t for _, t in outs}) == 1
    return [o.tolist() for o, _ in outs], outs[0][1]


def test_interleaved_owners():
    offs, total = offsets([[(0, 10), (4, 7)], [(2, 5), (6, 3)]])
    assert offs == [[0, 15], [10, 22]] and total == 25


def test_a_block_without_bytes_keeps_its_place():
    offs, total = offsets([[(0, 10), (9, 0), (12, 4)], [(3, 6)]])
    assert offs == [[0, 16, 16], [10]] and total == 20


def test_one_part_empty_and_no_part_at_all():
    offs, total = offsets([[], [(1, 8), (2, 9)], []])
    assert offs == [[], [0, 8], []] and total == 17
    offs, total = offsets([[], []])
    assert offs == [[], []] and total == 0


def test_the_two_sides_of_one_record_in_different_parts():
    """record 5 introduces its query sequence (key 10) in part 1 and its target sequence (key 11) in part 0: query first"""
    offs, total = offsets([[(11, 7), (40, 1)], [(10, 3), (13, 2)]])
    assert offs == [[3, 12], [0, 10]] and total == 13


def info(code, stage, record, aux=0):
    return SimpleNamespace(error=SimpleNamespace(code=code, stage=stage, record=record, aux=aux))


def test_failure_selection():
    f = shard.part_failure
    assert f(info(0, 0, 0), side=0, record=3) is None
    t_side = f(info(19, 0, 4, 2), side=1, record=7)   # local record 4 is global record 7
    q_side = f(info(19, 0, 1, 1), side=0, record=7)
    e = shard.least_failure([t_side, q_side])
    assert e == {"code": 19, "stage": 0, "record": 7, "aux": 1}           # the query side of a record before its target side
    assert shard.least_failure([q_side, t_side]) == e
    parse = f(info(2, -1, 0, ord("*")), side=-1, record=7)
    assert shard.least_failure([t_side, q_side, parse])["code"] == 2       # a line that does not parse: before either side
    assert shard.least_failure([parse, parse])["code"] == 2                # both copies of one line: reported once
    earlier = f(info(19, 0, 9, 2), side=1, record=6)
    assert shard.least_failure([q_side, parse, earlier])["record"] == 6    # the lower global record wins whatever its side
    assert shard.first_failure(None, q_side) == e and shard.first_failure(None, None) is None
    # chain's use of part_failure is unchanged
    assert f(info(22, 0, 5, 0)) == ((0, 5, 0), (22, 0, 5, 0)) and f(info(6, 0, 5, 0), fail=(100, 3, 1)) == ((3, 1, 0), (6, 0, 5, 0))

"""to_bed in parts (include/paffy_hip.h): `paffy to_bed` sharded by sequence -- with -n a line travels to the owners of both its
names, every copy with a side mask -- so that the parts, one context each, write together, byte for byte, what one context writes
for the whole input, which is what the oracle writes (tests/test_gpu_to_bed.py); a failing record is the one a single context reports."""
import json
import os
import random
import socket
import subprocess
import sys

import pytest
import torch

import oracle_lib as O
import synth_lib
from paffy_amd import shard
from test_gpu_to_bed import OPTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (1, 2, 3, 5)
OK = b"q\t30\t2\t12\t+\tt\t40\t5\t15\t10\t10\t60\tcg:Z:10M\n"


@pytest.fixture(scope="module")
def engines():
    import paffy_amd

    es = [paffy_amd.Engine() for _ in range(max(PARTS) + 1)]  # the last one runs the whole input
    yield es
    for e in es:
        e.close()


@pytest.fixture(scope="module")
def piles():
    return synth_lib.Synth4(0x5EED0004, 512, n_contigs=5, tlen_min=1_500_000, tlen_span=1_000_000).records(0, 3000)


def tobytes(t):
    return bytes(t.cpu().numpy().tobytes())


def whole_run(engines, data, **kw):
    """the oracle and one context on the whole input: (bytes, PlanInfo of the context)"""
    want, werr = O.to_bed(data, **kw)
    got, info = engines[-1].to_bed(data, raise_on_error=False, **kw)
    assert info.error.code == werr.code, (kw, info.error.code, werr.code)
    if werr.code:
        assert got == b"" and info.error.record == werr.record
    else:
        assert got == want, kw
    return want, info


def parts_run(engines, data, k, batch_bytes=None, owner_of=None, **kw):
    workers = [shard.GpuBedWorker(e) for e in engines[:k]]
    pieces = engines[0].split_lines(data, batch_bytes) if batch_bytes else ([data] if data else [])
    res = shard.to_bed_in_parts(workers, [(engines[0].to_device(p), len(p)) for p in pieces], kw, owner_of=owner_of)
    for e in engines[:k]:
        e.sync()
    return res


def same_as_whole(res, want, info, what):
    if info.error.code:
        e = res["error"]
        assert e is not None and res["out"] is None and res["total"] == 0, what  # nothing is written
        assert (e["code"], e["stage"], e["record"]) == (info.error.code, info.error.stage, info.error.record), what
    else:
        assert res["error"] is None and res["total"] == len(want), what
        assert tobytes(res["out"]) == want, what


def check(engines, data, ks=PARTS, batch_bytes=None, **kw):
    want, info = whole_run(engines, data, **kw)
    for k in ks:
        same_as_whole(parts_run(engines, data, k, batch_bytes, **kw), want, info, (k, kw))
    return want, info


def owners(k, **part_of):
    return {shard.name_hash(n.encode()): p for n, p in part_of.items()}, k


def check_owned(engines, data, deal, **kw):
    """with an explicit deal of the names: -> the side masks that were sent"""
    owner_of, k = deal
    want, info = whole_run(engines, data, **kw)
    res = parts_run(engines, data, k, owner_of=owner_of, **kw)
    same_as_whole(res, want, info, (k, kw))
    return sorted(res["sides"].cpu().tolist()), info


def test_option_sets_on_the_fixture(engines, human_chimp):
    """without -n the oracle's bytes; with -n the length assert (the chromosomes of both species share their names) at the record one
    context reports, for every K"""
    for kw in OPTS:
        _, info = check(engines, human_chimp, **kw)
        assert (info.error.code == 19) == bool(kw.get("include_inverted"))


def test_option_sets_on_synthetic_piles(engines, piles):
    for kw in OPTS:  # sequences over several 1 Mi slices, more parts than some runs have names
        _, info = check(engines, piles, **kw)
        assert info.error.code == 0


def test_shuffled_subset_with_inverted(engines, piles):
    lines = piles.splitlines(keepends=True)
    random.Random(3).shuffle(lines)
    check(engines, b"".join(lines[:700]), include_inverted=True)


def test_both_names_in_one_part_and_in_two(engines):
    data = OK + b"q\t30\t8\t20\t-\tt\t40\t0\t10\t10\t12\t60\tcg:Z:4M2I6M\n"
    for inv in (False, True):
        check(engines, data, include_inverted=inv)
        sides, _ = check_owned(engines, data, owners(2, q=0, t=0), include_inverted=inv)
        assert sides == ([3, 3] if inv else [1, 1])                       # one copy, both sides counted where it lies
        sides, _ = check_owned(engines, data, owners(2, q=0, t=1), include_inverted=inv)
        assert sides == ([1, 1, 2, 2] if inv else [1, 1])                 # two copies, a side each
        sides, _ = check_owned(engines, data, owners(2, q=1, t=0), include_inverted=inv)
        assert sides == ([1, 1, 2, 2] if inv else [1, 1])


def test_a_sequence_in_both_roles(engines):
    same = OK + b"t\t40\t0\t10\t+\tq\t30\t0\t10\t10\t10\t60\tcg:Z:10M\n"
    other = OK + b"t\t41\t0\t10\t+\tq\t30\t0\t10\t10\t10\t60\tcg:Z:10M\n" + OK
    for inv in (False, True):
        _, info = check(engines, same, include_inverted=inv)
        assert info.error.code == 0
        _, info = check(engines, other, include_inverted=inv)
        assert (info.error.code, info.error.record) == ((19, 1) if inv else (0, 0))  # t: 40 bases as a target, 41 as a query
        for deal in (owners(2, q=0, t=1), owners(2, q=1, t=0), owners(2, q=1, t=1)):
            check_owned(engines, same, deal, include_inverted=inv)
            check_owned(engines, other, deal, include_inverted=inv)


def test_failures_of_one_side(engines):
    t_only = OK + b"q\t30\t2\t12\t+\tt\t40\t5\t16\t10\t10\t60\tcg:Z:10M\n" + OK   # the target walk does not end at target_end
    both = OK + b"q\t31\t2\t12\t+\tt\t40\t5\t16\t10\t10\t60\tcg:Z:10M\n" + OK     # query: another length; target: the walk
    strand = OK + b"q\t30\t2\t12\t*\tt\t40\t5\t15\t10\t10\t60\tcg:Z:10M\n"          # does not parse: no target name is read
    cigar = OK + b"q\t30\t2\t12\t+\tt\t40\t5\t15\t10\t10\t60\tcg:Z:10Q\n"           # fails on both copies alike
    tp = OK + b"q\t30\t2\t12\t+\tt\t40\t5\t15\t10\t10\t60\ttp:A:Z\tcg:Z:10M\n"      # does not parse, both names read: two copies
    for inv in (False, True):
        _, info = check(engines, t_only, include_inverted=inv)
        assert (info.error.code, info.error.record) == ((19, 1) if inv else (0, 0))
        _, info = check(engines, both, include_inverted=inv)
        assert (info.error.code, info.error.record) == (19, 1)
        for data in (strand, cigar, tp):
            _, info = check(engines, data, include_inverted=inv)
            assert info.error.code != 0 and info.error.record == 1
        for deal in (owners(2, q=0, t=1), owners(2, q=1, t=0)):  # the two sides of the failing record in different parts
            for data in (t_only, both, strand, cigar, tp):
                check_owned(engines, data, deal, include_inverted=inv)
    # the target side of record 0 fails in part 1 although the query side of record 1 fails in part 0: the lower record
    data = b"q\t30\t2\t12\t+\tt\t40\t5\t16\t10\t10\t60\tcg:Z:10M\n" + b"q\t30\t2\t13\t+\tt\t40\t5\t15\t10\t10\t60\tcg:Z:10M\n"
    _, info = check_owned(engines, data, owners(2, q=0, t=1), include_inverted=True)
    assert (info.error.code, info.error.record) == (19, 0)


def test_order_of_first_appearance_across_parts(engines):
    """part 0's first sequence is the TARGET of record 0, part 1's the query of record 1, part 2's the query of record 0"""
    data = (b"qa\t30\t2\t12\t+\tt\t40\t5\t15\t10\t10\t60\tcg:Z:10M\n" + b"qb\t30\t0\t10\t+\tt\t40\t20\t30\t10\t10\t60\tcg:Z:10M\n" +
            b"qc\t30\t0\t10\t-\tqa\t30\t20\t30\t10\t10\t60\tcg:Z:10M\n")
    for inv in (False, True):
        want, _ = check(engines, data, include_inverted=inv)
        assert [ln.split()[0] for ln in want.splitlines() if ln.split()[1] == b"0"] == ([b"qa", b"t", b"qb", b"qc"] if inv else [b"qa", b"qb", b"qc"])
        check_owned(engines, data, owners(3, t=0, qb=1, qa=2, qc=1), include_inverted=inv)
        check_owned(engines, data, owners(3, t=0, qb=1, qa=2, qc=0), include_inverted=inv)


def test_a_block_without_bytes(engines):
    """exclude_aligned on a fully covered sequence: 0 bytes between two blocks that have some"""
    data = OK + b"full\t10\t0\t10\t+\tt\t40\t0\t10\t10\t10\t60\tcg:Z:10M\n" + b"r\t30\t5\t15\t+\tt\t40\t5\t15\t10\t10\t60\tcg:Z:10M\n"
    for inv in (False, True):
        want, _ = check(engines, data, exclude_aligned=True, include_inverted=inv)
        assert b"full" not in want and b"q " in want and b"r " in want
        check_owned(engines, data, owners(3, q=0, full=1, r=2, t=1), exclude_aligned=True, include_inverted=inv)
        check_owned(engines, data, owners(2, q=0, full=1, r=0, t=0), exclude_aligned=True, include_inverted=inv)  # part 1: keys, no bytes


def test_edges(engines):
    with open(os.path.join(ROOT, "tests", "golden", "fnv_collision.txt")) as fh:
        n1, n2 = fh.read().split()[:2]
    assert n1 != n2 and shard.name_hash(n1.encode()) == shard.name_hash(n2.encode())
    twins = OK.replace(b"q\t30", n1.encode() + b"\t30") + OK.replace(b"q\t30", n2.encode() + b"\t40") + OK.replace(b"\tt\t40", b"\t" + n2.encode() + b"\t40")
    for inv in (False, True):
        for k in PARTS:  # the empty input
            res = parts_run(engines, b"", k, include_inverted=inv)
            assert res["error"] is None and res["total"] == 0 and tobytes(res["out"]) == b""
        check(engines, OK, include_inverted=inv)
        check(engines, OK + OK[:-1], include_inverted=inv)                      # an unterminated last line
        check(engines, b"q\t30\t4\t4\t+\tt\t40\t5\t5\t0\t0\t60\n", include_inverted=inv)  # no cigar, empty ranges
        want, info = check(engines, twins, include_inverted=inv)                # two names under one hash stay two sequences
        assert info.error.code == 0 and want.count(n1.encode() + b" 0 ") == 1 and want.count(n2.encode() + b" 0 ") == 1


def test_counters_saturate_inside_one_part(engines):
    for inv in (False, True):
        want, _ = check(engines, OK * 40000, include_inverted=inv)  # two names: with K = 3 and 5 some parts are empty
        assert b" 32766\n" in want
    check_owned(engines, OK * 40000, owners(2, q=0, t=1), include_inverted=True)


def test_several_batches(engines):
    data = synth_lib.Synth4(0x5EED0004, 512, n_contigs=4, tlen_min=200_000, tlen_span=300_000).records(0, 2500)
    for kw in (dict(), dict(include_inverted=True), dict(binary=True, min_size=20)):
        want, info = whole_run(engines, data, **kw)
        assert info.error.code == 0
        for k in PARTS:
            same_as_whole(parts_run(engines, data, k, batch_bytes=150_000, **kw), want, info, (k, kw))
    bad = data + b"q\t30\t2\t13\t+\tt\t40\t5\t15\t10\t10\t60\tcg:Z:10M\n"
    want, info = whole_run(engines, bad, include_inverted=True)
    for k in (2, 5):
        same_as_whole(parts_run(engines, bad, k, batch_bytes=150_000, include_inverted=True), want, info, k)


def test_add_sides_with_no_mask_and_with_every_side(engines, piles):
    eng = engines[0]
    lines = piles.splitlines(keepends=True)
    random.Random(3).shuffle(lines)
    inputs = [piles, b"".join(lines[:700]), OK + b"q\t30\t8\t20\t-\tt\t40\t0\t10\t10\t12\t60\tcg:Z:4M2I6M\n", OK * 40000,
              OK + b"q\t30\t2\t12\t+\tt\t40\t5\t16\t10\t10\t60\tcg:Z:10M\n" + OK]
    for data in inputs:
        whole, _ = engines[-1].to_bed(data, include_inverted=True, raise_on_error=False)
        # the baseline: paffy_hip_bed_begin / bed_add / bed_run over the same batches on the same context
        want, winfo = eng.to_bed(data, include_inverted=True, raise_on_error=False, batch_bytes=150_000)
        assert want == whole
        pieces = eng.split_lines(data, 150_000)
        bufs = [(eng.to_device(p), len(p)) for p in pieces]
        full = [torch.full((p.count(b"\n"),), 3, dtype=torch.uint8, device=eng.device) for p in pieces]
        for sides in (None, full, [full[0]] + [None] * (len(full) - 1)):
            info = eng.bed_part(bufs, sides, include_inverted=True)
            assert (info.error.code, info.error.record, info.out_bytes) == (winfo.error.code, winfo.error.record, len(want))
            if info.out_bytes:
                out = eng.alloc_out(info.out_bytes)
                eng.emit(out)
                eng.sync()
                assert tobytes(out[: info.out_bytes]) == want
                keys = eng.bed_sequence_keys().cpu()
                assert int(keys[:, 1].sum()) == len(want) and int(keys[:, 2].sum()) == want.count(b"\n")
                assert keys[:, 0].tolist() == sorted(keys[:, 0].tolist())


def run_ranks(tmp_path, args, n_ranks=2):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "to_bed_sharded_run.py"), "--one-device", "--batch-bytes", "200000"] + args
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), WORLD_SIZE=str(n_ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE) for r in range(n_ranks)]  # fresh processes, two contexts on this GPU
    outs = [p.communicate(timeout=330) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err.decode()[-2000:]


def test_two_ranks_over_gloo_on_one_gpu(engines, piles, tmp_path):
    """shard.to_bed_sharded in two fresh processes that share this GPU, gloo carrying the exchanges; the output gathered on rank 0
    equals the oracle's, and a failing record is reported alike by both ranks"""
    data = piles[: piles.index(b"\n", len(piles) // 2) + 1]
    want, info = whole_run(engines, data, include_inverted=True)
    assert info.error.code == 0
    src, dst, errf = tmp_path / "in.paf", tmp_path / "out.bed", tmp_path / "err.json"
    src.write_bytes(data)
    run_ranks(tmp_path, ["--input", str(src), "--output", str(dst), "-n"])
    assert dst.read_bytes() == want
    bad = data + b"q\t30\t2\t12\t+\tt\t40\t5\t16\t10\t10\t60\tcg:Z:10M\n" + OK
    _, info = whole_run(engines, bad, include_inverted=True)
    assert info.error.code == 19
    src.write_bytes(bad)
    dst.unlink()
    run_ranks(tmp_path, ["--input", str(src), "--output", str(dst), "--error", str(errf), "-n"])
    e0, e1 = json.loads(errf.read_text()), json.loads((tmp_path / "err.json.1").read_text())
    assert not dst.exists() and e0 == e1
    assert (e0["code"], e0["stage"], e0["record"]) == (info.error.code, info.error.stage, info.error.record)

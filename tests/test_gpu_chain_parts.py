"""Chain in parts (include/paffy_hip.h): `paffy chain` cut where its global decisions begin, so that the parts of an input partitioned by
query name -- one context each -- write together, byte for byte, what one context writes for the whole input, which in turn is what
the oracle's po_chain writes with the fresh-iterator walk switched off (the comparison of tests/test_gpu_chain.py)."""
import json
import os
import random
import socket
import subprocess
import sys

import pytest
import torch

import oracle_lib as O
from paffy_amd import shard
from test_gpu_chain import collinear_set, line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def engines():
    import paffy_amd

    es = [paffy_amd.Engine() for _ in range(max(PARTS) + 1)]  # the last one runs the whole input
    yield es
    for e in es:
        e.close()


def tobytes(t):
    return bytes(t.cpu().numpy().tobytes())


def whole_run(engines, data, **kw):
    """one context on the whole input == the oracle without the fresh walk"""
    got, info = engines[-1].chain(data, raise_on_error=False, **kw)
    want, err, _ = O.chain(data, fresh_walk=False, **kw)
    assert info.error.code == err.code
    if err.code == 0:
        assert got == want
    else:
        assert info.error.record == err.record and got == b""
    return got, info


def parts_run(engines, data, k, batch_bytes=None, **kw):
    workers = [shard.GpuChainWorker(e, **kw) for e in engines[:k]]
    pieces = engines[0].split_lines(data, batch_bytes) if batch_bytes else ([data] if data else [])
    res = shard.chain_in_parts(workers, [(engines[0].to_device(p), len(p)) for p in pieces])
    for e in engines[:k]:
        e.sync()
    return res, workers


def check(engines, data, ks=PARTS, **kw):
    want, info = whole_run(engines, data, **kw)
    assert info.error.code == 0
    for k in ks:
        res, workers = parts_run(engines, data, k, **kw)
        assert res["error"] is None and res["total"] == len(want), k
        assert tobytes(res["out"]) == want, k
        for w in workers:
            w.release()
    return want


def tag(ln, name):
    return int(ln.split(b"\t" + name + b":i:")[1].split(b"\t")[0])


def test_random_sets_both_strands(engines):
    for seed, kw in [(1, {}), (2, dict(gap_open=100, gap_extend=3)), (4, dict(trim=0.0)), (6, dict(gap_open=50, max_gap=5000, trim=0.0))]:
        rng = random.Random(seed)
        for n, n_q in ((1, 3), (7, 3), (60, 12), (400, 3), (3000, 12)):
            data = collinear_set(rng, n, n_q=n_q, exact=0.0 if seed % 2 else 0.3, score_hi=50 if seed == 6 else 20000)
            assert n < 60 or (b"\t+\t" in data and b"\t-\t" in data)
            check(engines, data, **kw)


def test_chain_ends_of_different_parts_tie_on_score(engines):
    """the same records under eight query names: every chain has seven twins in other parts with the same end score and the same
    processing key, and only the global input number tells them apart"""
    rng = random.Random(9)
    base = []
    for strand in "+-":
        qs = ts = 1000
        for _ in range(12):
            ln = rng.randrange(100, 900)
            base.append((qs, qs + ln, ts, ts + ln, rng.choice([300, 300, 7000]), strand))
            step = rng.choice([0, 50, 2_000_000])
            qs, ts = qs + ln + step, ts + ln + step
    rows = [line("q%d" % q, qs, qe, "t", ts, te, sc, st) for q in range(8) for qs, qe, ts, te, sc, st in base]
    rng.shuffle(rows)
    want = check(engines, b"".join(rows), gap_open=10, max_gap=100000, trim=0.0)
    by_score = {}
    for ln in want.splitlines():
        by_score.setdefault((tag(ln, b"s1"), ln.split(b"\t")[4]), set()).add(tag(ln, b"cn"))
    assert max(len(v) for v in by_score.values()) >= 8  # chains that tie on score got different numbers


def test_chain_numbers_change_their_digit_count_between_parts(engines):
    """more than 10 and more than 100 chains: a part's own numbering would write shorter cn tags than the global one"""
    rng = random.Random(3)
    for n_chains in (14, 130):
        rows = [line("q%d" % (c % 9), 10_000 * c, 10_000 * c + 500, "t%d" % c, 5, 505, rng.randrange(10, 9000), rng.choice("+-")) for c in range(n_chains)]
        rows += [line("q%d" % (c % 9), 10_000 * c + 600, 10_000 * c + 900, "t%d" % c, 610, 910, 40, "+") for c in range(0, n_chains, 3)]
        rng.shuffle(rows)
        want = check(engines, b"".join(rows), gap_open=5, trim=0.0)
        assert max(tag(ln, b"cn") for ln in want.splitlines()) >= n_chains - 1
        res, workers = parts_run(engines, b"".join(rows), 3, gap_open=5, trim=0.0)
        local = [int(t.shape[0]) for t in res["tail_keys"]]
        assert sum(local) > n_chains - 1 and max(local) < sum(local)  # no part holds all the chains: local numbers would be smaller


def test_few_names_and_the_empty_input(engines):
    rng = random.Random(21)
    check(engines, collinear_set(rng, 300, n_q=1))  # K - 1 empty parts
    check(engines, collinear_set(rng, 300, n_q=2))  # fewer names than parts
    for k in PARTS:  # the empty input
        res, _ = parts_run(engines, b"", k)
        assert res["error"] is None and res["total"] == 0 and tobytes(res["out"]) == b"" == engines[-1].chain(b"")[0]
    check(engines, line("q", 0, 100, "t", 0, 100, 100))
    check(engines, line("q", 0, 100, "t", 0, 100, 100)[:-1])  # the last line without its newline


def test_fixture_and_several_batches(engines, human_chimp):
    check(engines, human_chimp)
    data = collinear_set(random.Random(77), 5000, n_q=5, n_t=4)
    want, _ = whole_run(engines, data)
    for k in (2, 5):
        res, _ = parts_run(engines, data, k, batch_bytes=40_000)  # 20-odd batches into one send buffer
        assert tobytes(res["out"]) == want


def test_tags_and_rows_after_renumber(engines):
    data = collinear_set(random.Random(31), 2000, n_q=7)
    in_lines = data.splitlines()
    want, _ = whole_run(engines, data)
    res, workers = parts_run(engines, data, 3)
    assert tobytes(res["out"]) == want
    seen = []
    for w in workers:
        out = tobytes(w.emit()).splitlines()
        ids, scores = w.eng.chain_tags(len(out))
        assert ids == [tag(ln, b"cn") for ln in out] and scores == [tag(ln, b"s1") for ln in out]
        recs = w.global_records().cpu().tolist()  # paffy_hip_plan_rows through the part's global record numbers
        assert len(recs) == len(out)
        for g, ln in zip(recs, out):
            assert in_lines[g].split(b"\t")[:12] == ln.split(b"\t")[:12]
        seen += recs
    assert sorted(seen) == list(range(len(in_lines)))
    assert sorted(res["chain_ids"].cpu().tolist()) == list(range(res["chain_ids"].numel()))


def test_global_numbers_stand_in_for_creation_order(engines):
    """one context gets the lines in another order than the input's, with their input numbers: exact ties (duplicated records, exactly
    abutting alignments) are settled by those numbers, and the output is the one of the input in its own order"""
    rng = random.Random(13)
    lines = collinear_set(rng, 600, n_q=2, n_t=2, exact=0.4, score_hi=30).splitlines(keepends=True)
    lines += rng.sample(lines, 150)  # duplicates: equal in every key but the input number
    rng.shuffle(lines)
    data = b"".join(lines)
    want, _ = whole_run(engines, data, gap_open=3, trim=0.0)
    perm = list(range(len(lines)))
    rng.shuffle(perm)
    eng = engines[0]
    text = b"".join(lines[i] for i in perm)
    w = shard.GpuChainWorker(eng, gap_open=3, trim=0.0)
    info = w.run_part(eng.to_device(text), torch.tensor(perm, dtype=torch.int64, device=eng.device), [(0, len(text))])
    assert info.error.code == 0
    info, fail = w.renumber(shard.global_chain_ids(w.tail_keys()))
    assert info.error.code == 0 and fail is None
    assert tobytes(w.emit()) == want


def deal(data, k):
    """{query name: part} as chain_in_parts deals them: by the bytes of their lines, heaviest first (shard.owner_table)"""
    weights = {}
    for ln in data.splitlines(keepends=True):
        q = ln.split(b"\t", 1)[0]
        weights[q] = weights.get(q, 0) + len(ln) + (0 if ln.endswith(b"\n") else 1)
    owner = shard.owner_table({shard.name_hash(q): w for q, w in weights.items()}, k)
    return {q.decode(): owner[shard.name_hash(q)] for q in weights}


def test_errors_equal_the_one_context_run(engines):
    names = ["qa", "qb", "qc", "qd", "qe", "qf"]
    rows_of = {q: 20 + 4 * i for i, q in enumerate(names)}  # unequal weights: a line more or less does not change the deal

    def good(q, k):
        return line(q, 1000 * k, 1000 * k + 900, "t", 1000 * k, 1000 * k + 900, 100 + k)

    def build(extra):
        """the rows of all names interleaved; extra: {(name, row): line}"""
        rows = [extra.get((q, k), good(q, k)) for k in range(max(rows_of.values())) for q in names if k < rows_of[q]]
        return b"".join(rows)

    bad = lambda q: (q + "\t10\t0\t5\t*\tt\t10\t0\t5\t5\t5\t60\n").encode()  # noqa: E731
    broken = lambda q, k: line(q, 1000 * k, 1000 * k + 900, "t", 1000 * k, 1000 * k + 900, 100 + k, ql=150)  # noqa: E731
    cases = []
    for k in (3, 2, 5):
        part_of = deal(build({}), k)
        assert len(set(part_of.values())) == min(k, len(names))
        p_parse = [q for q in names if part_of[q] == 1][0]  # a line that does not parse in part 2 (of 3)
        p_check = [q for q in names if part_of[q] != 1][0]  # a failing paf_check in another part
        cases += [(k, p_parse, p_check, {(p_parse, 7): bad(p_parse)}), (k, p_parse, p_check, {(p_check, 4): broken(p_check, 4)}),
                  (k, p_parse, p_check, {(p_check, 2): broken(p_check, 2), (p_parse, 7): bad(p_parse)}),
                  # two lines that do not parse in different parts: the lower global record; two failing checks in different parts
                  (k, p_parse, p_check, {(p_check, 9): bad(p_check), (p_parse, 3): bad(p_parse)}),
                  (k, p_parse, p_check, {(p_check, 3): bad(p_check), (p_parse, 9): bad(p_parse)}),
                  (k, p_parse, p_check, {(p_check, 9): broken(p_check, 9), (p_parse, 3): broken(p_parse, 3)}),
                  (k, p_parse, p_check, {(p_check, 3): broken(p_check, 3), (p_parse, 9): broken(p_parse, 9)})]
    for k, p_parse, p_check, extra in cases:
        data = build(extra)
        part_of = deal(data, k)
        assert part_of[p_parse] == 1 and part_of[p_check] != 1
        out, info = whole_run(engines, data, gap_open=10, max_gap=100000)
        assert info.error.code != 0 and out == b""
        res, workers = parts_run(engines, data, k, gap_open=10, max_gap=100000)
        e = res["error"]
        assert e is not None and res["out"] is None and res["total"] == 0  # nothing is written
        assert (e["code"], e["stage"], e["record"]) == (info.error.code, info.error.stage, info.error.record), (k, sorted(extra))
    # the asserts of the trim (every record of every part fails: the lowest global record)
    data = build({})
    out, info = whole_run(engines, data, trim=1.5)
    res, _ = parts_run(engines, data, 3, trim=1.5)
    assert info.error.code == O.ERR_CHAIN_ASSERT == res["error"]["code"] and res["error"]["record"] == info.error.record == 0


def test_two_ranks_over_gloo_on_one_gpu(engines, tmp_path):
    """shard.chain_sharded in two fresh processes that share this GPU, gloo carrying the exchanges; the output gathered on rank 0
    equals the one-process output"""
    data = collinear_set(random.Random(55), 4000, n_q=9, n_t=3)
    want, info = whole_run(engines, data)
    assert info.error.code == 0
    src, dst = tmp_path / "in.paf", tmp_path / "out.paf"
    src.write_bytes(data)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "chain_sharded_run.py"), "--input", str(src), "--output", str(dst), "--one-device",
           "--batch-bytes", "200000"]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE) for r in range(2)]
    outs = [p.communicate(timeout=330) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err.decode()[-2000:]
    assert dst.read_bytes() == want
    # a failing record: both ranks agree, rank 0 reports, nothing is written
    bad = data + line("q1", 110, 200, "t", 120, 200, 80, ql=150)
    _, info = whole_run(engines, bad)
    src.write_bytes(bad)
    dst.unlink()
    errf = tmp_path / "err.json"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen(cmd + ["--error", str(errf)], env=dict(env, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(2)]
    outs = [p.communicate(timeout=330) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err.decode()[-2000:]
    e = json.loads(errf.read_text())
    assert not dst.exists() and (e["code"], e["record"]) == (info.error.code, info.error.record)

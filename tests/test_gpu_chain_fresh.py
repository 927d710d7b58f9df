"""`paffy chain` with the reference's walk from a fresh iterator switched on (paffy_hip_chain_fresh_walk; impl/chaining.c:71-86): every
output against the oracle AS COMMITTED, walk on, byte for byte -- no input is skipped and none is compared with the switched-off oracle
except to show that the switch is off by default. tests/test_chain_fresh_cpu.py shows on the oracle that each input hits its case;
tests/test_chain_fresh_abi.py has what needs no GPU of T8 (the launcher under PAFFY_GPUS=2, the exported symbols).
Stats: [records of leading runs the flag kernel processed, flagged fresh, links only the walk gives, candidates the first recurrence
skipped]."""
import os
import subprocess

import pytest

import chain_fresh_cases as K
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
E_UNSUPPORTED = -3


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    e = paffy_amd.Engine()
    yield e
    e.close()


def on(eng, data, **kw):
    """the run with the switch on: the oracle's bytes, and the stats"""
    want, code, _, _ = K.want(data, **kw)
    assert code == 0
    got, info = eng.chain(data, fresh_walk=True, **kw)
    assert info.error.code == 0 and got == want
    return eng.chain_fresh_stats()


def test_t1_the_pair(eng):
    got, _ = eng.chain(K.T1, fresh_walk=True, **K.T1_KW)
    assert got == K.want(K.T1, **K.T1_KW)[0] and got.count(b"s1:i:200") == 2
    st = eng.chain_fresh_stats()
    assert st[0] == 2 and st[1] >= 1 and st[2:] == [1, 1]
    # the switch is off again, through the same engine: today's two chains, and nothing counted
    got, _ = eng.chain(K.T1, **K.T1_KW)
    assert got == K.want(K.T1, fresh_walk=False, **K.T1_KW)[0] and got.count(b"s1:i:100") == 2
    assert eng.chain_fresh_stats() == [0, 0, 0, 0]
    # sticky through chain_fresh_walk
    eng.chain_fresh_walk(True)
    try:
        assert eng.chain(K.T1, **K.T1_KW)[0].count(b"s1:i:200") == 2
    finally:
        eng.chain_fresh_walk(False)
    st = on(eng, K.T1_NEG, **K.T1_KW)
    assert st[0] == 2 and st[2:] == [1, 1]
    assert on(eng, K.A + K.B, **K.T1_KW) == [0, 0, 0, 0]  # a + b: nothing skipped, nothing sequential ran
    import paffy_amd

    assert paffy_amd.chain(K.T1, trim=0.0, fresh_walk=True) == K.want(K.T1, **K.T1_KW)[0]
    assert paffy_amd.chain(K.T1, trim=0.0) == K.want(K.T1, fresh_walk=False, **K.T1_KW)[0]


def test_t2_removal_history(eng):
    st = on(eng, K.T2, **K.T2_KW_REMOVED)  # the walk of J removed E: the search of S is fresh
    assert st[2] == 1 and st[3] == 1
    st = on(eng, K.T2, **K.T2_KW_KEPT)  # E stays: S's search is not fresh although it skipped P
    assert st[2] == 0 and st[3] == 1 and st[0] > 0
    assert eng.chain(K.T2, fresh_walk=True, **K.T2_KW_KEPT)[0].count(b"s1:i:100") == 4


@pytest.mark.parametrize("which", sorted(K.T3_THIRD))
@pytest.mark.parametrize("first", [True, False])
def test_t3_the_end_of_the_leading_run(eng, which, first):
    st = on(eng, K.t3(which, first), trim=0.0)
    assert st[2] == K.t3_fresh_links(which, first)


def test_t4_two_candidates(eng):
    st = on(eng, K.T4, trim=0.0)
    assert st[2] == 1 and st[3] == 2
    assert eng.chain(K.T4, fresh_walk=True, trim=0.0)[0].count(b"s1:i:400") == 2


def test_t5_lane_and_window_edges(eng):
    data, _ = K.t5()
    st = on(eng, data, **K.T5_KW)
    assert st[0] == 200  # exactly up to the last pair, at run position 199
    assert st[3] == len(K.T5_PAIRS) and st[2] >= 3


def test_t6_the_big_group_kernel(eng):
    data, _ = K.t6()
    st = on(eng, data, **K.T6_KW)
    assert st[0] == K.T6_N and st[2] == 3 and st[3] == 3
    data0, _ = K.t6(False)
    assert on(eng, data0, **K.T6_KW) == [0, 0, 0, 0]  # no pair: nothing sequential ran


@pytest.mark.parametrize("seed", K.T7_SEEDS)
def test_t7_random_sets(eng, seed):
    kw = K.t7_kw(seed)
    for data in K.t7(seed):
        on(eng, data, **kw)
    if seed == 101:  # one of them in batches too: 3000 records, some twenty fresh candidates
        data = K.t7(seed)[4]
        assert K.t7_takes_the_walk(seed, 4)
        got, _ = eng.chain(data, fresh_walk=True, batch_bytes=40_000, **kw)
        assert got == K.want(data, **kw)[0]


def test_t7_enough_of_them_take_the_walk():
    assert sum(K.t7_takes_the_walk(seed, i) for seed in K.T7_SEEDS for i in range(len(K.T7_SIZES))) >= 20


def test_t8_the_cli_and_the_refusals(eng, tmp_path):
    from paffy_amd import shard

    kw = K.T2_KW_REMOVED
    args = ["chain", "-t", "0", "-d", str(kw["gap_open"]), "-e", str(kw["gap_extend"]), "-g", str(kw["max_gap"])]
    want_on, want_off = K.want(K.T2, **kw)[0], K.want(K.T2, fresh_walk=False, **kw)[0]
    assert want_on != want_off
    p = tmp_path / "in.paf"
    p.write_bytes(K.T2)
    env_on = dict(os.environ, PAFFY_CHAIN_FRESH_WALK="1")
    env_off = {k: v for k, v in os.environ.items() if k != "PAFFY_CHAIN_FRESH_WALK"}
    r = subprocess.run([PAFFY] + args + ["-i", str(p)], capture_output=True, env=env_on)
    assert r.returncode == 0 and r.stdout == want_on, r.stderr[-400:]
    r = subprocess.run([PAFFY] + args, input=K.T2, capture_output=True, env=env_on)
    assert r.returncode == 0 and r.stdout == want_on, r.stderr[-400:]
    r = subprocess.run([PAFFY] + args, input=K.T2, capture_output=True, env=env_off)
    assert r.returncode == 0 and r.stdout == want_off, r.stderr[-400:]
    # chain in parts under the switch: refused, nothing changed
    eng.chain_fresh_walk(True)
    try:
        buf = eng.to_device(K.T2)
        with pytest.raises(RuntimeError, match=r"paffy_hip_chain_run_part failed \(%d\)" % E_UNSUPPORTED):
            eng.chain_part([(buf, len(K.T2))], trim=0.0)
    finally:
        eng.chain_fresh_walk(False)
    assert eng.chain_part([(buf, len(K.T2))], trim=0.0).error.code == 0
    with pytest.raises(ValueError, match="leading single-group run"):
        shard.chain_in_parts([shard.GpuChainWorker(eng, trim=0.0)], [K.T2], fresh_walk=True)
    with pytest.raises(ValueError, match="leading single-group run"):
        shard.chain_sharded(shard.GpuChainWorker(eng, trim=0.0), None, 0, 1, [K.T2], 0, fresh_walk=True)


def test_t9_errors_unchanged_under_the_switch(eng):
    for data, kw in ((K.T9_BAD_LINE, {}), (K.T2, dict(trim=1.5)), (K.T9_BROKEN, {})):
        _, code, record, _ = K.want(data, **kw)
        assert code != 0
        out, info = eng.chain(data, fresh_walk=True, raise_on_error=False, **kw)
        assert out == b"" and info.error.code == code and info.error.record == record
    env = dict(os.environ, PAFFY_CHAIN_FRESH_WALK="1")
    r = subprocess.run([PAFFY, "chain"], input=K.T9_BROKEN, capture_output=True, env=env)
    r0 = subprocess.run([PAFFY, "chain"], input=K.T9_BROKEN, capture_output=True)
    assert r.returncode == r0.returncode == 1 and r.stdout == b"" and r.stderr == r0.stderr
    assert O.ERR_CHECK_QEND == K.want(K.T9_BROKEN)[1]

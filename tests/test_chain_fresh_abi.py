"""The fresh-iterator switch of `paffy chain` without a GPU: the two entry points are exported and declared, the Python layer binds
them and refuses the switch for chain in parts, and the N-GPU launcher leaves `chain` to one worker while PAFFY_CHAIN_FRESH_WALK is set
(a strand's leading run is a property of the whole input, not of a part)."""
import inspect
import os
import re
import subprocess

import pytest

import chain_fresh_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
STANDIN = os.path.join(ROOT, "tests", "standin_chain_worker.py")


def test_the_entry_points_are_exported_and_declared():
    from paffy_amd import engine

    lib = engine.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        header = fh.read()
    for name, args in (("paffy_hip_chain_fresh_walk", r"paffy_hip_ctx \*ctx, int on"), ("paffy_hip_chain_fresh_stats", r"paffy_hip_ctx \*ctx, int64_t out\[4\]")):
        assert re.search(r"\bT %s\b" % name, nm.stdout), name
        assert re.search(r"^int %s\(%s\);" % (name, args), header, re.M), name
    # paffy_chain_opts keeps its layout: the switch is the context's
    body = re.search(r"typedef struct \{([^}]*)\} paffy_chain_opts;", header).group(1)
    fields = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", f)).strip() for f in body.split(";")]
    assert [f for f in fields if f] == ["int64_t gap_open, gap_extend", "int64_t max_gap_length", "float trim_fraction"]


def test_the_python_layer_has_the_switch_and_parts_refuse_it():
    import paffy_amd
    from paffy_amd import shard

    assert inspect.signature(paffy_amd.Engine.chain).parameters["fresh_walk"].default is False
    assert inspect.signature(paffy_amd.chain).parameters["fresh_walk"].default is False
    assert inspect.signature(paffy_amd.Engine.chain_fresh_walk).parameters["on"].default is True
    assert callable(paffy_amd.Engine.chain_fresh_stats)
    # refused before anything touches a device
    with pytest.raises(ValueError, match="leading single-group run"):
        shard.chain_in_parts([None], [K.T2], fresh_walk=True)
    with pytest.raises(ValueError, match="leading single-group run"):
        shard.chain_sharded(None, None, 0, 1, [K.T2], 0, fresh_walk=True)


def test_the_launcher_leaves_chain_to_one_worker_under_the_switch(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s", "../bin/paffy"])
    base = {k: v for k, v in os.environ.items() if k != "PAFFY_CHAIN_FRESH_WALK"}
    data = b"".join(K.line("c%d" % (k % 3), 100 * k, 100 * k + 50, "t", 100 * k, 100 * k + 50, 50) for k in range(30))
    log = tmp_path / "log.txt"
    # without the variable the command is cut: two stand-in workers, as in tests/test_launcher_chain.py
    env = dict(base, PAFFY_GPUS="2", PAFFY_WORKER=STANDIN, PAFFY_ONE_DEVICE="1", PAFFY_TMPDIR=str(tmp_path), STANDIN_CHAIN_LOG=str(log))
    r = subprocess.run([PAFFY, "chain", "-g", "5"], input=data, capture_output=True, env=env, timeout=60)
    assert r.returncode == 0 and len(log.read_text().splitlines()) == 2
    # with it: one worker gets the command line as it was given (the worker here says what it was started with), nothing is spooled
    echo = dict(base, PAFFY_WORKER="/bin/echo", PAFFY_TMPDIR=str(tmp_path), PAFFY_CHAIN_FRESH_WALK="1")
    one = subprocess.run([PAFFY, "chain", "-g", "5"], input=data, capture_output=True, env=dict(echo, PAFFY_GPUS="1"), timeout=30)
    two = subprocess.run([PAFFY, "chain", "-g", "5"], input=data, capture_output=True, env=dict(echo, PAFFY_GPUS="2"), timeout=30)
    assert one.stdout == two.stdout == b"chain -g 5\n" and two.stderr == b""
    assert [f for f in os.listdir(tmp_path) if f.startswith("paffy.")] == []
    said = subprocess.run([PAFFY, "chain", "-l", "INFO", "-g", "5"], input=data, capture_output=True, env=dict(echo, PAFFY_GPUS="2"), timeout=30)
    assert said.stdout == b"chain -l INFO -g 5\n" and b"PAFFY_CHAIN_FRESH_WALK" in said.stderr and b"one worker" in said.stderr
    # PAFFY_CHAIN_FRESH_WALK=0 is off
    off = subprocess.run([PAFFY, "chain", "-g", "5"], input=data, capture_output=True, env=dict(env, PAFFY_CHAIN_FRESH_WALK="0"), timeout=60)
    assert off.returncode == 0 and off.stdout == r.stdout

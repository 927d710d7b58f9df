"""bench.py's own contract: a plain run prints the headline line alone, `--dump-outputs DIR` writes what the last timed step computed
(compared here with the CPU oracle over the same records of the stream), and `--full` adds the per-kernel and CPU figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import oracle_lib as O
import synth_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_by_kernel", "kernel_ms", "cpu_baseline")


def _bench(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _dumped(d):
    files = sorted(os.listdir(d))
    assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
    assert all(f.endswith(".npy") and a.dtype in (np.float32, np.float64) for f, a in zip(files, out.values()))
    return out


def _expected(tmp_path, text, counts):
    d = str(tmp_path / "want")
    bench.dump_outputs(d, torch.frombuffer(bytearray(text), dtype=torch.uint8) if text else torch.zeros(0, dtype=torch.uint8), counts)
    return _dumped(d)


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("flags, seed, mean_ops, r0, n, kinds", [
    # cfg3, 3 steps of 512 records: the last timed step reads batch 2 of the stream
    (("--batch", "512", "--steps", "2", "--warmup", "1"), 0x5EED0003, 2048, 1024, 512, (O.INVERT, O.TRIM_IDENTITY, O.SHATTER)),
    # more steps than one pass over the stream holds batches (4 of 250 000 records): step 5 reads batch 1 again
    (("--workload", "cfg2", "--mean-ops", "16", "--batch", "250000", "--steps", "5", "--warmup", "1"), 0x5EED0002, 16, 250000, 250000, (O.SHATTER,)),
])
def test_plain_run_dumps_the_last_step(tmp_path, flags, seed, mean_ops, r0, n, kinds):
    d = str(tmp_path / "got")
    line = _bench(*flags, "--dump-outputs", d)
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["steps"] == int(flags[flags.index("--steps") + 1]) and line["ms_per_step"] > 0 and line["value"] > 0
    data = synth_lib.generate(seed, mean_ops, r0, n)
    want, err = O.run([O.stage(k) for k in kinds], data)
    assert err.code == 0
    got = _dumped(d)
    assert got["text_windows"].shape == (256, 16384)
    _same(got, _expected(tmp_path, want, (n, want.count(b"\n"), len(data), len(want))))


def test_tile_run_dumps_the_last_step(tmp_path):
    """cfg5, 2 steps of 3000 records: the last one tiles records 3000..5999."""
    d = str(tmp_path / "got")
    line = _bench("--workload", "cfg5", "--batch", "3000", "--steps", "1", "--warmup", "1", "--dump-outputs", d)
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    data = synth_lib.generate(0x5EED0005, 2048, 3000, 3000)
    want, err = O.tile(data)
    assert err.code == 0
    _same(_dumped(d), _expected(tmp_path, want, (3000, want.count(b"\n"), len(data), len(want))))


def test_full_run_adds_the_kernel_and_cpu_figures():
    line = _bench("--full", "--batch", "512", "--steps", "2", "--warmup", "1", "--cpu-sample", "256")
    assert all(k in line for k in HEADLINE + FULL_ONLY + ("cpu_baseline_all_cores", "end_to_end", "flat_pass"))
    assert line["roofline"]["kernel_events"] == "dominant" and line["kernel_ms"]
    assert line["cpu_baseline"]["gpu_output_matches"] is True and line["cpu_baseline_all_cores"]["ok"] is True

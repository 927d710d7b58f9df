"""One recorded run of `bin/paffy dedupe -a` behind the CLI: one worker (PAFFY_GPUS unset) against PAFFY_GPUS=2 and 4 with
PAFFY_ONE_DEVICE=1, on one file of cfg3 records (bench.py's default stream), a quarter of them repeats of earlier records. The workers
share ONE GPU, so this is no scaling figure: it shows what the host steps of the sharded command cost next to the one-worker command --
the launcher's copy of the round's segments (its own stderr line at -l INFO), the exchange files and the waiting at the four barriers of
every round (every worker's stderr line at -l INFO). PAFFY_CHUNK_MB sets the share, so --chunk-mb decides the number of rounds. Every
sharded output is compared with the one-worker output. Nothing is asserted on the times."""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--mean-ops", type=int, default=2048)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--dir", default=None, help="where the input, the outputs and the spools go (default: /dev/shm if it has room, else the temp dir)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()

    import paffy_amd

    eng = paffy_amd.Engine()
    fresh = a.records * 3 // 4
    buf, nbytes = eng.synth(0x5EED0003, a.mean_ops, 0, fresh)
    text = buf[:nbytes].cpu().numpy()
    buf, n2 = eng.synth(0x5EED0003, a.mean_ops, 0, a.records - fresh)  # the first records once more, behind all of them
    again = buf[:n2].cpu().numpy()
    del buf
    eng.close()
    nbytes += n2
    base = a.dir
    if base is None:
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 6 * nbytes else tempfile.gettempdir()
    work = tempfile.mkdtemp(prefix="dedupe_cli_", dir=base)
    runs, want = [], None
    try:
        src = os.path.join(work, "in.paf")
        with open(src, "wb") as fh:
            text.tofile(fh)
            again.tofile(fh)
        del text, again
        for gpus in (1, 2, 4):
            env = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_WORKER", "PAFFY_ONE_DEVICE") and not k.startswith("PAFFY_DEDUPE")}
            env.update(PAFFY_TMPDIR=work, PAFFY_CHUNK_MB=str(a.chunk_mb))
            shown = f"PAFFY_CHUNK_MB={a.chunk_mb} bin/paffy dedupe -a -l INFO -i in.paf -o out.paf"
            if gpus > 1:
                env.update(PAFFY_GPUS=str(gpus), PAFFY_ONE_DEVICE="1")
                shown = f"PAFFY_GPUS={gpus} PAFFY_ONE_DEVICE=1 " + shown
            dst = os.path.join(work, f"out{gpus}.paf")
            t0 = time.perf_counter()
            p = subprocess.run([os.path.join(ROOT, "bin", "paffy"), "dedupe", "-a", "-l", "INFO", "-i", src, "-o", dst], env=env, capture_output=True, timeout=900)
            wall = time.perf_counter() - t0
            if p.returncode != 0:
                raise SystemExit(f"{shown}: status {p.returncode}\n{p.stderr.decode()[-2000:]}")
            got, out_bytes = digest(dst), os.path.getsize(dst)
            os.unlink(dst)
            want = want or got
            run = {"command": shown, "workers": gpus, "wall_s": round(wall, 3), "records_per_s": round(a.records / wall), "out_bytes": out_bytes, "equals_one_worker": got == want}
            m = re.search(rb"(\d+) workers, (\d+) rounds; launcher: copy ([0-9.]+) s of ([0-9.]+) s", p.stderr)
            if m:
                run.update(workers_started=int(m.group(1)), rounds=int(m.group(2)), launcher_s={"copy": float(m.group(3)), "whole": float(m.group(4))})
            parts = re.findall(rb"part (\d+) of \d+, \d+ rounds: exchange files ([0-9.]+) s, waiting for the others ([0-9.]+) s of ([0-9.]+) s", p.stderr)
            if parts:
                run["worker_s"] = [{"part": int(r), "exchange_files": float(f), "waiting": float(w), "whole": float(t)} for r, f, w, t in sorted(parts, key=lambda x: int(x[0]))]
            runs.append(run)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    res = {"what": "bin/paffy dedupe -a behind the CLI, wall time of the whole command (file in, file out)", "records": a.records, "mean_ops": a.mean_ops, "in_bytes": int(nbytes),
           "chunk_mb": a.chunk_mb, "files_under": base,
           "note": "the workers of the sharded runs share ONE GPU (PAFFY_ONE_DEVICE=1): no scaling figure, and no run of this command on N GPUs has been measured; "
                   "launcher_s.copy is the launcher's copy of the rounds' segments to the output, worker_s.exchange_files a worker's time in the entry, count and "
                   "verdict files, worker_s.waiting its time between a report and the answer (the other workers' work included); the rest of a worker's time is "
                   "its reads of the input, the GPU calls and the spool write",
           "runs": runs}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if not all(r["equals_one_worker"] for r in runs):
        raise SystemExit("a sharded output differs from the one-worker output")


if __name__ == "__main__":
    main()

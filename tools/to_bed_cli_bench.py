"""One recorded run of `bin/paffy to_bed` behind the CLI, without and with -n: one worker (PAFFY_GPUS unset) against PAFFY_GPUS=2 and 4 with
PAFFY_ONE_DEVICE=1, on one file of cfg3 records (the generator of tools/bench_extra.py). The workers share ONE GPU, so this is no scaling
figure: it shows what the launcher's host steps (partition and merge -- its own stderr line at -l INFO) and the spool files cost next to
the one-worker command; with -n most lines are spooled twice. Every sharded output is compared with the one-worker output. Nothing is
asserted on the times."""
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
    ap.add_argument("--records", type=int, default=300000)
    ap.add_argument("--mean-ops", type=int, default=2048)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--dir", default=None, help="where the input, the outputs and the spools go (default: /dev/shm if it has room, else the temp dir)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()

    import paffy_amd

    eng = paffy_amd.Engine()
    buf, nbytes = eng.synth(0x5EED0005, a.mean_ops, 0, a.records, n_contigs=a.contigs)
    text = buf[:nbytes].cpu().numpy()
    del buf
    eng.close()
    base = a.dir
    if base is None:
        base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 6 * nbytes else tempfile.gettempdir()
    work = tempfile.mkdtemp(prefix="to_bed_cli_", dir=base)
    runs = []
    try:
        src = os.path.join(work, "in.paf")
        text.tofile(src)
        del text
        for flags in ([], ["-n"]):
            want = None
            for gpus in (1, 2, 4):
                env = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_WORKER", "PAFFY_ONE_DEVICE")}
                env["PAFFY_TMPDIR"] = work
                shown = " ".join(["bin/paffy to_bed"] + flags + ["-l INFO -i in.paf -o out.bed"])
                if gpus > 1:
                    env.update(PAFFY_GPUS=str(gpus), PAFFY_ONE_DEVICE="1")
                    shown = f"PAFFY_GPUS={gpus} PAFFY_ONE_DEVICE=1 " + shown
                dst = os.path.join(work, f"out{gpus}.bed")
                t0 = time.perf_counter()
                p = subprocess.run([os.path.join(ROOT, "bin", "paffy"), "to_bed"] + flags + ["-l", "INFO", "-i", src, "-o", dst], env=env, capture_output=True,
                                   timeout=900)
                wall = time.perf_counter() - t0
                if p.returncode != 0:
                    raise SystemExit(f"{shown}: status {p.returncode}\n{p.stderr.decode()[-2000:]}")
                got = digest(dst)
                out_bytes = os.path.getsize(dst)
                os.unlink(dst)
                want = want or got
                run = {"command": shown, "workers": gpus, "wall_s": round(wall, 3), "records_per_s": round(a.records / wall), "out_bytes": out_bytes,
                       "equals_one_worker": got == want}
                m = re.search(rb"(\d+) workers; launcher: partition ([0-9.]+) s, merge ([0-9.]+) s", p.stderr)
                if m:
                    run["workers_started"] = int(m.group(1))
                    run["launcher_s"] = {"partition": float(m.group(2)), "merge": float(m.group(3))}
                runs.append(run)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    res = {"what": "bin/paffy to_bed behind the CLI, wall time of the whole command (file in, file out), without and with -n", "records": a.records, "mean_ops": a.mean_ops,
           "contigs": a.contigs, "in_bytes": int(nbytes), "files_under": base,
           "note": "the workers of the sharded runs share ONE GPU (PAFFY_ONE_DEVICE=1): no scaling figure; launcher_s is the launcher's own time for "
                   "its host steps, the rest of the wall time is the workers (file read, GPU, spool write); with -n a line whose two names have different "
                   "owners is spooled twice",
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

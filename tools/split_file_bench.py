"""Wall time of `bin/paffy split_file -q` behind the CLI on the synthetic stream of paffy_hip_synth_contigs, once with few contigs and
once with many (the host's share of the command grows with the number of names), files written under /dev/shm. Per contig count: one
warm-up run, then the wall times of --runs runs (median, min, max). With --paffy the same measurement runs on another build's binary
(the commit before, say), so that two JSON lines can be put side by side. Without --paffy the time inside paffy_hip_split_plan is
read per kernel from paffy_hip_profile_read on one batch of --profile-records records. Nothing is asserted on the times; the
directories of the two contig counts are compared between the runs of one binary (same files, same bytes)."""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dir_digest(d):
    h = hashlib.sha256()
    names = sorted(os.listdir(d))
    for n in names:
        h.update(n.encode() + b"\0")
        with open(os.path.join(d, n), "rb") as fh:
            for block in iter(lambda: fh.read(1 << 24), b""):
                h.update(block)
    return len(names), h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--mean-ops", type=int, default=2048)
    ap.add_argument("--contigs", type=int, nargs="+", default=[25, 2000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--profile-records", type=int, default=20000)
    ap.add_argument("--paffy", default=os.path.join(ROOT, "bin", "paffy"), help="the binary to time")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--dir", default=None, help="where the input and the output directories go (default: /dev/shm if it has room, else the temp dir)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()

    import paffy_amd

    eng = paffy_amd.Engine()
    cases = []
    for n_contigs in a.contigs:
        buf, nbytes = eng.synth(0x5EED0003, a.mean_ops, 0, a.records, n_contigs=n_contigs)
        text = buf[:nbytes].cpu().numpy()
        del buf
        base = a.dir
        if base is None:
            base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 4 * nbytes else tempfile.gettempdir()
        work = tempfile.mkdtemp(prefix="split_file_", dir=base)
        try:
            src = os.path.join(work, "in.paf")
            with open(src, "wb") as fh:
                text.tofile(fh)
            del text
            walls, seen = [], None
            for k in range(a.runs + 1):  # run 0 warms up
                out = os.path.join(work, f"out{k}")
                os.mkdir(out)
                t0 = time.perf_counter()
                p = subprocess.run([a.paffy, "split_file", "-q", "-i", src, "-p", out + "/s_"], capture_output=True, timeout=600)
                wall = time.perf_counter() - t0
                if p.returncode != 0:
                    raise SystemExit(f"{a.paffy} split_file -q: status {p.returncode}\n{p.stderr.decode()[-2000:]}")
                got = dir_digest(out)
                shutil.rmtree(out)
                if seen is not None and got != seen:
                    raise SystemExit("two runs of one binary wrote different directories")
                seen = got
                if k:
                    walls.append(wall)
            case = {"contigs": n_contigs, "in_bytes": int(nbytes), "files": seen[0], "sha256_of_directory": seen[1], "wall_s": [round(w, 3) for w in walls],
                    "median_s": round(statistics.median(walls), 3), "min_s": round(min(walls), 3), "max_s": round(max(walls), 3)}
        finally:
            shutil.rmtree(work, ignore_errors=True)
        if a.paffy == ap.get_default("paffy"):  # this build: the time inside paffy_hip_split_plan, per kernel, on one batch
            buf, nb = eng.synth(0x5EED0003, a.mean_ops, 0, a.profile_records, n_contigs=n_contigs)
            eng.split_begin(True, 0)
            eng.split_plan(buf, nb)  # sizes the buffers
            eng.profile(True)
            eng.split_begin(True, 0)
            t0 = time.perf_counter()
            info = eng.split_plan(buf, nb)
            whole = time.perf_counter() - t0
            prof = eng.profile_read()
            eng.profile(False)
            case["split_plan"] = {"records": info.n_records, "in_bytes": nb, "files": len(eng.split_groups()), "host_wall_ms": round(whole * 1e3, 3),
                                  "kernel_ms": {k: round(v[0], 4) for k, v in prof.items()},
                                  "k_split_ms": round(sum(v[0] for k, v in prof.items() if k.startswith("k_split_")), 4)}
            del buf
        cases.append(case)
    eng.close()
    res = {"what": "bin/paffy split_file -q behind the CLI, wall time of the whole command (file in, one file per query contig out)", "label": a.label,
           "records": a.records, "mean_ops": a.mean_ops, "runs": a.runs, "cases": cases}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

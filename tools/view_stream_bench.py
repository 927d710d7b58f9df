"""Wall time of `bin/paffy view` behind the CLI: `view -s`, `view -s -t` and `view -a -s` on records of the cfg4 generator with its FASTA
(Synth4(0x5EED0004, 2048, n_contigs=6, tlen_min=200_000, tlen_span=200_000), the input of `tools/bench_extra.py --cmd view_lines`'s CLI
figure), input and output under /dev/shm. Several builds are timed in one call, alternating (--build LABEL=PATH of a bin/paffy; a
LABEL that ends in @N runs it with PAFFY_GPUS=N PAFFY_ONE_DEVICE=1, a rehearsal on one GPU and labelled as such): one untimed run of
every form and build first, then --runs rounds, the order of the builds rotated from round to round so that no build always runs
first; per form and build the wall times, their median and their spread (max - min), and the SHA-256 of the output, taken after every
run outside the timed span, which must be the same for every build and run. Every run sets PAFFY_STREAM_TIMES=1: a worker that knows it
prints where its stream loop's time went (open, read, submit, drain, close), and the medians of those phases are kept per form and
build; "outside_loop_s" is the wall time less their sum (process start, context, FASTA load, teardown). `view -a -s` runs on the first
--rows-records records: the rows of all 200 000 would be 25 GB of text. The records are generated on the device (paffy_hip_synth4) and checked against the host
generator's first records; the genomes come from the host generator. Nothing is asserted on the times."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
FORMS = {"view -s": ["-s"], "view -s -t": ["-s", "-t"], "view -a -s": ["-a", "-s"]}


def file_digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def make_input(work, records, rows_records):
    import numpy as np

    import paffy_amd
    import synth_lib

    cfg = dict(n_contigs=6, tlen_min=200_000, tlen_span=200_000)
    host = synth_lib.Synth4(0x5EED0004, 2048, **cfg)
    fa = os.path.join(work, "g.fa")
    with open(fa, "wb") as fh:
        for name, s in host.genomes().items():
            fh.write(b">" + (name if isinstance(name, bytes) else name.encode()) + b"\n" + s + b"\n")
    eng = paffy_amd.Engine()
    eng.synth4_setup(0x5EED0004, 2048, genomes=False, **cfg)
    buf, nbytes = eng.synth4(0, records)
    text = buf[:nbytes].cpu().numpy()
    eng.close()
    generator = "device"
    head = host.records(0, min(records, 64))
    if text[:len(head)].tobytes() != head:  # the two generators are meant to agree; the host's is the one the tests use
        generator = "host"
        text = np.frombuffer(host.records(0, records, threads=16), dtype=np.uint8)
        nbytes = text.size
    paf = os.path.join(work, "in.paf")
    with open(paf, "wb") as fh:
        text.tofile(fh)
    rows_paf, rows_bytes = paf, int(nbytes)
    if rows_records < records:  # the first rows_records lines
        rows_bytes = int(np.flatnonzero(text == 10)[rows_records - 1]) + 1
        rows_paf = os.path.join(work, "rows.paf")
        with open(rows_paf, "wb") as fh:
            text[:rows_bytes].tofile(fh)
    return paf, rows_paf, fa, int(nbytes), rows_bytes, generator


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--rows-records", type=int, default=20000, help="records of the `view -a -s` input")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--build", action="append", default=[], help="LABEL=PATH of a bin/paffy; LABEL@N: with PAFFY_GPUS=N PAFFY_ONE_DEVICE=1")
    ap.add_argument("--dir", default=None, help="where input and output go (default: /dev/shm if there is one)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    builds = []
    for b in a.build or ["this commit=" + os.path.join(ROOT, "bin", "paffy")]:
        label, path = b.split("=", 1)
        gpus = int(label.rsplit("@", 1)[1]) if "@" in label else 1
        builds.append((label, path, gpus))
    base = a.dir or ("/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    work = tempfile.mkdtemp(prefix="view_stream_", dir=base)
    try:
        paf, rows_paf, fa, in_bytes, rows_in_bytes, generator = make_input(work, a.records, min(a.rows_records, a.records))
        out = os.path.join(work, "out.txt")
        walls = {f: {b[0]: [] for b in builds} for f in FORMS}
        phases = {f: {b[0]: [] for b in builds} for f in FORMS}
        seen = {}
        env0 = {k: v for k, v in os.environ.items() if k not in ("PAFFY_GPUS", "PAFFY_ONE_DEVICE", "PAFFY_CHUNK_MB")}
        for k in range(a.runs + 1):  # round 0 warms up
            for form, flags in FORMS.items():
                src = rows_paf if "-a" in flags else paf
                order = builds[k % len(builds):] + builds[:k % len(builds)]  # rotated: no build always follows the same one
                for label, path, gpus in order:
                    env = dict(env0, PAFFY_TMPDIR=work, PAFFY_STREAM_TIMES="1")
                    if gpus > 1:
                        env.update(PAFFY_GPUS=str(gpus), PAFFY_ONE_DEVICE="1")
                    t0 = time.perf_counter()
                    p = subprocess.run([path, "view", *flags, "-i", src, "-o", out, fa], env=env, capture_output=True, timeout=900)
                    wall = time.perf_counter() - t0
                    if p.returncode != 0:
                        raise SystemExit(f"{label}: {form}: status {p.returncode}\n{p.stderr.decode()[-2000:]}")
                    got = (os.path.getsize(out), file_digest(out))
                    if form in seen and got != seen[form]:
                        raise SystemExit(f"{label}: {form}: the output differs from another run's")
                    seen[form] = got
                    os.unlink(out)
                    if k:
                        walls[form][label].append(wall)
                        for ln in p.stderr.decode(errors="replace").splitlines():
                            if ln.startswith("paffy stream times:") and gpus == 1:
                                w = ln.split()[3:]
                                ph = {w[i]: float(w[i + 1]) for i in range(0, len(w), 2)}
                                ph["outside_loop"] = wall - sum(v for name, v in ph.items() if name != "chunks")
                                phases[form][label].append(ph)
        forms = []
        for form, flags in FORMS.items():
            rows = "-a" in flags
            entry = {"form": form, "records": min(a.rows_records, a.records) if rows else a.records, "in_bytes": rows_in_bytes if rows else in_bytes,
                     "out_bytes": seen[form][0], "sha256": seen[form][1], "builds": {}}
            for label, _, gpus in builds:
                w = walls[form][label]
                entry["builds"][label] = {"gpus": gpus, "rehearsal_on_one_gpu": gpus > 1, "wall_s": [round(x, 3) for x in w], "median_s": round(statistics.median(w), 3),
                                          "min_s": round(min(w), 3), "max_s": round(max(w), 3), "spread_s": round(max(w) - min(w), 3)}
                if phases[form][label]:
                    entry["builds"][label]["median_phase_s"] = {name: round(statistics.median(ph[name] for ph in phases[form][label]), 4)
                                                                for name in phases[form][label][0]}
            forms.append(entry)
        res = {"what": "bin/paffy view behind the CLI, wall time of the whole command (file in, file out, both under " + base +
                       "), builds alternating, their order rotated from round to round",
               "runs": a.runs, "warmup_runs": 1, "record_generator": generator, "forms": forms,
               "note": "view -a -s runs on the first %d records: the rows of all %d would be too much text" % (min(a.rows_records, a.records), a.records),
               # what the device-side layout keeps off the bus: the sizes to the host and their running sums back, 8 bytes each per record
               "pcie_bytes_per_record_saved": {"sizes_to_host": 8, "offsets_to_device": 8, "records": a.records, "total_bytes": 16 * a.records}}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

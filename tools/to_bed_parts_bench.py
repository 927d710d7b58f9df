#!/usr/bin/env python3
"""Times `paffy to_bed` on the Synth4 stream of tests/test_gpu_to_bed.py (5 contigs of 1.5-2.5 Mb, both strands), resident in HBM:
the one-context run without and with -n (paffy_hip_bed_plan + emit), and, where the library has it, to_bed in parts
(paffy_amd.shard.to_bed_in_parts, -n) with --parts contexts on the one GPU taken in turn. Parts that share a GPU show the cost of
the partition, the split and the scatter, not a speed-up. One JSON line per figure; the smallest of --reps timed runs after a
warm-up. --tree DIR: import paffy_amd (with its built library) from another checkout, for example the parent commit's, so that one
copy of this script times both; it runs unchanged on a tree without the parts and then prints the one-context lines only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--label", default="")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose paffy_amd is timed (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import paffy_amd
    from paffy_amd import shard

    E = paffy_amd.engine
    eng = paffy_amd.Engine()
    eng.synth4_setup(0x5EED0004, 512, n_contigs=5, tlen_min=1_500_000, tlen_span=1_000_000, genomes=False)
    buf, nbytes = eng.synth4(0, a.records)
    torch.cuda.synchronize()

    sizes = {}

    def one_context(inverted):
        opts, info = E.BedOpts(0, 0, 0, inverted, 1), E.PlanInfo()
        assert E.lib().paffy_hip_bed_plan(eng._ctx, buf.data_ptr(), nbytes, opts, info) == 0 and info.error.code == 0
        out = eng.alloc_out(info.out_bytes)
        eng.emit(out)
        eng.sync()
        sizes[inverted] = info.out_bytes
        return out[: info.out_bytes]

    def timed(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return ts

    for inverted in (0, 1):
        ts = timed(lambda: one_context(inverted))
        print(json.dumps({"label": a.label, "cmd": "to_bed -n" if inverted else "to_bed", "records": a.records, "in_bytes": nbytes, "out_bytes": sizes[inverted], "ms": round(min(ts) * 1e3, 2),
                          "ms_all": [round(t * 1e3, 2) for t in ts], "records_per_s": round(a.records / min(ts), 1)}), flush=True)
    if not hasattr(shard, "to_bed_in_parts"):
        return 0
    want = one_context(1).clone()
    for k in a.parts:
        engines = [paffy_amd.Engine() for _ in range(k)]
        workers = [shard.GpuBedWorker(e) for e in engines]
        res = shard.to_bed_in_parts(workers, [(buf, nbytes)], dict(include_inverted=True))
        torch.cuda.synchronize()
        assert res["error"] is None and torch.equal(res["out"], want), "the parts do not write the one-context output"
        ts = timed(lambda: shard.to_bed_in_parts(workers, [(buf, nbytes)], dict(include_inverted=True)))
        print(json.dumps({"label": a.label, "cmd": "to_bed -n in parts", "parts": k, "records": a.records, "verified_against_one_context": True,
                          "ms": round(min(ts) * 1e3, 2), "ms_all": [round(t * 1e3, 2) for t in ts], "records_per_s": round(a.records / min(ts), 1)}), flush=True)
        for e in engines:
            e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

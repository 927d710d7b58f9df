#!/usr/bin/env python3
"""Times `paffy dedupe -a` on cfg3 records (bench.py's default stream: mean 2048 cigar ops) resident in HBM, a quarter of them
duplicates -- half of those of a record of the same round, half of a record of an earlier round: the one-context run
(paffy_hip_dedupe_plan + emit per round through one context) and, where the library has it, dedupe in parts
(paffy_amd.shard.dedupe_in_parts) with --parts contexts on the one GPU taken in turn. Parts that share a GPU show what the protocol
costs -- entries, owner's sort, verdicts, and k plans in turn --, not a speed-up. The input is --rounds rounds of --records / --rounds
records (a batch stays below 2 GiB); a round is cut into k consecutive shares of equal record counts.

One JSON line per figure: HIP events on the stream around the whole step (every round, plan and emit), one warm-up, the smallest and
the median of --reps runs. --tree DIR: import paffy_amd (with its built library) from another checkout, for example the parent
commit's, so that one copy of this script times both; on a tree without the parts it prints the one-context line only.

--decide-until M: times paffy_hip_dedupe_part_decide alone, the owner's step whose cost grows with its memory: rounds of --decide-round
fresh classes (random 128-bit class keys, no text) into one context until its memory holds at least M classes, the whole series --reps
times from a reset. One JSON line per round: the classes held before it, the milliseconds of every repeat, their smallest, median and
spread (largest - smallest). Run it on two builds (--tree, or PAFFY_HIP_LIB) to compare how they keep the memory sorted."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, MEAN_OPS = 0x5EED0003, 2048


def decide_series(a, torch, paffy_amd, eng):
    import ctypes as C

    L, n = paffy_amd.engine.lib(), a.decide_round
    n_rounds = -(-a.decide_until // n)
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    rounds = []
    for r in range(n_rounds):  # entries: class hi, class lo, global number, flags (bit 0: the own key is the class key)
        e = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, generator=gen)
        e[:, 2] = torch.arange(r * n, (r + 1) * n)
        e[:, 3] = 1
        rounds.append(e.to(eng.device))
    verdicts = torch.zeros(n + 64, dtype=torch.uint8, device=eng.device)
    ms = [[] for _ in range(n_rounds)]
    for rep in range(a.reps + 1):  # the first series warms up (buffers, code objects) and is not kept
        eng.dedupe_reset()
        for r, e in enumerate(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            rc = L.paffy_hip_dedupe_part_decide(eng._ctx, C.c_void_p(e.data_ptr()), n, 1, C.c_void_p(verdicts.data_ptr()))
            e1.record()
            torch.cuda.synchronize()
            assert rc == 0, rc
            if rep == 0:
                assert int((verdicts[:n] & 1).sum().item()) == n  # every class is new: all of them enter the memory
            else:
                ms[r].append(e0.elapsed_time(e1))
    for r in range(n_rounds):
        print(json.dumps({"label": a.label, "cmd": "part_decide", "round": r, "entries": n, "memory_before": r * n, "memory_after": (r + 1) * n, "ms": round(min(ms[r]), 3),
                          "ms_median": round(statistics.median(ms[r]), 3), "ms_spread": round(max(ms[r]) - min(ms[r]), 3), "ms_all": [round(t, 3) for t in ms[r]]}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--label", default="")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose paffy_amd is timed (default: this one)")
    ap.add_argument("--decide-until", type=int, default=0, help="time part_decide alone until the memory holds this many classes")
    ap.add_argument("--decide-round", type=int, default=131072, help="fresh classes per round of --decide-until")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import paffy_amd
    from paffy_amd import shard

    eng = paffy_amd.Engine()
    if a.decide_until > 0:
        return decide_series(a, torch, paffy_amd, eng)
    per_round = a.records // a.rounds
    fresh, dup = per_round * 3 // 4, per_round - per_round * 3 // 4

    def synth(r0, n):
        buf, nbytes = eng.synth(SEED, MEAN_OPS, r0, n)
        return buf[:nbytes]

    rounds = []  # uint8 tensors: 3/4 new records, 1/8 repeats of this round's first records, 1/8 repeats of the round before (round 0: its own)
    for r in range(a.rounds):
        near, far = dup // 2, dup - dup // 2
        rounds.append(torch.cat([synth(r * fresh, fresh), synth(r * fresh, near), synth(max(0, r - 1) * fresh + near, far)]))
    torch.cuda.synchronize()
    in_bytes = sum(int(t.numel()) for t in rounds)

    def padded(t):
        buf = torch.zeros((t.numel() + 15) // 16 * 16 + 16, dtype=torch.uint8, device=t.device)
        buf[: t.numel()] = t
        return buf, int(t.numel())

    whole = [padded(t) for t in rounds]

    def one_context():
        eng.dedupe_reset() if hasattr(eng, "dedupe_reset") else paffy_amd.engine.lib().paffy_hip_dedupe_reset(eng._ctx)
        outs = []
        for buf, n in whole:
            info = eng.dedupe_plan(buf, n, True)
            assert info.error.code == 0
            out = eng.alloc_out(info.out_bytes)
            eng.emit(out)
            outs.append(out[: info.out_bytes])
        eng.sync()
        return torch.cat(outs)

    def timed(fn):
        fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def line(cmd, ms, **more):
        return json.dumps(dict({"label": a.label, "cmd": cmd, "records": per_round * a.rounds, "rounds": a.rounds, "in_bytes": in_bytes, "ms": round(min(ms), 2),
                                "ms_median": round(statistics.median(ms), 2), "ms_all": [round(t, 2) for t in ms], "records_per_s": round(per_round * a.rounds / (min(ms) * 1e-3), 1)},
                               **more))

    want = one_context().clone()
    kept = int((want == 10).sum().item())
    print(line("dedupe -a, one context", timed(one_context), out_bytes=int(want.numel()), records_written=kept), flush=True)
    if not hasattr(shard, "dedupe_in_parts"):
        return 0
    for k in a.parts:
        cut = []
        for t in rounds:
            ends = (t == 10).nonzero().flatten() + 1
            n, at, shares = int(ends.numel()), 0, []
            for p in range(k):
                stop = int(ends[(p + 1) * n // k - 1].item()) if (p + 1) * n // k > 0 else 0
                shares.append(padded(t[at:stop]))
                at = stop
            cut.append(shares)
        engines = [paffy_amd.Engine() for _ in range(k)]
        workers = [shard.GpuDedupeWorker(e) for e in engines]
        res = shard.dedupe_in_parts(workers, cut, True)
        torch.cuda.synchronize()
        assert res["error"] is None and torch.equal(res["out"], want), "the parts do not write the one-context output"
        ms = timed(lambda: shard.dedupe_in_parts(workers, cut, True))
        print(line("dedupe -a in parts", ms, parts=k, verified_against_one_context=True, exchanged_bytes=res["exchanged"],
                   exchanged_bytes_per_record=round(res["exchanged"] / res["records"], 2), exchanged_share_of_input=round(res["exchanged"] / in_bytes, 5)), flush=True)
        for e in engines:
            e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Side measurements for DESIGN.md (not the driver's bench contract): `tile` and single commands
on the synthetic stream, records/s with inputs resident in HBM. dechunk / pass / upconvert: the cfg3 stream, chunk-named for the first two.
remove_eqx: `add_mismatches -a` on the cfg4 stream as `add_mismatches` wrote it (= and X runs: the command's real input; `remove` times
the plain M/I/D stream, where almost nothing merges). view / view_stats_only: what `paffy view` plans on the cfg4 stream -- [ADD_MISMATCHES,
STATS] and its sums, nothing emitted -- by the default plan and under Engine.stats_only (plan-only rates, inputs resident in HBM).
view_lines: the sums-only plan, then the per-record stats lines of `paffy view` written into device memory (paffy_hip_plan_view_sizes /
_view_text, view_line_kernel.h): plan + sizes + text, everything resident. shatter / invert_trim_shatter --names short: the cfg3 stream
with hs.chrN / pt.chrN renamed to chrN (first row pieces of 15 and 16 bytes, half and half): the share of such records, flat_stats and,
for shatter, the rows each row writer wrote. add_trim / add_filter: `paffy add_mismatches | paffy trim -r` and `| paffy filter -u 0.9`
as the fused stage lists [ADD_MISMATCHES, TRIM_IDENTITY] and [ADD_MISMATCHES, FILTER] on the cfg4 stream (flat_add_pipe_kernel.h), sequences
resident: the plan alone and plan + emit per repetition (the first two warm up and are not counted), median and spread (largest - smallest)
of the others, flat_stats, the per-kernel times, and with --sha the SHA-256 of the output (to compare two builds of the library, chosen by
PAFFY_HIP_LIB, byte for byte before their times)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chunk_encode(text, chunk=1_000_000):
    """every name becomes name|length|c, c its start rounded down to `chunk`; the coordinates shift by -c (what `faffy chunk` names)"""
    out = []
    for line in text.split(b"\n")[:-1]:
        f = line.split(b"\t", 9)
        for ni, li, si, ei in ((0, 1, 2, 3), (5, 6, 7, 8)):
            ln, s, e = int(f[li]), int(f[si]), int(f[ei])
            c = s // chunk * chunk
            f[ni] += b"|%d|%d" % (ln, c)
            f[li], f[si], f[ei] = b"%d" % (ln - c), b"%d" % (s - c), b"%d" % (e - c)
        out.append(b"\t".join(f))
    return b"\n".join(out) + b"\n"


def one_group_stream(n, seed=7):
    """n collinear records of one (query, target, strand) on one diagonal, 200-2000 bases long with gaps of 1-2000, shuffled; the last one
    in processing order abuts the one before it exactly and stands in front of it in the input (chain --one-group)"""
    import random

    rng = random.Random(seed)
    rows, at = [], 0
    for k in range(n):
        ln = rng.randrange(200, 2000)
        if k:
            at += 0 if k == n - 1 else rng.randrange(1, 2000)
        rows.append(b"chrA\t4000000000\t%d\t%d\t+\tchrB\t4000000000\t%d\t%d\t%d\t%d\t60\tAS:i:%d\tcg:Z:%dM\n" % (at, at + ln, at, at + ln, ln, ln, rng.randrange(500, 30000), ln))
        at += ln
    last, before = rows[n - 1], rows[n - 2]
    body = rows[:n - 2]
    rng.shuffle(body)
    return b"".join([last] + body + [before])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200000)
    ap.add_argument("--mean-ops", type=int, default=2048)
    ap.add_argument("--contigs", type=int, default=24, help="contigs of the synthetic stream (chain: fewer contigs = larger groups)")
    ap.add_argument("--cmd", default="tile", choices=["tile", "invert", "trim", "trimf", "trimf_invert", "trimf_filter", "trimf_stats", "shatter", "remove", "remove_eqx", "filter", "add", "add_trim", "add_filter", "view", "view_stats_only", "view_lines", "dedupe", "bed", "stats", "chain",
                                                    "dechunk", "upconvert", "pass", "faffy_chunk", "faffy_extract", "faffy_merge", "seqload", "ivload", "invert_trim_shatter"])
    ap.add_argument("--names", default="std", choices=["std", "short"],
                    help="shatter, invert_trim_shatter: `short` renames hs.chrN / pt.chrN to chrN on the host (outside the timed region): chr1-chr9 "
                         "then have a first row piece of 15 bytes, chr10-chr24 one of 16 -- about half and half, like a human assembly")
    ap.add_argument("--genome-gb", type=float, default=3.1, help="faffy_*: bases of the synthetic genome (24 contigs)")
    ap.add_argument("--intervals", type=int, default=1_000_000, help="faffy_extract: BED intervals")
    ap.add_argument("--sha256", action="store_true", help="faffy_*: copy the last repetition's output to the host and print its SHA-256")
    ap.add_argument("--scaffolds", type=int, default=0, help="seqload: an assembly of this many scaffolds (1-2000 bases) instead of the genome; ivload: this many chunk records "
                                                                  "scaf<i>|<len>|<start> (1-200 bases) instead of the genome's 24 contigs")
    ap.add_argument("--repeats", type=int, default=3, help="timed repeats of the plan (the smallest counts); seqload, faffy_*: repetitions, the first warms up; ivload: "
                                                                "the same, the median counts, and one more repetition under the profile")
    ap.add_argument("--skip-host-strings", action="store_true", help="seqload: do not time paffy_hip_set_sequences on the records as host strings")
    ap.add_argument("--sha", action="store_true", help="add_trim, add_filter: copy the last repetition's output to the host and print its SHA-256")
    ap.add_argument("--parts", type=int, default=0, help="chain: chain in parts -- this many contexts on the one GPU, taken in turn (0: the plain one-context run)")
    ap.add_argument("--fresh-walk", action="store_true", help="chain: with paffy_hip_chain_fresh_walk on (the reference's walk from a fresh iterator)")
    ap.add_argument("--one-group", action="store_true",
                    help="chain: instead of the synthetic stream, --records collinear records of ONE (query, target, strand), shuffled, chained with -t 0; the "
                         "last one in processing order abuts its predecessor exactly and stands in front of it in the input, so that under --fresh-walk "
                         "the flag kernel takes the whole input one record after the other: its worst case")
    a = ap.parse_args()
    if a.cmd == "chain" and a.parts > 0:
        return chain_parts_bench(a)
    if a.cmd.startswith("faffy_"):
        return faffy_bench(a)
    if a.cmd == "seqload":
        return seqload_bench(a)
    if a.cmd == "ivload":
        return ivload_bench(a)
    import torch

    import paffy_amd

    eng = paffy_amd.Engine()
    view = a.cmd in ("view", "view_stats_only", "view_lines")
    add_pipe = {"add_trim": [paffy_amd.ADD_MISMATCHES, paffy_amd.TRIM_IDENTITY], "add_filter": [paffy_amd.ADD_MISMATCHES, paffy_amd.FILTER]}.get(a.cmd)
    if a.cmd in ("add", "remove_eqx") or view or add_pipe:
        # cfg4: 24 + 24 contigs of 50-250 Mb generated on the device, records on homologous bases (2 % substitutions)
        t0 = time.perf_counter()
        if os.environ.get("PAFFY_X_SMALL_GENOME"):  # experiment: genomes small enough to stay in the caches
            eng.synth4_setup(0x5EED0004, a.mean_ops, n_contigs=4, tlen_min=2_000_000, tlen_span=1_000_000)
        else:
            eng.synth4_setup(0x5EED0004, a.mean_ops)
        print(f"cfg4 genomes resident in HBM ({time.perf_counter() - t0:.1f} s to generate)", file=sys.stderr)
        buf, nbytes = eng.synth4(0, a.records)
        if a.cmd == "remove_eqx":  # encoded once on the device, outside the timed region: the = / X text is the input
            info = eng.plan([paffy_amd.stage(paffy_amd.ADD_MISMATCHES)], buf, nbytes)
            assert info.error.code == 0
            enc = eng.alloc_out(info.out_bytes)
            eng.emit(enc)
            eng.sync()
            buf, nbytes = enc, int(info.out_bytes)
    elif a.cmd in ("dechunk", "upconvert", "pass"):
        # the cfg3 stream; dechunk and pass read it chunk-named (rewritten on the host once, outside the timed region), upconvert plain
        # with one interval per contig (every side renamed) and a thousand that match nothing
        buf, nbytes = eng.synth(0x5EED0003, a.mean_ops, 0, a.records, n_contigs=a.contigs)
        text = bytes(buf[:nbytes].cpu().numpy().tobytes())
        if a.cmd == "upconvert":
            contigs = {}
            for line in text.split(b"\n")[:-1]:
                f = line.split(b"\t", 9)
                contigs[f[0]] = int(f[1])
                contigs[f[5]] = int(f[6])
            heads = [b"%s|%d|0" % (k, v) for k, v in contigs.items()] + [b"zz%d|100|0" % k for k in range(1000)]
            eng.set_intervals(heads, list(contigs.values()) + [100] * 1000)
        else:
            text = chunk_encode(text)
            nbytes = len(text)
            buf = eng.to_device(text)
    elif a.cmd == "chain" and a.one_group:
        text = one_group_stream(a.records)
        buf, nbytes = eng.to_device(text), len(text)
        del text
    else:
        buf, nbytes = eng.synth(0x5EED0005, a.mean_ops, 0, a.records, n_contigs=a.contigs)
    rows_cmd = a.cmd in ("shatter", "invert_trim_shatter")
    short_share = None
    if rows_cmd:  # the share of records whose first row piece (name, tab, length, tab) is shorter than 16 bytes, as read and behind an invert
        text = bytes(buf[:nbytes].cpu().numpy().tobytes())
        if a.names == "short":
            text = text.replace(b"hs.chr", b"chr").replace(b"pt.chr", b"chr")
            nbytes = len(text)
            buf = eng.to_device(text)
        n_q = n_t = n = 0
        m_ops = []  # M ops per record: the rows `shatter` alone writes for it
        for line in text.split(b"\n")[:-1]:
            f = line.split(b"\t", 7)
            n += 1
            n_q += len(f[0]) + len(f[1]) + 2 < 16
            n_t += len(f[5]) + len(f[6]) + 2 < 16
            m_ops.append(line.rsplit(b"cg:Z:", 1)[1].count(b"M"))
        short_share = {"as_read": round(n_q / max(1, n), 4), "behind_an_invert": round(n_t / max(1, n), 4)}
        del text
    torch.cuda.synchronize()
    kinds = {"invert": paffy_amd.INVERT, "trim": paffy_amd.TRIM_IDENTITY, "shatter": paffy_amd.SHATTER, "remove": paffy_amd.REMOVE_MISMATCHES, "filter": paffy_amd.FILTER}
    eng.set_filter(min_identity=0.9)
    kinds["add"] = paffy_amd.ADD_MISMATCHES
    kinds["remove_eqx"] = paffy_amd.REMOVE_MISMATCHES
    kinds["stats"] = paffy_amd.STATS
    kinds["pass"] = paffy_amd.PASS
    kinds["upconvert"] = paffy_amd.UPCONVERT
    # a fixed trim in front of another stage, on the stream of `trimf`: sized by the flat pass's wave kernel (flat_left 0), by the record kernels before (-1)
    fixed_pipe = {"trimf_invert": paffy_amd.INVERT, "trimf_filter": paffy_amd.FILTER, "trimf_stats": paffy_amd.STATS}.get(a.cmd)
    res = []
    eng.profile(True)
    if a.cmd in ("view_stats_only", "view_lines"):
        eng.stats_only(True)
    sums = None
    text_out, text_bytes = None, 0
    plan_s = []
    for rep in range(a.repeats + (2 if add_pipe else 0)):
        t0 = time.perf_counter()
        if add_pipe:  # the plan alone (it synchronises on its own), then the emit; no events round the launches while the clock runs
            eng.profile(False)
            info = eng.plan([paffy_amd.stage(k) for k in add_pipe], buf, nbytes)
            t1 = time.perf_counter()
            out = eng.alloc_out(info.out_bytes)
            eng.emit(out)
            eng.sync()
            dt = time.perf_counter() - t0
            assert info.error.code == 0
            if rep < 2:  # warm-up: buffers grown, the second try of the encoder and the allocator's first blocks behind it
                continue
            plan_s.append(t1 - t0)
            res.append(dt)
            continue
        if view:  # the plan and its sums; nothing is emitted (the plan synchronises on its own)
            info = eng.plan([paffy_amd.stage(paffy_amd.ADD_MISMATCHES), paffy_amd.stage(paffy_amd.STATS)], buf, nbytes)
            sums = eng.plan_stats()
            if a.cmd == "view_lines":  # the lines of all records into one device buffer (allocated by the first repeat, kept)
                import ctypes as C

                import numpy as np

                L, n = paffy_amd.engine.lib(), info.n_records
                sizes = np.empty(n, dtype=np.int64)
                assert L.paffy_hip_plan_view_sizes(eng._ctx, 0, n, 0, sizes.ctypes.data_as(C.POINTER(C.c_int64))) == 0
                off = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(sizes, out=off[1:])
                text_bytes = int(off[n])
                if text_out is None or text_out.numel() < text_bytes:
                    text_out = eng.alloc_out(text_bytes)
                err = paffy_amd.engine._Error()
                assert L.paffy_hip_plan_view_text(eng._ctx, 0, n, 0, off.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(text_out.data_ptr()), text_bytes, C.byref(err)) == 0
                assert err.code == 0
            dt = time.perf_counter() - t0
            assert info.error.code == 0
            res.append(dt)
            continue
        if a.cmd == "bed":
            opts = paffy_amd.engine.BedOpts(0, 0, 0, 1, 1)  # -n: both sides of every record
            info = paffy_amd.engine.PlanInfo()
            rc = paffy_amd.engine.lib().paffy_hip_bed_plan(eng._ctx, buf.data_ptr(), nbytes, opts, info)
            assert rc == 0, rc
        elif a.cmd == "chain":
            L = paffy_amd.engine.lib()
            assert L.paffy_hip_chain_begin(eng._ctx) == 0 and L.paffy_hip_chain_add(eng._ctx, buf.data_ptr(), nbytes) == 0
            info = paffy_amd.engine.PlanInfo()
            opts = paffy_amd.engine.ChainOpts(5000, 1, 1000000, 0.0 if a.one_group else 1.0)
            eng.chain_fresh_walk(a.fresh_walk) if a.fresh_walk else None
            assert L.paffy_hip_chain_run(eng._ctx, opts, info) == 0
        elif a.cmd == "dedupe":
            paffy_amd.engine.lib().paffy_hip_dedupe_reset(eng._ctx)
            info = eng.dedupe_plan(buf, nbytes, True)
        else:
            st = paffy_amd.stage(paffy_amd.TRIM_FIXED, 0.05, 0.1) if a.cmd == "trimf" else (paffy_amd.stage_dechunk() if a.cmd == "dechunk" else None)
            if a.cmd == "invert_trim_shatter":
                info = eng.plan([paffy_amd.stage(paffy_amd.INVERT), paffy_amd.stage(paffy_amd.TRIM_IDENTITY), paffy_amd.stage(paffy_amd.SHATTER)], buf, nbytes)
            elif fixed_pipe:
                info = eng.plan([paffy_amd.stage(paffy_amd.TRIM_FIXED, 0.05, 0.1), paffy_amd.stage(fixed_pipe)], buf, nbytes)
            else:
                info = eng.tile_plan(buf, nbytes) if a.cmd == "tile" else eng.plan([st or paffy_amd.stage(kinds[a.cmd])], buf, nbytes)
        out = eng.alloc_out(info.out_bytes)
        eng.emit(out)
        eng.sync()
        dt = time.perf_counter() - t0
        assert info.error.code == 0
        res.append(dt)
    dt = min(res)
    if add_pipe:  # the per-kernel times: one more repetition, with events
        eng.profile(True)
        eng.plan([paffy_amd.stage(k) for k in add_pipe], buf, nbytes)
        eng.emit(out)
        eng.sync()
    prof = {k: round(v[0] / max(1, v[1]), 3) for k, v in eng.profile_read().items()}
    extra = {"flat_left": eng.flat_stats()[0]} if a.cmd in ("dechunk", "pass", "remove", "remove_eqx", "trimf") or fixed_pipe or view else {}
    if view:
        extra["sums"] = list(sums)
    if a.cmd == "chain":
        import statistics

        extra.update(fresh_walk=bool(a.fresh_walk), one_group=bool(a.one_group), median_s=round(statistics.median(res), 5), spread_s=round(max(res) - min(res), 5),
                     lib=os.path.basename(os.path.dirname(paffy_amd.engine.library_path())) + "/" + os.path.basename(paffy_amd.engine.library_path()))
        if a.fresh_walk:
            extra["fresh_stats"] = eng.chain_fresh_stats()
    if rows_cmd:
        left, why = eng.flat_stats()
        extra.update(names=a.names, piece_a_below_16=short_share, flat_left=left, flat_why=list(why), rows=int(info.n_rows))
        if a.cmd == "shatter":  # rows per writer, from the records' RecPlan flags (bit 6 k_emit_rows, bit 19 its segments, bit 23 k_emit_rows_short)
            flags, _ = eng.record_layout(0, len(m_ops))
            by = {"k_emit_rows": 0, "k_emit_rows_short": 0, "other": 0}
            for f, r in zip(flags, m_ops):
                by["k_emit_rows_short" if f & 0x800000 else "k_emit_rows" if f & 0x80040 else "other"] += r
            extra["rows_by_kernel"] = by
    if a.cmd == "view_lines":
        extra["text_bytes"] = text_bytes
    if add_pipe:
        import statistics

        left, why = eng.flat_stats()
        extra.update(flat_left=left, flat_why=list(why), median_s=round(statistics.median(res), 5), spread_s=round(max(res) - min(res), 5),
                     plan_median_s=round(statistics.median(plan_s), 5), plan_spread_s=round(max(plan_s) - min(plan_s), 5), plan_repeats=[round(x, 5) for x in plan_s],
                     lib=os.path.basename(os.path.dirname(paffy_amd.engine.library_path())) + "/" + os.path.basename(paffy_amd.engine.library_path()))
        if a.sha:
            import hashlib

            extra["out_sha256"] = hashlib.sha256(out[:info.out_bytes].cpu().numpy().tobytes()).hexdigest()
    print(json.dumps({**extra, "cmd": a.cmd, "records": a.records, "mean_ops": a.mean_ops, "in_bytes": nbytes, "out_bytes": int(info.out_bytes),
                      "seconds": round(dt, 4), "repeats": [round(x, 4) for x in res], "records_per_s": round(a.records / dt, 1),
                      "GBps": round((nbytes + info.out_bytes) / dt / 1e9, 1), "kernel_ms": prof}))


def chain_parts_bench(a):
    """`paffy chain` in parts (paffy_amd.shard.chain_in_parts): partition by query name, the parts one after the other on one GPU, key
    exchange in device memory, renumber, ordered write into one buffer. The output is compared with the one-context output before
    anything is timed. One GPU runs the parts in turn: the figure bounds the added work, it says nothing about N GPUs."""
    import torch

    import paffy_amd
    from paffy_amd import shard

    engines = [paffy_amd.Engine() for _ in range(a.parts)]
    eng = engines[0]
    buf, nbytes = eng.synth(0x5EED0005, a.mean_ops, 0, a.records, n_contigs=a.contigs)
    whole = paffy_amd.Engine()
    L = paffy_amd.engine.lib()
    assert L.paffy_hip_chain_begin(whole._ctx) == 0 and L.paffy_hip_chain_add(whole._ctx, buf.data_ptr(), nbytes) == 0
    info, opts = paffy_amd.engine.PlanInfo(), paffy_amd.engine.ChainOpts(5000, 1, 1000000, 1.0)
    assert L.paffy_hip_chain_run(whole._ctx, opts, info) == 0 and info.error.code == 0
    want = whole.alloc_out(info.out_bytes)
    whole.emit(want)
    whole.sync()
    workers = [shard.GpuChainWorker(e) for e in engines]
    res = shard.chain_in_parts(workers, [(buf, nbytes)])
    torch.cuda.synchronize()
    assert res["error"] is None and res["total"] == info.out_bytes and torch.equal(res["out"], want[: info.out_bytes]), "the parts do not write the one-context output"
    del want
    whole.close()
    times = []
    for rep in range(4):
        if rep == 1:
            for e in engines:
                e.profile(True)  # the first repetition warms up
        t0 = time.perf_counter()
        res = shard.chain_in_parts(workers, [(buf, nbytes)])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = min(times[1:])
    prof = {}
    for e in engines:
        for k, v in e.profile_read().items():
            prof[k] = (prof.get(k, (0.0, 0))[0] + v[0], max(prof.get(k, (0.0, 0))[1], v[1]))
    print(json.dumps({"cmd": "chain", "parts": a.parts, "records": a.records, "mean_ops": a.mean_ops, "in_bytes": nbytes, "out_bytes": int(res["total"]),
                      "chains": int(res["chain_ids"].numel()), "verified_against_one_context": True, "seconds": round(dt, 4), "records_per_s": round(a.records / dt, 1),
                      "GBps": round((nbytes + res["total"]) / dt / 1e9, 1), "kernel_ms_all_parts_per_run": {k: round(ms / max(1, cnt), 3) for k, (ms, cnt) in prof.items()}}))


def synth_genome(torch, dev, gb, n_contigs=24, seed=0x5EED00FA, chunk_headers=False):
    """a seeded genome written as FASTA text on the device: 60-column lines, mixed case, runs of N (about 2 % of the lines);
    returns (text tensor, text bytes, [(name, length)]). chunk_headers: every contig is named as the chunk chr<k>|<length>|0 of itself"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    w = torch.rand(n_contigs, generator=g, device=dev).cpu() + 0.5
    lens = [int(x) for x in (w / w.sum() * gb * 1e9).tolist()]
    heads = [b">chr%d|%d|0\n" % (k, n) if chunk_headers else b">chr%d\n" % k for k, n in enumerate(lens)]
    total = sum(len(h) + n + (n + 59) // 60 for h, n in zip(heads, lens))
    text = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    lut = torch.tensor(list(b"ACGTacgt"), dtype=torch.uint8, device=dev)
    at = 0
    for h, n in zip(heads, lens):
        text[at:at + len(h)] = torch.tensor(list(h), dtype=torch.uint8, device=dev)
        at += len(h)
        full, tail = n // 60, n % 60
        rows = text[at:at + full * 61].view(full, 61)
        step = 1 << 22
        for r0 in range(0, full, step):
            r1 = min(full, r0 + step)
            rows[r0:r1, :60] = lut[torch.randint(0, 8, (r1 - r0, 60), generator=g, device=dev)]
        rows[:, 60] = 10
        n_runs = full // 5000
        if n_runs:
            starts = torch.randint(0, max(1, full - 100), (n_runs,), generator=g, device=dev)
            idx = (starts[:, None] + torch.arange(100, device=dev)[None, :]).reshape(-1)
            rows[idx, :60] = ord("N")
        at += full * 61
        if tail:
            text[at:at + tail] = lut[torch.randint(0, 8, (tail,), generator=g, device=dev)]
            text[at + tail] = 10
            at += tail + 1
    assert at == total
    return text, total, [(h[1:-1], n) for h, n in zip(heads, lens)]


def faffy_bench(a):
    """faffy chunk / extract / merge with the text resident in HBM: index + plan + emit per repetition, kernel times by HIP events.
    seconds_plan is a host clock round the plan call alone, which ends in a synchronise (extract: the BED is host text, so the plan
    includes its copy to the device). The CLI itself is bound by its disk reads and writes; these figures are the device part."""
    import ctypes as C

    import numpy as np
    import torch

    import paffy_amd
    from paffy_amd import engine as E

    L = E.lib()
    eng = paffy_amd.Engine()
    dev = eng.device
    t0 = time.perf_counter()
    text, nbytes, contigs = synth_genome(torch, dev, a.genome_gb)
    starts = [0]
    bed = b""
    if a.cmd == "faffy_merge":  # the input is faffy chunk's output (-c 1000000 -o 10000), one file per chunk group
        eng.fasta_index(text, nbytes, [0])
        info = E.PlanInfo()
        assert L.paffy_hip_faffy_chunk_plan(eng._ctx, 1000000, 10000, C.byref(info)) == 0 and info.error.code == 0
        chunked = eng.alloc_out(info.out_bytes + 64)
        err = E._Error()
        assert L.paffy_hip_faffy_emit(eng._ctx, C.c_void_p(chunked.data_ptr()), chunked.numel(), C.byref(err)) == 0 and err.code == 0
        n = L.paffy_hip_faffy_chunk_files(eng._ctx, 0, None)
        ends = (C.c_int64 * n)()
        L.paffy_hip_faffy_chunk_files(eng._ctx, n, ends)
        starts = [0] + list(ends[:-1])
        del text
        text, nbytes = chunked, int(info.out_bytes)
    elif a.cmd == "faffy_extract":
        rng = np.random.default_rng(7)
        k = rng.integers(0, len(contigs), a.intervals)
        ln = np.array([n for _, n in contigs])[k]
        size = rng.integers(100, 10000, a.intervals)
        st = (rng.random(a.intervals) * (ln - size)).astype(np.int64)
        bed = b"".join(b"%s\t%d\t%d\n" % (contigs[x][0], s, s + z) for x, s, z in zip(k.tolist(), st.tolist(), size.tolist()))
    torch.cuda.synchronize()
    print(f"{a.cmd}: input of {nbytes / 1e9:.2f} GB resident in HBM ({time.perf_counter() - t0:.1f} s to generate)", file=sys.stderr)
    res, plan = [], []
    out = None
    for rep in range(max(2, a.repeats)):
        if rep == 1:
            eng.profile(True)  # the first repetition warms up; kernel figures from the others
        t0 = time.perf_counter()
        n_rec, n_bases = eng.fasta_index(text, nbytes, starts)
        info = E.PlanInfo()
        t1 = time.perf_counter()  # the plan call alone: it ends in a synchronise
        if a.cmd == "faffy_chunk":
            rc = L.paffy_hip_faffy_chunk_plan(eng._ctx, 1000000, 10000, C.byref(info))
        elif a.cmd == "faffy_extract":
            rc = L.paffy_hip_faffy_extract_plan(eng._ctx, bed, len(bed), 10, 100, 1, C.byref(info))
        else:
            rc = L.paffy_hip_faffy_merge_plan(eng._ctx, C.byref(info))
        plan.append(time.perf_counter() - t1)
        assert rc == 0 and info.error.code == 0, (rc, info.error.code)
        if out is None or out.numel() < info.out_bytes + 16:
            out = eng.alloc_out(info.out_bytes)
        err = E._Error()
        assert L.paffy_hip_faffy_emit(eng._ctx, C.c_void_p(out.data_ptr()), out.numel(), C.byref(err)) == 0 and err.code == 0
        eng.sync()
        res.append(time.perf_counter() - t0)
    prof = {k: (v[0], v[1]) for k, v in eng.profile_read().items()}
    kernel_ms = {k: round(ms / max(1, cnt), 3) for k, (ms, cnt) in prof.items()}
    total_ms = sum(kernel_ms.values())
    moved = nbytes + int(info.out_bytes)
    extra = name_sort_figures(eng, prof, len(res) - 1) if a.cmd == "faffy_extract" else {}
    if a.sha256:
        import hashlib

        h = hashlib.sha256()
        for at in range(0, int(info.out_bytes), 1 << 28):
            h.update(out[at:min(at + (1 << 28), int(info.out_bytes))].cpu().numpy().tobytes())
        extra["out_sha256"] = h.hexdigest()
    print(json.dumps({"cmd": a.cmd, "in_bytes": nbytes, "out_bytes": int(info.out_bytes), "records": n_rec, "bases": n_bases, "items": int(info.n_rows),
                      "seconds_index_plan_emit": round(min(res[1:]), 4), "seconds_plan": round(min(plan[1:]), 5),
                      "seconds_index_plan_emit_all": [round(x, 4) for x in res], "seconds_plan_all": [round(x, 5) for x in plan], **extra,
                      "kernel_ms": kernel_ms, "kernel_ms_total": round(total_ms, 3),
                      "GBps_text_in_out_over_kernel_time": round(moved / (total_ms / 1e3) / 1e9, 1),
                      "fraction_of_8TBps": round(moved / (total_ms / 1e3) / 8e12, 3)}))
    eng.close()


def name_sort_figures(eng, prof, reps):
    """The device name sort's share of the profiled repetitions (its kernels and the rocPRIM sorts and scans between them: the k_ns_* and
    ns_* rows, summed per repetition) and what the last sort took; nothing under a library that has no name sort."""
    from paffy_amd import engine as E

    if not hasattr(E.lib(), "paffy_hip_name_sort_stats"):
        return {}
    ms = sum(v[0] for k, v in prof.items() if k.startswith(("k_ns_", "ns_")))
    return {"name_sort_ms_per_repetition": round(ms / max(1, reps), 3), "name_sort_stats": eng.name_sort_stats()}


def seqload_bench(a):
    """The sequence store of add_mismatches / view from FASTA text: paffy_hip_set_sequences_fasta on text resident in HBM (index + store
    kernels, names sorted on the device: the k_ns_* and ns_* rows) against paffy_hip_set_sequences on the same records held as host strings (one copy per record +
    k_seq_canon; the host parse of the former CLI path is not included). The text is freed by neither call."""
    import ctypes as C

    import numpy as np
    import torch

    import paffy_amd
    from paffy_amd import engine as E

    L = E.lib()
    eng = paffy_amd.Engine()
    dev = eng.device
    if a.scaffolds:
        rng = np.random.default_rng(11)
        lens = rng.integers(1, 2001, a.scaffolds)
        seq = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, int(lens.sum()))].tobytes()
        parts, at = [], 0
        for i, n in enumerate(lens.tolist()):
            parts.append(b">scaffold_%d\n%s\n" % (i, seq[at:at + n]))
            at += n
        host = b"".join(parts)
        text = eng.to_device(host)
        nbytes = len(host)
    else:
        text, nbytes, _ = synth_genome(torch, dev, a.genome_gb)
    torch.cuda.synchronize()
    st = (C.c_int64 * 1)(0)
    n_rec = C.c_int64()
    new = []
    for rep in range(max(2, a.repeats)):
        if rep == 1:
            eng.profile(True)
        t0 = time.perf_counter()
        assert L.paffy_hip_set_sequences_fasta(eng._ctx, C.c_void_p(text.data_ptr()), nbytes, st, 1, C.byref(n_rec)) == 0
        eng.sync()
        new.append(time.perf_counter() - t0)
    prof = {k: (v[0], v[1]) for k, v in eng.profile_read().items()}
    eng.profile(False)
    kernel_ms = {k: round(ms / max(1, cnt), 3) for k, (ms, cnt) in prof.items()}
    extra = name_sort_figures(eng, prof, len(new) - 1)
    if a.skip_host_strings:
        print(json.dumps({"cmd": "seqload", "text_bytes": nbytes, "records": n_rec.value, "seconds_set_sequences_fasta": round(min(new[1:]), 4),
                          "seconds_set_sequences_fasta_all": [round(x, 4) for x in new], **extra, "kernel_ms": kernel_ms}))
        eng.close()
        return
    # the records as host strings (what the former host parse produced), then the host-string call
    recs = eng.fasta_records([bytes(text[:nbytes].cpu().numpy().tobytes())]) if a.scaffolds else None
    if recs is None:
        eng.fasta_index(text, nbytes, [0])
        table = eng.fasta_table()
        total = table[-1][2] + table[-1][3]
        buf = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        eng.fasta_bases(0, total, buf)
        bases = buf[:total].cpu().numpy().tobytes()
        recs = [(b"chr%d" % k, bases[s:s + n]) for k, (_, _, s, n) in enumerate(table)]
        del buf
    del text
    torch.cuda.empty_cache()
    names = (C.c_char_p * len(recs))(*[h for h, _ in recs])
    seqs = (C.c_char_p * len(recs))(*[s for _, s in recs])
    lns = (C.c_int64 * len(recs))(*[len(s) for _, s in recs])
    old = []
    for rep in range(3):
        t0 = time.perf_counter()
        assert L.paffy_hip_set_sequences(eng._ctx, len(recs), names, seqs, lns) == 0
        eng.sync()
        old.append(time.perf_counter() - t0)
    n_bases = sum(len(s) for _, s in recs)
    store_ms = kernel_ms.get("k_seq_store", 0.0)
    moved = 3 * n_bases  # k_seq_store: the bases read once, written upper-cased and complemented (no raw copy here)
    print(json.dumps({"cmd": "seqload", "text_bytes": nbytes, "records": n_rec.value, "bases": n_bases,
                      "seconds_set_sequences_fasta": round(min(new[1:]), 4), "seconds_set_sequences_host_strings": round(min(old[1:]), 4),
                      "seconds_set_sequences_fasta_all": [round(x, 4) for x in new], **extra, "kernel_ms": kernel_ms, "k_seq_store_GBps": round(moved / (store_ms / 1e3) / 1e9, 1) if store_ms else None,
                      "k_seq_store_fraction_of_8TBps": round(moved / (store_ms / 1e3) / 8e12, 3) if store_ms else None}))
    eng.close()


def ivload_bench(a):
    """The interval table of upconvert from FASTA text: paffy_hip_set_intervals_fasta on text resident in HBM (index + the table's build).
    --repeats R: a warm-up and R - 1 timed repetitions without the profile (median and spread = max - min), then one repetition under
    the profile for the kernels' times by HIP events. Uses nothing but that call, so it runs on a library that builds the table on the
    host as well; what the device build reports about itself is added where the library has it."""
    import ctypes as C
    import statistics

    import numpy as np
    import torch

    import paffy_amd
    from paffy_amd import engine as E

    L = E.lib()
    eng = paffy_amd.Engine()
    if a.scaffolds:
        rng = np.random.default_rng(13)
        lens = rng.integers(1, 201, a.scaffolds).tolist()
        starts = rng.integers(0, 1 << 33, a.scaffolds).tolist()
        host = b"".join(b">scaf%d|%d|%d\n%s\n" % (i, s + n, s, b"A" * n) for i, (n, s) in enumerate(zip(lens, starts)))
        text = eng.to_device(host)
        nbytes = len(host)
        del host
    else:
        text, nbytes, _ = synth_genome(torch, eng.device, a.genome_gb, chunk_headers=True)
    torch.cuda.synchronize()
    st = (C.c_int64 * 1)(0)
    n_rec = C.c_int64()

    def load():
        t0 = time.perf_counter()
        assert L.paffy_hip_set_intervals_fasta(eng._ctx, C.c_void_p(text.data_ptr()), nbytes, st, 1, C.byref(n_rec)) == 0
        eng.sync()
        return time.perf_counter() - t0

    secs = [load() for _ in range(max(2, a.repeats))][1:]
    eng.profile(True)
    load()
    prof = eng.profile_read()
    eng.profile(False)
    kernel_ms = {k: {"ms": round(v[0], 3), "launches": v[1]} for k, v in sorted(prof.items())}
    extra = {}
    if hasattr(L, "paffy_hip_intervals_info"):
        extra = {"intervals_info": eng.intervals_info(), "name_sort_stats": eng.name_sort_stats(),
                 "build_ms": round(sum(v[0] for k, v in prof.items() if k.startswith(("k_up_", "k_ns_", "ns_"))), 3)}
    print(json.dumps({"cmd": "ivload", "text_bytes": nbytes, "records": n_rec.value, "seconds_median": round(statistics.median(secs), 5),
                      "seconds_spread": round(max(secs) - min(secs), 5), "seconds_all": [round(x, 5) for x in secs], **extra, "kernel_ms": kernel_ms}))
    eng.close()


if __name__ == "__main__":
    main()

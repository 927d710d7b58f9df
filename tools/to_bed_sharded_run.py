#!/usr/bin/env python3
"""One rank of `paffy to_bed` sharded by sequence (paffy_amd.shard.to_bed_sharded): start WORLD_SIZE of these with RANK,
WORLD_SIZE, MASTER_ADDR and MASTER_PORT set, as torchrun does. Every rank reads its contiguous share of the lines of --input, the
blocks of BED lines travel to rank 0, which writes --output (nothing when a record fails: the failure goes to --error as JSON).
--one-device: all ranks share GPU 0 (gloo carries the exchanges; RCCL cannot put two ranks on one GPU)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--error", default=None)
    ap.add_argument("--backend", default="gloo", choices=["gloo", "nccl"])
    ap.add_argument("--one-device", action="store_true")
    ap.add_argument("--batch-bytes", type=int, default=1 << 30)
    ap.add_argument("-b", "--binary", action="store_true")
    ap.add_argument("-e", "--excludeUnaligned", dest="exclude_unaligned", action="store_true")
    ap.add_argument("-f", "--excludeAligned", dest="exclude_aligned", action="store_true")
    ap.add_argument("-m", "--minSize", dest="min_size", type=int, default=1)
    ap.add_argument("-n", "--includeInverted", dest="include_inverted", action="store_true")
    a = ap.parse_args()
    import torch
    import torch.distributed as dist

    import paffy_amd
    from paffy_amd import shard

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0 if a.one_device else rank % torch.cuda.device_count())
    dist.init_process_group(a.backend, rank=rank, world_size=world)
    try:
        eng = paffy_amd.Engine()
        comm = eng.device if a.backend == "nccl" else "cpu"
        with open(a.input, "rb") as fh:
            lines = fh.read().splitlines(keepends=True)
        first, n = shard.share_of_rank(rank, world, len(lines))
        text = b"".join(lines[first: first + n])
        batches = [(eng.to_device(p), len(p)) for p in eng.split_lines(text, a.batch_bytes)]
        opts = {k: getattr(a, k) for k in shard.BED_OPTS}
        worker = shard.GpuBedWorker(eng)
        res = shard.to_bed_sharded(worker, dist, rank, world, batches, first, opts, comm)
        if res["error"]:
            if a.error:
                with open(a.error + (".%d" % rank if rank else ""), "w") as fh:
                    json.dump(res["error"], fh)
            return 0
        out = shard.gather_ordered_output(worker, dist, rank, world, worker.emit(), res["keys"][:, 1].contiguous(), res["offsets"], res["total"], comm)
        eng.sync()
        if rank == 0:
            with open(a.output, "wb") as fh:
                fh.write(bytes(out.cpu().numpy().tobytes()))
        return 0
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())

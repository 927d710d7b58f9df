"""Sharding of the stream commands across GPUs.

Records of shatter / invert / trim / add_mismatches are independent (each iteration of the
reference loop touches one Paf, impl/paf_invert.c:84-89), so the N-GPU path is a partition of
the record stream with no data-path collective: rank r owns batches r, r+N, r+2N, ... of
`batch` records each. Output order is restored by concatenating per-batch outputs in batch
order; the only exchange is an all-gather of per-batch output byte counts (8 bytes per batch) so
that every rank knows where its bytes go in the ordered output: each rank pwrites its ranges, or the batches travel to one
writer in order (gather_to_writer: point-to-point sends over xGMI with the nccl backend).
`tile` shards by query contig instead (its state is keyed by query name, impl/paf.c:675-688).
"""


def batches_of_rank(rank, world, total_records, batch):
    """[(batch_index, first_record, n_records)] owned by `rank`: round-robin over the stream's batches."""
    out = []
    n_batches = (total_records + batch - 1) // batch
    for b in range(rank, n_batches, world):
        r0 = b * batch
        out.append((b, r0, min(batch, total_records - r0)))
    return out


def output_offsets(sizes_by_batch):
    """Exclusive prefix sum of the per-batch output sizes (index = batch index) -> byte offset of every batch."""
    offs, acc = [], 0
    for s in sizes_by_batch:
        offs.append(acc)
        acc += s
    return offs, acc


def gather_batch_sizes(dist, local, n_batches, device="cpu"):
    """All-gather of {batch_index: out_bytes}: every rank ends with the full size table.

    `local` maps the batch indices this rank processed to their output byte counts. Works with
    any torch.distributed backend (nccl = RCCL on the GPU box, gloo in the CPU tests).
    """
    import torch

    t = torch.zeros(n_batches, dtype=torch.int64, device=device)
    for b, s in local.items():
        t[b] = s
    dist.all_reduce(t, op=dist.ReduceOp.SUM)  # disjoint ownership: a sum is a gather
    return [int(x) for x in t.tolist()]


def gather_to_writer(dist, rank, world, local, sizes_by_batch, write, device="cpu", writer=0):
    """The ordered write: batch outputs travel to the writer rank in batch order (a gatherv with per-batch sizes).

    `local` maps the batch indices this rank owns to uint8 tensors (on `device`; with the nccl backend they stay on the GPU and
    move over xGMI as point-to-point sends, RCCL send/recv); `sizes_by_batch` is the table from gather_batch_sizes. The writer
    calls `write(batch_index, tensor)` for batch 0, 1, 2, ... -- receives are posted a few batches ahead so that the links stay
    busy while the writer drains. Other ranks return once their sends are done.
    """
    import torch

    n_batches = len(sizes_by_batch)
    owner = [b % world for b in range(n_batches)]  # = batches_of_rank's round robin
    # No tags: the nccl backend ignores them. A send is matched with a receive by ORDER per peer alone -- every sender posts its batches
    # in ascending batch order and the writer posts its receives in ascending batch order, so the k-th send of rank r meets the k-th
    # receive from rank r on any backend.
    if rank != writer:
        mine = [b for b in range(n_batches) if owner[b] == rank and sizes_by_batch[b] > 0]
        assert mine == sorted(mine)
        reqs = [dist.isend(local[b].contiguous(), dst=writer) for b in mine]
        for r in reqs:
            r.wait()
        return
    ahead, pending = 4, {}

    def post(b):
        if b < n_batches and owner[b] != writer and sizes_by_batch[b] > 0:
            buf = torch.empty(sizes_by_batch[b], dtype=torch.uint8, device=device)
            pending[b] = (dist.irecv(buf, src=owner[b]), buf)  # post() is called with ascending b: ascending per peer too

    for b in range(min(ahead, n_batches)):
        post(b)
    for b in range(n_batches):
        post(b + ahead)
        if sizes_by_batch[b] == 0:
            continue
        if owner[b] == writer:
            write(b, local[b])
        else:
            req, buf = pending.pop(b)
            req.wait()
            write(b, buf)


def contig_partition(weights, world):
    """`tile`: assign query contigs to ranks, heaviest first onto the lightest rank (weights: name -> work)."""
    loads = [0] * world
    owner = {}
    for name, w in sorted(weights.items(), key=lambda kv: (-kv[1], kv[0])):
        r = min(range(world), key=lambda i: (loads[i], i))
        owner[name] = r
        loads[r] += w
    return owner


# ---- tile across ranks -------------------------------------------------------------------------
#
# `paffy tile` visits all records in (s1 desc, AS desc, input order) order but its state is per QUERY sequence, so records of
# different query sequences never interact (impl/paf_tile.c:164-175, impl/paf.c:675-709). Sharded over N ranks:
#   1. every rank holds a contiguous share of the input; the distinct query names and the bytes of their lines are merged over the
#      ranks (merge_name_weights: one all-gather of a few hundred bytes) and dealt to the ranks, heaviest first (owner_table);
#   2. exchange_lines: the lines travel to the owner of their query sequence -- ONE all-to-all of the text (RCCL over xGMI with the
#      nccl backend) plus one of the records' global input indices (8 bytes per record);
#   3. every rank tiles what it received (its sequences, complete, in input order);
#   4. gather_tile_keys: an all-gather of (chain_score, score, global input index, line bytes) -- 32 bytes per record -- lets every
#      rank order ALL records as the single process would and scan their sizes: global_line_offsets gives every local line its
#      byte offset in the ordered output. The lines themselves are written at those offsets (scatter) or stay where they are.
# Everything here is tensor plumbing over torch.distributed; the device work (hashing, regrouping, tiling, writing) is the C-ABI's.


def name_hash(name):
    """The 64-bit hash the device uses for a sequence name (cov_name_hash, coverage_kernel.h): FNV-1a over the bytes, then the length."""
    h, mask = 0xcbf29ce484222325, (1 << 64) - 1
    for b in name:
        h = ((h ^ b) * 0x100000001b3) & mask
    h = ((h ^ (0x100 + len(name))) * 0x100000001b3) & mask
    return h ^ (h >> 29)


def _comm(t, comm_device):
    return t if str(t.device) == str(comm_device) else t.to(comm_device)


def merge_name_weights(dist, local, comm_device="cpu"):
    """local: {name hash: weight} of this rank's share -> the same table summed over all ranks (identical on every rank)."""
    import torch

    if dist is None:
        return dict(local)
    world = dist.get_world_size()
    n = torch.tensor([len(local)], dtype=torch.int64, device=comm_device)
    counts = torch.zeros(world, dtype=torch.int64, device=comm_device)
    dist.all_gather_into_tensor(counts, n)
    cap = max(1, int(counts.max().item()))
    mine = torch.zeros(cap, 2, dtype=torch.int64, device=comm_device)
    if local:
        keys = sorted(local)
        mine[: len(keys), 0] = torch.tensor([k - (1 << 64) if k >= (1 << 63) else k for k in keys], dtype=torch.int64)  # hashes as two's complement
        mine[: len(keys), 1] = torch.tensor([local[k] for k in keys], dtype=torch.int64)
    everyone = torch.zeros(world * cap, 2, dtype=torch.int64, device=comm_device)
    dist.all_gather_into_tensor(everyone, mine)
    everyone = everyone.cpu().reshape(world, cap, 2)
    out = {}
    for r in range(world):
        for k, w in everyone[r, : int(counts[r].item())].tolist():
            k &= (1 << 64) - 1
            out[k] = out.get(k, 0) + w
    return out


def owner_table(weights, world):
    """{name hash: weight} -> {name hash: owning rank}: contig_partition's deal, the same on every rank."""
    return contig_partition(weights, world)


EXCHANGE_CHUNK = 256 << 20  # bytes per send / receive operation


def big_buffer_bytes(n):
    """Size to allocate for a buffer that must hold n bytes of a rank's share (send, receive and output buffers): rounded up to 1/64 of
    its size in 2 MiB units. A second tile of an input of about the same size (another step of the bench, another file of a pipeline)
    then asks torch's caching allocator for the very block it let go -- a buffer a few kilobytes larger than the cached one cannot
    use it, and with a share of 54 GB per buffer the allocator then has to return everything it caches to the driver and allocate
    again (1.5 s per step in the 10 M-record run of round 3)."""
    n = int(n)
    if n < (64 << 20):
        return n
    unit = max(2 << 20, (n >> 6) >> 21 << 21)
    return (n + unit - 1) // unit * unit


def _pairwise_exchange(dist, rank, world, src, send_counts, dst, recv_counts, chunk, recv_offsets=None, verify=True):
    """dst <- what every rank holds for this rank in src (both flat, grouped by peer, counts in elements): the all-to-all as explicit
    sends and receives per peer in pieces of at most `chunk` elements, the rank's own part as a plain copy. Over the nccl backend
    these are RCCL send / recv pairs -- point-to-point over xGMI, which is what the fabric is. Why not all_to_all_single: one call
    with several GB per peer came back without its bytes (tools/probes/rccl_a2a_sizes.py: wrong from 768 MiB on at world size 1)."""
    so, ro = [0], [0]
    for r in range(world):
        so.append(so[-1] + int(send_counts[r]))
        ro.append(ro[-1] + int(recv_counts[r]))
    re = ro[1:]  # where every peer's part ends in dst
    if recv_offsets is not None:  # parts at given places (16-byte aligned segments) instead of back to back
        ro = [int(x) for x in recv_offsets]
        re = [ro[r] + int(recv_counts[r]) for r in range(world)]
    if send_counts[rank]:
        dst[ro[rank]: re[rank]].copy_(src[so[rank]: so[rank + 1]])
    if verify:
        sent = _edge_sums(src, so[:-1], so[1:])
    rounds = max([0] + [(int(c) + chunk - 1) // chunk for r, c in enumerate(send_counts) if r != rank] +
                 [(int(c) + chunk - 1) // chunk for r, c in enumerate(recv_counts) if r != rank])
    for k in range(rounds):
        ops = []
        for step in range(1, world):  # peer order: everyone sends "to the right by step", receives "from the left by step"
            to, frm = (rank + step) % world, (rank - step) % world
            a, b = so[to] + k * chunk, min(so[to] + (k + 1) * chunk, so[to + 1])
            if a < b:
                ops.append(dist.P2POp(dist.isend, src[a:b], to))
            a, b = ro[frm] + k * chunk, min(ro[frm] + (k + 1) * chunk, re[frm])
            if a < b:
                ops.append(dist.P2POp(dist.irecv, dst[a:b], frm))
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()
    if verify:
        # every posted byte arrived: the sender's fingerprint of each part (element count, sums over its first and last 64 Ki elements)
        # travels as a 24-byte all-to-all and must equal what the receiver finds where the part landed. An RCCL collective that returns
        # without its bytes (tools/probes/rccl_a2a_sizes.py saw one do that from 768 MiB per peer on) fails here, loudly, not downstream.
        import torch

        theirs = torch.zeros_like(sent)
        dist.all_to_all_single(theirs, sent)
        got = _edge_sums(dst, ro[:world], re[:world])
        if not torch.equal(theirs.cpu(), got.cpu()):
            bad = [r for r in range(world) if not torch.equal(theirs[r].cpu(), got[r].cpu())]
            raise RuntimeError(f"_pairwise_exchange: rank {rank} did not receive what ranks {bad} sent (fingerprints differ)")


EDGE_ELEMENTS = 1 << 16


def _edge_sums(buf, starts, ends):
    """int64 [parts, 3]: (elements, sum of the first EDGE_ELEMENTS, sum of the last EDGE_ELEMENTS) of buf[start:end] for every part"""
    import torch

    out = torch.zeros(len(starts), 3, dtype=torch.int64, device=buf.device)
    for r, (a, b) in enumerate(zip(starts, ends)):
        a, b = int(a), int(b)
        if b > a:
            out[r, 0] = b - a
            out[r, 1] = buf[a: min(b, a + EDGE_ELEMENTS)].to(torch.int64).sum()
            out[r, 2] = buf[max(a, b - EDGE_ELEMENTS): b].to(torch.int64).sum()
    return out


def exchange_lines(dist, send_buf, send_bytes, send_gidx, send_records, comm_device="cpu", pieces=None):
    """The all-to-all of the partition. send_buf: uint8 tensor holding the lines grouped by destination rank; send_gidx: int64
    tensor, the global input index of every line in the same order; send_bytes / send_records: per destination.
    Returns (recv_buf uint8, recv_gidx int64, pieces): what this rank owns -- the lines of every source rank as one segment of
    recv_buf that starts at a multiple of 16 bytes, pieces = [(offset, bytes)] of the segments in source order. Every source sent its
    lines in input order and sources hold consecutive shares, so the pieces one after the other are in global input order -- and each
    is a whole number of lines at an aligned address: a text batch the library can take where it is, no copy.
    Without ranks nothing moves: the send buffer and the pieces the splitter laid out come back."""
    import torch

    world = dist.get_world_size() if dist is not None else 1
    if dist is not None:
        rank = dist.get_rank()
        sizes = torch.tensor([list(send_bytes), list(send_records)], dtype=torch.int64, device=comm_device).t().contiguous()  # [world, 2]
        got = torch.zeros_like(sizes)
        dist.all_to_all_single(got, sizes)  # 16 bytes per peer
        recv_bytes, recv_records = [int(x) for x in got[:, 0].tolist()], [int(x) for x in got[:, 1].tolist()]
    if world == 1:
        # One rank owns everything: the splitter laid every batch's lines out at a multiple of 16 bytes (`pieces`, with up to 15 bytes
        # of padding between them -- the buffer is NOT sum(send_bytes) contiguous bytes), and a rank's own part never travels anyway.
        # With a process group of one (bench.py --force-dist) the size exchange above still ran over the backend.
        n = int(send_bytes[0])
        if dist is not None and (recv_bytes[0] != n or recv_records[0] != int(send_records[0])):
            raise RuntimeError("exchange_lines: the size exchange of a one-rank group returned other sizes than were sent")
        return send_buf, send_gidx[: int(send_records[0])], (pieces if pieces is not None else [(0, n)])
    offs, at = [], 0
    for r in range(world):
        offs.append(at)
        at += (recv_bytes[r] + 15) // 16 * 16
    src = _comm(send_buf[: sum(send_bytes)], comm_device)
    recv_buf = torch.empty(big_buffer_bytes(at + 16), dtype=torch.uint8, device=comm_device)
    _pairwise_exchange(dist, rank, world, src, list(send_bytes), recv_buf, recv_bytes, EXCHANGE_CHUNK, offs)
    for r in range(world):  # the few bytes between a segment's end and the next multiple of 16 are read with the segment's last chunk
        if recv_bytes[r] % 16:
            recv_buf[offs[r] + recv_bytes[r]: offs[r] + (recv_bytes[r] + 15) // 16 * 16] = 0
    gsrc = _comm(send_gidx[: sum(send_records)], comm_device)
    recv_gidx = torch.empty(sum(recv_records), dtype=torch.int64, device=comm_device)
    _pairwise_exchange(dist, rank, world, gsrc, list(send_records), recv_gidx, recv_records, EXCHANGE_CHUNK // 8)
    return recv_buf, recv_gidx, [(offs[r], recv_bytes[r]) for r in range(world) if recv_bytes[r]]


KEY_ROWS_PER_GATHER = 1 << 22  # 128 MiB of keys per rank and collective


def gather_tile_keys(dist, keys, comm_device="cpu"):
    """keys: int64 [n_local, 4] = (chain_score, score, global input index, line bytes) of this rank's output lines, in its output
    order. Returns (all keys [N, 4], owner rank of every row [N]) on comm_device: an all-gather padded to the longest share."""
    import torch

    if dist is None:
        return keys, torch.zeros(keys.shape[0], dtype=torch.int64, device=keys.device)
    world = dist.get_world_size()
    keys = _comm(keys.contiguous(), comm_device)
    n = torch.tensor([keys.shape[0]], dtype=torch.int64, device=comm_device)
    counts = torch.zeros(world, dtype=torch.int64, device=comm_device)
    dist.all_gather_into_tensor(counts, n)
    counts = [int(x) for x in counts.tolist()]
    cap = max(1, max(counts))
    rows = [torch.empty(counts[r], 4, dtype=torch.int64, device=comm_device) for r in range(world)]
    step = KEY_ROWS_PER_GATHER  # rows of every rank per collective: bounded pieces instead of one multi-GB all-gather
    mine = torch.zeros(min(cap, step), 4, dtype=torch.int64, device=comm_device)
    everyone = torch.zeros(world * mine.shape[0], 4, dtype=torch.int64, device=comm_device)
    for lo in range(0, cap, step):
        k = min(step, cap - lo)
        have = max(0, min(keys.shape[0] - lo, k))
        if have:
            mine[:have] = keys[lo: lo + have]
        dist.all_gather_into_tensor(everyone[: world * k], mine[:k])
        got = everyone[: world * k].reshape(world, k, 4)
        for r in range(world):
            m = max(0, min(counts[r] - lo, k))
            if m:
                rows[r][lo: lo + m] = got[r, :m]
    owner = [torch.full((counts[r],), r, dtype=torch.int64, device=comm_device) for r in range(world)]
    return torch.cat(rows), torch.cat(owner)


def global_line_offsets(all_keys, owner, rank):
    """The single-process order of ALL records -- chain_score desc, score desc, input index (paf_cmp_by_descending_score,
    impl/paf_tile.c:28-34, ties in input order) -- and the scan of their line sizes. Returns (byte offset of every line of `rank`, in
    that rank's own output order; total bytes). Three stable sorts, least significant key first (torch.sort on whatever device the
    keys are on)."""
    import torch

    order = torch.sort(all_keys[:, 2], stable=True).indices
    order = order[torch.sort(all_keys[order, 1], descending=True, stable=True).indices]
    order = order[torch.sort(all_keys[order, 0], descending=True, stable=True).indices]
    sizes = all_keys[order, 3]
    ends = torch.cumsum(sizes, 0)
    offs = ends - sizes
    mine = owner[order] == rank  # a rank's lines keep their relative order in the global order: same comparator, disjoint sequences
    return offs[mine], int(ends[-1].item()) if ends.numel() else 0


def share_of_rank(rank, world, total):
    """Contiguous share [first, first + n) of `total` records held by `rank` before the partition."""
    base, extra = divmod(total, world)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def query_name(line):
    return line.split(b"\t", 1)[0]


def line_cuts(buf, max_bytes):
    """Cut points of a uint8 tensor of '\\n'-terminated lines into pieces of at most max_bytes that end on line boundaries
    (a longer single line stays whole). Returns [(start, end), ...]."""
    n = int(buf.numel())
    cuts, at = [], 0
    while at < n:
        end = min(n, at + max_bytes)
        if end < n:
            lo = end
            while True:  # last newline in front of `end`, looking back through windows of 64 KiB
                lo2 = max(at, lo - 65536)
                hits = (buf[lo2:lo] == 10).nonzero()
                if hits.numel():
                    end = lo2 + int(hits[-1].item()) + 1
                    break
                if lo2 == at:  # one line longer than max_bytes: take it whole (forward through windows of 1 MiB, never a whole-buffer scan)
                    hi = end
                    while hi < n:
                        hi2 = min(n, hi + (1 << 20))
                        fwd = (buf[hi:hi2] == 10).nonzero()
                        if fwd.numel():
                            hi = hi + int(fwd[0].item()) + 1
                            break
                        hi = hi2
                    end = hi
                    break
                lo = lo2
        cuts.append((at, end))
        at = end
    return cuts


class GpuTileWorker:
    """The device side of a rank in tile_sharded(): everything through the C-ABI of libpaffy_hip (paffy_amd.Engine).

    Memory: a rank never holds its share of the text more than twice. split() writes every batch's lines straight into ONE send
    buffer (paffy_hip_split_to: no per-batch regrouped copy, no concatenation) and, when the caller hands its batches over
    (`consume`), lets go of each batch as soon as it has been split; after the exchange the send buffer is dropped before tile() cuts
    what was received into 16-byte aligned batches of at most batch_bytes, and the receive buffer is dropped once they are cut."""

    def __init__(self, eng, batch_bytes=(1 << 30) + (1 << 29)):
        self.eng, self.batch_bytes, self.keep = eng, batch_bytes, []
        self._recv = self.pieces = None

    def release(self):
        """Let go of the text of the last tile (the received lines stay referenced until then: emit() reads them)."""
        self.keep = []
        self._recv = None
        self.pieces = None

    def query_names(self, batches):
        """-> ({name hash: bytes of its lines} over all batches, [per batch: {name hash: (bytes, lines)}])"""
        self.release()  # a new input: the text of the tile before it is no longer needed (it would stand beside the new send buffer)
        out, per_batch = {}, []
        for buf, nbytes in batches:
            names = self.eng.query_names_counts(buf, nbytes)
            per_batch.append(names)
            for h, (w, _) in names.items():
                out[h] = out.get(h, 0) + w
        return out, per_batch

    def split(self, batches, owner_of, world, first_record, per_batch_names=None, consume=False):
        """-> (send buffer grouped by destination, bytes per destination, global input index of every line, records per destination).
        per_batch_names: what query_names returned for the same batches: the bytes and lines every batch sends to every destination
        are known beforehand, so the send buffer and the index array are allocated once at their exact size and every batch's lines go
        straight to their place (paffy_hip_split_to). consume: `batches` is emptied batch by batch -- the caller's last reference gone,
        a batch is freed as soon as it has been split."""
        t = self.eng.torch
        dev = self.eng.device
        if per_batch_names is None:
            per_batch_names = [self.eng.query_names_counts(buf, nbytes) for buf, nbytes in batches]
        n_batches = len(batches)
        need_b = [[0] * world for _ in range(n_batches)]  # bytes / lines of batch b for destination d
        need_r = [[0] * world for _ in range(n_batches)]
        for b, names in enumerate(per_batch_names):
            for h, (w, r) in names.items():
                d = owner_of.get(h)
                d = min(h % world if d is None else d, world - 1)
                need_b[b][d] += w
                need_r[b][d] += r
        dest_bytes = [sum(need_b[b][d] for b in range(n_batches)) for d in range(world)]
        dest_recs = [sum(need_r[b][d] for b in range(n_batches)) for d in range(world)]
        total_r = sum(dest_recs)
        # One rank: nothing will be exchanged, so every batch's lines start at a multiple of 16 bytes in the buffer -- they are tiled
        # right there as text batches (`pieces`). Several ranks: the parts of a destination stand back to back, as they are sent.
        pad = (lambda x: (x + 15) // 16 * 16) if world == 1 else (lambda x: x)
        total = sum(pad(need_b[b][d]) for b in range(n_batches) for d in range(world))
        send = t.empty(big_buffer_bytes((total + 15) // 16 * 16 + 16), dtype=t.uint8, device=dev)
        gidx = t.empty(max(1, total_r), dtype=t.int64, device=dev)
        at_b, at_r = [0] * world, [0] * world
        for d in range(1, world):
            at_b[d] = at_b[d - 1] + dest_bytes[d - 1]
            at_r[d] = at_r[d - 1] + dest_recs[d - 1]
        arrays = self.eng.owner_arrays(owner_of)
        base = first_record
        pieces = []
        for b in range(n_batches):
            buf, n = batches[0] if consume else batches[b]
            pb, pr, nrec = self.eng.split_to(buf, n, world, arrays, send, at_b, gidx, at_r, base)
            if pb != need_b[b] or pr != need_r[b]:
                raise RuntimeError("split: a batch changed between query_names and split (bytes / lines per destination differ)")
            if world == 1 and pb[0]:
                pieces.append((at_b[0], pb[0]))
                if pb[0] % 16:
                    send[at_b[0] + pb[0]: at_b[0] + pad(pb[0])] = 0
            for d in range(world):
                at_b[d] += pad(pb[d])
                at_r[d] += pr[d]
            base += nrec
            if consume:
                self.eng.sync()  # the copy kernel reads the batch
                del buf
                batches.pop(0)
        self.pieces = pieces if world == 1 else None
        return send[:total], dest_bytes, gidx[:total_r], dest_recs

    def _cut(self, recv, pieces=None):
        """[(uint8 tensor, bytes)]: the pieces of recv as text batches -- where they were received when they are 16-byte aligned and
        short enough, else cut at line ends into 16-byte aligned copies of at most batch_bytes."""
        t = self.eng.torch
        if pieces is None:
            pieces = [(0, int(recv.numel()))]
        keep = []
        in_place = recv.data_ptr() % 16 == 0
        for off, n in pieces:
            room = (n + 15) // 16 * 16
            if n == 0:
                continue
            if in_place and off % 16 == 0 and n <= self.batch_bytes and off + room <= recv.numel():
                keep.append((recv[off: off + room], n))  # where it was received
                continue
            part = recv[off: off + n]
            for a, b in line_cuts(part, self.batch_bytes):
                piece = t.empty((b - a + 15) // 16 * 16 + 16, dtype=t.uint8, device=self.eng.device)  # batches are 16-byte aligned
                piece[: b - a] = part[a:b]
                piece[b - a:] = 0
                keep.append((piece, b - a))
        return keep

    def tile(self, recv_buf, pieces=None):
        """paffy tile over the lines this rank owns -> int64 [n, 5] per output line: chain_score, score, local record, bytes, level.
        pieces: [(offset, bytes)] -- whole lines starting at multiples of 16 bytes of recv_buf (what exchange_lines / split lay
        out): they are tiled where they are; a piece too long for a batch, or a buffer without pieces, is cut at line ends into
        16-byte aligned copies. recv_buf may be a one-element list (tile_sharded hands over its only reference)."""
        holder = recv_buf if isinstance(recv_buf, list) else [recv_buf]
        recv = holder[0].to(self.eng.device)
        self.keep = self._cut(recv, pieces)
        if isinstance(recv_buf, list):
            recv_buf.clear()
        self._recv = recv if any(x.data_ptr() >= recv.data_ptr() and x.data_ptr() < recv.data_ptr() + max(1, recv.numel()) for x, _ in self.keep) else None
        del recv, holder
        self.info = self.eng.tile_batches(self.keep)
        if self.info.error.code:
            raise RuntimeError(f"tile failed on this rank: code {self.info.error.code} at local record {self.info.error.record}")
        return self.eng.tile_keys(self.info.n_rows)

    def tile_direct(self, batches, consume=False):
        """paffy tile over text batches [(uint8 tensor, bytes)] as they are (16-byte aligned, whole lines, below 2 GiB each): what a
        single rank does, no partition. Same return value as tile(). consume: the list is emptied (the worker holds the batches until
        the lines have been written -- the text is read where it is)."""
        self.release()
        self.keep = [(buf, n) for buf, n in batches if n]
        if consume:
            del batches[:]
        self.info = self.eng.tile_batches(self.keep)
        if self.info.error.code:
            raise RuntimeError(f"tile failed on this rank: code {self.info.error.code} at local record {self.info.error.record}")
        return self.eng.tile_keys(self.info.n_rows)

    def emit(self):
        """-> uint8 tensor with this rank's output lines in its output order"""
        out = self.eng.alloc_out(big_buffer_bytes(self.info.out_bytes))
        if self.info.out_bytes:
            self.eng.emit(out)
        return out[: self.info.out_bytes]

    def scatter(self, src, src_off, dst_off, dst):
        self.eng.scatter_lines(src, src_off, dst_off, dst)


def tile_sharded(worker, dist, rank, world, batches, first_record, comm_device="cpu", consume=False):
    """`paffy tile` over an input spread over the ranks (this rank holds `batches`, whose first record is global record
    first_record). Returns {"offsets": byte offset of every local output line in the ordered output (int64 tensor), "total": bytes
    of the whole output, "keys": the worker's [n, 5] keys}; worker.emit() then gives the local lines.
    consume: the list `batches` is emptied as its batches are split (hand over the only reference and a rank holds its share of the
    text at most twice at any time: batches + send buffer, send + receive buffer, receive buffer + tile batches)."""
    import os
    import time

    import torch

    timing, t0 = {}, time.perf_counter()
    trace = bool(os.environ.get("PAFFY_SHARD_TIMING"))

    peak, live = [0], [0]

    def lap(name):
        nonlocal t0
        if trace:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
                free_b, total_b = torch.cuda.mem_get_info()
                peak[0] = max(peak[0], total_b - free_b)
                # live = in use minus what torch's caching allocator holds without a tensor in it
                live[0] = max(live[0], total_b - free_b - (torch.cuda.memory_reserved() - torch.cuda.memory_allocated()))
            t1 = time.perf_counter()
            timing[name] = timing.get(name, 0.0) + (t1 - t0) * 1e3
            t0 = t1

    if world == 1 and hasattr(worker, "tile_direct"):
        # One rank owns every query sequence: there is nothing to partition, the batches are tiled where they are (the reference's
        # single process, impl/paf_tile.c:156-178). The key exchange and the offsets below are the N-rank code with N = 1.
        keys = worker.tile_direct(batches, consume)
        lap("tile_ms")
        k4 = torch.stack([keys[:, 0], keys[:, 1], keys[:, 2] + first_record, keys[:, 3]], dim=1) if keys.shape[0] else torch.zeros(0, 4, dtype=torch.int64, device=keys.device)
        all_keys, owner = gather_tile_keys(dist, k4, comm_device)
        offsets, total = global_line_offsets(all_keys, owner, rank)
        lap("keys_ms")
        return {"offsets": offsets, "total": total, "keys": keys, "owner_of": None, "timing": timing, "hbm_peak": peak[0] or None, "hbm_live_peak": live[0] or None}
    local, per_batch = worker.query_names(batches)
    weights = merge_name_weights(dist, local, comm_device)
    owner_of = owner_table(weights, world)
    lap("names_ms")
    try:
        send, send_bytes, send_gidx, send_records = worker.split(batches, owner_of, world, first_record, per_batch, consume)
    except Exception:
        worker.eng.drop_index()  # no kept index outlives a failed partition
        raise
    lap("split_ms")
    recv, recv_gidx, pieces = exchange_lines(dist, send, send_bytes, send_gidx, send_records, comm_device, getattr(worker, "pieces", None))
    del send  # with ranks: the receive buffer holds this rank's lines now; without: recv is the send buffer itself
    lap("exchange_ms")
    holder = [recv]
    del recv
    keys = worker.tile(holder, pieces)
    lap("tile_ms")
    gidx = recv_gidx.to(keys.device)
    k4 = torch.stack([keys[:, 0], keys[:, 1], gidx[keys[:, 2]], keys[:, 3]], dim=1) if keys.shape[0] else torch.zeros(0, 4, dtype=torch.int64, device=keys.device)
    all_keys, owner = gather_tile_keys(dist, k4, comm_device)
    offsets, total = global_line_offsets(all_keys, owner, rank)
    lap("keys_ms")
    return {"offsets": offsets, "total": total, "keys": keys, "owner_of": owner_of, "timing": timing, "hbm_peak": peak[0] or None, "hbm_live_peak": live[0] or None}


def gather_ordered_output(worker, dist, rank, world, lines, line_bytes, offsets, total, comm_device="cpu", writer=0):
    """The ordered write for outputs that fit one rank: every rank's lines (uint8 tensor `lines`, sizes `line_bytes`, places
    `offsets`) travel to `writer`, which scatters them to their offsets. Returns the whole output on the writer, None elsewhere."""
    import torch

    if dist is None:
        src_off = torch.zeros(line_bytes.numel() + 1, dtype=torch.int64, device=lines.device)
        src_off[1:] = torch.cumsum(line_bytes, 0)
        out = torch.zeros(max(16, (total + 15) // 16 * 16), dtype=torch.uint8, device=lines.device)
        worker.scatter(lines, src_off, offsets.to(lines.device), out)
        return out[:total]
    meta = torch.tensor([int(lines.numel()), int(line_bytes.numel())], dtype=torch.int64, device=comm_device)
    metas = torch.zeros(world * 2, dtype=torch.int64, device=comm_device)
    dist.all_gather_into_tensor(metas, meta)
    metas = metas.reshape(world, 2)
    cap_b, cap_n = max(1, int(metas[:, 0].max().item())), max(1, int(metas[:, 1].max().item()))
    pad_b = torch.zeros(cap_b, dtype=torch.uint8, device=comm_device)
    pad_b[: lines.numel()] = _comm(lines, comm_device)
    pad_n = torch.zeros(cap_n, 2, dtype=torch.int64, device=comm_device)
    pad_n[: line_bytes.numel(), 0] = _comm(line_bytes, comm_device)
    pad_n[: offsets.numel(), 1] = _comm(offsets, comm_device)
    all_b = [torch.zeros(cap_b, dtype=torch.uint8, device=comm_device) for _ in range(world)] if rank == writer else None
    all_n = [torch.zeros(cap_n, 2, dtype=torch.int64, device=comm_device) for _ in range(world)] if rank == writer else None
    dist.gather(pad_b, all_b, dst=writer)
    dist.gather(pad_n, all_n, dst=writer)
    if rank != writer:
        return None
    dev = lines.device
    out = torch.zeros(max(16, (total + 15) // 16 * 16), dtype=torch.uint8, device=dev)
    for r in range(world):
        nb, nl = int(metas[r, 0].item()), int(metas[r, 1].item())
        if nl == 0:
            continue
        sizes = all_n[r][:nl, 0].to(dev)
        src_off = torch.zeros(nl + 1, dtype=torch.int64, device=dev)
        src_off[1:] = torch.cumsum(sizes, 0)
        worker.scatter(all_b[r][:nb].to(dev), src_off, all_n[r][:nl, 1].to(dev).contiguous(), out)
    return out[:total]


# ---- chain across ranks -------------------------------------------------------------------------
#
# `paffy chain` links records of one (query, target, strand) only (impl/chaining.c:37-54), so a partition by query name keeps every
# group whole and the links, chain scores and cuts of a part are those of the whole input. Steps 1-2 are tile's (names, partition,
# exchange_lines). Then:
#   3. every rank runs its part up to the cut of the chains (paffy_hip_chain_run_part), the records carrying their global input numbers;
#   4. an all-gather of (strand class, chain-end score, processing key, global number) -- 32 bytes per chain -- and global_chain_ids give
#      every chain the number (cn) one process would;
#   5. paffy_hip_chain_renumber finishes the part with those numbers: output order, tags, paf_check, line sizes;
#   6. an all-gather of (own score, chain id, link, line bytes) -- 32 bytes per line -- and chain_line_offsets give every local line its
#      byte offset in the ordered output; the lines are written there (scatter) or stay where they are.
# Failures: a part's parse / assert error ends the run for everyone before step 4 (the lowest stage, then the lowest global record, is
# what one process reports); a failed paf_check after step 5 (the smallest (chain id, link): the order the reference checks in).


def global_chain_ids(all_tail_keys):
    """all_tail_keys: int64 [N, 4] = (strand class, chain-end score, processing key, global record number) of ALL chains, the parts
    one after the other. Returns int64 [N]: every chain's number in the whole input -- its rank by (class asc, score desc, key desc,
    number desc), the order one process pulls the chains out in (impl/chaining.c:213-230, '+' before '-', :304-305). Four stable
    sorts, least significant key first; pure torch, on whatever device the keys are on."""
    import torch

    k = all_tail_keys
    order = torch.sort(k[:, 3], descending=True, stable=True).indices
    order = order[torch.sort(k[order, 2], descending=True, stable=True).indices]
    order = order[torch.sort(k[order, 1], descending=True, stable=True).indices]
    order = order[torch.sort(k[order, 0], stable=True).indices]
    ids = torch.empty(k.shape[0], dtype=torch.int64, device=k.device)
    ids[order] = torch.arange(k.shape[0], dtype=torch.int64, device=k.device)
    return ids


def chain_line_offsets(all_line_keys, owner, rank):
    """all_line_keys: int64 [N, 4] = (own score, chain id, link, line bytes) of ALL output lines, every part's in its own output order;
    owner: the part of every row. The single-process order -- own score desc, then chain id, then link (paf_cmp_by_score over the
    chains as they were written out, impl/chaining.c:337) -- and the scan of the sizes. Returns (byte offset of every line of `rank`,
    in that rank's output order; total bytes): global_line_offsets with chain's three keys."""
    import torch

    k = all_line_keys
    order = torch.sort(k[:, 2], stable=True).indices
    order = order[torch.sort(k[order, 1], stable=True).indices]
    order = order[torch.sort(k[order, 0], descending=True, stable=True).indices]
    sizes = k[order, 3]
    ends = torch.cumsum(sizes, 0)
    offs = ends - sizes
    mine = owner[order] == rank  # a rank's lines keep their relative order: same comparator, disjoint chains
    return offs[mine], int(ends[-1].item()) if ends.numel() else 0


def first_failure(dist, mine, comm_device="cpu"):
    """mine: None, or (sort key: three ints, (code, stage, record, aux)) of this rank's failure. Every rank gets the failure with the
    smallest key over all ranks as a dict, or None when nobody failed: 64 bytes per rank."""
    import torch

    row = [0] * 8 if mine is None else [1, *mine[0], *mine[1]]
    rows = torch.tensor([row], dtype=torch.int64, device=comm_device)
    if dist is not None:
        everyone = torch.zeros(dist.get_world_size(), 8, dtype=torch.int64, device=comm_device)
        dist.all_gather_into_tensor(everyone, rows)
        rows = everyone
    return least_failure([(tuple(r[1:4]), tuple(r[4:])) for r in rows.cpu().tolist() if r[0]])


def least_failure(failures):
    """[(sort key, (code, stage, record, aux))] -> the failure with the smallest key as a dict, None for an empty list"""
    if not failures:
        return None
    code, stage, record, aux = min(failures)[1]
    return {"code": code, "stage": stage, "record": record, "aux": aux}


def part_failure(info, fail=None, side=None, record=None):
    """A part's PlanInfo (and the failing line's key after renumber) as first_failure / least_failure take it. read_pafs parses every
    line before anything is chained, so stage -1 sorts before the asserts of the trim (stage 0), the lowest global record first; a
    failed paf_check sorts by (chain id, link): the order the reference checks in (impl/chaining.c:321-334).
    side (to_bed in parts: -1 the line did not parse, 0 query side, 1 target side) and record (the failing line's global input
    number): to_bed reads, counts and checks record by record (impl/paf_to_bed.c:166-180), a record's query side before its target
    side, so its failures sort by (global record, parse before query side before target side)."""
    e = info.error
    if not e.code:
        return None
    if side is not None:
        rec = e.record if record is None else record
        return (rec, side + 1, 0), (e.code, e.stage, rec, e.aux)
    return ((fail[1], fail[2], 0) if fail else (e.stage, e.record, 0)), (e.code, e.stage, e.record, e.aux)


class GpuChainWorker(GpuTileWorker):
    """The device side of a rank in chain_sharded(): the partition is the tile worker's (query_names, split); the part runs through
    the chain-in-parts calls of libpaffy_hip. opts: gap_open, gap_extend, max_gap, trim (the command's -d -e -g -t)."""

    def __init__(self, eng, batch_bytes=(1 << 30) + (1 << 29), **opts):
        super().__init__(eng, batch_bytes)
        self.opts = opts
        self.gidx = None

    def release(self):
        super().release()
        self.gidx = None

    def run_part(self, recv_buf, recv_gidx, pieces=None):
        """The part over the lines this rank owns (recv_buf / pieces as for tile(); recv_gidx: the global input number of every line,
        in the order of the pieces): every piece is added where it lies, with its slice of the numbers. Returns the PlanInfo."""
        t = self.eng.torch
        holder = recv_buf if isinstance(recv_buf, list) else [recv_buf]
        recv = holder[0].to(self.eng.device)
        self.keep = self._cut(recv, pieces) if recv.numel() else []
        if isinstance(recv_buf, list):
            recv_buf.clear()
        self._recv = recv
        del holder
        gidx = recv_gidx.to(device=self.eng.device, dtype=t.int64).contiguous()
        self.gidx, per_batch, at = gidx, [], 0
        for buf, n in self.keep:  # every line ends with a newline (the splitter adds the last one)
            lines = int((buf[:n] == 10).sum().item())
            per_batch.append(gidx[at: at + lines])
            at += lines
        if at != gidx.numel():
            raise RuntimeError(f"run_part: {gidx.numel()} record numbers for {at} lines")
        self.info = self.eng.chain_part(self.keep, per_batch, **self.opts)
        return self.info

    def tail_keys(self):
        return self.eng.chain_tail_keys(self.info.n_records)

    def renumber(self, ids):
        self.info, fail = self.eng.chain_renumber(ids)
        return self.info, fail

    def line_keys(self):
        return self.eng.chain_line_keys(self.info.n_rows)

    def global_records(self):
        """The global input number of every output line, in output order (paffy_hip_plan_rows through the received numbers)."""
        rec, _ = self.eng.plan_rows(self.info.n_rows)
        return self.gidx[self.eng.torch.tensor(rec, dtype=self.eng.torch.int64, device=self.eng.device)] if rec else self.gidx[:0]


_NO_FRESH_IN_PARTS = ("chain in parts does not restate the walk from a fresh iterator: whether a search is fresh depends on the strand's "
                      "leading single-group run, a property of the whole input and not of a part; chain it in one context (Engine.chain)")


def chain_sharded(worker, dist, rank, world, batches, first_record, comm_device="cpu", consume=False, fresh_walk=False):
    """`paffy chain` over an input spread over the ranks (this rank holds `batches`, whose first record is global record
    first_record); one rank runs the same code with world = 1 and dist = None. Returns {"error": None, "offsets": byte offset of every
    local output line in the ordered output, "total": bytes of the whole output, "keys": the [n, 4] line keys (column 3: the line
    sizes), "chain_ids": the numbers this rank's chains got}; worker.emit() then gives the local lines. When any record of any rank
    fails: {"error": {"code", "stage", "record", "aux"}, "total": 0, ...} -- the failure one process reports, the same on every rank --
    and nothing is to be written."""
    import torch

    if fresh_walk:
        raise ValueError("chain_sharded(fresh_walk=True): " + _NO_FRESH_IN_PARTS)
    dev = worker.eng.device
    empty = {"offsets": torch.zeros(0, dtype=torch.int64, device=comm_device), "total": 0, "keys": torch.zeros(0, 4, dtype=torch.int64, device=dev), "chain_ids": None}
    local, per_batch = worker.query_names(batches)
    weights = merge_name_weights(dist, local, comm_device)
    owner_of = owner_table(weights, world)
    try:
        send, send_bytes, send_gidx, send_records = worker.split(batches, owner_of, world, first_record, per_batch, consume)
    except Exception:
        worker.eng.drop_index()  # no kept index outlives a failed partition
        raise
    recv, recv_gidx, pieces = exchange_lines(dist, send, send_bytes, send_gidx, send_records, comm_device, getattr(worker, "pieces", None))
    del send
    holder = [recv]
    del recv
    err = first_failure(dist, part_failure(worker.run_part(holder, recv_gidx, pieces)), comm_device)
    if err:
        return dict(empty, error=err, owner_of=owner_of)
    all_tails, tail_owner = gather_tile_keys(dist, worker.tail_keys(), comm_device)
    ids = global_chain_ids(all_tails)[tail_owner == rank]
    err = first_failure(dist, part_failure(*worker.renumber(ids)), comm_device)
    if err:
        return dict(empty, error=err, owner_of=owner_of)
    keys = worker.line_keys()
    all_keys, owner = gather_tile_keys(dist, keys, comm_device)
    offsets, total = chain_line_offsets(all_keys, owner, rank)
    return {"error": None, "offsets": offsets, "total": total, "keys": keys, "chain_ids": ids, "owner_of": owner_of}


def chain_in_parts(workers, batches, first_record=0, fresh_walk=False):
    """chain_sharded without ranks: one process, one GpuChainWorker (one context) per part on the same GPU, taken in turn -- the
    partition with the real query_names / split_to, the keys exchanged in device memory, every part's lines scattered into one
    buffer. Returns {"error": None, "out": uint8 tensor with the ordered output, ...} or {"error": {...}, "out": None}."""
    import torch

    if fresh_walk:
        raise ValueError("chain_in_parts(fresh_walk=True): " + _NO_FRESH_IN_PARTS)
    k_parts, w0 = len(workers), workers[0]
    local, per_batch = w0.query_names(batches)
    owner_of = owner_table(local, k_parts)
    send, send_bytes, send_gidx, send_records = w0.split(batches, owner_of, k_parts, first_record, per_batch)
    failures, at_b, at_r = [], 0, 0
    for w, nb, nr in zip(workers, send_bytes, send_records):  # a part's lines stand back to back in the send buffer
        failures.append(part_failure(w.run_part(send, send_gidx[at_r: at_r + nr], [(at_b, nb)] if k_parts > 1 else w0.pieces)))
        at_b, at_r = at_b + nb, at_r + nr
    err = least_failure([f for f in failures if f])
    if err:
        return {"error": err, "out": None, "total": 0}
    tails = [w.tail_keys() for w in workers]
    ids = global_chain_ids(torch.cat(tails))
    at = 0
    for w, t in zip(workers, tails):
        failures.append(part_failure(*w.renumber(ids[at: at + t.shape[0]])))
        at += t.shape[0]
    err = least_failure([f for f in failures if f])
    if err:
        return {"error": err, "out": None, "total": 0}
    keys = [w.line_keys() for w in workers]
    all_keys = torch.cat(keys)
    owner = torch.cat([torch.full((k.shape[0],), p, dtype=torch.int64, device=k.device) for p, k in enumerate(keys)])
    out = total = None
    for p, (w, k) in enumerate(zip(workers, keys)):
        offsets, total = chain_line_offsets(all_keys, owner, p)
        if out is None:
            out = torch.zeros(max(16, (total + 15) // 16 * 16), dtype=torch.uint8, device=all_keys.device)
        if k.shape[0]:
            src_off = torch.zeros(k.shape[0] + 1, dtype=torch.int64, device=k.device)
            src_off[1:] = torch.cumsum(k[:, 3], 0)
            w.scatter(w.emit(), src_off, offsets.contiguous(), out)
    return {"error": None, "out": out[:total], "total": total, "chain_ids": ids, "tail_keys": tails, "line_keys": keys}


# ---- to_bed across ranks -----------------------------------------------------------------------
#
# `paffy to_bed` keeps two bytes per base of every sequence and all records that count on a sequence must meet in one place, so it is
# sharded by SEQUENCE. Without -n that is tile's partition by query name. With -n (--includeInverted) a record also counts on its target
# sequence, as the inverted record would (impl/paf_to_bed.c:170-177), and the two sequences may have different owners:
#   1. side_names: the distinct names of the counted sides and the bytes of the lines that name them, merged over the ranks and dealt
#      (merge_name_weights, owner_table);
#   2. split_sides: a line goes to owner(query name) and, when that is another rank, to owner(target name) too; every copy carries a side
#      mask (bit 0: count the query side here, bit 1: the target side) and its global input number. exchange_lines moves text and numbers,
#      exchange_sides the masks;
#   3. run_part: the rank counts the sides it was given and plans its BED lines: one block of lines per sequence, the blocks in the
#      order its sequences first appeared in;
#   4. an all-gather of (2 * global record of first appearance + side, block bytes) -- 32 bytes per sequence -- and bed_block_offsets give
#      every block its place: one process writes the sequences in order of first appearance, a record's query side before its target side.
# The -q tail of the command (sequences of a FASTA file that no record names, impl/paf_to_bed.c:187-190) is not part of this: the caller
# appends it from the union of the names seen, as the command line does after its single run. The counters a rank holds afterwards
# (Engine / paffy_hip_bed_counts) are those of its own sequences only.


def bed_block_offsets(all_keys, owner, rank):
    """all_keys: int64 [N, >= 2] = (2 * global record of first appearance + side, bytes of the block, ...) of ALL sequences, every
    part's in its own output order; owner: the part of every row. The single-process order is ascending key. Returns (byte offset of
    every block of `rank`, in that rank's own order; total bytes). A block of 0 bytes (every line excluded) keeps its place."""
    import torch

    order = torch.sort(all_keys[:, 0], stable=True).indices
    sizes = all_keys[order, 1]
    ends = torch.cumsum(sizes, 0)
    offs = ends - sizes
    mine = owner[order] == rank  # a part's records stand in global input order: its blocks keep their relative order
    return offs[mine], int(ends[-1].item()) if ends.numel() else 0


def exchange_sides(dist, send_sides, send_records, comm_device="cpu"):
    """The side masks of exchange_lines' lines: uint8, one per line, grouped by destination like the global input numbers. Returns
    (masks, lines received from every source rank): the second says how many lines each of exchange_lines' pieces holds."""
    import torch

    if dist is None or dist.get_world_size() == 1:
        return send_sides[: int(sum(send_records))], [int(send_records[0])]
    rank, world = dist.get_rank(), dist.get_world_size()
    sizes = torch.tensor(list(send_records), dtype=torch.int64, device=comm_device)
    got = torch.zeros_like(sizes)
    dist.all_to_all_single(got, sizes)
    recv_records = [int(x) for x in got.tolist()]
    src = _comm(send_sides[: sum(send_records)], comm_device)
    recv = torch.empty(sum(recv_records), dtype=torch.uint8, device=comm_device)
    _pairwise_exchange(dist, rank, world, src, list(send_records), recv, recv_records, EXCHANGE_CHUNK)
    return recv, recv_records


BED_OPTS = ("binary", "exclude_unaligned", "exclude_aligned", "min_size", "include_inverted")


class GpuBedWorker(GpuTileWorker):
    """The device side of a rank in to_bed_sharded(): the partition by the names of both sides and the masked coverage run, through
    the to_bed-in-parts calls of libpaffy_hip."""

    def __init__(self, eng, batch_bytes=(1 << 30) + (1 << 29)):
        super().__init__(eng, batch_bytes)
        self.gidx = self.piece_lines = None

    def release(self):
        super().release()
        self.gidx = self.piece_lines = None

    def side_names(self, batches, include_inverted):
        """-> ({name hash: bytes of the lines that count on it} over all batches, [per batch: {name hash: (bytes, lines)}])"""
        self.release()
        out, per_batch = {}, []
        for buf, nbytes in batches:
            names = self.eng.side_names_counts(buf, nbytes, include_inverted)
            per_batch.append(names)
            for h, (w, _) in names.items():
                out[h] = out.get(h, 0) + w
        return out, per_batch

    def split_sides(self, batches, owner_of, world, first_record, include_inverted, consume=False):
        """-> (send buffer grouped by destination, bytes per destination, global input index of every written line, its side mask,
        lines per destination). A counting pass over every batch (paffy_hip_split_sides_count) gives the exact sizes first -- a line
        whose two names share an owner is sent once --, so the send buffer, the index array and the mask array are allocated once at
        their exact size, as split() does from the per-name counts."""
        t = self.eng.torch
        dev = self.eng.device
        arrays = self.eng.owner_arrays(owner_of)
        n_batches = len(batches)
        need_b, need_r = [], []
        for buf, n in batches:
            pb, pr, _ = self.eng.split_sides_count(buf, n, include_inverted, world, arrays)
            need_b.append(pb)
            need_r.append(pr)
        dest_bytes = [sum(need_b[b][d] for b in range(n_batches)) for d in range(world)]
        dest_recs = [sum(need_r[b][d] for b in range(n_batches)) for d in range(world)]
        total_r = sum(dest_recs)
        pad = (lambda x: (x + 15) // 16 * 16) if world == 1 else (lambda x: x)  # one rank: every batch's lines are run where they are
        total = sum(pad(need_b[b][d]) for b in range(n_batches) for d in range(world))
        send = t.empty(big_buffer_bytes((total + 15) // 16 * 16 + 16), dtype=t.uint8, device=dev)
        gidx = t.empty(max(1, total_r), dtype=t.int64, device=dev)
        sides = t.empty(max(1, total_r), dtype=t.uint8, device=dev)
        at_b, at_r = [0] * world, [0] * world
        for d in range(1, world):
            at_b[d] = at_b[d - 1] + dest_bytes[d - 1]
            at_r[d] = at_r[d - 1] + dest_recs[d - 1]
        base = first_record
        pieces, piece_lines = [], []
        for b in range(n_batches):
            buf, n = batches[0] if consume else batches[b]
            pb, pr, nrec = self.eng.split_sides_to(buf, n, include_inverted, world, arrays, send, at_b, gidx, sides, at_r, base)
            if pb != need_b[b] or pr != need_r[b]:
                raise RuntimeError("split_sides: a batch changed between its count and its split (bytes / lines per destination differ)")
            if world == 1 and pb[0]:
                pieces.append((at_b[0], pb[0]))
                piece_lines.append(pr[0])
                if pb[0] % 16:
                    send[at_b[0] + pb[0]: at_b[0] + pad(pb[0])] = 0
            for d in range(world):
                at_b[d] += pad(pb[d])
                at_r[d] += pr[d]
            base += nrec
            if consume:
                self.eng.sync()  # the copy kernel reads the batch
                del buf
                batches.pop(0)
        self.pieces, self.piece_lines = (pieces, piece_lines) if world == 1 else (None, None)
        return send[:total], dest_bytes, gidx[:total_r], sides[:total_r], dest_recs

    def run_part(self, recv_buf, recv_gidx, recv_sides, pieces=None, opts=None, piece_lines=None):
        """to_bed over the lines this rank owns (recv_buf / pieces as for tile(); recv_gidx / recv_sides: the global input number and
        the side mask of every line, in the order of the pieces; piece_lines: the lines of every piece, as the split counted them and
        the exchange passed them on -- only a piece that has to be cut into several batches, or pieces without counts, are counted
        by their newlines). Returns (keys, None) -- int64 [sequences, 4] per block of BED lines,
        in output order: 2 * global record of first appearance + side, bytes, lines, local entry -- or (None, failure) with the
        failure as part_failure gives it (the record a global input number)."""
        t = self.eng.torch
        opts = {k: v for k, v in (opts or {}).items() if k in BED_OPTS}
        holder = recv_buf if isinstance(recv_buf, list) else [recv_buf]
        recv = holder[0].to(self.eng.device)
        self.keep, lines_of = [], []
        if recv.numel() and piece_lines is not None and pieces is not None and len(piece_lines) == len(pieces):
            for piece, lines in zip(pieces, piece_lines):
                cut = self._cut(recv, [piece])
                self.keep += cut  # one batch: its lines are the piece's; several: every line ends with a newline (the splitter's)
                lines_of += [int(lines)] if len(cut) == 1 else [int((buf[:n] == 10).sum().item()) for buf, n in cut]
        elif recv.numel():
            self.keep = self._cut(recv, pieces)
            lines_of = [int((buf[:n] == 10).sum().item()) for buf, n in self.keep]
        if isinstance(recv_buf, list):
            recv_buf.clear()
        self._recv = recv
        del holder
        gidx = recv_gidx.to(device=self.eng.device, dtype=t.int64).contiguous()
        sides = recv_sides.to(device=self.eng.device, dtype=t.uint8).contiguous()
        self.gidx, per_batch, at = gidx, [], 0
        for lines in lines_of:
            per_batch.append(sides[at: at + lines])
            at += lines
        if at != gidx.numel() or at != sides.numel():
            raise RuntimeError(f"run_part: {gidx.numel()} record numbers and {sides.numel()} side masks for {at} lines")
        self.info = self.eng.bed_part(self.keep, per_batch, **opts)
        if self.info.error.code:
            return None, part_failure(self.info, side=self.eng.bed_failure_side(), record=int(gidx[self.info.error.record].item()))
        k3 = self.eng.bed_sequence_keys()
        if not k3.shape[0]:
            return t.zeros(0, 4, dtype=t.int64, device=self.eng.device), None
        return t.stack([2 * gidx[k3[:, 0] >> 1] + (k3[:, 0] & 1), k3[:, 1], k3[:, 2], k3[:, 0]], dim=1), None

    def scatter(self, src, src_off, dst_off, dst):
        """Blocks to their places. A part whose sequences all have 0-byte blocks (every line excluded by -e / -f / -m) has keys and
        no bytes: there is nothing to place, and an empty tensor has no address to hand to the library."""
        if src.numel():
            super().scatter(src, src_off, dst_off, dst)


def to_bed_sharded(worker, dist, rank, world, batches, first_record, opts, comm_device="cpu", consume=False):
    """`paffy to_bed` over an input spread over the ranks (this rank holds `batches`, whose first record is global record
    first_record; opts: binary, exclude_unaligned, exclude_aligned, min_size, include_inverted); one rank runs the same code with
    world = 1 and dist = None. Returns {"error": None, "offsets": byte offset of every local block of BED lines (one per sequence, in
    local output order) in the one-process output, "total": bytes of the whole output, "keys": the [n, 4] block keys (column 1: the
    block sizes)}; worker.emit() then gives the local blocks back to back. When any record of any rank fails: {"error": {"code",
    "stage", "record", "aux"}, "total": 0, ...} -- the failure one process reports, the same on every rank -- and nothing is to be
    written. The -q tail of the command is the caller's (see above)."""
    import torch

    dev = worker.eng.device
    inv = bool((opts or {}).get("include_inverted"))
    empty = {"offsets": torch.zeros(0, dtype=torch.int64, device=comm_device), "total": 0, "keys": torch.zeros(0, 4, dtype=torch.int64, device=dev)}
    local, _ = worker.side_names(batches, inv)
    weights = merge_name_weights(dist, local, comm_device)
    owner_of = owner_table(weights, world)
    try:
        send, send_bytes, send_gidx, send_sides, send_records = worker.split_sides(batches, owner_of, world, first_record, inv, consume)
    except Exception:
        worker.eng.drop_index()  # no kept index outlives a failed partition
        raise
    recv, recv_gidx, pieces = exchange_lines(dist, send, send_bytes, send_gidx, send_records, comm_device, getattr(worker, "pieces", None))
    recv_sides, recv_records = exchange_sides(dist, send_sides, send_records, comm_device)
    del send
    holder = [recv]
    del recv
    # a piece per source rank that sent bytes (several ranks), or per batch as the splitter laid them out (one rank)
    piece_lines = [n for n in recv_records if n] if world > 1 else getattr(worker, "piece_lines", None)
    keys, fail = worker.run_part(holder, recv_gidx, recv_sides, pieces, opts, piece_lines)
    err = first_failure(dist, fail, comm_device)
    if err:
        return dict(empty, error=err, owner_of=owner_of)
    all_keys, owner = gather_tile_keys(dist, keys, comm_device)
    offsets, total = bed_block_offsets(all_keys, owner, rank)
    return {"error": None, "offsets": offsets, "total": total, "keys": keys, "owner_of": owner_of}


def to_bed_in_parts(workers, batches, opts, first_record=0, owner_of=None):
    """to_bed_sharded without ranks: one process, one GpuBedWorker (one context) per part on the same GPU, taken in turn -- the
    partition with the real side_names / split_sides, the block keys exchanged in device memory, every part's blocks scattered into
    one buffer. owner_of ({name hash: part}): a deal of the caller's instead of owner_table's. Returns {"error": None, "out": uint8
    tensor with the ordered output, ...} or {"error": {...}, "out": None}."""
    import torch

    k_parts, w0 = len(workers), workers[0]
    inv = bool((opts or {}).get("include_inverted"))
    local, _ = w0.side_names(batches, inv)
    if owner_of is None:
        owner_of = owner_table(local, k_parts)
    try:
        send, send_bytes, send_gidx, send_sides, send_records = w0.split_sides(batches, owner_of, k_parts, first_record, inv)
    except Exception:
        w0.eng.drop_index()
        raise
    keys, failures, at_b, at_r = [], [], 0, 0
    for w, nb, nr in zip(workers, send_bytes, send_records):  # a part's lines stand back to back in the send buffer
        k, fail = w.run_part(send, send_gidx[at_r: at_r + nr], send_sides[at_r: at_r + nr], [(at_b, nb)] if k_parts > 1 else w0.pieces, opts,
                             [nr] if k_parts > 1 else w0.piece_lines)
        keys.append(k)
        failures.append(fail)
        at_b, at_r = at_b + nb, at_r + nr
    err = least_failure([f for f in failures if f])
    if err:
        return {"error": err, "out": None, "total": 0, "owner_of": owner_of, "sides": send_sides}
    all_keys = torch.cat(keys)
    owner = torch.cat([torch.full((k.shape[0],), p, dtype=torch.int64, device=k.device) for p, k in enumerate(keys)])
    out = total = None
    for p, (w, k) in enumerate(zip(workers, keys)):
        offsets, total = bed_block_offsets(all_keys, owner, p)
        if out is None:
            out = torch.zeros(max(16, (total + 15) // 16 * 16), dtype=torch.uint8, device=all_keys.device)
        if k.shape[0]:
            src_off = torch.zeros(k.shape[0] + 1, dtype=torch.int64, device=k.device)
            src_off[1:] = torch.cumsum(k[:, 1], 0)
            w.scatter(w.emit(), src_off, offsets.contiguous(), out)
    return {"error": None, "out": out[:total], "total": total, "keys": keys, "owner_of": owner_of, "sides": send_sides}


# ---- dedupe across ranks -----------------------------------------------------------------------
#
# `paffy dedupe [-a]` writes the first record of every class -- a class is a key (names, strand, four coordinates; the device compares
# 128-bit hashes of them), with -a a key and its swapped key -- and ends at the first record that fails (impl/paf_dedupe.c:117-143). The
# decision needs a class's records in one place, not the input, so it is sharded by the OWNER of the class key: every rank holds a
# consecutive share of the records and per round (one batch per rank)
#   1. keys: one 32-byte entry per record (class key, global input number, flags), grouped by owner -- a pure function of the class key;
#   2. the entries travel to their owners (_pairwise_exchange: 32 bytes per record);
#   3. decide: the owner sorts what it got by (class, number), finds every class's first record and looks the class up in its memory of
#      the classes written in earlier rounds: one verdict byte per entry (bit 0 written, bit 1 fails);
#   4. the bytes travel back the way the entries came (the counts transposed: 1 byte per record);
#   5. verdicts: every rank finds its lowest failing record, an all-reduce (min) finds the run's;
#   6. plan / emit: every rank writes its records with bit 0 in front of that record, in input order.
# The text never moves; the ordered output is the ranks' outputs in rank order, round by round (gather_batch_sizes, gather_to_writer).

DEDUPE_ENTRY_BYTES, DEDUPE_VERDICT_BYTES = 32, 1


def dedupe_owner(class_hi, class_lo, n_parts):
    """The part that owns a class key: what dd_owner computes on the device (paffy_amd/csrc/dedupe_parts_kernel.h) -- the 64-bit
    finalizer of hi ^ lo, mapped to [0, n_parts) by the high half of the 128-bit product."""
    mask = (1 << 64) - 1
    x = (class_hi ^ class_lo) & mask
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & mask
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & mask
    x ^= x >> 33
    return (x * n_parts) >> 64


class GpuDedupeWorker:
    """The device side of a part in dedupe_sharded() / dedupe_in_parts(): one Engine (one context), source and owner at once."""

    def __init__(self, eng):
        self.eng = eng
        self.info = None

    def reset(self):
        self.eng.dedupe_reset()

    def count_records(self, batch):
        """lines of a device batch (uint8 tensor, bytes): a last line without a newline is a record"""
        buf, n = batch
        return 0 if n == 0 else int((buf[:n] == 10).sum().item()) + (0 if int(buf[n - 1].item()) == 10 else 1)

    def keys(self, batch, check_inverse, rec_base, n_parts):
        buf, n = batch
        self.batch = batch  # the lines are written from it
        return self.eng.dedupe_part_keys(buf, n, check_inverse, rec_base, n_parts)

    def decide(self, entries, check_inverse):
        return self.eng.dedupe_part_decide(entries, check_inverse)

    def verdicts(self, v):
        return self.eng.dedupe_part_verdicts(v)

    def plan(self, first_bad_global):
        self.info = self.eng.dedupe_part_plan(first_bad_global)
        return self.info

    def emit(self):
        out = self.eng.alloc_out(self.info.out_bytes)
        if self.info.out_bytes:
            self.eng.emit(out)
            self.eng.sync()
        return out[: self.info.out_bytes]


def _dedupe_failure(info):
    e = info.error
    return ((e.record, 0, 0), (e.code, e.stage, e.record, e.aux)) if e.code else None


def dedupe_in_parts(workers, rounds, check_inverse, first_record=0):
    """dedupe_sharded without ranks: one process, one worker (one context) per part on the same GPU, the parts taken in turn. rounds: a
    list of rounds, each a list with one device batch (uint8 tensor, bytes) per part; the records count on from first_record, part by
    part, round by round. Returns {"error": None or the failure one process reports ({"code", "stage", "record", "aux"}), "out": uint8
    tensor -- the parts' outputs in part order, round by round: everything in front of the failing record --, "total": its bytes,
    "records": records read, "exchanged": bytes that would have travelled between the parts}."""
    import torch

    k = len(workers)
    for w in workers:
        w.reset()
    outs, base, error, exchanged = [], first_record, None, 0
    for rnd in rounds:
        if len(rnd) != k:
            raise ValueError("a round has one batch per part")
        sent = []
        for w, batch in zip(workers, rnd):
            entries, counts, n_rec = w.keys(batch, check_inverse, base, k)
            sent.append((entries, [0] + [sum(counts[: p + 1]) for p in range(k)]))
            base += n_rec
        answers = [[None] * k for _ in range(k)]  # [source][owner]
        for p, w in enumerate(workers):
            segs = [e[at[p]: at[p + 1]] for e, at in sent]
            v, a = w.decide(torch.cat(segs), check_inverse), 0
            for s, seg in enumerate(segs):
                answers[s][p] = v[a: a + seg.shape[0]]
                a += seg.shape[0]
                if s != p:
                    exchanged += seg.shape[0] * (DEDUPE_ENTRY_BYTES + DEDUPE_VERDICT_BYTES)
        bads = [w.verdicts(torch.cat(answers[s])) for s, w in enumerate(workers)]
        first_bad = min([b for b in bads if b >= 0], default=-1)
        failures = []
        for w in workers:
            failures.append(_dedupe_failure(w.plan(first_bad)))
            outs.append(w.emit())
        if first_bad >= 0:
            error = least_failure([f for f in failures if f])
            break
    out = torch.cat(outs) if outs else torch.zeros(0, dtype=torch.uint8)
    return {"error": error, "out": out, "total": int(out.numel()), "records": base - first_record, "exchanged": exchanged}


def dedupe_sharded(worker, dist, rank, world, rounds, check_inverse, first_record=0, comm_device="cpu", write=None, writer=0):
    """`paffy dedupe [-a]` over an input spread over the ranks: this rank holds `rounds`, one device batch (uint8 tensor, bytes) per round
    -- every rank the same number of rounds, an empty batch where it has nothing --, and within a round the ranks' batches follow each
    other in rank order. One rank runs the same code with world = 1 and dist = None. No text is exchanged: 33 bytes per record.
    Returns {"error": None or the failure one process reports, the same on every rank, "total": bytes of the whole output (everything in
    front of a failing record), "sizes": bytes per (round, rank), "local": {round * world + rank: uint8 tensor} this rank's outputs};
    with `write` the outputs travel to rank `writer`, which calls write(index, tensor) in output order (gather_to_writer)."""
    import torch

    worker.reset()
    dev = getattr(getattr(worker, "eng", None), "device", "cpu")
    local, base, error, none = {}, first_record, None, (1 << 63) - 1
    for r, batch in enumerate(rounds):
        n_mine = worker.count_records(batch)
        shares = torch.tensor([n_mine], dtype=torch.int64, device=comm_device)
        if dist is not None:
            everyone = torch.zeros(world, dtype=torch.int64, device=comm_device)
            dist.all_gather_into_tensor(everyone, shares)
            shares = everyone
        shares = [int(x) for x in shares.tolist()]
        entries, send_counts, n_rec = worker.keys(batch, check_inverse, base + sum(shares[:rank]), world)
        if n_rec != n_mine:
            raise RuntimeError(f"dedupe_sharded: {n_rec} records in a batch of {n_mine} lines")
        base += sum(shares)
        if world == 1:
            back = worker.decide(entries, check_inverse)
        else:
            sent = torch.tensor(send_counts, dtype=torch.int64, device=comm_device)
            got = torch.zeros_like(sent)
            dist.all_to_all_single(got, sent)  # 8 bytes per peer
            recv_counts = [int(x) for x in got.tolist()]
            mine = torch.empty(4 * sum(recv_counts), dtype=torch.int64, device=comm_device)
            _pairwise_exchange(dist, rank, world, _comm(entries.reshape(-1), comm_device), [4 * c for c in send_counts], mine, [4 * c for c in recv_counts], EXCHANGE_CHUNK // 8)
            v = worker.decide(mine.reshape(-1, 4).to(dev), check_inverse)
            back = torch.empty(sum(send_counts), dtype=torch.uint8, device=comm_device)
            _pairwise_exchange(dist, rank, world, _comm(v, comm_device), recv_counts, back, send_counts, EXCHANGE_CHUNK)
        bad = worker.verdicts(back.to(dev))
        first = torch.tensor([bad if bad >= 0 else none], dtype=torch.int64, device=comm_device)
        if dist is not None:
            dist.all_reduce(first, op=dist.ReduceOp.MIN)
        first_bad = int(first.item())
        first_bad = -1 if first_bad == none else first_bad
        info = worker.plan(first_bad)
        local[r * world + rank] = worker.emit()
        if first_bad >= 0:
            error = first_failure(dist, _dedupe_failure(info), comm_device)
            break
    n_batches = len(rounds) * world
    sizes = {b: int(t.numel()) for b, t in local.items()}
    sizes = gather_batch_sizes(dist, sizes, n_batches, comm_device) if dist is not None else [sizes.get(b, 0) for b in range(n_batches)]
    if write is not None:
        if dist is None:
            for b in sorted(local):
                if sizes[b]:
                    write(b, local[b])
        else:
            gather_to_writer(dist, rank, world, {b: _comm(t, comm_device) for b, t in local.items()}, sizes, write, comm_device, writer)
    return {"error": error, "total": sum(sizes), "sizes": sizes, "local": local}


# ---- `paffy view` behind PAFFY_GPUS=N (host/paffy_launch.c, run_stream with the view totals) ----
def stream_cuts(data, n):
    """The launcher's cut of a stream command's input: n contiguous byte ranges, range r from the first line end at or after
    len(data) // n * r (never in front of the cut before it). Returns n + 1 offsets."""
    size = len(data)
    cuts = [0]
    for r in range(1, n):
        pos = max(size // n * r, cuts[-1])
        nl = data.find(b"\n", pos)
        cuts.append(size if nl < 0 else nl + 1)
    cuts.append(size)
    return cuts


def view_in_parts(data, seqs, n, text=1, range_bytes=128 << 20, chunk_bytes=None, engine=None):
    """`PAFFY_GPUS=n paffy view` without processes: the launcher's cut of `data` (stream_cuts), the parts taken in turn on one engine --
    each through a stream in view mode of its own, as a worker would, in chunks of whole lines of at most chunk_bytes (default: a part
    is one chunk) --, their texts put together in part order and their sums added up, as the launcher adds up the workers' sums files.
    A failing part ends the run: the text of the parts before it and its own stays. seqs: {name: bases}; text: 0 sums only, 1 stats
    lines, 2 lines and base-level rows. Returns {"text", "sums", "records", "error": None or (part, the failure Engine.view_stream
    reports, its record counted from the part's first record), "parts": records per part}."""
    from . import engine as E

    eng = engine or E.Engine()
    try:
        if text == 2:
            eng.keep_raw_sequences(True)
        eng.stats_only(text != 2)
        eng.set_sequences(seqs)
        cuts = stream_cuts(data, n)
        texts, sums, records, error, parts = [], [0] * 6, 0, None, []
        for r in range(n):
            part = data[cuts[r]:cuts[r + 1]]
            chunks = [part] if part else []
            if chunk_bytes and part:
                chunks, lines, cur = [], part.splitlines(keepends=True), b""
                for ln in lines:
                    if cur and len(cur) + len(ln) > chunk_bytes:
                        chunks.append(cur)
                        cur = b""
                    cur += ln
                if cur:
                    chunks.append(cur)
            got = eng.view_stream(chunks, text=text, range_bytes=range_bytes)
            texts.append(got["text"])
            if got["error"]:
                error = (r, got["error"])
                break
            sums = [a + b for a, b in zip(sums, got["sums"])]
            records += got["records"]
            parts.append(got["records"])
        return {"text": b"".join(texts), "sums": sums, "records": records, "error": error, "parts": parts}
    finally:
        if engine is None:
            eng.close()

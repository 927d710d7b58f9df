/*
 * bed_parts_kernel.h -- `paffy to_bed` sharded by sequence (include/paffy_hip.h, "to_bed in parts"): the device side of the partition
 * by the names of BOTH sides of a record and of the block keys the parts exchange. Included by paffy_hip.hip behind the line copy of the
 * query-name partition (copy_line), whose layout of the send buffer it shares.
 *
 * With -n a record bumps the counters of its query sequence and, as the inverted record would, those of its target sequence
 * (impl/paf_to_bed.c:170-177). The two sequences may have different owners, so a record is up to two ITEMS: item r (the query side of
 * record r) goes to owner(query name) and item n + r (its target side) to owner(target name) when that is another part. Every copy
 * carries a side mask: bit 0 = count the query side, bit 1 = count the target side; one copy with mask 3 where the owners coincide.
 */
#ifndef PAFFY_BED_PARTS_KERNEL_H_
#define PAFFY_BED_PARTS_KERNEL_H_

/* a line has a target name when its sixth token was read (k_header stops at the first token the reference aborts on) */
__device__ __forceinline__ bool side_has_target(const RecMeta &m) { return m.tname_len > 0; }

/* names of both sides: item r = the query name of line r, item n + r = its target name; a line without one mentions its query name
   again, with no bytes */
__global__ __launch_bounds__(PAFFY_NT) void k_side_hash(const uint8_t *in, const RecMeta *meta, const uint32_t *sep_pos, const uint32_t *nl_idx, uint32_t n, uint64_t *hash,
                                                         uint64_t *line_len, uint32_t *idx) {
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n) return;
    const RecMeta &m = meta[r];
    const uint32_t start = r == 0 ? 0u : sep_pos[nl_idx[r - 1]] + 1u, end = sep_pos[nl_idx[r]];
    const uint64_t len = (uint64_t)(end - start) + 1u; /* with its newline (a last line without one gets one) */
    const uint64_t hq = cov_name_hash(in, m.qname_off, m.qname_len);
    const bool has_t = side_has_target(m);
    hash[r] = hq;
    line_len[r] = len;
    idx[r] = r;
    hash[n + r] = has_t ? cov_name_hash(in, m.tname_off, m.tname_len) : hq;
    line_len[n + r] = has_t ? len : 0u;
    idx[n + r] = n + r;
}

__device__ __forceinline__ uint32_t side_owner(uint64_t h, const uint64_t *tab_hash, const uint32_t *tab_owner, uint32_t n_tab, uint32_t n_parts) {
    uint32_t lo = 0, hi = n_tab; /* first entry >= h */
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab_hash[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t owner = (lo < n_tab && tab_hash[lo] == h) ? tab_owner[lo] : (uint32_t)(h % n_parts); /* a name the table does not know */
    return owner < n_parts ? owner : n_parts - 1;
}
/* key of an item = part << 33 | record << 1 | side: sorted, the items of a part stand in input order. An item that is not sent (the
   target side of a record whose two names share an owner, or that has no target name, or any target side without -n) gets part n_parts
   and sorts behind every real part. mask[item] = the side mask its copy carries. */
__global__ __launch_bounds__(PAFFY_NT) void k_side_owner_keys(const uint8_t *in, const RecMeta *meta, uint32_t n, uint32_t with_target, const uint64_t *tab_hash,
                                                               const uint32_t *tab_owner, uint32_t n_tab, uint32_t n_parts, uint64_t *key, uint8_t *mask) {
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n) return;
    const RecMeta &m = meta[r];
    const uint32_t qo = side_owner(cov_name_hash(in, m.qname_off, m.qname_len), tab_hash, tab_owner, n_tab, n_parts);
    key[r] = ((uint64_t)qo << 33) | ((uint64_t)r << 1);
    if (!with_target) {
        mask[r] = 1;
        return;
    }
    const bool has_t = side_has_target(m);
    const uint32_t to = has_t ? side_owner(cov_name_hash(in, m.tname_off, m.tname_len), tab_hash, tab_owner, n_tab, n_parts) : qo;
    const bool apart = has_t && to != qo;
    mask[r] = has_t && !apart ? 3 : 1;
    key[n + r] = ((uint64_t)(apart ? to : n_parts) << 33) | ((uint64_t)r << 1) | 1u;
    mask[n + r] = 2;
}
__global__ __launch_bounds__(PAFFY_NT) void k_side_gather_len(const uint64_t *sorted_key, const uint64_t *line_len, uint32_t n_items, uint32_t n_parts, uint64_t *out) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n_items) out[i] = (uint32_t)(sorted_key[i] >> 33) == n_parts ? 0u : line_len[(uint32_t)(sorted_key[i] >> 1)];
    if (i == 0) out[n_items] = 0;
}
/* where every part (n_parts + 1 of them: the last holds what is not sent) starts in the sorted order; parts without items keep -1 */
__global__ __launch_bounds__(PAFFY_NT) void k_side_part_bounds(const uint64_t *sorted_key, const uint64_t *off, uint32_t n_items, int64_t *first, int64_t *start) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t p = (uint32_t)(sorted_key[i] >> 33);
    if (i == 0 || (uint32_t)(sorted_key[i - 1] >> 33) != p) {
        first[p] = i;
        start[p] = (int64_t)off[i];
    }
}
/* item blockIdx.x of the sorted order (the grid ends where the items that are not sent begin): its line to out + part_dst[p] + (its
   place inside the part), its global record index and its side mask to slot rec_dst[p] + (its rank inside the part) of rec_index / sides */
__global__ __launch_bounds__(PAFFY_NT) void k_split_sides_copy(const uint8_t *in, uint32_t in_len, const uint32_t *sep_pos, const uint32_t *nl_idx, const uint64_t *sorted_key,
                                                                const uint64_t *off, uint8_t *out, const int64_t *part_first, const int64_t *part_start, const int64_t *part_dst,
                                                                const int64_t *rec_dst, uint32_t n, const uint8_t *item_mask, int64_t *rec_index, uint8_t *sides, int64_t rec_base) {
    const uint64_t key = sorted_key[blockIdx.x];
    const uint32_t p = (uint32_t)(key >> 33), r = (uint32_t)(key >> 1), side = (uint32_t)key & 1u;
    const uint32_t start = r == 0 ? 0u : sep_pos[nl_idx[r - 1]] + 1u, end = sep_pos[nl_idx[r]];
    const uint64_t at = (uint64_t)part_dst[p] + (off[blockIdx.x] - (uint64_t)part_start[p]);
    const int64_t slot = rec_dst[p] + ((int64_t)blockIdx.x - part_first[p]);
    if (threadIdx.x == 0) {
        if (rec_index) rec_index[slot] = (int64_t)r + rec_base;
        sides[slot] = item_mask[side * n + r];
    }
    copy_line(in + start, (uint64_t)(end - start) + 1u, out + at, end >= in_len);
}

/* After a bed run: sequence blockIdx.x (order of first appearance = ascending counter base) -> the bytes and the number of its BED
   lines. The runs are in counter order and a run starts at every sequence's first counter, so its block is the runs from the one at
   contig_base[s] up to the one at contig_base[s + 1]. keys[3 s] (the entry it first appeared with) is the host's. */
__device__ __forceinline__ uint64_t bed_first_run_at(const uint64_t *starts, uint64_t n_runs, uint64_t g) {
    uint64_t lo = 0, hi = n_runs; /* first run that starts at or behind counter g */
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (starts[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(PAFFY_NT) void k_bed_seq_keys(const uint64_t *starts, uint64_t n_runs, const int64_t *len, const int64_t *off, int64_t total, const uint64_t *contig_base,
                                                            uint32_t n_seqs, const int64_t *first_entry, int64_t *keys) {
    __shared__ unsigned long long lines;
    const uint32_t s = blockIdx.x;
    if (threadIdx.x == 0) lines = 0;
    __syncthreads();
    const uint64_t i0 = bed_first_run_at(starts, n_runs, contig_base[s]);
    const uint64_t i1 = s + 1 < n_seqs ? bed_first_run_at(starts, n_runs, contig_base[s + 1]) : n_runs;
    unsigned long long mine = 0;
    for (uint64_t k = i0 + threadIdx.x; k < i1; k += PAFFY_NT) mine += len[k] > 0 ? 1u : 0u;
    if (mine) atomicAdd(&lines, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t b0 = i0 < n_runs ? off[i0] : total, b1 = i1 < n_runs ? off[i1] : total;
        keys[3 * s + 0] = first_entry[s];
        keys[3 * s + 1] = b1 - b0;
        keys[3 * s + 2] = (int64_t)lines;
    }
}

#endif

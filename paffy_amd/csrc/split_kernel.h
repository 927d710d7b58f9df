/*
 * paffy split_file on the device (impl/paf_split_file.c:142-170): the records of a batch grouped by output file. A group is a contig
 * name -- the query's under by_query, else the target's -- with the "small" bit of the record's own line (min_length > 0 and contig
 * length < min_length): a name seen with lengths on both sides of min_length is two groups, as in the reference's loop.
 *
 * Names are keyed by the salted 64-bit hash of coverage_kernel.h (cov_name_hash) with the small bit in bit 0; one stable radix sort of
 * (key, record) makes every group a run whose head is the group's first record of the batch, and every member's name is then CHECKED
 * byte for byte against its head's (the reference keys its tables by string equality): two names under one key -> the grouping again
 * with the next salt (split_host.h). The groups are numbered by their first record (a scan over the records of the "opens a group"
 * flag), sized by their run, and every record lands at start[group] + its place in the run: line_order, grouped, groups in order of
 * first appearance, input order inside a group. The line writer of tile / dedupe then writes the text in that order.
 *
 * A small_<k> file holds several contigs, and the reference writes their lines in input order. Which groups share a file is the host's
 * decision (split_host.h, once per group); where two groups of a batch do, the records are sorted once more, stably, by the file's
 * number within the batch (k_split_file_keys): one stretch of the output per file, input order inside it.
 * Included by split_host.h (paffy_hip.hip).
 */
#pragma once

/* one group of the batch, as the host fetches it */
struct SplitGroupDev {
    uint32_t name_off, name_len; /* slice of the input text: the contig name of the group's first record */
    int64_t contig_len;          /* contig length of the group's first record */
    uint32_t first_record, lines;
    uint32_t is_small, pad;
};

__device__ __forceinline__ void split_contig(const RecMeta &m, int by_query, uint32_t &off, uint32_t &len, int64_t &clen) {
    off = by_query ? m.qname_off : m.tname_off;
    len = by_query ? m.qname_len : m.tname_len;
    clen = by_query ? m.qlen : m.tlen;
}

/* narrow: the hash cut to two bits (the test knob of salt 0, split_host.h) */
__global__ __launch_bounds__(PAFFY_NT) void k_split_keys(const uint8_t *in, const RecMeta *meta, uint32_t n, int by_query, int64_t min_length, uint32_t salt, int narrow,
                                                       uint64_t *keys, uint32_t *idx) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n) return;
    uint32_t off, len;
    int64_t clen;
    split_contig(meta[i], by_query, off, len, clen);
    uint64_t h = cov_name_hash(in, off, len, salt);
    if (narrow) h &= 3u;
    const uint64_t small = (min_length > 0 && clen < min_length) ? 1u : 0u;
    keys[i] = (h << 1) | small;
    idx[i] = i;
}

/* position p of the sorted order: head[p] = p where a run of equal keys opens, else 0 (a running maximum gives every position its
   run's head); opens[record] = the record is the first of its run, opens[n] = 0 (the scan's total) */
__global__ __launch_bounds__(PAFFY_NT) void k_split_heads(const uint64_t *skeys, const uint32_t *order, uint32_t n, uint32_t *head, uint32_t *opens) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p > n) return;
    if (p == n) {
        opens[n] = 0;
        return;
    }
    const bool h = p == 0 || skeys[p] != skeys[p - 1];
    head[p] = h ? p : 0u;
    opens[order[p]] = h ? 1u : 0u;
}

/* every member of a run against the run's head: the name bytes (equal keys already share the small bit) */
__global__ __launch_bounds__(PAFFY_NT) void k_split_verify(const uint8_t *in, const RecMeta *meta, const uint32_t *order, const uint32_t *head_of, uint32_t n, int by_query,
                                                         uint32_t *collide) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p >= n) return;
    const uint32_t hp = head_of[p];
    if (hp == p) return;
    uint32_t ao, al, bo, bl;
    int64_t unused;
    split_contig(meta[order[p]], by_query, ao, al, unused);
    split_contig(meta[order[hp]], by_query, bo, bl, unused);
    bool same = al == bl;
    for (uint32_t k = 0; same && k < al; k++) same = in[ao + k] == in[bo + k];
    if (!same) *collide = 1u;
}

/* rank[record] = groups that open before the record (exclusive scan of opens): the last position of every run writes the run's size
   under its group's number; count[n_groups] = 0 (the scan's total) */
__global__ __launch_bounds__(PAFFY_NT) void k_split_counts(const uint64_t *skeys, const uint32_t *order, const uint32_t *head_of, const uint32_t *rank, uint32_t n,
                                                         uint32_t n_groups, uint32_t *count) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p >= n) return;
    if (p == 0) count[n_groups] = 0;
    if (p + 1 < n && skeys[p + 1] == skeys[p]) return;
    const uint32_t hp = head_of[p];
    count[rank[order[hp]]] = p - hp + 1;
}

/* the record at sorted position p is line start[group] + (its place in the run); group_of[record] = its group */
__global__ __launch_bounds__(PAFFY_NT) void k_split_place(const uint32_t *order, const uint32_t *head_of, const uint32_t *rank, const uint32_t *start, uint32_t n,
                                                        uint32_t *line_order, uint32_t *group_of) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p >= n) return;
    const uint32_t hp = head_of[p], g = rank[order[hp]], r = order[p];
    line_order[start[g] + (p - hp)] = r;
    group_of[r] = g;
}

/* the group table. name_len[g] (and a zero behind the last): sizes of the name blob */
__global__ __launch_bounds__(PAFFY_NT) void k_split_table(const RecMeta *meta, const uint32_t *line_order, const uint32_t *start, const uint32_t *count, uint32_t n_groups,
                                                        int by_query, int64_t min_length, SplitGroupDev *table, uint32_t *name_len) {
    const uint32_t g = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (g > n_groups) return;
    if (g == n_groups) {
        name_len[g] = 0;
        return;
    }
    const uint32_t s = start[g], cnt = count[g], r = line_order[s];
    SplitGroupDev t;
    split_contig(meta[r], by_query, t.name_off, t.name_len, t.contig_len);
    t.first_record = r;
    t.lines = cnt;
    t.is_small = (min_length > 0 && t.contig_len < min_length) ? 1u : 0u;
    t.pad = 0;
    table[g] = t;
    name_len[g] = t.name_len;
}

/* the names of the groups side by side (name_pos: exclusive scan of name_len): what the host keys its files by */
__global__ __launch_bounds__(PAFFY_NT) void k_split_names(const uint8_t *in, const SplitGroupDev *table, const uint32_t *name_pos, uint32_t n_groups, uint8_t *blob) {
    const uint32_t g = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (g >= n_groups) return;
    const SplitGroupDev t = table[g];
    uint8_t *dst = blob + name_pos[g];
    for (uint32_t k = 0; k < t.name_len; k++) dst[k] = in[t.name_off + k];
}

/* groups that share a file: the records keyed by their file's number within the batch (file_of[group], the host's), in input order */
__global__ __launch_bounds__(PAFFY_NT) void k_split_file_keys(const uint32_t *group_of, const uint32_t *file_of, uint32_t n, uint64_t *keys, uint32_t *idx) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n) return;
    keys[i] = file_of[group_of[i]];
    idx[i] = i;
}

/* first output byte of every stretch: line_off (n_lines + 1 entries) at the stretches' first lines (first[n_stretches] = n_lines) */
__global__ __launch_bounds__(PAFFY_NT) void k_split_offsets(const uint64_t *line_off, const uint32_t *first, uint32_t n, uint64_t *out) {
    const uint32_t s = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (s < n) out[s] = line_off[first[s]];
}

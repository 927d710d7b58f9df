/*
 * name_sort_kernel.h -- the FASTA names of an index in find_seq's order, sorted on the device.
 *
 * Key. Record r's key is its header up to the first NUL byte, so a key holds no NUL (a caller may give shorter keys: prefixes of that
 * one, as the upconvert interval table's names are). Keys order by unsigned bytes, then the shorter first,
 * then the record's input index.
 *
 * Rounds over runs. A run is a stretch of the current order whose members are equal in every byte before its depth d; it is named by the
 * place of its first member. The sort starts with one run over all records at depth 0 in input order. A round works on the members of the
 * unresolved runs only (they are kept compact: place, run, depth per member):
 *   k_ns_lcp    the run's depth advances by the minimum, over its adjacent pairs, of the pair's common prefix counted from d (the longest
 *               common prefix is an ultrametric, so adjacent pairs suffice whatever the order inside the run). The minimum is taken per
 *               wave and run first, so a run of 10^6 members costs one atomic per wave, not one per member.
 *   k_ns_word   each member's word: its 8 bytes at the new depth, big-endian, zero-filled past the key's end. Unsigned order of the words is
 *               memcmp plus shorter-first, because keys hold no NUL.
 *   (host)      a stable radix sort by word, then (when there is more than one run) a stable one by run: stability keeps the tie rule by
 *               input index without carrying the index in the key.
 *   k_ns_heads  the members go to their new places; a sub-run starts where the run or the word changes (there the key differs from the one
 *               before it: flag[place] = 1). A sub-run of one member is resolved, and so is one whose word ends in a zero byte (its keys end
 *               inside the word: they are equal). Every other sub-run goes on at depth d + 8.
 *   k_ns_compact the members that go on, side by side, under their sub-run's name.
 * One number per round goes back to the host: the members left. The rounds do not grow with the length of a shared prefix, only with the
 * number of distinct branch depths over 8.
 *
 * Tables. From the final order and the flags: k_ns_lens (key lengths, of the distinct keys or of all), k_ns_names (the name table of
 * fasta_host.h: blob, offsets, name_of, name_rec) and k_ns_store (the sequence store's names and SeqEntry table).
 */
#pragma once

#define NS_NT 256u
#define NS_NONE 0xffffffffu

struct NsScan {
    uint32_t head; /* inclusive maximum: the member that starts this member's sub-run */
    uint32_t cnt;  /* inclusive sum: members that go on */
};
struct NsScanOp {
    __host__ __device__ NsScan operator()(const NsScan &a, const NsScan &b) const {
        NsScan r;
        r.head = a.head > b.head ? a.head : b.head;
        r.cnt = a.cnt + b.cnt;
        return r;
    }
};

/* Minimum (MAX: maximum) of v over the lanes of the wave that hold the same key; lanes of one key are side by side. The first lane of
   every key (is_first) ends up with the result. Every lane of the wave calls this. */
template <bool MAX, typename T>
__device__ __forceinline__ T ns_seg_reduce(T v, uint32_t key, bool &is_first) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const T o = __shfl_down(v, d, 64);
        const uint32_t ok = __shfl_down(key, d, 64);
        if (lane + d < 64u && ok == key) v = MAX ? (o > v ? o : v) : (o < v ? o : v);
    }
    const uint32_t before = __shfl_up(key, 1, 64);
    is_first = lane == 0u || before != key;
    return v;
}

/* per record: the key length (saturated: a key of 4 GiB fails the blob's limit on the host), or key_len[r] where the caller has one (a
   prefix of the header that holds no NUL: upconvert_build_kernel.h); the start of the sort: input order, one run at depth 0. */
__global__ __launch_bounds__(NS_NT) void k_ns_init(const FaRec *recs, const int64_t *hdr_off, const uint8_t *blob, const uint32_t *key_len, uint32_t n,
                                                   uint32_t *klen, uint32_t *ord, uint32_t *flag, uint32_t *pos, uint32_t *run, uint32_t *depth,
                                                   uint32_t *run_skip) {
    const uint32_t r = blockIdx.x * NS_NT + threadIdx.x;
    if (r >= n) return;
    if (key_len) {
        klen[r] = key_len[r];
    } else {
        const int64_t hl = recs[r].hdr_len;
        const uint8_t *p = blob + hdr_off[r];
        int64_t k = 0;
        while (k < hl && p[k]) k++;
        klen[r] = k < (int64_t)NS_NONE ? (uint32_t)k : NS_NONE;
    }
    ord[r] = r;
    flag[r] = r == 0u ? 1u : 0u;
    pos[r] = r;
    run[r] = 0u;
    depth[r] = 0u;
    if (r == 0u) run_skip[0] = NS_NONE;
}

/* run_skip[run] = the shortest common prefix, from the run's depth on, of two members that are neighbours in the current order */
__global__ __launch_bounds__(NS_NT) void k_ns_lcp(uint32_t m, const uint32_t *pos, const uint32_t *run, const uint32_t *depth, const uint32_t *ord,
                                                  const uint32_t *klen, const int64_t *hdr_off, const uint8_t *blob, uint32_t *run_skip) {
    const uint32_t j = blockIdx.x * NS_NT + threadIdx.x;
    uint32_t my = NS_NONE, v = NS_NONE;
    if (j < m) {
        my = run[j];
        if (j > 0u && run[j - 1u] == my) {
            const uint32_t d = depth[j], a = ord[pos[j - 1u]], b = ord[pos[j]];
            const uint32_t la = klen[a], lb = klen[b];
            const uint32_t shorter = la < lb ? la : lb;
            const uint32_t lim = shorter > d ? shorter - d : 0u; /* every member of a run has its depth's bytes */
            const uint8_t *pa = blob + hdr_off[a] + d, *pb = blob + hdr_off[b] + d;
            uint32_t k = 0;
            while (k < lim && pa[k] == pb[k]) k++;
            v = k;
        }
    }
    bool first;
    v = ns_seg_reduce<false>(v, my, first);
    if (first && v != NS_NONE) atomicMin(&run_skip[my], v);
}

/* the member's word at its run's new depth; depth[j] becomes that depth */
__global__ __launch_bounds__(NS_NT) void k_ns_word(uint32_t m, const uint32_t *pos, const uint32_t *run, uint32_t *depth, const uint32_t *ord, const uint32_t *klen,
                                                   const int64_t *hdr_off, const uint8_t *blob, const uint32_t *run_skip, uint64_t *word, uint32_t *rec,
                                                   uint32_t *idx) {
    const uint32_t j = blockIdx.x * NS_NT + threadIdx.x;
    if (j >= m) return;
    const uint32_t r = ord[pos[j]];
    const uint32_t d = depth[j] + run_skip[run[j]];
    const uint32_t len = klen[r];
    const uint8_t *p = blob + hdr_off[r];
    uint64_t w = 0;
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
        const uint64_t at = (uint64_t)d + b;
        w = (w << 8) | (at < len ? (uint64_t)p[at] : 0ull);
    }
    depth[j] = d;
    word[j] = w;
    rec[j] = r;
    idx[j] = j;
}

/* the second sort's key: the run of the member that the first sort put at place i */
__global__ __launch_bounds__(NS_NT) void k_ns_runkey(uint32_t m, const uint32_t *run, const uint32_t *idx, uint32_t *key) {
    const uint32_t i = blockIdx.x * NS_NT + threadIdx.x;
    if (i < m) key[i] = run[idx[i]];
}

/* after the sort: idx[i] is the member that comes to active place i (the runs keep their stretches, so run[i] is its run too) */
__global__ __launch_bounds__(NS_NT) void k_ns_heads(uint32_t m, const uint32_t *pos, const uint32_t *run, const uint64_t *word, const uint32_t *idx,
                                                    const uint32_t *rec, uint32_t *ord, uint32_t *flag, NsScan *scan, uint32_t *run_skip) {
    const uint32_t i = blockIdx.x * NS_NT + threadIdx.x;
    if (i >= m) return;
    const uint32_t js = idx[i], my = run[i];
    const uint64_t w = word[js];
    const bool head = i == 0u || run[i - 1u] != my || word[idx[i - 1u]] != w;
    const bool next_head = i + 1u == m || run[i + 1u] != my || word[idx[i + 1u]] != w;
    const uint32_t place = pos[i];
    ord[place] = rec[js];
    if (head) flag[place] = 1u;
    const bool goes_on = !(head && next_head) && (w & 0xffull) != 0ull;
    NsScan s;
    s.head = head ? i : 0u;
    s.cnt = goes_on ? 1u : 0u;
    scan[i] = s;
    if (head && goes_on) run_skip[place] = NS_NONE;
}

/* in: what k_ns_heads wrote, out: its inclusive scan; depth: the depth of the round that ends */
__global__ __launch_bounds__(NS_NT) void k_ns_compact(uint32_t m, const NsScan *in, const NsScan *out, const uint32_t *pos, const uint32_t *depth, uint32_t *pos2,
                                                      uint32_t *run2, uint32_t *depth2) {
    const uint32_t i = blockIdx.x * NS_NT + threadIdx.x;
    if (i >= m || !in[i].cnt) return;
    const uint32_t dst = out[i].cnt - 1u;
    pos2[dst] = pos[i];
    run2[dst] = pos[out[i].head];
    depth2[dst] = depth[i] + 8u;
}

/* len[k] = the key length of place k (flag: of the places that start a distinct key only, else 0); len[n] = 0 */
__global__ __launch_bounds__(NS_NT) void k_ns_lens(uint32_t n, const uint32_t *ord, const uint32_t *klen, const uint32_t *flag, uint64_t *len) {
    const uint32_t k = blockIdx.x * NS_NT + threadIdx.x;
    if (k > n) return;
    len[k] = k < n && (!flag || flag[k]) ? (uint64_t)klen[ord[k]] : 0ull;
}

/* the name table: nidx[k] - 1 is the name of place k, off[k] where it starts in the blob (off[n]: the blob's size). name_rec is -1
   everywhere on entry; it gets the last record of the name whose whole header is the key (records of one name stand in input order). */
__global__ __launch_bounds__(NS_NT) void k_ns_names(uint32_t n, const uint32_t *ord, const uint32_t *klen, const int64_t *hdr_off, const uint8_t *blob,
                                                    const FaRec *recs, const uint32_t *flag, const uint32_t *nidx, const uint64_t *off, uint8_t *names,
                                                    uint32_t *name_off, int32_t *name_of, long long *name_rec) {
    const uint32_t k = blockIdx.x * NS_NT + threadIdx.x;
    uint32_t name = NS_NONE;
    long long whole = -1;
    if (k < n) {
        const uint32_t r = ord[k], len = klen[r];
        name = nidx[k] - 1u;
        name_of[r] = (int32_t)name;
        if ((int64_t)len == recs[r].hdr_len) whole = (long long)r;
        if (flag[k]) {
            const uint64_t o = off[k];
            name_off[name] = (uint32_t)o;
            const uint8_t *p = blob + hdr_off[r];
            for (uint32_t b = 0; b < len; b++) names[o + b] = p[b];
        }
        if (k + 1u == n) name_off[name + 1u] = (uint32_t)off[n];
    }
    bool first;
    whole = ns_seg_reduce<true>(whole, name, first);
    if (first && whole >= 0) atomicMax(&name_rec[name], whole);
}

/* the sequence store's tables: every key, duplicates included, at its place */
__global__ __launch_bounds__(NS_NT) void k_ns_store(uint32_t n, const uint32_t *ord, const uint32_t *klen, const int64_t *hdr_off, const uint8_t *blob,
                                                    const FaRec *recs, const uint64_t *off, uint8_t *names, uint32_t *name_off, SeqEntry *table) {
    const uint32_t k = blockIdx.x * NS_NT + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = ord[k], len = klen[r];
    const uint64_t o = off[k];
    name_off[k] = (uint32_t)o;
    if (k + 1u == n) name_off[n] = (uint32_t)off[n];
    const uint8_t *p = blob + hdr_off[r];
    for (uint32_t b = 0; b < len; b++) names[o + b] = p[b];
    SeqEntry e;
    e.off = (uint64_t)recs[r].seq_off;
    e.len = recs[r].seq_len;
    table[k] = e;
}

/* to_bed -q: the flag of every record's name */
__global__ __launch_bounds__(NS_NT) void k_ns_seen(uint32_t n, const int32_t *name_of, const uint8_t *seen, uint8_t *out) {
    const uint32_t r = blockIdx.x * NS_NT + threadIdx.x;
    if (r < n) out[r] = seen[name_of[r]];
}

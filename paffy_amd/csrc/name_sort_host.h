/*
 * name_sort_host.h -- host side of the device name sort (name_sort_kernel.h): the rounds, and the two tables made of the final order
 * (the name table of fasta_host.h, the sequence store's names of seqload_host.h). Included by fasta_host.h in front of FastaState.
 */
#pragma once

#include "name_sort_kernel.h"

struct NsDev {
    DevBuf klen, ord, flag, nidx; /* per record: key length; per place: the record, 1 where a distinct key starts, the inclusive sum of that */
    DevBuf len, off;              /* per place (+ 1): the bytes its key adds to a blob, where they start */
    /* a round's members: place, run, depth (two sets: a round compacts from one into the other), the words and the sorts' buffers */
    DevBuf pos[2], run[2], depth[2], skip, word, word_s, rec, idx, idx1, idx2, key, key_s, scan_in, scan_out, tmp;
    uint32_t n_names = 0;
};

/* HIP events around launches that are not ours (rocPRIM's sorts and scans), under a name of the profile */
struct NsSpan {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const char *name = nullptr;
};
static NsSpan ns_span_begin(paffy_hip_ctx *c, const char *name) {
    NsSpan s;
    if (!prof_wants(c, name)) return s;
    s.name = name;
    s.e0 = prof_event(c);
    s.e1 = prof_event(c);
    (void)hipEventRecord(s.e0, c->stream);
    return s;
}
static void ns_span_end(paffy_hip_ctx *c, const NsSpan &s) {
    if (!s.name) return;
    (void)hipEventRecord(s.e1, c->stream);
    c->pending.push_back({prof_slot(c, s.name), {s.e0, s.e1}});
}

template <typename K>
static int ns_sort_pairs(paffy_hip_ctx *c, NsDev &D, const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t n) {
    size_t bytes = 0;
    RPCHK(c, rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0, 8 * sizeof(K), c->stream));
    if (ensure(c, D.tmp, bytes + 16)) return PAFFY_E_HIP;
    const NsSpan s = ns_span_begin(c, "ns_radix_sort");
    RPCHK(c, rocprim::radix_sort_pairs(D.tmp.p, bytes, kin, kout, vin, vout, n, 0, 8 * sizeof(K), c->stream));
    ns_span_end(c, s);
    return 0;
}
template <typename T, typename Op>
static int ns_inclusive_scan(paffy_hip_ctx *c, NsDev &D, const T *in, T *out, size_t n, Op op) {
    size_t bytes = 0;
    RPCHK(c, rocprim::inclusive_scan(nullptr, bytes, in, out, n, op, c->stream));
    if (ensure(c, D.tmp, bytes + 16)) return PAFFY_E_HIP;
    const NsSpan s = ns_span_begin(c, "ns_scan");
    RPCHK(c, rocprim::inclusive_scan(D.tmp.p, bytes, in, out, n, op, c->stream));
    ns_span_end(c, s);
    return 0;
}
static int ns_exclusive_sum64(paffy_hip_ctx *c, NsDev &D, const uint64_t *in, uint64_t *out, size_t n) {
    size_t bytes = 0;
    RPCHK(c, rocprim::exclusive_scan(nullptr, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), c->stream));
    if (ensure(c, D.tmp, bytes + 16)) return PAFFY_E_HIP;
    const NsSpan s = ns_span_begin(c, "ns_scan");
    RPCHK(c, rocprim::exclusive_scan(D.tmp.p, bytes, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), c->stream));
    ns_span_end(c, s);
    return 0;
}

static dim3 ns_grid(uint64_t n) { return dim3((unsigned)((n + NS_NT - 1) / NS_NT)); }

/*
 * The order of n records' keys (n < 2^31): D.ord[k] is the record at place k, D.flag[k] = 1 where the key differs from the one before it,
 * D.nidx its inclusive sum, D.n_names the distinct keys. hdr_off / blob: the headers back to back as fa_index leaves them.
 * key_len (device, one per record; may be null): the keys' lengths where they are not the headers up to a NUL byte but prefixes of those.
 * The context's name_sort_stats tell what it took.
 */
static int name_sort(paffy_hip_ctx *c, NsDev &D, const FaRec *recs, const int64_t *hdr_off, const uint8_t *blob, int64_t n_rec,
                     const uint32_t *key_len = nullptr) {
    const uint32_t n = (uint32_t)n_rec;
    D.n_names = 0;
    c->name_sort_stats[0] = n_rec;
    c->name_sort_stats[1] = c->name_sort_stats[2] = c->name_sort_stats[3] = 0;
    if (n == 0) return 0;
    const size_t b4 = sizeof(uint32_t) * (size_t)n;
    if (ensure(c, D.klen, b4) || ensure(c, D.ord, b4) || ensure(c, D.flag, b4) || ensure(c, D.nidx, b4) || ensure(c, D.skip, b4) || ensure(c, D.rec, b4) ||
        ensure(c, D.idx, b4) || ensure(c, D.idx1, b4) || ensure(c, D.idx2, b4) || ensure(c, D.key, b4) || ensure(c, D.key_s, b4) || ensure(c, D.word, 2 * b4) ||
        ensure(c, D.word_s, 2 * b4) || ensure(c, D.scan_in, sizeof(NsScan) * (size_t)n) || ensure(c, D.scan_out, sizeof(NsScan) * (size_t)n))
        return PAFFY_E_HIP;
    for (int k = 0; k < 2; k++)
        if (ensure(c, D.pos[k], b4) || ensure(c, D.run[k], b4) || ensure(c, D.depth[k], b4)) return PAFFY_E_HIP;
    auto U32 = [](DevBuf &b) { return static_cast<uint32_t *>(b.p); };
    uint32_t *klen = U32(D.klen), *ord = U32(D.ord), *flag = U32(D.flag), *skip = U32(D.skip), *rec = U32(D.rec), *idx = U32(D.idx), *idx1 = U32(D.idx1),
             *idx2 = U32(D.idx2), *key = U32(D.key), *key_s = U32(D.key_s);
    uint64_t *word = static_cast<uint64_t *>(D.word.p), *word_s = static_cast<uint64_t *>(D.word_s.p);
    NsScan *scan_in = static_cast<NsScan *>(D.scan_in.p), *scan_out = static_cast<NsScan *>(D.scan_out.p);
    const dim3 block(NS_NT);
    LAUNCH(c, "k_ns_init", k_ns_init, ns_grid(n), block, 0, recs, hdr_off, blob, key_len, n, klen, ord, flag, U32(D.pos[0]), U32(D.run[0]), U32(D.depth[0]), skip);
    uint32_t m = n >= 2u ? n : 0u; /* a run of one record is resolved */
    int64_t rounds = 0;
    int cur = 0;
    while (m) {
        uint32_t *pos = U32(D.pos[cur]), *run = U32(D.run[cur]), *depth = U32(D.depth[cur]);
        LAUNCH(c, "k_ns_lcp", k_ns_lcp, ns_grid(m), block, 0, m, static_cast<const uint32_t *>(pos), static_cast<const uint32_t *>(run),
               static_cast<const uint32_t *>(depth), static_cast<const uint32_t *>(ord), static_cast<const uint32_t *>(klen), hdr_off, blob, skip);
        LAUNCH(c, "k_ns_word", k_ns_word, ns_grid(m), block, 0, m, static_cast<const uint32_t *>(pos), static_cast<const uint32_t *>(run), depth,
               static_cast<const uint32_t *>(ord), static_cast<const uint32_t *>(klen), hdr_off, blob, static_cast<const uint32_t *>(skip), word, rec, idx);
        if (ns_sort_pairs(c, D, static_cast<const uint64_t *>(word), word_s, static_cast<const uint32_t *>(idx), idx1, m)) return PAFFY_E_HIP;
        const uint32_t *sorted = idx1;
        if (rounds > 0) { /* the first round has one run */
            LAUNCH(c, "k_ns_runkey", k_ns_runkey, ns_grid(m), block, 0, m, static_cast<const uint32_t *>(run), static_cast<const uint32_t *>(idx1), key);
            if (ns_sort_pairs(c, D, static_cast<const uint32_t *>(key), key_s, static_cast<const uint32_t *>(idx1), idx2, m)) return PAFFY_E_HIP;
            sorted = idx2;
        }
        LAUNCH(c, "k_ns_heads", k_ns_heads, ns_grid(m), block, 0, m, static_cast<const uint32_t *>(pos), static_cast<const uint32_t *>(run),
               static_cast<const uint64_t *>(word), sorted, static_cast<const uint32_t *>(rec), ord, flag, scan_in, skip);
        if (ns_inclusive_scan(c, D, static_cast<const NsScan *>(scan_in), scan_out, m, NsScanOp())) return PAFFY_E_HIP;
        LAUNCH(c, "k_ns_compact", k_ns_compact, ns_grid(m), block, 0, m, static_cast<const NsScan *>(scan_in), static_cast<const NsScan *>(scan_out),
               static_cast<const uint32_t *>(pos), static_cast<const uint32_t *>(depth), U32(D.pos[cur ^ 1]), U32(D.run[cur ^ 1]), U32(D.depth[cur ^ 1]));
        NsScan last;
        HIPCHK(c, hipMemcpyAsync(&last, scan_out + (m - 1), sizeof(last), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        m = last.cnt;
        if (++rounds == 1) c->name_sort_stats[2] = m;
        cur ^= 1;
    }
    if (ns_inclusive_scan(c, D, static_cast<const uint32_t *>(flag), U32(D.nidx), n, rocprim::plus<uint32_t>())) return PAFFY_E_HIP;
    HIPCHK(c, hipMemcpyAsync(&D.n_names, U32(D.nidx) + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->name_sort_stats[1] = rounds;
    c->name_sort_stats[3] = D.n_names;
    return 0;
}

/* D.off[k] = where place k's key starts in a blob of the distinct keys (distinct) or of all keys, D.off[n] = *total, the blob's size */
static int name_sort_offsets(paffy_hip_ctx *c, NsDev &D, int64_t n_rec, bool distinct, uint64_t *total) {
    const uint32_t n = (uint32_t)n_rec;
    if (ensure(c, D.len, sizeof(uint64_t) * ((size_t)n + 1)) || ensure(c, D.off, sizeof(uint64_t) * ((size_t)n + 1))) return PAFFY_E_HIP;
    LAUNCH(c, "k_ns_lens", k_ns_lens, ns_grid((uint64_t)n + 1), dim3(NS_NT), 0, n, static_cast<const uint32_t *>(D.ord.p), static_cast<const uint32_t *>(D.klen.p),
           distinct ? static_cast<const uint32_t *>(D.flag.p) : nullptr, static_cast<uint64_t *>(D.len.p));
    if (ns_exclusive_sum64(c, D, static_cast<const uint64_t *>(D.len.p), static_cast<uint64_t *>(D.off.p), (size_t)n + 1)) return PAFFY_E_HIP;
    HIPCHK(c, hipMemcpyAsync(total, static_cast<const uint64_t *>(D.off.p) + n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

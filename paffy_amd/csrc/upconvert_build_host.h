/*
 * upconvert_build_host.h -- host side of the device build of upconvert's interval table (upconvert_build_kernel.h): the launches on the
 * context's stream, and the two calls that show the table whichever path built it. Included by seqload_host.h.
 */
#pragma once

#include "upconvert_build_kernel.h"

/*
 * c->up_table / c->up_names / c->n_intervals from the index F (headers only, on the device), as paffy_hip_set_intervals builds them from
 * the same headers and sequence lengths. Two numbers come to the host besides the name sort's: whether a header failed, and the blob's
 * size. Nothing of the table is published on a failure.
 */
static int upconvert_build(paffy_hip_ctx *c, FastaState &F) {
    const int64_t n_rec = F.n_rec;
    c->n_intervals = 0;
    c->up_blob_bytes = 0;
    c->up_on_device = true;
    c->up_rounds = 0;
    if (n_rec >= (1ll << 31)) return PAFFY_E_ARG;
    if (n_rec == 0) return 0;
    const uint32_t n = (uint32_t)n_rec;
    FastaState::Dev &D = F.dev;
    const FaRec *recs = static_cast<const FaRec *>(D.recs.p);
    const int64_t *hdr_off = static_cast<const int64_t *>(D.hdr_off.p);
    const uint8_t *blob = static_cast<const uint8_t *>(D.hdr_blob.p);
    const dim3 block(NS_NT);

    /* 1. decode: start, length, end, name length per record and the failure word, in one allocation */
    DevBuf work;
    HIPCHK(c, work.alloc((3 * sizeof(int64_t) + sizeof(uint32_t)) * (size_t)n + sizeof(uint32_t)));
    int64_t *start = static_cast<int64_t *>(work.p), *length = start + n, *end = length + n;
    uint32_t *name_len = reinterpret_cast<uint32_t *>(end + n), *failed = name_len + n;
    HIPCHK(c, hipMemsetAsync(failed, 0, sizeof(uint32_t), c->stream));
    LAUNCH(c, "k_up_decode", k_up_decode, ns_grid(n), block, 0, recs, hdr_off, blob, n, name_len, start, length, end, failed);
    uint32_t h_failed = 0;
    HIPCHK(c, hipMemcpyAsync(&h_failed, failed, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_failed) {
        if (c->profile) prof_collect(c);
        c->last_error = "upconvert: a FASTA header does not end in |length|start";
        return PAFFY_E_HEADER;
    }

    /* 2. by name */
    NsDev &S = D.ns;
    int rc = name_sort(c, S, recs, hdr_off, blob, n_rec, name_len);
    if (rc) return rc;
    c->up_rounds = c->name_sort_stats[1];

    /* 3. by start inside a name: the name sort's round buffers are free again */
    int64_t *key = static_cast<int64_t *>(S.word.p), *key_s = static_cast<int64_t *>(S.word_s.p);
    uint32_t *idx = static_cast<uint32_t *>(S.idx.p), *idx1 = static_cast<uint32_t *>(S.idx1.p), *place = static_cast<uint32_t *>(S.idx2.p);
    uint32_t *nkey = static_cast<uint32_t *>(S.key.p), *nkey_s = static_cast<uint32_t *>(S.key_s.p);
    const uint32_t *ord = static_cast<const uint32_t *>(S.ord.p);
    LAUNCH(c, "k_up_gather", k_up_gather, ns_grid(n), block, 0, n, ord, static_cast<const int64_t *>(start), key, idx);
    if (ns_sort_pairs(c, S, static_cast<const int64_t *>(key), key_s, static_cast<const uint32_t *>(idx), idx1, n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_ns_runkey", k_ns_runkey, ns_grid(n), block, 0, n, static_cast<const uint32_t *>(S.nidx.p), static_cast<const uint32_t *>(idx1), nkey);
    if (ns_sort_pairs(c, S, static_cast<const uint32_t *>(nkey), nkey_s, static_cast<const uint32_t *>(idx1), place, n)) return PAFFY_E_HIP;

    /* 4. layout and the table */
    if (ensure(c, S.len, sizeof(uint64_t) * ((size_t)n + 1)) || ensure(c, S.off, sizeof(uint64_t) * ((size_t)n + 1))) return PAFFY_E_HIP;
    uint64_t *len = static_cast<uint64_t *>(S.len.p), *off = static_cast<uint64_t *>(S.off.p);
    LAUNCH(c, "k_up_lens", k_up_lens, ns_grid((uint64_t)n + 1), block, 0, n, ord, static_cast<const uint32_t *>(place), static_cast<const uint32_t *>(name_len),
           static_cast<const int64_t *>(start), static_cast<const int64_t *>(length), len);
    if (ns_exclusive_sum64(c, S, static_cast<const uint64_t *>(len), off, (size_t)n + 1)) return PAFFY_E_HIP;
    uint64_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (total >= 0xffffffffull) { /* the slices are 32-bit */
        if (c->profile) prof_collect(c);
        return PAFFY_E_ARG;
    }
    if (ensure(c, c->up_table, sizeof(UpInterval) * (size_t)n) || ensure(c, c->up_names, (size_t)total + 16)) return PAFFY_E_HIP;
    LAUNCH(c, "k_up_table", k_up_table, ns_grid(n), block, 0, n, ord, static_cast<const uint32_t *>(place), static_cast<const uint32_t *>(name_len),
           static_cast<const int64_t *>(start), static_cast<const int64_t *>(length), static_cast<const int64_t *>(end), hdr_off, blob,
           static_cast<const uint64_t *>(off), static_cast<UpInterval *>(c->up_table.p), static_cast<uint8_t *>(c->up_names.p));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* the index and the scratch go when the caller returns */
    if (c->profile) prof_collect(c);
    c->up_blob_bytes = total;
    c->n_intervals = n;
    return 0;
}

extern "C" {

int paffy_hip_intervals_info(paffy_hip_ctx *c, int64_t out[4]) {
    if (!c || !out) return PAFFY_E_ARG;
    out[0] = c->n_intervals;
    out[1] = (int64_t)c->up_blob_bytes;
    out[2] = c->up_on_device ? 1 : 0;
    out[3] = c->up_rounds;
    return 0;
}

int paffy_hip_intervals_read(paffy_hip_ctx *c, int64_t cap, int64_t blob_cap, int64_t *nums, uint32_t *slices, void *blob) {
    if (!c) return PAFFY_E_ARG;
    const int64_t n = c->n_intervals;
    if (cap < n || blob_cap < (int64_t)c->up_blob_bytes) return PAFFY_E_CAPACITY;
    if (n && (nums || slices)) {
        std::vector<UpInterval> tab((size_t)n);
        HIPCHK(c, hipMemcpyAsync(tab.data(), c->up_table.p, sizeof(UpInterval) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int64_t k = 0; k < n; k++) {
            const UpInterval &t = tab[(size_t)k];
            if (nums) {
                nums[3 * k] = t.start;
                nums[3 * k + 1] = t.end;
                nums[3 * k + 2] = t.length;
            }
            if (slices) {
                slices[4 * k] = t.name_off;
                slices[4 * k + 1] = t.name_len;
                slices[4 * k + 2] = t.out_off;
                slices[4 * k + 3] = t.out_len;
            }
        }
    }
    if (n && blob && c->up_blob_bytes) {
        HIPCHK(c, hipMemcpyAsync(blob, c->up_names.p, (size_t)c->up_blob_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

} /* extern "C" */

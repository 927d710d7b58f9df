/*
 * seqload_host.h -- FASTA files in HBM to the sequence store (add_mismatches, view), the upconvert intervals (built by upconvert_build_host.h) and the to_bed -q name query
 * (include/paffy_hip.h). The text is indexed by fa_index (fasta_host.h) into a state of the loader's own, so a faffy index
 * of the context is left alone, and that state is freed before the call returns. Included at the end of paffy_hip.hip.
 */
#pragma once

#include "upconvert_build_host.h"

/* seq_blob holds the bases (input order) from n_bases on: upper case, complement and the raw copy in one pass */
static int seq_store_fill(paffy_hip_ctx *c, int64_t n_bases) {
    uint64_t n16 = ((uint64_t)n_bases + 64 + 15) / 16; /* the bases and the 64 bytes past them that seq_store_layout keeps too */
    if (n16 > c->seq_blob.cap / 16) n16 = c->seq_blob.cap / 16;
    if (ensure(c, c->seq_comp, n16 * 16)) return PAFFY_E_HIP;
    if (c->keep_raw && ensure(c, c->seq_raw, n16 * 16)) return PAFFY_E_HIP;
    if (n16) {
        const uint64_t blocks = (n16 + PAFFY_NT - 1) / PAFFY_NT;
        LAUNCH(c, "k_seq_store", k_seq_store, dim3((unsigned)(blocks < SL_GRID_MAX ? blocks : SL_GRID_MAX)), dim3(PAFFY_NT), 0,
               static_cast<uint8_t *>(c->seq_blob.p), static_cast<uint8_t *>(c->seq_comp.p), c->keep_raw ? static_cast<uint8_t *>(c->seq_raw.p) : nullptr,
               n16);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->profile) prof_collect(c);
    }
    return 0;
}

static int seq_store_from_index(paffy_hip_ctx *c, FastaState &F) {
    const int64_t n = F.n_rec;
    if (n >= (1ll << 31)) {
        c->last_error = "sequence store: more than 2^31 - 1 records";
        return PAFFY_E_ARG;
    }
    /* the store's tables as seq_store_layout lays them out over the compact bases: all n keys in find_seq's order (name_sort_kernel.h),
       records of one name in input order */
    c->n_seqs = 0;
    FastaState::Dev &D = F.dev;
    int rc = name_sort(c, D.ns, static_cast<const FaRec *>(D.recs.p), static_cast<const int64_t *>(D.hdr_off.p), static_cast<const uint8_t *>(D.hdr_blob.p), n);
    if (rc) return rc;
    uint64_t blob = 0;
    if ((rc = name_sort_offsets(c, D.ns, n, false, &blob))) return rc;
    if (blob >= 0xffffffffull) { /* seq_name_off is 32-bit */
        c->last_error = "sequence store: the names pass 4 GiB";
        return PAFFY_E_ARG;
    }
    if (ensure(c, c->seq_table, sizeof(SeqEntry) * (size_t)n) || ensure(c, c->seq_names, (size_t)blob + 16) ||
        ensure(c, c->seq_name_off, sizeof(uint32_t) * ((size_t)n + 1)))
        return PAFFY_E_HIP;
    LAUNCH(c, "k_ns_store", k_ns_store, ns_grid((uint64_t)n), dim3(NS_NT), 0, (uint32_t)n, static_cast<const uint32_t *>(D.ns.ord.p),
           static_cast<const uint32_t *>(D.ns.klen.p), static_cast<const int64_t *>(D.hdr_off.p), static_cast<const uint8_t *>(D.hdr_blob.p),
           static_cast<const FaRec *>(D.recs.p), static_cast<const uint64_t *>(D.ns.off.p), static_cast<uint8_t *>(c->seq_names.p),
           static_cast<uint32_t *>(c->seq_name_off.p), static_cast<SeqEntry *>(c->seq_table.p));
    std::swap(c->seq_blob, F.dev.bases); /* the compact bases are the store; the old store goes with F */
    return seq_store_fill(c, F.n_bases);
}

extern "C" {

int paffy_hip_set_sequences_fasta(paffy_hip_ctx *c, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, int64_t *n_records) {
    if (!c) return PAFFY_E_ARG;
    c->n_seqs = 0;
    FastaState F;
    int rc = fa_index(c, F, d_text, text_len, file_starts, n_files, true);
    if (!rc && F.n_rec > 0) rc = seq_store_from_index(c, F);
    fasta_release(F);
    if (rc) return rc;
    c->n_seqs = (int32_t)F.n_rec;
    if (n_records) *n_records = F.n_rec;
    return 0;
}

int paffy_hip_set_intervals_fasta(paffy_hip_ctx *c, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, int64_t *n_records) {
    if (!c) return PAFFY_E_ARG;
    c->n_intervals = 0;
    FastaState F;
    int rc = fa_index(c, F, d_text, text_len, file_starts, n_files, false, false); /* the headers stay on the device: the table is built there */
    if (rc) return rc;
    if (n_records) *n_records = F.n_rec;
    return upconvert_build(c, F);
}

int paffy_hip_fasta_index_headers(paffy_hip_ctx *c, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, int64_t *n_records) {
    if (!c) return PAFFY_E_ARG;
    FastaState &F = fasta_state(c);
    const int rc = fa_index(c, F, d_text, text_len, file_starts, n_files, false);
    if (rc) return rc;
    if (n_records) *n_records = F.n_rec;
    return 0;
}

int paffy_hip_fasta_seen(paffy_hip_ctx *c, const void *d_paf, int64_t paf_len, int with_target, uint8_t *seen) {
    if (!c) return PAFFY_E_ARG;
    if (!c->fasta || !c->fasta->indexed) return PAFFY_E_STATE;
    if (paf_len < 0 || (paf_len > 0 && !d_paf) || (reinterpret_cast<uintptr_t>(d_paf) & 15u)) return PAFFY_E_ARG;
    FastaState &F = *c->fasta;
    const int64_t n = F.n_rec;
    if (n == 0) return 0;
    if (!seen) return PAFFY_E_ARG;
    /* the distinct names, sorted as find_seq expects: the index's name table (fasta_host.h), built once per index */
    {
        const int rc = fa_name_table(c, F);
        if (rc) return rc;
    }
    const int32_t n_names = F.n_names;
    if (paf_len == 0) {
        memset(seen, 0, (size_t)n);
        return 0;
    }
    if (ensure(c, F.dev.seen, (size_t)n_names) || ensure(c, F.dev.seen_rec, (size_t)n)) return PAFFY_E_HIP;
    HIPCHK(c, hipMemsetAsync(F.dev.seen.p, 0, (size_t)n_names, c->stream));
    const int64_t blocks = (paf_len + FA_TILE - 1) / FA_TILE;
    LAUNCH(c, "k_fa_seen", k_fa_seen, dim3((unsigned)blocks), dim3(FA_NT), 0, static_cast<const uint8_t *>(d_paf), paf_len, with_target ? 1 : 0,
           static_cast<const uint8_t *>(F.dev.seen_names.p), static_cast<const uint32_t *>(F.dev.seen_off.p), n_names, static_cast<uint8_t *>(F.dev.seen.p));
    /* every record gets its name's flag on the device: n bytes come back */
    LAUNCH(c, "k_ns_seen", k_ns_seen, ns_grid((uint64_t)n), dim3(NS_NT), 0, (uint32_t)n, static_cast<const int32_t *>(F.dev.name_of.p),
           static_cast<const uint8_t *>(F.dev.seen.p), static_cast<uint8_t *>(F.dev.seen_rec.p));
    HIPCHK(c, hipMemcpyAsync(seen, F.dev.seen_rec.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->profile) prof_collect(c);
    return 0;
}

} /* extern "C" */

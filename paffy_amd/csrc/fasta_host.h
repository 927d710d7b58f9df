/*
 * fasta_host.h -- host side of `faffy chunk | extract | merge` (include/paffy_hip.h): the device FASTA index of
 * fasta_kernel.h, the item plans of chunk and merge (small host logic over the record table), the device plan of extract
 * (fasta_extract_kernel.h) and the emit.
 * Included by paffy_hip.hip behind the context.
 */
#pragma once

#include <climits>
#include <map>

#include "fasta_extract_kernel.h"
#include "name_sort_host.h"

struct FastaState {
    struct Dev { /* all of the state's device memory: fasta_release lets it go while the state lives */
        DevBuf starts, tiles, totals, recs, bases, hdr_off, hdr_blob, items, bad;
        DevBuf seen_names, seen_off, seen; /* the distinct names (fa_name_table) and paffy_hip_fasta_seen's flag per name */
        DevBuf name_rec;                   /* per distinct name: the record a BED line of that name means */
        DevBuf name_of, seen_rec;          /* per record: its name in the table (int32), paffy_hip_fasta_seen's flag */
        NsDev ns;                          /* the name sort (name_sort_host.h): ns.ord is the records in the names' order */
        /* the extract plan (fasta_extract_kernel.h): the host form's copy of the BED text, per slice, per line, per kept interval */
        DevBuf bed, bed_count, bed_first, bed_iv, bed_sorted, bed_keep, bed_pos, bed_lo, bed_hi, bed_rank, bed_clo, bed_chi, bed_max, bed_run, bed_scan,
            bed_stat, bed_tmp;
    } dev;
    const uint8_t *text = nullptr; /* the caller's text: emit reads the header names from it */
    int64_t text_len = 0, n_rec = 0, n_bases = 0;
    bool indexed = false, planned = false;
    bool with_bases = false; /* false: paffy_hip_fasta_index_headers, no compact base buffer */
    std::vector<FaRec> h_recs;
    std::vector<char> h_hdr;       /* all headers back to back */
    std::vector<int64_t> h_hdr_at; /* record r's header is h_hdr[h_hdr_at[r] .. h_hdr_at[r + 1]) */
    std::vector<FaItem> h_items;   /* chunk, merge: the items as the host plans them (extract writes dev.items itself) */
    int64_t n_items = 0;           /* items of the plan in dev.items */
    bool names_ready = false;      /* fa_name_table has run for this index */
    int32_t n_names = 0;
    std::vector<int64_t> file_ends; /* chunk: end of each output file in the output */
    int64_t out_bytes = 0;
};

static void fasta_release(FastaState &F) {
    F.dev = FastaState::Dev();
    F.names_ready = false;
}

static FastaState &fasta_state(paffy_hip_ctx *c) {
    if (!c->fasta) c->fasta.reset(new FastaState());
    return *c->fasta;
}

/* the header of record r as the host holds it */
static std::string fa_header(const FastaState &F, int64_t r) { return std::string(F.h_hdr.data() + F.h_hdr_at[r], (size_t)(F.h_hdr_at[r + 1] - F.h_hdr_at[r])); }

static void fa_fail(paffy_plan_info *info, int32_t code, int64_t record) {
    info->error.code = code;
    info->error.stage = -1;
    info->error.record = record;
    info->error.aux = 0;
}

/* an item that writes record r's bases [s, e) with the header line of `kind` */
static void fa_push(FastaState &F, int64_t r, int32_t kind, int32_t name_len, int64_t num1, int64_t num2, int64_t s, int64_t e, bool check) {
    FaItem it;
    it.out_off = F.out_bytes;
    it.name_off = F.h_recs[r].hdr_off;
    it.name_len = name_len;
    it.num1 = num1;
    it.num2 = num2;
    it.src_off = F.h_recs[r].seq_off + s;
    it.src_len = e - s;
    it.kind = kind;
    it.check = check ? 1 : 0;
    it.hdr_len = fa_header_len(kind, name_len, num1, num2);
    F.h_items.push_back(it);
    F.out_bytes += it.hdr_len + it.src_len + 1;
}

static int fa_plan_begin(paffy_hip_ctx *c, paffy_plan_info *info) {
    if (!c || !info || !c->fasta || !c->fasta->indexed || !c->fasta->with_bases) return PAFFY_E_STATE;
    FastaState &F = *c->fasta;
    memset(info, 0, sizeof(*info));
    F.planned = false;
    F.h_items.clear();
    F.n_items = 0;
    F.file_ends.clear();
    F.out_bytes = 0;
    return 0;
}

static int fa_plan_end(paffy_hip_ctx *c, paffy_plan_info *info) {
    FastaState &F = *c->fasta;
    info->n_records = F.n_rec;
    info->in_bytes = F.text_len;
    if (info->error.code) { /* nothing is written after an error of the plan */
        F.h_items.clear();
        F.file_ends.clear();
        F.out_bytes = 0;
    }
    F.n_items = (int64_t)F.h_items.size();
    info->n_rows = F.n_items;
    info->out_bytes = F.out_bytes;
    if (!F.h_items.empty()) {
        if (ensure(c, F.dev.items, sizeof(FaItem) * F.h_items.size())) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(F.dev.items.p, F.h_items.data(), sizeof(FaItem) * F.h_items.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* h_items may change with the next plan */
    }
    F.planned = true;
    return 0;
}

/* The index of the text into F (the context's state, or one of a loader's own). with_bases = false: the record table and the headers
   only; the compact base buffer is neither allocated nor written (upconvert and to_bed -q need the lengths alone). host_headers = false:
   the header blob stays on the device (dev.hdr_blob) and h_hdr is left empty, for a caller that reads the headers there. */
static int fa_index(paffy_hip_ctx *c, FastaState &F, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, bool with_bases,
                    bool host_headers = true) {
    if (!c || text_len < 0 || (text_len > 0 && !d_text) || (reinterpret_cast<uintptr_t>(d_text) & 15u)) return PAFFY_E_ARG;
    if (n_files < 0 || (n_files > 0 && !file_starts)) return PAFFY_E_ARG;
    std::vector<int64_t> starts(file_starts, file_starts + n_files);
    if (starts.empty()) starts.push_back(0);
    if (starts[0] != 0) return PAFFY_E_ARG;
    for (size_t k = 1; k < starts.size(); k++)
        if (starts[k] < starts[k - 1] || starts[k] > text_len) return PAFFY_E_ARG;
    F.indexed = F.planned = F.names_ready = false;
    F.with_bases = with_bases;
    F.text = static_cast<const uint8_t *>(d_text);
    F.text_len = text_len;
    F.n_rec = F.n_bases = 0;
    F.h_recs.clear();
    F.h_hdr.clear();
    F.h_hdr_at.assign(1, 0);
    const int32_t nf = (int32_t)starts.size();
    const uint32_t n_tiles = (uint32_t)((text_len + FA_TILE - 1) / FA_TILE);
    if (n_tiles) {
        if (ensure(c, F.dev.starts, sizeof(int64_t) * starts.size())) return PAFFY_E_HIP;
        if (ensure(c, F.dev.tiles, sizeof(FaTile) * n_tiles)) return PAFFY_E_HIP;
        if (ensure(c, F.dev.totals, sizeof(int64_t) * 2)) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(F.dev.starts.p, starts.data(), sizeof(int64_t) * starts.size(), hipMemcpyHostToDevice, c->stream));
        const int64_t *d_starts = static_cast<const int64_t *>(F.dev.starts.p);
        FaTile *tiles = static_cast<FaTile *>(F.dev.tiles.p);
        LAUNCH(c, "k_fa_count", k_fa_count, dim3(n_tiles), dim3(FA_NT), 0, F.text, text_len, d_starts, nf, tiles);
        LAUNCH(c, "k_fa_scan", k_fa_scan, dim3(1), dim3(FA_NT), 0, tiles, n_tiles, static_cast<int64_t *>(F.dev.totals.p));
        int64_t tot[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(tot, F.dev.totals.p, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        F.n_rec = tot[0];
        F.n_bases = tot[1];
        if (ensure(c, F.dev.recs, sizeof(FaRec) * (size_t)(F.n_rec + 1))) return PAFFY_E_HIP;
        if (with_bases && ensure(c, F.dev.bases, (size_t)F.n_bases + 64)) return PAFFY_E_HIP; /* k_fa_emit reads up to 32 bytes past the last base */
        LAUNCH(c, "k_fa_write", k_fa_write, dim3(n_tiles), dim3(FA_NT), 0, F.text, text_len, d_starts, nf, static_cast<const FaTile *>(F.dev.tiles.p),
               with_bases ? static_cast<uint8_t *>(F.dev.bases.p) : nullptr, static_cast<FaRec *>(F.dev.recs.p));
        if (F.n_rec) {
            LAUNCH(c, "k_fa_records", k_fa_records, dim3((unsigned)((F.n_rec + FA_NT - 1) / FA_NT)), dim3(FA_NT), 0, F.text, text_len, d_starts, nf,
                   static_cast<FaRec *>(F.dev.recs.p), F.n_rec, F.n_bases);
            F.h_recs.resize((size_t)F.n_rec);
            HIPCHK(c, hipMemcpyAsync(F.h_recs.data(), F.dev.recs.p, sizeof(FaRec) * (size_t)F.n_rec, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            F.h_hdr_at.resize((size_t)F.n_rec + 1);
            for (int64_t r = 0; r < F.n_rec; r++) F.h_hdr_at[r + 1] = F.h_hdr_at[r] + F.h_recs[r].hdr_len;
            const int64_t blob = F.h_hdr_at[F.n_rec];
            if (host_headers) F.h_hdr.resize((size_t)blob + 1);
            /* the name sort reads both, empty headers or not; 16 bytes past the blob are allocated as past the other texts */
            if (ensure(c, F.dev.hdr_off, sizeof(int64_t) * (size_t)F.n_rec)) return PAFFY_E_HIP;
            if (ensure(c, F.dev.hdr_blob, (size_t)blob + 16)) return PAFFY_E_HIP;
            HIPCHK(c, hipMemcpyAsync(F.dev.hdr_off.p, F.h_hdr_at.data(), sizeof(int64_t) * (size_t)F.n_rec, hipMemcpyHostToDevice, c->stream));
            if (blob) {
                LAUNCH(c, "k_fa_headers", k_fa_headers, dim3((unsigned)((F.n_rec + FA_NT / 64 - 1) / (FA_NT / 64))), dim3(FA_NT), 0, F.text,
                       static_cast<const FaRec *>(F.dev.recs.p), F.n_rec, static_cast<const int64_t *>(F.dev.hdr_off.p), static_cast<uint8_t *>(F.dev.hdr_blob.p));
                if (host_headers) HIPCHK(c, hipMemcpyAsync(F.h_hdr.data(), F.dev.hdr_blob.p, (size_t)blob, hipMemcpyDeviceToHost, c->stream));
            }
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->profile) prof_collect(c);
    }
    F.indexed = true;
    return 0;
}

/* record r's header as host/paffy_cmds.c's former fasta_read keyed it: a C string, so up to its first NUL byte */
static std::string fa_key(const FastaState &F, int64_t r) {
    const char *h = F.h_hdr.data() + F.h_hdr_at[r];
    return std::string(h, strnlen(h, (size_t)(F.h_hdr_at[r + 1] - F.h_hdr_at[r])));
}

/*
 * The table of the index's distinct names, once per index: dev.seen_names / dev.seen_off hold them sorted as find_seq expects (bytes,
 * then the shorter first), so a name's index is its strcmp rank; dev.name_of[r] is record r's name. dev.name_rec[k] is the record a BED
 * line named k means: the last record whose whole header is that name (a header with a NUL byte is keyed up to it for to_bed -q, but
 * no BED token equals it), -1 where there is none. Sorted and built on the device (name_sort_kernel.h); the host sees the number of
 * names and the blob's size.
 */
static int fa_name_table(paffy_hip_ctx *c, FastaState &F) {
    if (F.names_ready) return 0;
    const int64_t n = F.n_rec;
    if (n >= (1ll << 31) - 1) {
        c->last_error = "the FASTA index has more than 2^31 - 2 records: no name table";
        return PAFFY_E_UNSUPPORTED;
    }
    FastaState::Dev &D = F.dev;
    int rc = name_sort(c, D.ns, static_cast<const FaRec *>(D.recs.p), static_cast<const int64_t *>(D.hdr_off.p), static_cast<const uint8_t *>(D.hdr_blob.p), n);
    if (rc) return rc;
    uint64_t blob = 0;
    if (n && (rc = name_sort_offsets(c, D.ns, n, true, &blob))) return rc;
    if (blob >= 0xffffffffull) {
        c->last_error = "the FASTA names pass 4 GiB";
        return PAFFY_E_ARG;
    }
    F.n_names = (int32_t)D.ns.n_names;
    if (ensure(c, D.seen_names, (size_t)blob + 16) || ensure(c, D.seen_off, sizeof(uint32_t) * ((size_t)F.n_names + 1)) ||
        ensure(c, D.name_rec, sizeof(int64_t) * ((size_t)F.n_names + 1)) || ensure(c, D.name_of, sizeof(int32_t) * ((size_t)n + 1)))
        return PAFFY_E_HIP;
    if (n) {
        HIPCHK(c, hipMemsetAsync(D.name_rec.p, 0xff, sizeof(int64_t) * (size_t)F.n_names, c->stream));
        LAUNCH(c, "k_ns_names", k_ns_names, ns_grid((uint64_t)n), dim3(NS_NT), 0, (uint32_t)n, static_cast<const uint32_t *>(D.ns.ord.p),
               static_cast<const uint32_t *>(D.ns.klen.p), static_cast<const int64_t *>(D.hdr_off.p), static_cast<const uint8_t *>(D.hdr_blob.p),
               static_cast<const FaRec *>(D.recs.p), static_cast<const uint32_t *>(D.ns.flag.p), static_cast<const uint32_t *>(D.ns.nidx.p),
               static_cast<const uint64_t *>(D.ns.off.p), static_cast<uint8_t *>(D.seen_names.p), static_cast<uint32_t *>(D.seen_off.p),
               static_cast<int32_t *>(D.name_of.p), static_cast<long long *>(D.name_rec.p));
    } else {
        HIPCHK(c, hipMemsetAsync(D.seen_off.p, 0, sizeof(uint32_t), c->stream));
    }
    if (c->profile) prof_collect(c);
    F.names_ready = true;
    return 0;
}

template <typename T, typename Op>
static int fa_inclusive_scan(paffy_hip_ctx *c, FastaState &F, const T *in, T *out, size_t n, Op op) {
    size_t bytes = 0;
    RPCHK(c, rocprim::inclusive_scan(nullptr, bytes, in, out, n, op, c->stream));
    if (ensure(c, F.dev.bed_tmp, bytes + 16)) return PAFFY_E_HIP;
    RPCHK(c, rocprim::inclusive_scan(F.dev.bed_tmp.p, bytes, in, out, n, op, c->stream));
    return 0;
}
template <typename T>
static int fa_exclusive_sum(paffy_hip_ctx *c, FastaState &F, const T *in, T *out, size_t n) {
    size_t bytes = 0;
    RPCHK(c, rocprim::exclusive_scan(nullptr, bytes, in, out, (T)0, n, rocprim::plus<T>(), c->stream));
    if (ensure(c, F.dev.bed_tmp, bytes + 16)) return PAFFY_E_HIP;
    RPCHK(c, rocprim::exclusive_scan(F.dev.bed_tmp.p, bytes, in, out, (T)0, n, rocprim::plus<T>(), c->stream));
    return 0;
}
static int fa_fetch(paffy_hip_ctx *c, void *dst, const void *src, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/*
 * The extract plan over BED text in device memory (fasta_extract_kernel.h): line index, parse, sort, bounds, merge by prefix maximum,
 * items. The host sees four numbers on the way: the lines, the first failing line or interval, the kept intervals, the items with
 * their bytes. info->error is set as the reference fails; F.n_items / F.out_bytes and dev.items hold the plan.
 */
static int fa_extract_plan(paffy_hip_ctx *c, FastaState &F, const uint8_t *bed, int64_t bed_len, int64_t flank, int64_t min_size, int skip_missing,
                           paffy_plan_info *info) {
    if (bed_len == 0) return 0;
    int rc = fa_name_table(c, F);
    if (rc) return rc;
    FastaState::Dev &D = F.dev;
    const dim3 block(FA_NT);
    auto grid_of = [](int64_t n) { return dim3((unsigned)((n + FA_NT - 1) / FA_NT)); };
    const uint8_t *names = static_cast<const uint8_t *>(D.seen_names.p);
    const uint32_t *name_off = static_cast<const uint32_t *>(D.seen_off.p);
    const int64_t *name_rec = static_cast<const int64_t *>(D.name_rec.p);
    const FaRec *recs = static_cast<const FaRec *>(D.recs.p);

    /* 1. lines */
    const int64_t n_slices = (bed_len + FA_PER - 1) / FA_PER;
    if (n_slices + FA_NT > (int64_t)0xffffffffll * FA_NT / 2) { /* the grid */
        c->last_error = "faffy extract: a BED text of this size is not supported";
        return PAFFY_E_UNSUPPORTED;
    }
    if (ensure(c, D.bed_count, sizeof(int64_t) * (size_t)(n_slices + 1)) || ensure(c, D.bed_first, sizeof(int64_t) * (size_t)(n_slices + 1)) ||
        ensure(c, D.bed_stat, sizeof(BedStat)))
        return PAFFY_E_HIP;
    int64_t *count = static_cast<int64_t *>(D.bed_count.p), *first = static_cast<int64_t *>(D.bed_first.p);
    BedStat *stat = static_cast<BedStat *>(D.bed_stat.p);
    HIPCHK(c, hipMemsetAsync(count + n_slices, 0, sizeof(int64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(stat, 0xff, sizeof(BedStat), c->stream));
    LAUNCH(c, "k_bed_index", k_bed_index, grid_of(n_slices), block, 0, bed, bed_len, count);
    if (fa_exclusive_sum(c, F, static_cast<const int64_t *>(count), first, (size_t)n_slices + 1)) return PAFFY_E_HIP;
    int64_t n = 0;
    if (fa_fetch(c, &n, first + n_slices, sizeof(n))) return PAFFY_E_HIP;
    if (n > (int64_t)INT32_MAX) {
        c->last_error = "faffy extract: more than 2^31 - 1 BED lines";
        return PAFFY_E_UNSUPPORTED;
    }

    /* 2. parse, 3. sort */
    if (ensure(c, D.bed_iv, sizeof(BedIv) * (size_t)n) || ensure(c, D.bed_sorted, sizeof(BedIv) * (size_t)n)) return PAFFY_E_HIP;
    BedIv *iv = static_cast<BedIv *>(D.bed_iv.p), *sorted = static_cast<BedIv *>(D.bed_sorted.p);
    LAUNCH(c, "k_bed_parse", k_bed_parse, grid_of(n_slices), block, 0, bed, bed_len, static_cast<const int64_t *>(first), names, name_off, name_rec, F.n_names,
           skip_missing ? 1 : 0, iv, stat);
    {
        size_t bytes = 0;
        RPCHK(c, rocprim::merge_sort(nullptr, bytes, iv, sorted, (size_t)n, BedIvLess(), c->stream));
        if (ensure(c, D.bed_tmp, bytes + 16)) return PAFFY_E_HIP;
        RPCHK(c, rocprim::merge_sort(D.bed_tmp.p, bytes, iv, sorted, (size_t)n, BedIvLess(), c->stream));
    }

    /* 4. bounds, the kept intervals side by side */
    if (ensure(c, D.bed_keep, sizeof(uint32_t) * (size_t)(n + 1)) || ensure(c, D.bed_pos, sizeof(uint32_t) * (size_t)(n + 1)) ||
        ensure(c, D.bed_lo, sizeof(int64_t) * (size_t)n) || ensure(c, D.bed_hi, sizeof(int64_t) * (size_t)n))
        return PAFFY_E_HIP;
    uint32_t *keep = static_cast<uint32_t *>(D.bed_keep.p), *pos = static_cast<uint32_t *>(D.bed_pos.p);
    int64_t *lo = static_cast<int64_t *>(D.bed_lo.p), *hi = static_cast<int64_t *>(D.bed_hi.p);
    LAUNCH(c, "k_bed_bounds", k_bed_bounds, grid_of(n + 1), block, 0, static_cast<const BedIv *>(sorted), n, name_rec, recs, F.n_names, flank, min_size, keep,
           lo, hi, stat);
    if (fa_exclusive_sum(c, F, static_cast<const uint32_t *>(keep), pos, (size_t)n + 1)) return PAFFY_E_HIP;
    BedStat h_stat;
    uint32_t m = 0;
    HIPCHK(c, hipMemcpyAsync(&h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, c->stream));
    if (fa_fetch(c, &m, pos + n, sizeof(m))) return PAFFY_E_HIP;
    if (h_stat.parse_err != ~0ull) { /* the first failing line decides, whichever kind it is */
        fa_fail(info, (h_stat.parse_err & 1ull) == BED_KIND_MISSING ? PAFFY_ERR_FAFFY_MISSING_SEQ : PAFFY_ERR_FAFFY_ASSERT, (int64_t)(h_stat.parse_err >> 1));
        return 0;
    }
    if (h_stat.bounds_err != ~0ull) {
        fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, (int64_t)h_stat.bounds_err);
        return 0;
    }
    if (m == 0) return 0;
    if (ensure(c, D.bed_rank, sizeof(uint32_t) * (size_t)m) || ensure(c, D.bed_clo, sizeof(int64_t) * (size_t)m) || ensure(c, D.bed_chi, sizeof(int64_t) * (size_t)m) ||
        ensure(c, D.bed_max, sizeof(int64_t) * (size_t)m) || ensure(c, D.bed_run, sizeof(BedRun) * (size_t)m) || ensure(c, D.bed_scan, sizeof(BedRun) * (size_t)m))
        return PAFFY_E_HIP;
    uint32_t *c_rank = static_cast<uint32_t *>(D.bed_rank.p);
    int64_t *c_lo = static_cast<int64_t *>(D.bed_clo.p), *c_hi = static_cast<int64_t *>(D.bed_chi.p), *c_max = static_cast<int64_t *>(D.bed_max.p);
    BedRun *run = static_cast<BedRun *>(D.bed_run.p), *scan = static_cast<BedRun *>(D.bed_scan.p);
    LAUNCH(c, "k_bed_compact", k_bed_compact, grid_of(n), block, 0, static_cast<const BedIv *>(sorted), n, static_cast<const uint32_t *>(keep),
           static_cast<const uint32_t *>(pos), static_cast<const int64_t *>(lo), static_cast<const int64_t *>(hi), c_rank, c_lo, c_hi);

    /* 5. the merge: prefix maximum of the ends by name, then items, bytes and item starts in one scan */
    {
        size_t bytes = 0;
        const uint32_t *kin = c_rank;
        const int64_t *vin = c_hi;
        RPCHK(c, rocprim::inclusive_scan_by_key(nullptr, bytes, kin, vin, c_max, (size_t)m, BedMax64(), rocprim::equal_to<uint32_t>(), c->stream));
        if (ensure(c, D.bed_tmp, bytes + 16)) return PAFFY_E_HIP;
        RPCHK(c, rocprim::inclusive_scan_by_key(D.bed_tmp.p, bytes, kin, vin, c_max, (size_t)m, BedMax64(), rocprim::equal_to<uint32_t>(), c->stream));
    }
    LAUNCH(c, "k_bed_heads", k_bed_heads, grid_of(m), block, 0, static_cast<const uint32_t *>(c_rank), static_cast<const int64_t *>(c_lo),
           static_cast<const int64_t *>(c_max), (int64_t)m, name_rec, recs, run);
    if (fa_inclusive_scan(c, F, static_cast<const BedRun *>(run), scan, (size_t)m, BedRunPlus())) return PAFFY_E_HIP;
    BedRun total;
    if (fa_fetch(c, &total, scan + (m - 1), sizeof(total))) return PAFFY_E_HIP;

    /* 6. items */
    if (ensure(c, D.items, sizeof(FaItem) * (size_t)total.items)) return PAFFY_E_HIP;
    LAUNCH(c, "k_bed_items", k_bed_items, grid_of(m), block, 0, static_cast<const uint32_t *>(c_rank), static_cast<const int64_t *>(c_lo),
           static_cast<const int64_t *>(c_max), (int64_t)m, name_rec, recs, static_cast<const BedRun *>(scan), static_cast<FaItem *>(D.items.p));
    F.n_items = (int64_t)total.items;
    F.out_bytes = total.bytes;
    return 0;
}

/* the end of a plan whose items are in dev.items already */
static int fa_plan_end_device(paffy_hip_ctx *c, paffy_plan_info *info) {
    FastaState &F = *c->fasta;
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* the caller may free the BED text */
    if (c->profile) prof_collect(c);
    info->n_records = F.n_rec;
    info->in_bytes = F.text_len;
    if (info->error.code) F.n_items = F.out_bytes = 0; /* nothing is written after an error of the plan */
    info->n_rows = F.n_items;
    info->out_bytes = F.out_bytes;
    F.planned = true;
    return 0;
}

extern "C" {

int paffy_hip_fasta_index(paffy_hip_ctx *c, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, int64_t *n_records,
                          int64_t *n_bases) {
    if (!c) return PAFFY_E_ARG;
    FastaState &F = fasta_state(c);
    const int rc = fa_index(c, F, d_text, text_len, file_starts, n_files, true);
    if (rc) return rc;
    if (n_records) *n_records = F.n_rec;
    if (n_bases) *n_bases = F.n_bases;
    return 0;
}

int64_t paffy_hip_fasta_records(paffy_hip_ctx *c, int64_t first, int64_t cap, paffy_fasta_record *recs) {
    if (!c || !c->fasta || !c->fasta->indexed || first < 0 || cap < 0 || (cap > 0 && !recs)) return PAFFY_E_ARG;
    const FastaState &F = *c->fasta;
    int64_t n = 0;
    for (int64_t r = first; r < F.n_rec && n < cap; r++, n++) {
        recs[n].hdr_off = F.h_recs[r].hdr_off;
        recs[n].hdr_len = F.h_recs[r].hdr_len;
        recs[n].seq_off = F.h_recs[r].seq_off;
        recs[n].seq_len = F.h_recs[r].seq_len;
    }
    return F.n_rec;
}

int paffy_hip_fasta_copy_bases(paffy_hip_ctx *c, int64_t first, int64_t n, void *d_dst) {
    if (!c || !c->fasta || !c->fasta->indexed || !c->fasta->with_bases || first < 0 || n < 0 || first + n > c->fasta->n_bases || (n > 0 && !d_dst))
        return PAFFY_E_ARG;
    if (n) HIPCHK(c, hipMemcpyAsync(d_dst, static_cast<const uint8_t *>(c->fasta->dev.bases.p) + first, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int paffy_hip_fasta_name_order(paffy_hip_ctx *c, int64_t cap, void *d_order, void *d_name_of, int64_t *n_names) {
    if (!c) return PAFFY_E_ARG;
    if (!c->fasta || !c->fasta->indexed) return PAFFY_E_STATE;
    FastaState &F = *c->fasta;
    if (cap < F.n_rec) return PAFFY_E_CAPACITY;
    const int rc = fa_name_table(c, F);
    if (rc) return rc;
    const size_t bytes = sizeof(int32_t) * (size_t)F.n_rec;
    if (bytes && d_order) HIPCHK(c, hipMemcpyAsync(d_order, F.dev.ns.ord.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    if (bytes && d_name_of) HIPCHK(c, hipMemcpyAsync(d_name_of, F.dev.name_of.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_names) *n_names = F.n_names;
    return 0;
}

int paffy_hip_name_sort_stats(paffy_hip_ctx *c, int64_t out[4]) {
    if (!c || !out) return PAFFY_E_ARG;
    for (int k = 0; k < 4; k++) out[k] = c->name_sort_stats[k];
    return 0;
}

int paffy_hip_faffy_chunk_plan(paffy_hip_ctx *c, int64_t chunk_size, int64_t overlap, paffy_plan_info *info) {
    int rc = fa_plan_begin(c, info);
    if (rc) return rc;
    FastaState &F = *c->fasta;
    int64_t co = 0;
    if (chunk_size > overlap && (chunk_size <= 0 || __builtin_add_overflow(chunk_size, overlap, &co) || co < 0)) return PAFFY_E_ARG;
    bool open = false;
    int64_t remaining = chunk_size;
    for (int64_t r = 0; r < F.n_rec && !info->error.code; r++) {
        if (!(chunk_size > overlap)) { /* impl/fasta_chunk.c:74, for every record */
            fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, r);
            break;
        }
        const int64_t len = F.h_recs[r].seq_len, nl = F.h_recs[r].hdr_len;
        for (int64_t i = 0; i < len; i += chunk_size) {
            if (!open) {
                open = true;
                remaining = chunk_size;
            }
            const int64_t j = len - i < co ? len : i + co;
            fa_push(F, r, 0, (int32_t)nl, len, i, i, j, true);
            remaining -= j - i;
            if (remaining <= 0) {
                open = false;
                F.file_ends.push_back(F.out_bytes);
            }
            if (len - i <= chunk_size) break; /* i + chunk_size would reach len (and cannot overflow) */
        }
    }
    if (open) F.file_ends.push_back(F.out_bytes);
    return fa_plan_end(c, info);
}

int64_t paffy_hip_faffy_chunk_files(paffy_hip_ctx *c, int64_t cap, int64_t *file_end) {
    if (!c || !c->fasta || !c->fasta->planned || cap < 0 || (cap > 0 && !file_end)) return PAFFY_E_ARG;
    const FastaState &F = *c->fasta;
    for (int64_t k = 0; k < (int64_t)F.file_ends.size() && k < cap; k++) file_end[k] = F.file_ends[k];
    return (int64_t)F.file_ends.size();
}

int paffy_hip_faffy_extract_plan_device(paffy_hip_ctx *c, const void *d_bed, int64_t bed_len, int64_t flank, int64_t min_size, int skip_missing,
                                        paffy_plan_info *info) {
    int rc = fa_plan_begin(c, info);
    if (rc) return rc;
    if (bed_len < 0 || (bed_len > 0 && (!d_bed || (reinterpret_cast<uintptr_t>(d_bed) & 15u)))) return PAFFY_E_ARG;
    rc = fa_extract_plan(c, *c->fasta, static_cast<const uint8_t *>(d_bed), bed_len, flank, min_size, skip_missing, info);
    if (rc) return rc;
    return fa_plan_end_device(c, info);
}

/* host text: one copy to the device, then the plan above */
int paffy_hip_faffy_extract_plan(paffy_hip_ctx *c, const char *bed, int64_t bed_len, int64_t flank, int64_t min_size, int skip_missing, paffy_plan_info *info) {
    int rc = fa_plan_begin(c, info);
    if (rc) return rc;
    if (bed_len < 0 || (bed_len > 0 && !bed)) return PAFFY_E_ARG;
    FastaState &F = *c->fasta;
    if (bed_len > 0) {
        if (ensure(c, F.dev.bed, (size_t)bed_len + 16)) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(F.dev.bed.p, bed, (size_t)bed_len, hipMemcpyHostToDevice, c->stream));
    }
    return paffy_hip_faffy_extract_plan_device(c, F.dev.bed.p, bed_len, flank, min_size, skip_missing, info);
}

int paffy_hip_faffy_merge_plan(paffy_hip_ctx *c, paffy_plan_info *info) {
    int rc = fa_plan_begin(c, info);
    if (rc) return rc;
    FastaState &F = *c->fasta;
    const int64_t n = F.n_rec;
    /* per record: the offset (atol of the last '|'-token), the length of the name that is written (the header less its last two
       '|'-tokens; -1: fewer than two tokens) */
    std::vector<int64_t> off((size_t)n), name_len((size_t)n);
    for (int64_t r = 0; r < n; r++) {
        const std::string h = fa_header(F, r);
        const size_t last = h.rfind('|');
        off[r] = (int64_t)atol(h.c_str() + (last == std::string::npos ? 0 : last + 1));
        if (last == std::string::npos) name_len[r] = -1;
        else if (last == 0) name_len[r] = 0;
        else {
            const size_t second = h.rfind('|', last - 1);
            name_len[r] = second == std::string::npos ? 0 : (int64_t)second;
        }
    }
    /* pending before record r+1 is (pc, L) = (off[r] + s[r], len[r] - s[r]), so pc + L = off[r] + len[r]: every split point
       sp(r, r+1) = (off[r] + len[r] + off[r+1]) / 2 depends on two neighbours only */
    auto split = [&](int64_t r) -> __int128 { return ((__int128)off[r] + F.h_recs[r].seq_len + off[r + 1]) / 2; };
    std::vector<int64_t> s((size_t)n, 0);
    for (int64_t r = 0; r < n; r++) {
        if (off[r] < 0) { /* impl/fasta_merge.c: assert(offset >= 0) */
            fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, r);
            return fa_plan_end(c, info);
        }
        if (off[r] == 0) {
            if (name_len[r] < 0) { /* stList_pop of an empty list */
                fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, r);
                return fa_plan_end(c, info);
            }
            continue;
        }
        /* no pending sequence, pc > off, a gap (pc + L < off), or a split point past the end of this record's sequence */
        if (r == 0 || (__int128)off[r - 1] + s[r - 1] > off[r] || (__int128)off[r - 1] + F.h_recs[r - 1].seq_len < off[r]) {
            fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, r);
            return fa_plan_end(c, info);
        }
        const __int128 sr = split(r - 1) - off[r];
        if (sr > F.h_recs[r].seq_len) {
            fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, r);
            return fa_plan_end(c, info);
        }
        s[r] = (int64_t)sr;
    }
    for (int64_t r = 0; r < n; r++) {
        const int64_t e = r + 1 < n && off[r + 1] != 0 ? (int64_t)(split(r) - off[r]) : F.h_recs[r].seq_len;
        fa_push(F, r, off[r] == 0 ? 1 : 2, off[r] == 0 ? (int32_t)name_len[r] : 0, 0, 0, s[r], e, false);
    }
    return fa_plan_end(c, info);
}

int paffy_hip_faffy_emit(paffy_hip_ctx *c, void *d_out, int64_t out_cap, paffy_error *err) {
    if (!c || !c->fasta || !c->fasta->planned) return PAFFY_E_STATE;
    FastaState &F = *c->fasta;
    if (err) memset(err, 0, sizeof(*err));
    if (!F.out_bytes) return 0;
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 15u)) return PAFFY_E_ARG;
    if (out_cap < ((F.out_bytes + 15) & ~(int64_t)15)) return PAFFY_E_CAPACITY;
    if (ensure(c, F.dev.bad, sizeof(unsigned long long))) return PAFFY_E_HIP;
    HIPCHK(c, hipMemsetAsync(F.dev.bad.p, 0xff, sizeof(unsigned long long), c->stream));
    const int64_t n_win = (F.out_bytes + FA_WIN - 1) / FA_WIN;
    LAUNCH(c, "k_fa_emit", k_fa_emit, dim3((unsigned)((n_win + FA_EMIT_WAVES - 1) / FA_EMIT_WAVES)), dim3(64 * FA_EMIT_WAVES), 0,
           static_cast<const FaItem *>(F.dev.items.p), F.n_items, F.text, static_cast<const uint8_t *>(F.dev.bases.p),
           static_cast<uint8_t *>(d_out), F.out_bytes, static_cast<unsigned long long *>(F.dev.bad.p));
    unsigned long long bad = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&bad, F.dev.bad.p, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->profile) prof_collect(c);
    if (bad != ~0ull && err) {
        err->code = PAFFY_ERR_FAFFY_BASE;
        err->stage = -1;
        err->record = (int64_t)bad;
    }
    return 0;
}

} /* extern "C" */

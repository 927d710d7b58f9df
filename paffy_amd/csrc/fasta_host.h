/*
 * fasta_host.h -- host side of `faffy chunk | extract | merge` (include/paffy_hip.h): the device FASTA index of
 * fasta_kernel.h, the item plans of the three commands (small host logic over the record table) and the emit.
 * Included by paffy_hip.hip behind the context.
 */
#pragma once

#include <climits>
#include <map>

struct FastaState {
    struct Dev { /* all of the state's device memory: fasta_release lets it go while the state lives */
        DevBuf starts, tiles, totals, recs, bases, hdr_off, hdr_blob, items, bad;
        DevBuf seen_names, seen_off, seen; /* paffy_hip_fasta_seen (seqload_host.h): the distinct names and a flag per name */
    } dev;
    const uint8_t *text = nullptr; /* the caller's text: emit reads the header names from it */
    int64_t text_len = 0, n_rec = 0, n_bases = 0;
    bool indexed = false, planned = false;
    bool with_bases = false; /* false: paffy_hip_fasta_index_headers, no compact base buffer */
    std::vector<FaRec> h_recs;
    std::vector<char> h_hdr;       /* all headers back to back */
    std::vector<int64_t> h_hdr_at; /* record r's header is h_hdr[h_hdr_at[r] .. h_hdr_at[r + 1]) */
    std::vector<FaItem> h_items;
    std::vector<int64_t> file_ends; /* chunk: end of each output file in the output */
    int64_t out_bytes = 0;
};

static void fasta_release(FastaState &F) { F.dev = FastaState::Dev(); }

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
    info->n_rows = (int64_t)F.h_items.size();
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
   only; the compact base buffer is neither allocated nor written (upconvert and to_bed -q need the lengths alone). */
static int fa_index(paffy_hip_ctx *c, FastaState &F, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, bool with_bases) {
    if (!c || text_len < 0 || (text_len > 0 && !d_text) || (reinterpret_cast<uintptr_t>(d_text) & 15u)) return PAFFY_E_ARG;
    if (n_files < 0 || (n_files > 0 && !file_starts)) return PAFFY_E_ARG;
    std::vector<int64_t> starts(file_starts, file_starts + n_files);
    if (starts.empty()) starts.push_back(0);
    if (starts[0] != 0) return PAFFY_E_ARG;
    for (size_t k = 1; k < starts.size(); k++)
        if (starts[k] < starts[k - 1] || starts[k] > text_len) return PAFFY_E_ARG;
    F.indexed = F.planned = false;
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
            F.h_hdr.resize((size_t)blob + 1);
            if (blob) {
                if (ensure(c, F.dev.hdr_off, sizeof(int64_t) * (size_t)F.n_rec)) return PAFFY_E_HIP;
                if (ensure(c, F.dev.hdr_blob, (size_t)blob)) return PAFFY_E_HIP;
                HIPCHK(c, hipMemcpyAsync(F.dev.hdr_off.p, F.h_hdr_at.data(), sizeof(int64_t) * (size_t)F.n_rec, hipMemcpyHostToDevice, c->stream));
                LAUNCH(c, "k_fa_headers", k_fa_headers, dim3((unsigned)((F.n_rec + FA_NT / 64 - 1) / (FA_NT / 64))), dim3(FA_NT), 0, F.text,
                       static_cast<const FaRec *>(F.dev.recs.p), F.n_rec, static_cast<const int64_t *>(F.dev.hdr_off.p), static_cast<uint8_t *>(F.dev.hdr_blob.p));
                HIPCHK(c, hipMemcpyAsync(F.h_hdr.data(), F.dev.hdr_blob.p, (size_t)blob, hipMemcpyDeviceToHost, c->stream));
            }
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->profile) prof_collect(c);
    }
    F.indexed = true;
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

int paffy_hip_faffy_extract_plan(paffy_hip_ctx *c, const char *bed, int64_t bed_len, int64_t flank, int64_t min_size, int skip_missing, paffy_plan_info *info) {
    int rc = fa_plan_begin(c, info);
    if (rc) return rc;
    if (bed_len < 0 || (bed_len > 0 && !bed)) return PAFFY_E_ARG;
    FastaState &F = *c->fasta;
    std::unordered_map<std::string, int64_t> by_name; /* duplicate names: the last record wins */
    by_name.reserve((size_t)F.n_rec * 2);
    for (int64_t r = 0; r < F.n_rec; r++) by_name[fa_header(F, r)] = r;
    struct Iv {
        const std::string *name;
        int64_t rec, start, end;
    };
    std::vector<Iv> ivs;
    /* BED lines (stFile_getLineFromFile): split on white space, atol of tokens 1 and 2 */
    int64_t line_no = 0;
    for (int64_t p = 0; p < bed_len; line_no++) {
        int64_t e = p;
        while (e < bed_len && bed[e] != '\n') e++;
        std::string tok[3];
        int nt = 0;
        for (int64_t q = p; q < e && nt < 3;) {
            while (q < e && isspace((unsigned char)bed[q])) q++;
            if (q >= e) break;
            int64_t t = q;
            while (t < e && !isspace((unsigned char)bed[t])) t++;
            tok[nt++].assign(bed + q, (size_t)(t - q));
            q = t;
        }
        p = e + 1;
        if (nt < 3) { /* stList_get past the end of the tokens: an assert */
            fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, line_no);
            return fa_plan_end(c, info);
        }
        auto it = by_name.find(tok[0]);
        if (it == by_name.end()) {
            if (skip_missing) continue;
            fa_fail(info, PAFFY_ERR_FAFFY_MISSING_SEQ, line_no);
            return fa_plan_end(c, info);
        }
        ivs.push_back(Iv{&it->first, it->second, (int64_t)atol(tok[1].c_str()), (int64_t)atol(tok[2].c_str())});
    }
    std::sort(ivs.begin(), ivs.end(), [](const Iv &a, const Iv &b) {
        const int k = strcmp(a.name->c_str(), b.name->c_str());
        if (k) return k < 0;
        if (a.start != b.start) return a.start < b.start;
        return a.end < b.end;
    });
    int64_t p_rec = -1, p_start = -1, p_end = -1;
    for (size_t k = 0; k < ivs.size(); k++) {
        const Iv &iv = ivs[k];
        if ((int64_t)((uint64_t)iv.end - (uint64_t)iv.start) < min_size) continue; /* int64 arithmetic as the reference's (wrapping) */
        const int64_t len = F.h_recs[iv.rec].seq_len;
        const int64_t sf = (int64_t)((uint64_t)iv.start - (uint64_t)flank), ef = (int64_t)((uint64_t)iv.end + (uint64_t)flank);
        const int64_t i = sf > 0 ? sf : 0, j = ef <= len ? ef : len;
        if (!(0 <= i && i <= iv.start && iv.start <= iv.end && iv.end <= j && j <= len)) { /* impl/fasta_extract.c:211 */
            fa_fail(info, PAFFY_ERR_FAFFY_ASSERT, (int64_t)k);
            return fa_plan_end(c, info);
        }
        if (p_rec >= 0) {
            if (p_rec == iv.rec && p_end >= i) {
                p_end = p_end > j ? p_end : j;
                continue;
            }
            fa_push(F, p_rec, 0, (int32_t)F.h_recs[p_rec].hdr_len, F.h_recs[p_rec].seq_len, p_start, p_start, p_end, true);
        }
        p_rec = iv.rec;
        p_start = i;
        p_end = j;
    }
    if (p_rec >= 0) fa_push(F, p_rec, 0, (int32_t)F.h_recs[p_rec].hdr_len, F.h_recs[p_rec].seq_len, p_start, p_start, p_end, true);
    return fa_plan_end(c, info);
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
           static_cast<const FaItem *>(F.dev.items.p), (int64_t)F.h_items.size(), F.text, static_cast<const uint8_t *>(F.dev.bases.p),
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

/*
 * paffy split_file in the library: the plan that groups a batch's lines by output file (split_kernel.h) and the file assignment of
 * impl/paf_split_file.c:146-169, which runs here once per group -- a distinct (contig name, small bit) of the batch -- not once per
 * line. The files live in the context from paffy_hip_split_begin on, over any number of batches: two hash maps of name bytes (the
 * reference's contig_to_file and small_contig_to_file), the dense file ids in opening order with their name suffixes, and the
 * current small file with the contig lengths it holds so far.
 * Included by paffy_hip.hip behind dedupe_host.h (dedupe_plan_select, dedupe_plan_lines, RPCHK, rocPRIM).
 */
#pragma once

#include "split_kernel.h"

struct SplitState {
    /* device scratch of a plan */
    DevBuf keys, skeys, idx, order, head, head_of, opens, rank, count, start, collide, table, name_len, name_pos, blob, group_of, file_of, first, offs, tmp;
    /* the run (paffy_hip_split_begin) */
    bool begun = false;
    int by_query = 0;
    int64_t min_length = 0;
    int narrow_salt0 = 0; /* PAFFY_SPLIT_NARROW_SALT0: salt 0's hash cut to two bits, so that a test gets the regrouping to run */
    uint32_t salt = 0;    /* salt the last plan's grouping passed its byte check with (0 unless names collided) */
    std::unordered_map<std::string, int64_t> big, small; /* contig name -> file */
    std::vector<std::string> files;                      /* suffix of every file, in opening order */
    int64_t current_small = -1, current_small_length = 0, n_small_files = 0;
    std::vector<paffy_split_group> groups; /* of the current plan, in output order */
};

static int split_sort_pairs(paffy_hip_ctx *c, SplitState &S, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, size_t n, unsigned bits = 64) {
    size_t bytes = 0;
    RPCHK(c, rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0, bits, c->stream));
    if (ensure(c, S.tmp, bytes + 16)) return PAFFY_E_HIP;
    RPCHK(c, rocprim::radix_sort_pairs(S.tmp.p, bytes, kin, kout, vin, vout, n, 0, bits, c->stream));
    return 0;
}
static int split_max_scan(paffy_hip_ctx *c, SplitState &S, const uint32_t *in, uint32_t *out, size_t n) {
    size_t bytes = 0;
    RPCHK(c, rocprim::inclusive_scan(nullptr, bytes, in, out, n, DdMax(), c->stream));
    if (ensure(c, S.tmp, bytes + 16)) return PAFFY_E_HIP;
    RPCHK(c, rocprim::inclusive_scan(S.tmp.p, bytes, in, out, n, DdMax(), c->stream));
    return 0;
}
static int split_excl_scan(paffy_hip_ctx *c, SplitState &S, const uint32_t *in, uint32_t *out, size_t n) {
    size_t bytes = 0;
    RPCHK(c, rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    if (ensure(c, S.tmp, bytes + 16)) return PAFFY_E_HIP;
    RPCHK(c, rocprim::exclusive_scan(S.tmp.p, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    return 0;
}
static int split_fetch(paffy_hip_ctx *c, void *dst, const void *src, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* records [0, nk) of the indexed batch -> tile_order[0 .. nk) grouped (split_kernel.h), S.start / S.count per group, S.group_of per
   record. Returns the number of groups in *n_groups. */
static int split_group_records(paffy_hip_ctx *c, SplitState &S, const uint8_t *in, uint32_t nk, uint32_t *n_groups) {
    const size_t n = nk;
    if (ensure(c, S.keys, sizeof(uint64_t) * n) || ensure(c, S.skeys, sizeof(uint64_t) * n) || ensure(c, S.idx, sizeof(uint32_t) * n) ||
        ensure(c, S.order, sizeof(uint32_t) * n) || ensure(c, S.head, sizeof(uint32_t) * n) || ensure(c, S.head_of, sizeof(uint32_t) * n) ||
        ensure(c, S.opens, sizeof(uint32_t) * (n + 1)) || ensure(c, S.rank, sizeof(uint32_t) * (n + 1)) || ensure(c, S.group_of, sizeof(uint32_t) * n) ||
        ensure(c, S.collide, sizeof(uint32_t)))
        return PAFFY_E_HIP;
    const RecMeta *meta = static_cast<const RecMeta *>(c->meta.p);
    uint64_t *keys = static_cast<uint64_t *>(S.keys.p), *skeys = static_cast<uint64_t *>(S.skeys.p);
    uint32_t *idx = static_cast<uint32_t *>(S.idx.p), *order = static_cast<uint32_t *>(S.order.p), *head = static_cast<uint32_t *>(S.head.p);
    uint32_t *head_of = static_cast<uint32_t *>(S.head_of.p), *opens = static_cast<uint32_t *>(S.opens.p), *rank = static_cast<uint32_t *>(S.rank.p);
    uint32_t *collide = static_cast<uint32_t *>(S.collide.p);
    const dim3 grid((nk + PAFFY_NT - 1) / PAFFY_NT), grid1((nk + 1 + PAFFY_NT - 1) / PAFFY_NT), block(PAFFY_NT);
    /* groups: records sorted by name key, the names then checked against their group's first (the reference looks the name up by
       string equality, impl/paf_split_file.c:148, :42): two names under one key -> the grouping again with the next salt */
    for (uint32_t salt = 0;; salt++) {
        LAUNCH(c, "k_split_keys", k_split_keys, grid, block, 0, in, meta, nk, S.by_query, S.min_length, salt, (salt == 0 && S.narrow_salt0) ? 1 : 0, keys, idx);
        if (split_sort_pairs(c, S, keys, skeys, idx, order, n)) return PAFFY_E_HIP;
        LAUNCH(c, "k_split_heads", k_split_heads, grid1, block, 0, static_cast<const uint64_t *>(skeys), static_cast<const uint32_t *>(order), nk, head, opens);
        if (split_max_scan(c, S, head, head_of, n)) return PAFFY_E_HIP;
        uint32_t hit = 0;
        HIPCHK(c, hipMemsetAsync(collide, 0, sizeof(uint32_t), c->stream));
        LAUNCH(c, "k_split_verify", k_split_verify, grid, block, 0, in, meta, static_cast<const uint32_t *>(order), static_cast<const uint32_t *>(head_of), nk, S.by_query, collide);
        if (split_fetch(c, &hit, collide, sizeof(uint32_t))) return PAFFY_E_HIP;
        S.salt = salt;
        if (!hit) break;
        if (salt == 7) {
            c->last_error = "split_file: contig names keep colliding under eight differently salted 64-bit hashes";
            return PAFFY_E_UNSUPPORTED;
        }
    }
    /* groups in the order of their first record; the sort is stable, so a run's head is that record and a run keeps input order */
    if (split_excl_scan(c, S, opens, rank, n + 1)) return PAFFY_E_HIP;
    uint32_t ng = 0;
    if (split_fetch(c, &ng, rank + nk, sizeof(uint32_t))) return PAFFY_E_HIP;
    if (ensure(c, S.count, sizeof(uint32_t) * ((size_t)ng + 1)) || ensure(c, S.start, sizeof(uint32_t) * ((size_t)ng + 1))) return PAFFY_E_HIP;
    uint32_t *count = static_cast<uint32_t *>(S.count.p), *start = static_cast<uint32_t *>(S.start.p);
    LAUNCH(c, "k_split_counts", k_split_counts, grid, block, 0, static_cast<const uint64_t *>(skeys), static_cast<const uint32_t *>(order), static_cast<const uint32_t *>(head_of),
           static_cast<const uint32_t *>(rank), nk, ng, count);
    if (split_excl_scan(c, S, count, start, (size_t)ng + 1)) return PAFFY_E_HIP;
    LAUNCH(c, "k_split_place", k_split_place, grid, block, 0, static_cast<const uint32_t *>(order), static_cast<const uint32_t *>(head_of), static_cast<const uint32_t *>(rank),
           static_cast<const uint32_t *>(start), nk, static_cast<uint32_t *>(c->tile_order.p), static_cast<uint32_t *>(S.group_of.p));
    *n_groups = ng;
    return 0;
}

/* impl/paf_split_file.c:146-169 for one group: the file of (name, small bit), opened if the run has not seen the pair */
static void split_assign_file(SplitState &S, const std::string &name, int64_t contig_len, bool is_small, paffy_split_group &g) {
    g.new_file = 0;
    if (is_small) {
        auto it = S.small.find(name);
        if (it != S.small.end()) {
            g.file = it->second;
            return;
        }
        if (S.current_small < 0 || S.current_small_length + contig_len > S.min_length) { /* a new small file */
            S.current_small = (int64_t)S.files.size();
            S.files.push_back("small_" + std::to_string(S.n_small_files++));
            S.current_small_length = 0;
            g.new_file = 1;
        }
        S.current_small_length += contig_len;
        S.small.emplace(name, S.current_small);
        g.file = S.current_small;
        return;
    }
    auto it = S.big.find(name);
    if (it != S.big.end()) {
        g.file = it->second;
        return;
    }
    std::string suffix = name; /* sanitize_filename, impl/paf_split_file.c:26-36 */
    for (char &ch : suffix)
        if (ch == '/') ch = '_';
    g.file = (int64_t)S.files.size();
    S.files.push_back(suffix);
    S.big.emplace(name, g.file);
    g.new_file = 1;
}

int paffy_hip_split_begin(paffy_hip_ctx *c, int by_query, int64_t min_length) {
    if (!c) return PAFFY_E_ARG;
    if (!c->split) c->split.reset(new SplitState());
    SplitState &S = *c->split;
    S.begun = true;
    S.by_query = by_query ? 1 : 0;
    S.min_length = min_length;
    const char *knob = getenv("PAFFY_SPLIT_NARROW_SALT0");
    S.narrow_salt0 = (knob && *knob && strcmp(knob, "0") != 0) ? 1 : 0;
    S.salt = 0;
    S.big.clear();
    S.small.clear();
    S.files.clear();
    S.current_small = -1;
    S.current_small_length = 0;
    S.n_small_files = 0;
    S.groups.clear();
    c->plan_split = false;
    return 0;
}

int paffy_hip_split_plan(paffy_hip_ctx *c, const void *d_in, int64_t in_len, paffy_plan_info *info) {
    if (!c || !info) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    if (!c->split || !c->split->begun) {
        c->last_error = "paffy_hip_split_plan: no paffy_hip_split_begin on this context";
        return PAFFY_E_STATE;
    }
    SplitState &S = *c->split;
    plan_begin(c, PLAN_LINES, in_len, info); /* the writer of tile and dedupe: header + the cigar text as it was read */
    S.groups.clear();
    if (in_len == 0) {
        c->planned = true;
        c->plan_split = true;
        return 0;
    }
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint32_t n = 0, nk = 0;
    {
        int rc = dedupe_plan_select(c, in, in_len, PAFFY_DEDUPE_KEEP_ALL, &n, &nk); /* every record in front of the first failing one */
        if (rc) return rc;
    }
    if (n == 0) {
        *info = c->plan;
        c->planned = true;
        c->plan_split = true;
        return 0;
    }
    uint32_t ng = 0;
    if (nk > 0) {
        int rc = split_group_records(c, S, in, nk, &ng);
        if (rc) return rc;
    }
    /* the stretches of the output, one per file that gets lines of this batch; first_line[s] = its first line */
    std::vector<uint32_t> first_line;
    if (ng > 0) {
        if (ensure(c, S.table, sizeof(SplitGroupDev) * (size_t)ng) || ensure(c, S.name_len, sizeof(uint32_t) * ((size_t)ng + 1)) ||
            ensure(c, S.name_pos, sizeof(uint32_t) * ((size_t)ng + 1)))
            return PAFFY_E_HIP;
        SplitGroupDev *table = static_cast<SplitGroupDev *>(S.table.p);
        uint32_t *name_len = static_cast<uint32_t *>(S.name_len.p), *name_pos = static_cast<uint32_t *>(S.name_pos.p);
        LAUNCH(c, "k_split_table", k_split_table, dim3((ng + 1 + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(c->meta.p),
               static_cast<const uint32_t *>(c->tile_order.p), static_cast<const uint32_t *>(S.start.p), static_cast<const uint32_t *>(S.count.p), ng, S.by_query, S.min_length, table,
               name_len);
        if (split_excl_scan(c, S, name_len, name_pos, (size_t)ng + 1)) return PAFFY_E_HIP;
        uint32_t blob_bytes = 0;
        if (split_fetch(c, &blob_bytes, name_pos + ng, sizeof(uint32_t))) return PAFFY_E_HIP;
        if (ensure(c, S.blob, (size_t)blob_bytes + 16)) return PAFFY_E_HIP;
        LAUNCH(c, "k_split_names", k_split_names, dim3((ng + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, in, static_cast<const SplitGroupDev *>(table),
               static_cast<const uint32_t *>(name_pos), ng, static_cast<uint8_t *>(S.blob.p));
        /* the table, once per batch */
        std::vector<SplitGroupDev> h_table(ng);
        std::vector<uint32_t> h_pos((size_t)ng + 1);
        std::string h_blob(blob_bytes, '\0');
        HIPCHK(c, hipMemcpyAsync(h_table.data(), table, sizeof(SplitGroupDev) * (size_t)ng, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h_pos.data(), name_pos, sizeof(uint32_t) * ((size_t)ng + 1), hipMemcpyDeviceToHost, c->stream));
        if (blob_bytes) HIPCHK(c, hipMemcpyAsync(&h_blob[0], S.blob.p, blob_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        /* the file of every group; groups of one file (contigs of a small_<k>) become one stretch, numbered by the file's first record */
        std::unordered_map<int64_t, uint32_t> stretch_of;
        std::vector<uint32_t> file_of(ng);
        for (uint32_t g = 0; g < ng; g++) {
            const SplitGroupDev &t = h_table[g];
            paffy_split_group o;
            memset(&o, 0, sizeof(o));
            split_assign_file(S, h_blob.substr(h_pos[g], t.name_len), t.contig_len, t.is_small != 0, o);
            auto it = stretch_of.find(o.file);
            if (it == stretch_of.end()) {
                o.lines = t.lines;
                o.first_record = t.first_record;
                o.is_small = (int32_t)t.is_small;
                it = stretch_of.emplace(o.file, (uint32_t)S.groups.size()).first;
                S.groups.push_back(o);
            } else {
                S.groups[it->second].lines += t.lines; /* a group behind the file's first: it cannot have opened the file */
            }
            file_of[g] = it->second;
        }
        const uint32_t ns = (uint32_t)S.groups.size();
        if (ns < ng) { /* lines of one file in input order, whichever contig they belong to: a stable sort of the records by stretch */
            unsigned bits = 1;
            while (bits < 32 && (1u << bits) < ns) bits++;
            if (ensure(c, S.file_of, sizeof(uint32_t) * (size_t)ng)) return PAFFY_E_HIP;
            HIPCHK(c, hipMemcpyAsync(S.file_of.p, file_of.data(), sizeof(uint32_t) * (size_t)ng, hipMemcpyHostToDevice, c->stream));
            LAUNCH(c, "k_split_file_keys", k_split_file_keys, dim3((nk + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(S.group_of.p),
                   static_cast<const uint32_t *>(S.file_of.p), nk, static_cast<uint64_t *>(S.keys.p), static_cast<uint32_t *>(S.idx.p));
            if (split_sort_pairs(c, S, static_cast<const uint64_t *>(S.keys.p), static_cast<uint64_t *>(S.skeys.p), static_cast<const uint32_t *>(S.idx.p),
                                 static_cast<uint32_t *>(c->tile_order.p), nk, bits))
                return PAFFY_E_HIP;
            HIPCHK(c, hipStreamSynchronize(c->stream)); /* file_of is read from this frame */
        }
        first_line.resize((size_t)ns + 1);
        uint32_t at = 0;
        for (uint32_t s = 0; s < ns; s++) {
            first_line[s] = at;
            at += (uint32_t)S.groups[s].lines;
        }
        first_line[ns] = at; /* = nk */
    }
    {
        int rc = dedupe_plan_lines(c, in, nk, info); /* sizes and offsets of the lines in the grouped order */
        if (rc) return rc;
    }
    c->planned = false; /* until the stretches have their offsets */
    if (!S.groups.empty()) {
        const uint32_t ns = (uint32_t)S.groups.size();
        if (ensure(c, S.first, sizeof(uint32_t) * ((size_t)ns + 1)) || ensure(c, S.offs, sizeof(uint64_t) * ((size_t)ns + 1))) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(S.first.p, first_line.data(), sizeof(uint32_t) * ((size_t)ns + 1), hipMemcpyHostToDevice, c->stream));
        LAUNCH(c, "k_split_offsets", k_split_offsets, dim3((ns + 1 + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, c->line_off, static_cast<const uint32_t *>(S.first.p), ns + 1,
               static_cast<uint64_t *>(S.offs.p));
        std::vector<uint64_t> offs((size_t)ns + 1);
        if (split_fetch(c, offs.data(), S.offs.p, sizeof(uint64_t) * ((size_t)ns + 1))) return PAFFY_E_HIP;
        if (c->profile) prof_collect(c);
        for (uint32_t s = 0; s < ns; s++) {
            S.groups[s].out_off = (int64_t)offs[s];
            S.groups[s].bytes = (int64_t)(offs[s + 1] - offs[s]);
        }
    }
    c->planned = true;
    c->plan_split = true;
    return 0;
}

int64_t paffy_hip_split_groups(paffy_hip_ctx *c, int64_t cap, paffy_split_group *groups) {
    if (!c || cap < 0 || (cap > 0 && !groups)) return PAFFY_E_ARG;
    if (!c->planned || !c->plan_split || !c->split) return PAFFY_E_STATE;
    const SplitState &S = *c->split;
    const int64_t n = (int64_t)S.groups.size();
    if (cap < n) return PAFFY_E_CAPACITY;
    if (n > 0) memcpy(groups, S.groups.data(), sizeof(paffy_split_group) * (size_t)n);
    return n;
}

int64_t paffy_hip_split_file_name(paffy_hip_ctx *c, int64_t file, char *buf, int64_t cap) {
    if (!c || cap < 0 || (cap > 0 && !buf)) return PAFFY_E_ARG;
    if (!c->split || !c->split->begun) return PAFFY_E_STATE;
    const SplitState &S = *c->split;
    if (file < 0 || file >= (int64_t)S.files.size()) return PAFFY_E_ARG;
    const std::string &s = S.files[(size_t)file];
    if (cap < (int64_t)s.size() + 1) return PAFFY_E_CAPACITY;
    memcpy(buf, s.data(), s.size());
    buf[s.size()] = '\0';
    return (int64_t)s.size();
}

int64_t paffy_hip_split_file_count(paffy_hip_ctx *c) {
    if (!c) return PAFFY_E_ARG;
    if (!c->split || !c->split->begun) return PAFFY_E_STATE;
    return (int64_t)c->split->files.size();
}

int paffy_hip_split_salt(paffy_hip_ctx *c) {
    if (!c) return PAFFY_E_ARG;
    if (!c->split || !c->split->begun) return PAFFY_E_STATE;
    return (int)c->split->salt;
}

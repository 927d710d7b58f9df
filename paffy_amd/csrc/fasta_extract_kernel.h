/*
 * fasta_extract_kernel.h -- the plan of `faffy extract` on the device: BED text in HBM to the items of k_fa_emit.
 *
 * Lines. A line starts at byte 0 and after every '\n' that is not the text's last byte. Every thread owns FA_PER bytes (the slices of
 * k_fa_seen): k_bed_index counts the line starts of a slice, an exclusive scan numbers them, k_bed_parse walks them.
 * A line gives its first three runs of bytes that are not isspace() in the C locale; the first is looked up in the sorted distinct
 * FASTA names (find_seq: the index there is the strcmp rank), the other two go through glibc's atol. A line with fewer than three
 * tokens or, without skip_missing, an unknown name fails the plan: the lowest line wins (atomicMin on line * 2 + kind).
 * Intervals. Sorted by (rank, start, end), k_bed_bounds decides per interval whether it is kept (end - start >= min_size) and gives
 * its flanked [i, j) with the check of impl/fasta_extract.c:211; the first failing index wins. The kept ones are compacted.
 * Merge. Among the kept intervals of a name i does not fall, so an interval opens an item exactly when the maximum of j over all
 * earlier kept intervals of its name is below its i (k_bed_heads, after a max-scan by name), and an item ends at the inclusive maximum
 * of its last interval. One scan (BedRun) then carries the item's start to that last interval, counts the items and sums the output
 * bytes: an item's bytes are split into what its first interval knows (the header line, -start, the '\n') and its last (the end).
 * k_bed_items writes one FaItem per last interval.
 */
#pragma once

#define BED_KIND_SHORT 0ull   /* fewer than three tokens: PAFFY_ERR_FAFFY_ASSERT */
#define BED_KIND_MISSING 1ull /* no FASTA record of that name: PAFFY_ERR_FAFFY_MISSING_SEQ */

/* one BED line as parsed; rank == n_names: dropped (skip_missing) or failed */
struct BedIv {
    int64_t start, end;
    uint32_t rank, pad;
};
struct BedIvLess {
    __host__ __device__ __forceinline__ bool operator()(const BedIv &a, const BedIv &b) const {
        if (a.rank != b.rank) return a.rank < b.rank;
        if (a.start != b.start) return a.start < b.start;
        return a.end < b.end;
    }
};

/* what the host reads of a plan */
struct BedStat {
    unsigned long long parse_err;  /* line * 2 + kind of the first failing line, ~0: none */
    unsigned long long bounds_err; /* the first sorted interval that fails its check, ~0: none */
};

/* the scan over the kept intervals: output bytes and items so far, the start of the item that is open */
struct BedRun {
    int64_t bytes, start;
    uint32_t items, has_start;
};
struct BedRunPlus {
    __host__ __device__ __forceinline__ BedRun operator()(const BedRun &a, const BedRun &b) const {
        BedRun r;
        r.bytes = (int64_t)((uint64_t)a.bytes + (uint64_t)b.bytes);
        r.items = a.items + b.items;
        r.start = b.has_start ? b.start : a.start;
        r.has_start = a.has_start | b.has_start;
        return r;
    }
};
struct BedMax64 {
    __host__ __device__ __forceinline__ int64_t operator()(int64_t a, int64_t b) const { return a > b ? a : b; }
};

/* 0x80 in every byte of w that is '\n' (exact: no carry crosses a byte) */
__device__ __forceinline__ uint32_t bed_nl4(uint32_t w) {
    const uint32_t x = w ^ 0x0a0a0a0au;
    return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
/* the bytes of word k of a 16-byte load that lie inside the text (valid: how many of the 16 do) */
__device__ __forceinline__ uint32_t bed_word_mask(int64_t valid, int k) {
    const int64_t v = valid - 4 * k;
    return v >= 4 ? 0xffffffffu : v <= 0 ? 0u : (1u << (8 * (uint32_t)v)) - 1u;
}
/* isspace() of the C locale */
__device__ __forceinline__ bool bed_space(uint32_t b) { return b == 0x20u || (b - 0x09u) <= 4u; }

/* glibc's atol of the token [a, b) (no white space inside): sign, digits up to the first other byte, saturating */
__device__ __forceinline__ int64_t bed_atol(const uint8_t *bed, int64_t a, int64_t b) {
    int64_t p = a;
    bool neg = false;
    if (p < b && (bed[p] == '+' || bed[p] == '-')) {
        neg = bed[p] == '-';
        p++;
    }
    const uint64_t lim = neg ? (1ull << 63) : (1ull << 63) - 1ull;
    uint64_t acc = 0;
    bool over = false;
    for (; p < b; p++) {
        const uint32_t d = (uint32_t)bed[p] - '0';
        if (d > 9u) break;
        if (!over) {
            if (acc > (lim - d) / 10ull) over = true;
            else acc = acc * 10ull + d;
        }
    }
    if (over) return neg ? INT64_MIN : INT64_MAX;
    return neg ? (int64_t)(0ull - acc) : (int64_t)acc;
}

/* line starts per slice: 16-byte loads, the '\n' bytes of a word counted at once */
__global__ __launch_bounds__(FA_NT) void k_bed_index(const uint8_t *bed, int64_t len, int64_t *count) {
    const int64_t t = (int64_t)blockIdx.x * FA_NT + threadIdx.x;
    const int64_t g0 = t * (int64_t)FA_PER;
    if (g0 >= len) return;
    const int64_t g1 = g0 + (int64_t)FA_PER < len ? g0 + (int64_t)FA_PER : len;
    uint32_t n = 0;
    for (int64_t q = g0; q < g1; q += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bed + q);
        const int64_t valid = len - q;
        n += __popc(bed_nl4(v.x & bed_word_mask(valid, 0))) + __popc(bed_nl4(v.y & bed_word_mask(valid, 1))) +
             __popc(bed_nl4(v.z & bed_word_mask(valid, 2))) + __popc(bed_nl4(v.w & bed_word_mask(valid, 3)));
    }
    if (g1 == len && bed[len - 1] == '\n') n--; /* no line starts behind the text's last byte */
    count[t] = (int64_t)n + (t == 0 ? 1 : 0);   /* the line at byte 0 */
}

/* the line that starts at s, which is line number `line` */
__device__ __forceinline__ void bed_line(const uint8_t *bed, int64_t len, int64_t s, int64_t line, const uint8_t *names, const uint32_t *name_off,
                                         const int64_t *name_rec, int32_t n_names, int32_t skip_missing, BedIv *iv, BedStat *stat) {
    int64_t q = s, a0 = 0, b0 = 0, a1 = 0, b1 = 0, a2 = 0, b2 = 0;
    int nt = 0;
    while (nt < 3) {
        while (q < len && bed[q] != '\n' && bed_space(bed[q])) q++;
        if (q >= len || bed[q] == '\n') break;
        const int64_t a = q;
        while (q < len && !bed_space(bed[q])) q++;
        /* selects, no indexed array: no scratch */
        a0 = nt == 0 ? a : a0;
        b0 = nt == 0 ? q : b0;
        a1 = nt == 1 ? a : a1;
        b1 = nt == 1 ? q : b1;
        a2 = nt == 2 ? a : a2;
        b2 = nt == 2 ? q : b2;
        nt++;
    }
    BedIv o;
    o.start = o.end = 0;
    o.rank = (uint32_t)n_names;
    o.pad = 0;
    if (nt < 3) {
        atomicMin(&stat->parse_err, ((unsigned long long)line << 1) | BED_KIND_SHORT);
    } else {
        const int32_t k = b0 - a0 > (int64_t)0xffffffffll ? -1 : find_seq(bed + a0, 0, (uint32_t)(b0 - a0), names, name_off, n_names);
        if (k < 0 || name_rec[k] < 0) { /* no name, or one that only headers with a NUL byte are keyed by */
            if (!skip_missing) atomicMin(&stat->parse_err, ((unsigned long long)line << 1) | BED_KIND_MISSING);
        } else {
            o.rank = (uint32_t)k;
            o.start = bed_atol(bed, a1, b1);
            o.end = bed_atol(bed, a2, b2);
        }
    }
    iv[line] = o;
}

/* every line to iv[its number]; first[t]: the number of the first line that starts in slice t (thread 0: of the line at byte 0) */
__global__ __launch_bounds__(FA_NT) void k_bed_parse(const uint8_t *bed, int64_t len, const int64_t *first, const uint8_t *names, const uint32_t *name_off,
                                                     const int64_t *name_rec, int32_t n_names, int32_t skip_missing, BedIv *iv, BedStat *stat) {
    const int64_t t = (int64_t)blockIdx.x * FA_NT + threadIdx.x;
    const int64_t g0 = t * (int64_t)FA_PER;
    if (g0 >= len) return;
    const int64_t g1 = g0 + (int64_t)FA_PER < len ? g0 + (int64_t)FA_PER : len;
    int64_t line = first[t];
    if (t == 0) bed_line(bed, len, 0, line++, names, name_off, name_rec, n_names, skip_missing, iv, stat);
    for (int64_t q = g0; q < g1; q += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bed + q);
        const int64_t valid = len - q;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t w = k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
            uint32_t m = bed_nl4(w & bed_word_mask(valid, k));
            while (m) {
                const int64_t p = q + 4 * k + ((__ffs(m) - 1) >> 3);
                m &= m - 1u;
                if (p + 1 < len) bed_line(bed, len, p + 1, line++, names, name_off, name_rec, n_names, skip_missing, iv, stat);
            }
        }
    }
}

/* per sorted interval: kept or not, the flanked [i, j) and the check (impl/fasta_extract.c:211); keep has n + 1 entries, the last 0 */
__global__ __launch_bounds__(FA_NT) void k_bed_bounds(const BedIv *iv, int64_t n, const int64_t *name_rec, const FaRec *recs, int32_t n_names,
                                                      int64_t flank, int64_t min_size, uint32_t *keep, int64_t *lo, int64_t *hi, BedStat *stat) {
    const int64_t k = (int64_t)blockIdx.x * FA_NT + threadIdx.x;
    if (k > n) return;
    uint32_t kept = 0;
    if (k < n) {
        const BedIv v = iv[k];
        if (v.rank < (uint32_t)n_names && (int64_t)((uint64_t)v.end - (uint64_t)v.start) >= min_size) { /* int64 arithmetic as the reference's (wrapping) */
            const int64_t len = recs[name_rec[v.rank]].seq_len;
            const int64_t sf = (int64_t)((uint64_t)v.start - (uint64_t)flank), ef = (int64_t)((uint64_t)v.end + (uint64_t)flank);
            const int64_t i = sf > 0 ? sf : 0, j = ef <= len ? ef : len;
            if (0 <= i && i <= v.start && v.start <= v.end && v.end <= j && j <= len) {
                kept = 1;
                lo[k] = i;
                hi[k] = j;
            } else {
                atomicMin(&stat->bounds_err, (unsigned long long)k);
            }
        }
    }
    keep[k] = kept;
}

/* the kept intervals, in order, side by side */
__global__ __launch_bounds__(FA_NT) void k_bed_compact(const BedIv *iv, int64_t n, const uint32_t *keep, const uint32_t *pos, const int64_t *lo,
                                                       const int64_t *hi, uint32_t *c_rank, int64_t *c_lo, int64_t *c_hi) {
    const int64_t k = (int64_t)blockIdx.x * FA_NT + threadIdx.x;
    if (k >= n || !keep[k]) return;
    const uint32_t c = pos[k];
    c_rank[c] = iv[k].rank;
    c_lo[c] = lo[k];
    c_hi[c] = hi[k];
}

/* per kept interval: does it open an item, does it close one (c_max: the inclusive maximum of c_hi over the kept intervals of its name) */
__global__ __launch_bounds__(FA_NT) void k_bed_heads(const uint32_t *c_rank, const int64_t *c_lo, const int64_t *c_max, int64_t m, const int64_t *name_rec,
                                                    const FaRec *recs, BedRun *run) {
    const int64_t c = (int64_t)blockIdx.x * FA_NT + threadIdx.x;
    if (c >= m) return;
    const uint32_t rank = c_rank[c];
    const bool head = c == 0 || c_rank[c - 1] != rank || c_max[c - 1] < c_lo[c];
    const bool last = c + 1 == m || c_rank[c + 1] != rank || c_max[c] < c_lo[c + 1];
    BedRun r;
    r.bytes = 0;
    r.start = 0;
    r.items = last ? 1u : 0u;
    r.has_start = head ? 1u : 0u;
    if (head) {
        const FaRec rec = recs[name_rec[rank]];
        r.start = c_lo[c];
        r.bytes = (int64_t)fa_header_len(0, (int32_t)rec.hdr_len, rec.seq_len, r.start) - r.start + 1;
    }
    if (last) r.bytes += c_max[c];
    run[c] = r;
}

/* one item per interval that closes one (scan: the inclusive scan of run) */
__global__ __launch_bounds__(FA_NT) void k_bed_items(const uint32_t *c_rank, const int64_t *c_lo, const int64_t *c_max, int64_t m, const int64_t *name_rec,
                                                     const FaRec *recs, const BedRun *scan, FaItem *items) {
    const int64_t c = (int64_t)blockIdx.x * FA_NT + threadIdx.x;
    if (c >= m) return;
    const uint32_t rank = c_rank[c];
    const bool last = c + 1 == m || c_rank[c + 1] != rank || c_max[c] < c_lo[c + 1];
    if (!last) return;
    const BedRun s = scan[c];
    const FaRec rec = recs[name_rec[rank]];
    const int64_t p_start = s.start, p_end = c_max[c];
    FaItem it;
    it.name_off = rec.hdr_off;
    it.name_len = (int32_t)rec.hdr_len;
    it.num1 = rec.seq_len;
    it.num2 = p_start;
    it.src_off = rec.seq_off + p_start;
    it.src_len = p_end - p_start;
    it.kind = 0;
    it.check = 1;
    it.hdr_len = fa_header_len(0, it.name_len, it.num1, it.num2);
    it.out_off = s.bytes - (it.hdr_len + it.src_len + 1);
    items[s.items - 1u] = it;
}

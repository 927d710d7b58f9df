/*
 * view_line_kernel.h -- the stats line of paf_pretty_print (impl/paf.c:269-281), the line `paffy view` writes per record, as text in
 * device memory:
 *
 *   Query:<name>\tQ-start:<qs>\tQ-length:<qe - qs>\tTarget:<name>\tT-start:<ts>\tT-length:<te - ts>\tSame-strand:<0|1>\tScore:<AS>
 *   \tIdentity:<%f>\tIdentity-with-gaps<%f>\tAligned-bases:<s0 + s1>\tQuery-inserts:<s2>\tQuery-deletes:<s3>\n
 *
 * Nothing is parsed again: the fields are the header states k_header left in RecMeta (the record as it was read -- the stage list of
 * `view`, [ADD_MISMATCHES, STATS], changes none of them), the names are slices of the batch text, s0..s5 are rec_stats[6 rec] of the
 * PAFFY_STATS stage. So both kernels work after a default plan and after a sums-only plan (flat_view_kernel.h), which has no RecPlan.
 *
 *   k_view_line_size   one lane per record: the bytes of its line (added to what is there already: the bytes of its rows)
 *   k_view_line_emit   one wave per record, an item per lane as build_header does it: lane k turns label k and its value into text, a
 *                      wave scan places the items in three 16-byte aligned stretches of LDS (in front of the query name, between the
 *                      names, behind the target name), which go out 16 bytes per lane; the names are copied 16 bytes per lane from the
 *                      batch text. A stretch's last n % 16 bytes are single-byte stores of that many lanes: no store reaches outside
 *                      [off[i], off[i + 1]), whose neighbours other waves -- or, behind the last one, the caller -- own.
 *
 * The two %f fields are the reference's float arithmetic as glibc prints it. (float)a / b is a float division of (float)a by
 * (float)b: both conversions round to nearest even (__ll2float_rn), the quotient is correctly rounded (__fdiv_rn). a <= b, so the
 * quotient q lies in [0, 1], or b == 0 (then a == 0) and it is the NaN of 0.0f / 0.0f, which x86-64 glibc prints as "-nan".
 * (double)q * 1e6 is exact (24 bits times 20 bits), %f rounds the exact value to six decimals with ties to even, so the text is
 * n = __double2ll_rn(q * 1e6) printed as n / 10^6, '.', and the six digits of n % 10^6; n == 10^6 gives "1.000000".
 *
 * The emit kernel trusts no offset: a record whose off[i + 1] - off[i] is not the size of its block writes nothing and raises *bad.
 *
 * The layout of a whole batch stays on the device (paffy_hip_plan_view_layout): the blocks' sizes, their n + 1 running sums, and the
 * ranges of records the text is fetched in.
 *
 *   k_view_range_cut      one wave: the batch's records cut into ranges of at most range_bytes of text, greedily from record 0 (a range
 *                         takes records while the sum stays within range_bytes, and one record at least). The ranges depend on each
 *                         other in turn, so the wave walks them; what it searches is the end of each -- the last offset within
 *                         off[first] + range_bytes -- with 64 probes per step (a ballot gives the stretch to search next: three
 *                         steps for 200 000 records). It writes {first record, first byte} per range and the closing {n, total}.
 *   k_view_range_verdict  one lane behind the writers of a range: the rows' failure, the bytes the reference would have printed of the
 *                         range by then (every block in front of the failing record and that record's stats line) and *bad, in three
 *                         int64 the host reads with one copy -- after the next plan has replaced the offsets, if it likes.
 */
#ifndef PAFFY_VIEW_LINE_KERNEL_H_
#define PAFFY_VIEW_LINE_KERNEL_H_

#define VIEW_LINE_ITEMS 14u
#define VIEW_LINE_WAVES 4u
/* LDS per wave: "Query:" at 0, the items between the names at 16 (at most 9 + 20 + 10 + 20 + 8 = 67 bytes), the items behind the
   target name at 96 (at most 251 bytes) */
#define VIEW_LINE_SEG1 16u
#define VIEW_LINE_SEG2 96u
#define VIEW_LINE_LDS 352u

struct ViewLabel {
    uint64_t w[3]; /* the label's bytes, first byte lowest */
    uint32_t n, pad;
};
constexpr ViewLabel view_label(const char *s) {
    ViewLabel l = {{0, 0, 0}, 0, 0};
    for (; s[l.n]; l.n++) l.w[l.n >> 3] |= (uint64_t)(uint8_t)s[l.n] << (8 * (l.n & 7u));
    return l;
}
__device__ __constant__ ViewLabel VIEW_LABELS[VIEW_LINE_ITEMS] = {
    view_label("Query:"),           view_label("\tQ-start:"),       view_label("\tQ-length:"),      view_label("\tTarget:"),
    view_label("\tT-start:"),       view_label("\tT-length:"),      view_label("\tSame-strand:"),   view_label("\tScore:"),
    view_label("\tIdentity:"),      view_label("\tIdentity-with-gaps"), view_label("\tAligned-bases:"), view_label("\tQuery-inserts:"),
    view_label("\tQuery-deletes:"), view_label("\n")};
constexpr uint32_t view_labels_bytes() {
    const char *all[VIEW_LINE_ITEMS] = {"Query:", "\tQ-start:", "\tQ-length:", "\tTarget:", "\tT-start:", "\tT-length:", "\tSame-strand:", "\tScore:",
                                        "\tIdentity:", "\tIdentity-with-gaps", "\tAligned-bases:", "\tQuery-inserts:", "\tQuery-deletes:", "\n"};
    uint32_t n = 0;
    for (uint32_t k = 0; k < VIEW_LINE_ITEMS; k++) n += view_label(all[k]).n;
    return n;
}
static_assert(view_labels_bytes() == 147, "the labels of impl/paf.c:272-274");

struct ViewLineParams {
    const uint8_t *in;        /* the batch text */
    const RecMeta *meta;
    const int64_t *rec_stats; /* six sums per record */
    uint32_t first, count;    /* records [first, first + count) of the batch */
    /* k_view_line_emit */
    const int64_t *off;        /* count + 1: record first + i is written at out + off[i] - off_base */
    int64_t off_base;          /* 0, or the first byte of the range when off[] are the offsets of the whole batch */
    const int64_t *rows_bytes; /* with rows: the bytes of each record's rows (k_pretty_size); NULL without */
    int64_t *rows_off;         /* with rows: where k_pretty_rows writes them, off[i] + the line's bytes */
    uint8_t *out;
    int64_t out_cap;           /* bytes of out */
    uint32_t *bad;             /* raised by a record whose offsets are not its size or leave out */
};

/* six-decimal text of (float)a / b for 0 <= a <= b: n = the value in millionths, -1 for the NaN of b == 0 */
__device__ __forceinline__ int64_t view_ratio_micro(int64_t a, int64_t b) {
    if (b == 0) return -1;
    const float q = __fdiv_rn(__ll2float_rn((long long)a), __ll2float_rn((long long)b));
    return (int64_t)__double2ll_rn((double)q * 1e6);
}
__device__ __forceinline__ uint32_t view_ratio_len(int64_t n) { return n < 0 ? 4u : 8u; }
__device__ __forceinline__ uint64_t view_ratio_text(int64_t n) {
    if (n < 0) return (uint64_t)'-' | ((uint64_t)'n' << 8) | ((uint64_t)'a' << 16) | ((uint64_t)'n' << 24);
    const uint64_t g = ascii8((uint32_t)n); /* "0i" and the six decimals: n <= 10^6 */
    return (g & ~0xffffull) | ((g >> 8) & 0xffull) | ((uint64_t)'.' << 8);
}

struct ViewLineValues {
    int64_t v[VIEW_LINE_ITEMS]; /* the integer of item k; items 8 and 9: the ratio in millionths */
};
__device__ __forceinline__ void view_line_values(const RecMeta &m, const int64_t *s, ViewLineValues &x) {
    const int64_t aligned = s[0] + s[1];
    x.v[0] = 0; x.v[1] = m.qs; x.v[2] = m.qe - m.qs; x.v[3] = 0; x.v[4] = m.ts; x.v[5] = m.te - m.ts;
    x.v[6] = m.same_strand != 0 ? 1 : 0; x.v[7] = m.score;
    x.v[8] = view_ratio_micro(s[0], aligned);
    x.v[9] = view_ratio_micro(s[0], aligned + s[4] + s[5]);
    x.v[10] = aligned; x.v[11] = s[2]; x.v[12] = s[3]; x.v[13] = 0;
}

__global__ __launch_bounds__(256) void k_view_line_size(ViewLineParams P, int64_t *bytes, int add) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.count) return;
    const uint32_t rec = P.first + i;
    const RecMeta &m = P.meta[rec];
    ViewLineValues x;
    view_line_values(m, P.rec_stats + 6ull * rec, x);
    int64_t n = (int64_t)view_labels_bytes() + m.qname_len + m.tname_len + view_ratio_len(x.v[8]) + view_ratio_len(x.v[9]);
    n += dec_len(x.v[1]) + dec_len(x.v[2]) + dec_len(x.v[4]) + dec_len(x.v[5]) + dec_len(x.v[6]) + dec_len(x.v[7]) + dec_len(x.v[10]) +
         dec_len(x.v[11]) + dec_len(x.v[12]);
    bytes[i] = n + (add ? bytes[i] : 0);
}

/* n <= 256 bytes of a 16-byte aligned stretch of LDS to dst: whole 16 bytes by lanes 0.., the last n % 16 bytes one each by lanes 48.. */
__device__ __forceinline__ void view_copy_lds(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane) {
    const uint32_t full = n & ~15u;
    if (lane * 16u < full) *reinterpret_cast<u32x4_unaligned *>(dst + lane * 16u) = *reinterpret_cast<const u32x4 *>(src + lane * 16u);
    const uint32_t t = lane - 48u;
    if (lane >= 48u && t < n - full) dst[full + t] = src[full + t];
}
/* a name: 16 bytes per lane and step, the last n % 16 bytes one each */
__device__ __forceinline__ void view_copy_name(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane) {
    const uint32_t full = n & ~15u;
    for (uint32_t b = lane * 16u; b < full; b += 1024u)
        *reinterpret_cast<u32x4_unaligned *>(dst + b) = *reinterpret_cast<const u32x4_unaligned *>(src + b);
    if (lane < n - full) dst[full + lane] = src[full + lane];
}

__global__ __launch_bounds__(64 * VIEW_LINE_WAVES) void k_view_line_emit(ViewLineParams P) {
    __shared__ uint4 lds4[VIEW_LINE_WAVES * VIEW_LINE_LDS / 16u];
    const uint32_t lane = threadIdx.x & 63u, wave = uni(threadIdx.x >> 6);
    const uint32_t i = uni(blockIdx.x * VIEW_LINE_WAVES + wave);
    if (i >= P.count) return;
    const uint32_t rec = P.first + i;
    uint8_t *H = reinterpret_cast<uint8_t *>(lds4) + wave * VIEW_LINE_LDS;
    const RecMeta &m = P.meta[rec];
    ViewLineValues x;
    view_line_values(m, P.rec_stats + 6ull * rec, x);
    /* item `lane`: its label, then an integer (items 1, 2, 4-7, 10-12), a ratio (8, 9) or nothing (0, 3, 13) */
    const bool present = lane < VIEW_LINE_ITEMS;
    const uint32_t k = present ? lane : VIEW_LINE_ITEMS - 1u;
    const ViewLabel lab = VIEW_LABELS[k];
    int64_t val = 0;
#pragma unroll
    for (uint32_t j = 0; j < VIEW_LINE_ITEMS; j++)
        if (k == j) val = x.v[j];
    const bool ratio = k == 8u || k == 9u, numeric = !ratio && k != 0u && k != 3u && k != 13u;
    DecText d;
    dec_text(ratio ? 0 : val, d);
    const uint32_t vlen = numeric ? text_len(d) : (ratio ? view_ratio_len(val) : 0u);
    const uint32_t len = present ? lab.n + vlen : 0u;
    const uint32_t inc = wave_incl_scan_u32(len), ex = inc - len, total = wave_last_u32(inc);
    const uint32_t ex1 = (uint32_t)__builtin_amdgcn_readlane((int)ex, 1), ex4 = (uint32_t)__builtin_amdgcn_readlane((int)ex, 4);
    const uint32_t n0 = ex1, n1 = ex4 - ex1, n2 = total - ex4; /* the three stretches */
    const int64_t line = (int64_t)total + m.qname_len + m.tname_len;
    const int64_t at_out = P.off[i] - P.off_base;
    const int64_t want = line + (P.rows_bytes ? P.rows_bytes[i] : 0);
    if (P.rows_off && lane == 0) P.rows_off[i] = at_out + line;
    if (at_out < 0 || P.off[i + 1] - P.off_base - at_out != want || at_out + want > P.out_cap || n0 > VIEW_LINE_SEG1 || n1 > VIEW_LINE_SEG2 - VIEW_LINE_SEG1 || n2 > VIEW_LINE_LDS - VIEW_LINE_SEG2) {
        if (lane == 0) atomicOr(P.bad, 1u);
        return;
    }
    if (present) {
        uint32_t at = k == 0u ? 0u : (k < 4u ? VIEW_LINE_SEG1 + ex - ex1 : VIEW_LINE_SEG2 + ex - ex4);
        header_put(H, VIEW_LINE_LDS, at, lab.w[0], lab.n < 8u ? lab.n : 8u);
        if (lab.n > 8u) header_put(H, VIEW_LINE_LDS, at + 8u, lab.w[1], lab.n < 16u ? lab.n - 8u : 8u);
        if (lab.n > 16u) header_put(H, VIEW_LINE_LDS, at + 16u, lab.w[2], lab.n - 16u);
        at += lab.n;
        if (ratio) header_put(H, VIEW_LINE_LDS, at, view_ratio_text(val), vlen);
        if (numeric) {
            if (d.neg_separate) {
                header_put(H, VIEW_LINE_LDS, at, '-', 1);
                at += 1;
            }
            header_put(H, VIEW_LINE_LDS, at, d.top, d.ntop);
            at += d.ntop;
            if (d.groups == 2) {
                header_put(H, VIEW_LINE_LDS, at, ascii8(d.g1), 8);
                at += 8;
            }
            if (d.groups >= 1) header_put(H, VIEW_LINE_LDS, at, ascii8(d.g0), 8);
        }
    }
    __builtin_amdgcn_wave_barrier(); /* a wave's LDS operations execute in order */
    uint8_t *o = P.out + at_out;
    view_copy_lds(o, H, n0, lane);
    o += n0;
    view_copy_name(o, P.in + m.qname_off, m.qname_len, lane);
    o += m.qname_len;
    view_copy_lds(o, H + VIEW_LINE_SEG1, n1, lane);
    o += n1;
    view_copy_name(o, P.in + m.tname_off, m.tname_len, lane);
    o += m.tname_len;
    view_copy_lds(o, H + VIEW_LINE_SEG2, n2, lane);
}

/* ---- the layout of a batch: ranges of records of at most range_bytes of text ---- */
struct ViewRange {
    int64_t rec, byte; /* the range's first record and the offset of its first byte in the batch's text */
};

/* off: n + 1 running sums (off[0] = 0). tab: room for cap + 1 entries; more ranges than cap leave *n_ranges = cap + 1 and no closing entry */
__global__ __launch_bounds__(64) void k_view_range_cut(const int64_t *off, uint32_t n, int64_t range_bytes, ViewRange *tab, uint32_t cap, uint32_t *n_ranges) {
    const uint32_t lane = threadIdx.x;
    uint32_t r = 0, first = 0;
    while (first < n) {
        if (r >= cap) {
            if (lane == 0) *n_ranges = cap + 1u;
            return;
        }
        const int64_t at = off[first], limit = at + range_bytes;
        if (lane == 0) {
            tab[r].rec = (int64_t)first;
            tab[r].byte = at;
        }
        /* the last end in [first + 1, n] with off[end] <= limit; first + 1 whatever its offset */
        uint32_t lo = first + 1u, hi = n;
        while (hi > lo) {
            const uint32_t step = (hi - lo + 63u) / 64u;
            const uint64_t probe = (uint64_t)lo + (uint64_t)(lane + 1u) * step;
            const uint32_t p = probe < hi ? (uint32_t)probe : hi;
            const uint32_t k = (uint32_t)__popcll(__ballot(off[p] <= limit)); /* the offsets only grow: the lanes that hold are the first k */
            const uint64_t nlo = (uint64_t)lo + (uint64_t)k * step, nhi = (uint64_t)lo + (uint64_t)(k + 1u) * step;
            const uint32_t lo2 = k == 0u ? lo : (nlo < hi ? (uint32_t)nlo : hi);
            hi = k == 64u ? lo2 : (nhi < hi ? (uint32_t)nhi : hi) - 1u;
            lo = lo2;
        }
        first = lo;
        r++;
    }
    if (lane == 0) {
        tab[r].rec = (int64_t)n;
        tab[r].byte = off[n];
        *n_ranges = r;
    }
}

/* verdict[0]: the rows' failure (record << 8 | code; -1 none), [1]: the bytes of the range the reference would have printed before it
   (-1 none), [2]: whether a record's offsets were refused */
__global__ __launch_bounds__(64) void k_view_range_verdict(const unsigned long long *err, const uint32_t *bad, const int64_t *off, const int64_t *size,
                                                           const int64_t *rows_bytes, int64_t off_base, int64_t *verdict) {
    if (threadIdx.x != 0) return;
    const unsigned long long e = err ? *err : ~0ull;
    int64_t printed = -1;
    if (e != ~0ull) {
        const uint64_t rec = e >> 8;
        printed = off[rec] - off_base + size[rec] - rows_bytes[rec];
    }
    verdict[0] = (int64_t)e;
    verdict[1] = printed;
    verdict[2] = (int64_t)*bad;
}

#endif

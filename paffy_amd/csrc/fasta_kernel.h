/*
 * fasta_kernel.h -- `faffy chunk | extract | merge` on the device: the FASTA index and the item writer.
 *
 * Index. The text of one or more FASTA files lies back to back in HBM; starts[k] is the first byte of file k (starts[0] = 0).
 * What a byte is follows host/paffy_cmds.c:fasta_read, per file:
 *   - a line starts at the start of a file or after a '\n'; a line whose first byte is '>' is a header (a record starts there);
 *   - a line loses its trailing run of '\r' / '\n' bytes (a '\r' run that reaches the '\n' or the end of the file);
 *   - every other byte of a line that is not a header, ' ' or '\t' is a base of the current record, if the file has had a header
 *     before it (lines in front of a file's first header are dropped, they do not go to the record of the file before).
 * Three kernels with kernel boundaries between them: k_fa_count (per 64 KiB tile: the last line start, header start and file start
 * in the tile, the header count and the bases split by what they depend on in front of the tile), k_fa_scan (one workgroup: the
 * state in front of every tile, the record and base offset of every tile), k_fa_write (bases to the compact buffer, one entry per
 * header), then k_fa_records (header length, sequence length per record). All positions and counts are 64-bit.
 *
 * Items. An item is an optional header line, a slice of the compact bases and '\n'. k_fa_emit gives every wave 4 KiB of the output:
 * it finds its first item by binary search on the items' output offsets, builds the window in LDS (bases realigned with alignbyte,
 * 16 bytes per lane) and stores it with 16-byte stores. The base check of chunk and extract is fused: the first item with a byte
 * whose tolower() is not one of a, c, g, t, n is kept by an atomic min.
 */
#pragma once

#define FA_NT 256u                    /* threads per workgroup of the index kernels */
#define FA_PER 256u                   /* bytes per thread */
#define FA_TILE (FA_NT * FA_PER)      /* 64 KiB per workgroup */
#define FA_WIN 4096u                  /* output bytes per wave of k_fa_emit */
#define FA_EMIT_WAVES 4u

/* per tile: after k_fa_count the tile's own summary; k_fa_scan turns ls / h / fs into the state in front of the tile and fills
   rec_base / seq_base */
struct FaTile {
    int64_t ls, h, fs;      /* last line start / header start / file start (absolute positions; -1: none) */
    int64_t n_h;            /* header starts in the tile */
    int64_t c_a, c_dep, c_loc; /* bases before the tile's first line start; bases that depend on the file having had a header; the rest */
    int64_t rec_base, seq_base;
};

/* one record of the index (include/paffy_hip.h paffy_fasta_record) */
struct FaRec {
    int64_t hdr_off, hdr_len, seq_off, seq_len;
};

/* one item of the output (chunk, merge: planned on the host, fasta_host.h; extract: written by k_bed_items, fasta_extract_kernel.h) */
struct FaItem {
    int64_t out_off;          /* first output byte */
    int64_t name_off;         /* header name: a slice of the text */
    int64_t num1, num2;       /* kind 0: ">name|num1|num2\n" */
    int64_t src_off, src_len; /* slice of the compact bases */
    int32_t name_len;
    int32_t kind;             /* 0: ">name|num1|num2\n", 1: ">name\n", 2: no header line */
    int32_t check;            /* base check */
    int32_t hdr_len;          /* bytes of the header line, '>' and '\n' included */
};

/* the layout of a written record (parity unpinned): '>' + header + '\n' + all the bases on one line + '\n' */
__host__ __device__ inline int32_t fa_digits(int64_t v) { /* v >= 0 */
    int32_t n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}
__host__ __device__ inline int32_t fa_header_len(int32_t kind, int32_t name_len, int64_t num1, int64_t num2) {
    if (kind == 2) return 0;
    if (kind == 1) return name_len + 2;
    return name_len + 4 + fa_digits(num1) + fa_digits(num2);
}

/* tolower(c) is one of a, c, g, t, n (impl/fasta_chunk.c:94-97, impl/fasta_extract.c:40-43) */
__device__ __forceinline__ bool fa_base_ok(uint32_t c) {
    const uint32_t l = c | 0x20u; /* only 'A'..'Z' map onto 'a'..'z' this way among the bytes that can pass */
    return l == 'a' || l == 'c' || l == 'g' || l == 't' || l == 'n';
}
__device__ __forceinline__ bool fa_word_ok(uint32_t w) {
    return fa_base_ok(w & 0xffu) && fa_base_ok((w >> 8) & 0xffu) && fa_base_ok((w >> 16) & 0xffu) && fa_base_ok(w >> 24);
}

/* scan of one int64 per thread over a workgroup of FA_NT threads: wave shuffles, one LDS hop (lds: FA_NT / 64 slots); returns the
   exclusive scan, tot gets the total. MAX: running maximum with identity -1, else sum. (One value per call: arrays of values per
   thread ended up in scratch once the scans sat inside the tile loop of k_fa_scan.) */
template <bool MAX>
__device__ __forceinline__ int64_t fa_scan1(int64_t x, int64_t &tot, int64_t *lds) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int64_t id = MAX ? -1 : 0;
    int64_t inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc = MAX ? (o > inc ? o : inc) : inc + o;
    }
    const int64_t o = __shfl_up(inc, 1, 64);
    int64_t ex = lane ? o : id;
    if (lane == 63u) lds[wave] = inc;
    __syncthreads();
    int64_t pre = id, all = id;
#pragma unroll
    for (uint32_t j = 0; j < FA_NT / 64u; j++) {
        const int64_t y = lds[j];
        if (j < wave) pre = MAX ? (y > pre ? y : pre) : pre + y;
        all = MAX ? (y > all ? y : all) : all + y;
    }
    __syncthreads();
    tot = all;
    return MAX ? (pre > ex ? pre : ex) : pre + ex;
}

/* the state in front of a span: last line start, header start, file start (-1: none seen) */
struct FaState {
    int64_t ls, h, fs;
};

/* What the bases of a span depend on, given the state in front of it (-1 in `in`: not known inside this scope). Bases before the span's
   first line start (c_a) belong to the line of in.ls; bases of non-header lines before any header or file start of the span (c_dep) count
   when the file has had a header. Moves what `in` decides into c_loc (dropped bytes leave the counts). */
__device__ __forceinline__ void fa_resolve(const FaState in, int64_t &c_a, int64_t &c_dep, int64_t &c_loc) {
    /* selects, no conditional updates: those the compiler turns into stores through a chosen pointer, i.e. into scratch */
    const bool has_hdr = in.h >= 0 && in.h >= in.fs, a_known = in.ls >= 0, hdr_line = in.h == in.ls;
    const int64_t a_loc = a_known && !hdr_line && has_hdr ? c_a : 0;
    const int64_t a_dep = a_known && !hdr_line && !has_hdr && in.fs < 0 ? c_a : 0;
    const int64_t dep = c_dep + a_dep;
    c_loc += a_loc + (has_hdr ? dep : 0);
    c_dep = has_hdr || in.fs >= 0 ? 0 : dep;
    c_a = a_known ? 0 : c_a;
}

/* largest k with starts[k] <= p (starts[0] = 0, non-decreasing) */
__device__ __forceinline__ int32_t fa_file_of(const int64_t *starts, int32_t n, int64_t p) {
    int32_t lo = 0, hi = n; /* starts[lo] <= p < starts[hi] */
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (starts[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* Does a '\r' run that reaches q end its line? Yes when the bytes from q on are '\r' up to a '\n' or the end of the file (fe). */
__device__ __forceinline__ bool fa_eol_after(const uint8_t *in, int64_t q, int64_t fe) {
    while (q < fe && in[q] == '\r') q++;
    return q >= fe || in[q] == '\n';
}

/*
 * One thread's span [g0, g0 + FA_PER), byte by byte. WRITE = false: the span's summary (last ls / h / fs, header count, bases by
 * class relative to the span's own start). WRITE = true: with the full state in front of the span, the bases go to `dst` (LDS, from
 * dst_at on) and every header start to the record table. The '\r' runs are held back until the byte after them shows whether they end
 * the line.
 */
template <bool WRITE>
__device__ __forceinline__ void fa_span(const uint8_t *in, int64_t len, const int64_t *starts, int32_t n_files, int64_t g0, FaState &st,
                                        int64_t &n_h, int64_t &c_a, int64_t &c_dep, int64_t &c_loc, uint8_t *dst, uint32_t dst_at,
                                        FaRec *recs, int64_t rec_at, int64_t seq_at) {
    const int64_t end = g0 + (int64_t)FA_PER < len ? g0 + (int64_t)FA_PER : len;
    if (g0 >= end) return;
    int32_t fk = fa_file_of(starts, n_files, g0);
    int64_t next_fs = fk + 1 < n_files ? starts[fk + 1] : INT64_MAX;
    const bool fs_at_g0 = starts[fk] == g0;
    bool prev_nl = g0 > 0 && in[g0 - 1] == '\n';
    /* the line state inside the span: cls = 0 before the span's first line start (class a), then by the line and the header */
    bool seen_ls = false, hdr_line = false, local_hdr = false, local_fs = false;
    bool w_hdr_line = WRITE && st.ls >= 0 && st.h == st.ls;
    bool w_has_hdr = WRITE && st.h >= 0 && st.h >= st.fs;
    int64_t cr_run = 0; /* '\r' bytes held back */
    int cr_cls = 0;     /* their class: 0 a, 1 dep, 2 loc, 3 dropped */
    uint32_t wpos = dst_at;
    for (int64_t q0 = g0; q0 < end; q0 += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + q0);
        for (int j = 0; j < 16; j++) {
            const int64_t p = q0 + j;
            if (p < end) {
                const uint32_t word = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w; /* no indexed register array: no scratch */
                const uint32_t b = (word >> (8 * (j & 3))) & 0xffu;
                bool is_fs = false;
                if (p == next_fs || (p == g0 && fs_at_g0)) {
                    is_fs = true;
                    if (p == next_fs) {
                        while (fk + 1 < n_files && starts[fk + 1] <= p) fk++;
                        next_fs = fk + 1 < n_files ? starts[fk + 1] : INT64_MAX;
                    }
                }
                const bool is_ls = is_fs || prev_nl;
                if (is_fs || b == '\n') cr_run = 0; /* a held '\r' run ends its line (the end of a file, or the '\n') */
                else if (b != '\r' && cr_run) {    /* ... or it was inside the line: its bytes count */
                    if (WRITE) {
                        if (cr_cls == 2)
                            for (int64_t k = 0; k < cr_run; k++) dst[wpos++] = '\r';
                    } else {
                        c_a += cr_cls == 0 ? cr_run : 0;
                        c_dep += cr_cls == 1 ? cr_run : 0;
                        c_loc += cr_cls == 2 ? cr_run : 0;
                    }
                    cr_run = 0;
                }
                if (is_fs) {
                    st.fs = p;
                    local_fs = true;
                    w_has_hdr = false;
                }
                if (is_ls) {
                    st.ls = p;
                    seen_ls = true;
                    hdr_line = b == '>';
                    w_hdr_line = hdr_line;
                    if (hdr_line) {
                        st.h = p;
                        local_hdr = true;
                        w_has_hdr = true;
                        if (WRITE) {
                            recs[rec_at + n_h].hdr_off = p + 1;
                            recs[rec_at + n_h].seq_off = seq_at + (int64_t)(wpos - dst_at);
                        }
                        n_h++;
                    }
                }
                prev_nl = b == '\n';
                if (b != '\n' && b != ' ' && b != '\t') {
                    int cls;
                    if (WRITE) cls = (!w_hdr_line && w_has_hdr) ? 2 : 3;
                    else if (!seen_ls) cls = 0;
                    else if (hdr_line) cls = 3;
                    else if (local_hdr && st.h >= (local_fs ? st.fs : -1)) cls = 2;
                    else if (local_fs) cls = 3;
                    else cls = 1;
                    if (b == '\r') {
                        cr_run++;
                        cr_cls = cls;
                    } else if (WRITE) {
                        if (cls == 2) dst[wpos++] = (uint8_t)b;
                    } else {
                        c_a += cls == 0;
                        c_dep += cls == 1;
                        c_loc += cls == 2;
                    }
                }
            }
        }
    }
    if (cr_run) { /* a run that reaches the end of the span: look past it */
        const int64_t fe = next_fs < len ? next_fs : len;
        if (!fa_eol_after(in, end, fe)) {
            if (WRITE) {
                if (cr_cls == 2)
                    for (int64_t k = 0; k < cr_run; k++) dst[wpos++] = '\r';
            } else {
                c_a += cr_cls == 0 ? cr_run : 0;
                c_dep += cr_cls == 1 ? cr_run : 0;
                c_loc += cr_cls == 2 ? cr_run : 0;
            }
        }
    }
}

__global__ __launch_bounds__(FA_NT) void k_fa_count(const uint8_t *in, int64_t len, const int64_t *starts, int32_t n_files, FaTile *tiles) {
    __shared__ int64_t lds[FA_NT / 64];
    const int64_t g0 = (int64_t)blockIdx.x * FA_TILE + (int64_t)threadIdx.x * FA_PER;
    FaState st = {-1, -1, -1};
    int64_t n_h = 0, c_a = 0, c_dep = 0, c_loc = 0;
    fa_span<false>(in, len, starts, n_files, g0, st, n_h, c_a, c_dep, c_loc, nullptr, 0, nullptr, 0, 0);
    int64_t mt[3], tot[4];
    FaState before; /* in front of this span, inside the tile */
    before.ls = fa_scan1<true>(st.ls, mt[0], lds);
    before.h = fa_scan1<true>(st.h, mt[1], lds);
    before.fs = fa_scan1<true>(st.fs, mt[2], lds);
    fa_resolve(before, c_a, c_dep, c_loc);
    (void)fa_scan1<false>(n_h, tot[0], lds);
    (void)fa_scan1<false>(c_a, tot[1], lds);
    (void)fa_scan1<false>(c_dep, tot[2], lds);
    (void)fa_scan1<false>(c_loc, tot[3], lds);
    if (threadIdx.x == 0) {
        FaTile t;
        t.ls = mt[0];
        t.h = mt[1];
        t.fs = mt[2];
        t.n_h = tot[0];
        t.c_a = tot[1];
        t.c_dep = tot[2];
        t.c_loc = tot[3];
        t.rec_base = t.seq_base = 0;
        tiles[blockIdx.x] = t;
    }
}

/* one workgroup: the state in front of every tile (running maxima), its first record and first base; totals[0..1] = records, bases */
__global__ __launch_bounds__(FA_NT) void k_fa_scan(FaTile *tiles, uint32_t n_tiles, int64_t *totals) {
    __shared__ int64_t lds[FA_NT / 64];
    int64_t cls = -1, ch = -1, cfs = -1, crec = 0, cseq = 0; /* what the tiles before this round hold */
    for (uint32_t base = 0; base < n_tiles; base += FA_NT) {
        const uint32_t i = base + threadIdx.x;
        const bool in = i < n_tiles;
        int64_t m0 = -1, m1 = -1, m2 = -1, t0, t1, t2, c_a = 0, c_dep = 0, c_loc = 0, n_h = 0;
        if (in) {
            m0 = tiles[i].ls;
            m1 = tiles[i].h;
            m2 = tiles[i].fs;
            n_h = tiles[i].n_h;
            c_a = tiles[i].c_a;
            c_dep = tiles[i].c_dep;
            c_loc = tiles[i].c_loc;
        }
        m0 = fa_scan1<true>(m0, t0, lds);
        m1 = fa_scan1<true>(m1, t1, lds);
        m2 = fa_scan1<true>(m2, t2, lds);
        FaState before;
        before.ls = m0 > cls ? m0 : cls;
        before.h = m1 > ch ? m1 : ch;
        before.fs = m2 > cfs ? m2 : cfs;
        fa_resolve(before, c_a, c_dep, c_loc); /* what is still open now depends on nothing before the text: dropped */
        int64_t s0, s1, u0, u1;
        s0 = fa_scan1<false>(n_h, u0, lds);
        s1 = fa_scan1<false>(c_loc, u1, lds);
        if (in) {
            tiles[i].ls = before.ls;
            tiles[i].h = before.h;
            tiles[i].fs = before.fs;
            tiles[i].rec_base = crec + s0;
            tiles[i].seq_base = cseq + s1;
        }
        cls = t0 > cls ? t0 : cls;
        ch = t1 > ch ? t1 : ch;
        cfs = t2 > cfs ? t2 : cfs;
        crec += u0;
        cseq += u1;
    }
    if (threadIdx.x == 0) {
        totals[0] = crec;
        totals[1] = cseq;
    }
}

/* bases of a tile to the compact buffer (staged in LDS, stored with 16-byte stores where no other tile writes), record starts; bases =
   nullptr: record starts only */
__global__ __launch_bounds__(FA_NT) void k_fa_write(const uint8_t *in, int64_t len, const int64_t *starts, int32_t n_files, const FaTile *tiles,
                                                    uint8_t *bases, FaRec *recs) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[FA_TILE];
    __shared__ int64_t lds[FA_NT / 64];
    const FaTile t = tiles[blockIdx.x];
    const int64_t g0 = (int64_t)blockIdx.x * FA_TILE + (int64_t)threadIdx.x * FA_PER;
    FaState st = {-1, -1, -1};
    int64_t n_h = 0, c_a = 0, c_dep = 0, c_loc = 0;
    fa_span<false>(in, len, starts, n_files, g0, st, n_h, c_a, c_dep, c_loc, nullptr, 0, nullptr, 0, 0);
    int64_t t0, n_loc;
    const int64_t m0 = fa_scan1<true>(st.ls, t0, lds), m1 = fa_scan1<true>(st.h, t0, lds), m2 = fa_scan1<true>(st.fs, t0, lds);
    const FaState before = {m0 > t.ls ? m0 : t.ls, m1 > t.h ? m1 : t.h, m2 > t.fs ? m2 : t.fs};
    fa_resolve(before, c_a, c_dep, c_loc);
    const int64_t s0 = fa_scan1<false>(n_h, t0, lds), s1 = fa_scan1<false>(c_loc, n_loc, lds);
    FaState w = before;
    int64_t n_h2 = 0, x_a = 0, x_dep = 0, x_loc = 0;
    fa_span<true>(in, len, starts, n_files, g0, w, n_h2, x_a, x_dep, x_loc, stage, (uint32_t)s1, recs, t.rec_base + s0, t.seq_base + s1);
    __syncthreads();
    if (!bases) return; /* record starts only (every thread of the workgroup leaves here) */
    /* the tile's bases are [seq_base, seq_base + n): 16-byte stores inside, bytes at the two ends (shared with the neighbours) */
    const int64_t d0 = t.seq_base, d1 = d0 + n_loc;
    const int64_t a0 = (d0 + 15) & ~(int64_t)15, a1 = d1 & ~(int64_t)15;
    if (a0 < a1) {
        for (int64_t d = a0 + 16 * (int64_t)threadIdx.x; d < a1; d += 16 * (int64_t)FA_NT) {
            const uint32_t o = (uint32_t)(d - d0);
            uint32_t x[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                x[k] = (uint32_t)stage[o + 4 * k] | ((uint32_t)stage[o + 4 * k + 1] << 8) | ((uint32_t)stage[o + 4 * k + 2] << 16) |
                       ((uint32_t)stage[o + 4 * k + 3] << 24);
            *reinterpret_cast<uint4 *>(bases + d) = make_uint4(x[0], x[1], x[2], x[3]);
        }
        for (int64_t d = d0 + threadIdx.x; d < a0; d += FA_NT) bases[d] = stage[d - d0];
        for (int64_t d = a1 + threadIdx.x; d < d1; d += FA_NT) bases[d] = stage[d - d0];
    } else {
        for (int64_t d = d0 + threadIdx.x; d < d1; d += FA_NT) bases[d] = stage[d - d0];
    }
}

/* per record: the header's length (its line, less the trailing '\r' run) and the sequence length */
__global__ __launch_bounds__(FA_NT) void k_fa_records(const uint8_t *in, int64_t len, const int64_t *starts, int32_t n_files, FaRec *recs,
                                                      int64_t n_rec, int64_t n_bases) {
    const int64_t r = (int64_t)blockIdx.x * FA_NT + threadIdx.x;
    if (r >= n_rec) return;
    const int64_t h = recs[r].hdr_off; /* the byte after '>' */
    const int32_t fk = fa_file_of(starts, n_files, h - 1);
    int64_t fe = fk + 1 < n_files ? starts[fk + 1] : len;
    if (fe > len) fe = len;
    int64_t e = h;
    while (e < fe && in[e] != '\n') e++;
    while (e > h && in[e - 1] == '\r') e--;
    recs[r].hdr_len = e - h;
    recs[r].seq_len = (r + 1 < n_rec ? recs[r + 1].seq_off : n_bases) - recs[r].seq_off;
}

/* the headers' bytes, one after the other (offsets from the host) */
__global__ __launch_bounds__(FA_NT) void k_fa_headers(const uint8_t *in, const FaRec *recs, int64_t n_rec, const int64_t *off, uint8_t *out) {
    const int64_t r = (int64_t)blockIdx.x * (FA_NT / 64) + (threadIdx.x >> 6);
    if (r >= n_rec) return;
    const int64_t h = recs[r].hdr_off, n = recs[r].hdr_len, o = off[r];
    for (int64_t k = threadIdx.x & 63u; k < n; k += 64) out[o + k] = in[h + k];
}

/* byte k of an item's header line */
__device__ __forceinline__ uint8_t fa_header_byte(const FaItem &it, const uint8_t *text, int32_t k) {
    if (k == 0) return '>';
    if (k <= it.name_len) return text[it.name_off + k - 1];
    k -= it.name_len + 1;
    if (it.kind == 1) return '\n';
    if (k == 0) return '|';
    k -= 1;
    const int32_t d1 = fa_digits(it.num1);
    int64_t v;
    int32_t nd;
    if (k < d1) {
        v = it.num1;
        nd = d1;
    } else {
        k -= d1;
        if (k == 0) return '|';
        k -= 1;
        nd = fa_digits(it.num2);
        if (k >= nd) return '\n';
        v = it.num2;
    }
    for (int32_t j = nd - 1; j > k; j--) v /= 10;
    return (uint8_t)('0' + v % 10);
}

/* 16 bases from src (any alignment): two aligned 16-byte loads, realigned with alignbyte; the buffer has 32 readable bytes past its end */
__device__ __forceinline__ uint4 fa_load16(const uint8_t *src, int64_t p) {
    const int64_t a = p & ~(int64_t)15;
    const uint32_t sh = (uint32_t)(p - a), k = sh >> 2, s = (sh & 3u) * 8u;
    const uint4 A = *reinterpret_cast<const uint4 *>(src + a), B = *reinterpret_cast<const uint4 *>(src + a + 16);
    const uint32_t w0 = A.x, w1 = A.y, w2 = A.z, w3 = A.w, w4 = B.x, w5 = B.y, w6 = B.z, w7 = B.w;
    /* the five words from word k on, picked without indexing (no scratch) */
    const uint32_t x0 = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3;
    const uint32_t x1 = k == 0 ? w1 : k == 1 ? w2 : k == 2 ? w3 : w4;
    const uint32_t x2 = k == 0 ? w2 : k == 1 ? w3 : k == 2 ? w4 : w5;
    const uint32_t x3 = k == 0 ? w3 : k == 1 ? w4 : k == 2 ? w5 : w6;
    const uint32_t x4 = k == 0 ? w4 : k == 1 ? w5 : k == 2 ? w6 : w7;
    if (s == 0) return make_uint4(x0, x1, x2, x3);
    return make_uint4(__builtin_amdgcn_alignbyte(x1, x0, s / 8u), __builtin_amdgcn_alignbyte(x2, x1, s / 8u),
                      __builtin_amdgcn_alignbyte(x3, x2, s / 8u), __builtin_amdgcn_alignbyte(x4, x3, s / 8u));
}

/* one wave per FA_WIN bytes of output; out has room up to the next multiple of 16 past out_len */
__global__ __launch_bounds__(64 * FA_EMIT_WAVES) void k_fa_emit(const FaItem *items, int64_t n_items, const uint8_t *text, const uint8_t *bases,
                                                                uint8_t *out, int64_t out_len, unsigned long long *bad) {
    __shared__ __attribute__((aligned(16))) uint8_t win[FA_EMIT_WAVES][FA_WIN];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint8_t *st = win[wv];
    const int64_t W0 = ((int64_t)blockIdx.x * FA_EMIT_WAVES + wv) * FA_WIN;
    const int64_t W1 = W0 + FA_WIN < out_len ? W0 + FA_WIN : out_len;
    if (W0 < out_len) {
        int64_t lo = 0, hi = n_items; /* items[lo].out_off <= W0 < items[hi].out_off */
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (items[mid].out_off <= W0) lo = mid;
            else hi = mid;
        }
        for (int64_t i = lo; i < n_items; i++) {
            const FaItem it = items[i];
            if (it.out_off >= W1) break;
            const int64_t a = it.out_off, sa = a + it.hdr_len, sb = sa + it.src_len;
            /* header line */
            for (int64_t q = (a > W0 ? a : W0) + lane; q < (sa < W1 ? sa : W1); q += 64) st[q - W0] = fa_header_byte(it, text, (int32_t)(q - a));
            /* bases */
            const int64_t s0 = sa > W0 ? sa : W0, s1 = sb < W1 ? sb : W1;
            bool ok = true;
            if (s0 < s1) {
                const int64_t c0 = (s0 - W0) & ~(int64_t)15;
                for (int64_t c = c0 + 16 * lane; c < s1 - W0; c += 16 * 64) {
                    const int64_t q0 = W0 + c;
                    if (q0 >= s0 && q0 + 16 <= s1) {
                        const uint4 v = fa_load16(bases, it.src_off + (q0 - sa));
                        if (it.check) ok = ok && fa_word_ok(v.x) && fa_word_ok(v.y) && fa_word_ok(v.z) && fa_word_ok(v.w);
                        *reinterpret_cast<uint4 *>(st + c) = v;
                    } else {
                        for (int64_t q = q0 > s0 ? q0 : s0; q < (q0 + 16 < s1 ? q0 + 16 : s1); q++) {
                            const uint8_t b = bases[it.src_off + (q - sa)];
                            if (it.check) ok = ok && fa_base_ok(b);
                            st[q - W0] = b;
                        }
                    }
                }
            }
            if (!ok) atomicMin(bad, (unsigned long long)i);
            if (lane == 0 && sb >= W0 && sb < W1) st[sb - W0] = '\n';
        }
    }
    __syncthreads();
    if (W0 < out_len) {
        for (int64_t c = 16 * lane; W0 + c < W1; c += 16 * 64) *reinterpret_cast<uint4 *>(out + W0 + c) = *reinterpret_cast<const uint4 *>(st + c);
    }
}

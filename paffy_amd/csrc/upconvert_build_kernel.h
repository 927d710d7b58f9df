/*
 * upconvert_build_kernel.h -- the interval table of `paffy upconvert` (UpInterval, up_search) built on the device from a FASTA index
 * (DESIGN §3.4). It is what paffy_hip_set_intervals makes of the same headers and sequence lengths on the host.
 *
 * Header. Record r's header is its text up to the first NUL byte (the host path sees a C string; the name sort's key has the same rule).
 * decode_fasta_header (impl/paf.c:716-731) as dechunk_side restates it: the last '|'-token is the start, the one before it the length,
 * both read by scan_li_dev; the name is the text in front of the second-to-last '|', empty when there are two tokens only.
 *
 *   k_up_decode  one lane per record: name length, start, length, end = start + sequence length (wrapping). A header of one token, or a
 *                token that converts nothing, fails: its name length is UP_BAD and the one word `failed` is set.
 *   (host)       the name sort (name_sort_host.h) with the name lengths as key lengths: unsigned bytes, then the shorter first, which
 *                is strcmp because names hold no NUL; then k_up_gather and two stable radix sorts, by start (signed) and by the name's
 *                index, so that equal (name, start) keep input order, as glibc's merge-sort qsort gives the host path.
 *   k_up_lens    the bytes place k adds to the names blob: the name, then "name|length|start".
 *   k_up_table   after the exclusive sum of those: the UpInterval of place k and its bytes; the integers are printed here.
 */
#pragma once

#define UP_BAD NS_NONE

/* the characters "%lld" prints of v */
__device__ __forceinline__ uint32_t up_digits(int64_t v) {
    uint64_t m = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    uint32_t d = v < 0 ? 2u : 1u;
    while (m >= 10ull) {
        m /= 10ull;
        d++;
    }
    return d;
}

/* "%lld" of v at dst, d = up_digits(v) characters, written from the last digit back */
__device__ __forceinline__ void up_print(uint8_t *dst, int64_t v, uint32_t d) {
    uint64_t m = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    const uint32_t first = v < 0 ? 1u : 0u;
    if (first) dst[0] = '-';
    for (uint32_t i = d; i > first; i--) {
        dst[i - 1u] = (uint8_t)('0' + (uint32_t)(m % 10ull));
        m /= 10ull;
    }
}

__global__ __launch_bounds__(NS_NT) void k_up_decode(const FaRec *recs, const int64_t *hdr_off, const uint8_t *blob, uint32_t n, uint32_t *name_len,
                                                     int64_t *start, int64_t *length, int64_t *end, uint32_t *failed) {
    const uint32_t r = blockIdx.x * NS_NT + threadIdx.x;
    if (r >= n) return;
    const FaRec rec = recs[r];
    const uint8_t *h = blob + hdr_off[r];
    const int64_t hl = rec.hdr_len < (int64_t)NS_NONE ? rec.hdr_len : (int64_t)NS_NONE; /* a header of 4 GiB fails the blob's limit on the host */
    uint32_t e = 0;
    while ((int64_t)e < hl && h[e]) e++;
    uint32_t c1 = e, c2 = e; /* the last and the second-to-last '|' */
    for (uint32_t i = e; i > 0u; i--)
        if (h[i - 1u] == '|') {
            if (c1 == e) c1 = i - 1u;
            else {
                c2 = i - 1u;
                break;
            }
        }
    int64_t cs = 0, cl = 0;
    const bool ok = c1 != e && scan_li_dev(h, c1 + 1u, e, cs) && scan_li_dev(h, c2 == e ? 0u : c2 + 1u, c1, cl);
    name_len[r] = !ok ? UP_BAD : (c2 == e ? 0u : c2);
    start[r] = cs;
    length[r] = cl;
    end[r] = (int64_t)((uint64_t)cs + (uint64_t)rec.seq_len); /* i->start + strlen(sequence) */
    if (!ok) atomicOr(failed, 1u);
}

/* the first sort's input: the start of the record at place k of the names' order, and the place */
__global__ __launch_bounds__(NS_NT) void k_up_gather(uint32_t n, const uint32_t *ord, const int64_t *start, int64_t *key, uint32_t *idx) {
    const uint32_t k = blockIdx.x * NS_NT + threadIdx.x;
    if (k >= n) return;
    key[k] = start[ord[k]];
    idx[k] = k;
}

/* place[k]: the place in the names' order of the record that comes to place k of the table; len[n] = 0 */
__global__ __launch_bounds__(NS_NT) void k_up_lens(uint32_t n, const uint32_t *ord, const uint32_t *place, const uint32_t *name_len, const int64_t *start,
                                                   const int64_t *length, uint64_t *len) {
    const uint32_t k = blockIdx.x * NS_NT + threadIdx.x;
    if (k > n) return;
    uint64_t b = 0;
    if (k < n) {
        const uint32_t r = ord[place[k]];
        b = 2ull * name_len[r] + up_digits(length[r]) + up_digits(start[r]) + 2ull;
    }
    len[k] = b;
}

/* off: the exclusive sum of k_up_lens's bytes (the host has checked that the blob stays below 4 GiB) */
__global__ __launch_bounds__(NS_NT) void k_up_table(uint32_t n, const uint32_t *ord, const uint32_t *place, const uint32_t *name_len, const int64_t *start,
                                                    const int64_t *length, const int64_t *end, const int64_t *hdr_off, const uint8_t *blob,
                                                    const uint64_t *off, UpInterval *table, uint8_t *names) {
    const uint32_t k = blockIdx.x * NS_NT + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = ord[place[k]];
    const uint32_t nl = name_len[r];
    const int64_t s = start[r], l = length[r];
    const uint32_t dl = up_digits(l), ds = up_digits(s);
    const uint32_t o = (uint32_t)off[k];
    UpInterval t;
    t.start = s;
    t.end = end[r];
    t.length = l;
    t.name_off = o;
    t.name_len = nl;
    t.out_off = o + nl;
    t.out_len = nl + dl + ds + 2u;
    table[k] = t;
    const uint8_t *h = blob + hdr_off[r];
    uint8_t *a = names + o, *b = a + nl;
    for (uint32_t i = 0; i < nl; i++) {
        const uint8_t ch = h[i];
        a[i] = ch;
        b[i] = ch;
    }
    b += nl;
    b[0] = '|';
    up_print(b + 1u, l, dl);
    b += 1u + dl;
    b[0] = '|';
    up_print(b + 1u, s, ds);
}

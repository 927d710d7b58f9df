/*
 * seqload_kernel.h -- the sequence store of add_mismatches / view and the name query of to_bed -q, built from the device FASTA index
 * (fasta_kernel.h) instead of host strings.
 */
#pragma once

#define SL_GRID_MAX 2048u /* memory-bound: at most 8 workgroups per CU, grid-stride over the rest */

/*
 * The store in one pass over the index's compact bases, which become seq_blob in place: every 16-byte word is read once and written
 * upper-cased (seq), complemented (comp) and, with raw != nullptr, as it was (raw, for paf_pretty_print's rows). This is
 * seq_store_canon's device-to-device copy and k_seq_canon fused; the bytes are the same.
 */
__global__ __launch_bounds__(PAFFY_NT) void k_seq_store(uint8_t *seq, uint8_t *comp, uint8_t *raw, uint64_t n16) {
    const uint64_t stride = (uint64_t)gridDim.x * PAFFY_NT;
    for (uint64_t i = (uint64_t)blockIdx.x * PAFFY_NT + threadIdx.x; i < n16; i += stride) {
        uint4 w = reinterpret_cast<const uint4 *>(seq)[i];
        if (raw) reinterpret_cast<uint4 *>(raw)[i] = w;
        w.x = upper4(w.x); w.y = upper4(w.y); w.z = upper4(w.z); w.w = upper4(w.w);
        reinterpret_cast<uint4 *>(seq)[i] = w;
        w.x = comp4(w.x); w.y = comp4(w.y); w.z = comp4(w.z); w.w = comp4(w.w);
        reinterpret_cast<uint4 *>(comp)[i] = w;
    }
}

/* the end of the field that starts at q: the next '\t' (returned) or -1 when the line or the text ends first */
__device__ __forceinline__ int64_t sl_next_tab(const uint8_t *paf, int64_t len, int64_t q) {
    while (q < len && paf[q] != '\t' && paf[q] != '\n') q++;
    return q < len && paf[q] == '\t' ? q : -1;
}

/* a field that names a FASTA record marks that name (names: the distinct names, sorted as find_seq expects) */
__device__ __forceinline__ void sl_mark(const uint8_t *paf, int64_t s, int64_t e, const uint8_t *names, const uint32_t *name_off, int32_t n_names,
                                        uint8_t *seen) {
    if (e - s > (int64_t)0xffffffffll) return; /* longer than any name can be */
    const int32_t k = find_seq(paf + s, 0, (uint32_t)(e - s), names, name_off, n_names);
    if (k >= 0) seen[k] = 1;
}

/* the names one PAF line gives: its query (the bytes before its first '\t') and, with with_target, its target (between its fifth and
   sixth '\t'); a line without that tab names nothing on that side (host/paffy_cmds.c's former scan) */
__device__ __forceinline__ void sl_line(const uint8_t *paf, int64_t len, int64_t s, int32_t with_target, const uint8_t *names, const uint32_t *name_off,
                                        int32_t n_names, uint8_t *seen) {
    const int64_t t1 = sl_next_tab(paf, len, s);
    if (t1 < 0) return;
    sl_mark(paf, s, t1, names, name_off, n_names, seen);
    if (!with_target) return;
    int64_t t = t1;
    for (int col = 2; col <= 5 && t >= 0; col++) t = sl_next_tab(paf, len, t + 1);
    const int64_t t6 = t >= 0 ? sl_next_tab(paf, len, t + 1) : -1;
    if (t6 >= 0) sl_mark(paf, t + 1, t6, names, name_off, n_names, seen);
}

/* to_bed -q: one lookup per line. A thread owns the lines that start after a '\n' in its FA_PER bytes (thread 0 also the one at 0) and
   reads each only up to the tab it needs. */
__global__ __launch_bounds__(FA_NT) void k_fa_seen(const uint8_t *paf, int64_t len, int32_t with_target, const uint8_t *names, const uint32_t *name_off,
                                                   int32_t n_names, uint8_t *seen) {
    const int64_t g0 = ((int64_t)blockIdx.x * FA_NT + threadIdx.x) * FA_PER;
    if (g0 >= len) return;
    const int64_t g1 = g0 + (int64_t)FA_PER < len ? g0 + (int64_t)FA_PER : len;
    if (g0 == 0) sl_line(paf, len, 0, with_target, names, name_off, n_names, seen);
    for (int64_t p = g0; p < g1; p++)
        if (paf[p] == '\n' && p + 1 < len) sl_line(paf, len, p + 1, with_target, names, name_off, n_names, seen);
}

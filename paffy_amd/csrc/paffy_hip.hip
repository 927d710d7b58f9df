/*
 * paffy_hip.hip -- gfx950 implementation of include/paffy_hip.h.
 *
 * Kernels, in launch order for one batch of PAF text resident in HBM:
 *   k_sep_count / k_sep_write  one coalesced pass each over the bytes (16 B per lane): '\t' and
 *                              '\n' positions are compacted into sep_pos[], newline ranks into
 *                              nl_idx[] (replaces stFile_getLine + strtok_r, impl/paf.c:144-212)
 *   k_header                   one lane per record: fixed fields and tags (paf_parse, impl/paf.c:137-209)
 *   k_size_lds                 one workgroup per record: cigar -> LDS ops (mirrored to HBM) -> transforms -> exact size + plan
 *   k_arena_size               same for records whose ops do not fit LDS (ops in an HBM arena)
 *   k_scan_part / k_scan_fix   exclusive prefix sum of the sizes up to the first failing record (two levels)
 *   k_emit_lds<rows|line> / k_arena_emit   the lines: each wave formats its share of the record through its own
 *                              LDS ring and flushes 16-byte coalesced stores
 */
#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/paffy_hip.h"
#include "device_buffer.h"
#include "paf_synth_core.h"
#include "record_groups.h"
#include "flat_kernel.h"
#include "flat_add_kernel.h"
#include "flat_remove_kernel.h"
#include "flat_view_kernel.h"
#include "flat_add_pipe_kernel.h"
#include "coverage_kernel.h"
#include "bed_kernel.h"
#include "fasta_kernel.h"

#define SEP_TILE 65536u /* bytes per workgroup in the separator passes */
#define WAVE_OPS_CAP 2048u   /* op store of the one-wave sizing kernel: 8 KiB, sixteen workgroups per CU */
#define LVL0_LONG_BYTES 20000u /* cigars up to this length start at the first store level once a batch has shown that none of them overflows it */
#define WAVE_MAX_BYTES 6000u /* cigars up to this length go there (about 1950 ops at 3.08 bytes per op; the few denser ones are redone by the four-wave build) */

/* ------------------------------------------------------------------ */
/* separators                                                           */
/* ------------------------------------------------------------------ */

template <bool ND = false>
__device__ __forceinline__ void sep_masks(const uint8_t *in, uint32_t in_len, uint32_t g, uint32_t &tabs_nl, uint32_t &nl, uint32_t *nondigits = nullptr) {
    /* 16 bytes at g (multiple of 16): bit j of tabs_nl set for '\t' or '\n', of nl for '\n'; ND: *nondigits = bytes that are not ASCII digits
       (the flat sizing pass, flat_kernel.h, places a chunk's ops inside its record with the counts per 1 KiB tile) */
    tabs_nl = nl = 0;
    if (ND) *nondigits = 0;
    if (g >= in_len) return;
    uint4 v = *reinterpret_cast<const uint4 *>(in + g);
    if (ND) *nondigits = (uint32_t)__popc(nondigit16(v));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) { /* four bytes at a time: a byte equals the pattern where the xor has a zero byte */
        const uint32_t t = equal4(w[k], 0x09090909u), n = equal4(w[k], 0x0a0a0a0au);
        tabs_nl |= (t | n) << (4 * k);
        nl |= n << (4 * k);
    }
    if (in_len - g < 16u) { /* the text ends inside these 16 bytes */
        const uint32_t keep = (1u << (in_len - g)) - 1u;
        tabs_nl &= keep;
        nl &= keep;
    }
}

/*
 * The same masks and the non-digit count with fewer instructions (the one-pass index spends most of its time on them: 2 700 VALU
 * instructions per wave, two thirds of them here). Per 4-byte word: bytes 9 and 10 are the bytes b < 0x80 with ((b | 0x80) - 9) & 0xfe
 * == 0x80 -- one subtraction without borrows between the bytes, one zero-byte test -- and the newlines among them have bit 0 of the
 * difference set; the four flag bits of a word (bit 7 of each byte) are gathered by one multiplication; non-digit bytes are counted on
 * the flags themselves; the newline mask is only put together in the (few) rounds in which a lane of the wave has one.
 */
__device__ __forceinline__ void sep_masks_nd(const uint4 &v, uint32_t in_len, uint32_t g, uint32_t &tabs_nl, uint32_t &nl, uint32_t &nondigits) {
    /* v: the 16 bytes at g (a multiple of 16), loaded by the caller -- all the loads of a workgroup's tile are issued before the first is looked at */
    tabs_nl = nl = nondigits = 0;
    if (g >= in_len) return;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t nlf[4], any_nl = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        nondigits += (uint32_t)__popc(nondigit4(w[k]));
        const uint32_t u = (w[k] | 0x80808080u) - 0x09090909u;                       /* per byte: 0x80 for a tab, 0x81 for a newline; no borrows */
        const uint32_t z = ((u ^ 0x80808080u) & 0xfefefefeu) | (w[k] & 0x80808080u); /* zero byte <=> tab or newline */
        const uint32_t f = ~(((z & 0x7f7f7f7fu) + 0x7f7f7f7fu) | z) & 0x80808080u;   /* bit 7 of every zero byte */
        nlf[k] = f & (u << 7);
        any_nl |= nlf[k];
        tabs_nl |= ((f * 0x00204081u) >> 28) << (4 * k); /* bits 7, 15, 23, 31 -> 28 .. 31: the other partial products stay below bit 24 */
    }
    if (any_nl) {
#pragma unroll
        for (int k = 0; k < 4; k++) nl |= ((nlf[k] * 0x00204081u) >> 28) << (4 * k);
    }
    if (in_len - g < 16u) { /* the text ends inside these 16 bytes */
        const uint32_t keep = (1u << (in_len - g)) - 1u;
        tabs_nl &= keep;
        nl &= keep; /* (the non-digit count takes the 16 bytes as loaded, like sep_masks<true>: no cigar reaches beyond the text) */
    }
}

__global__ __launch_bounds__(PAFFY_NT) void k_sep_count(const uint8_t *in, uint32_t in_len, uint2 *tile_counts, uint16_t *nd) {
    __shared__ int64_t scratch_mem[2 * PAFFY_NWAVE * 4];
    BlockComm scratch{scratch_mem, 0};
    const uint32_t tile0 = blockIdx.x * SEP_TILE;
    int64_t acc[2] = {0, 0};
    for (uint32_t off = threadIdx.x * 16; off < SEP_TILE; off += PAFFY_NT * 16) {
        uint32_t a, b, c;
        uint4 txt = make_uint4(0, 0, 0, 0);
        if (tile0 + off < in_len) txt = *reinterpret_cast<const uint4 *>(in + tile0 + off);
        sep_masks_nd(txt, in_len, tile0 + off, a, b, c);
        acc[0] += __popc(a);
        acc[1] += __popc(b);
        c = wave_sum_u32(c); /* a wave's 64 x 16 bytes are one 1 KiB tile */
        if ((threadIdx.x & 63u) == 0 && nd && tile0 + off < in_len) nd[(tile0 + off) >> FLAT_TILE_SHIFT] = (uint16_t)c;
    }
    block_sum<2>(acc, scratch);
    if (threadIdx.x == 0) {
        /* a final line without '\n' still is a record (impl/paf.c:213): virtual newline at in_len */
        if (blockIdx.x == gridDim.x - 1 && in_len > 0 && in[in_len - 1] != '\n') {
            acc[0] += 1;
            acc[1] += 1;
        }
        tile_counts[blockIdx.x] = make_uint2((uint32_t)acc[0], (uint32_t)acc[1]);
    }
}

/* single workgroup: exclusive scan of the per-tile counts */
__global__ __launch_bounds__(PAFFY_NT) void k_scan_tiles(uint2 *tile_counts, uint32_t n_tiles, DevInfo *info) {
    __shared__ int64_t scratch_mem[2 * PAFFY_NWAVE * 4];
    BlockComm scratch{scratch_mem, 0};
    int64_t carry0 = 0, carry1 = 0;
    for (uint32_t base = 0; base < n_tiles; base += PAFFY_NT) {
        uint32_t i = base + threadIdx.x;
        uint2 c = i < n_tiles ? tile_counts[i] : make_uint2(0, 0);
        int64_t v[2] = {c.x, c.y}, tot[2];
        block_excl_scan<2>(v, tot, scratch);
        if (i < n_tiles) tile_counts[i] = make_uint2((uint32_t)(carry0 + v[0]), (uint32_t)(carry1 + v[1]));
        carry0 += tot[0];
        carry1 += tot[1];
    }
    if (threadIdx.x == 0) {
        info->n_seps = (uint32_t)carry0;
        info->n_lines = (uint32_t)carry1;
    }
}

__global__ __launch_bounds__(PAFFY_NT) void k_sep_write(const uint8_t *in, uint32_t in_len, const uint2 *tile_off, uint32_t *sep_pos,
                                                         uint32_t *nl_idx) {
    __shared__ int64_t scratch_mem[2 * PAFFY_NWAVE * 4];
    BlockComm scratch{scratch_mem, 0};
    /* tiles in reverse launch order: k_sep_count read the end of the text last, so it is the part most likely still in
       the Infinity Cache */
    const uint32_t tile = gridDim.x - 1 - blockIdx.x;
    const uint32_t tile0 = tile * SEP_TILE;
    uint2 base = tile_off[tile];
    uint32_t sbase = base.x, lbase = base.y;
    for (uint32_t off = threadIdx.x * 16; off < SEP_TILE; off += PAFFY_NT * 16) {
        uint32_t a, b;
        const uint32_t g = tile0 + off;
        sep_masks(in, in_len, g, a, b);
        uint32_t v[2] = {(uint32_t)__popc(a), (uint32_t)__popc(b)}, tot[2];
        block_excl_scan_u32<2>(v, tot, scratch);
        uint32_t si = sbase + v[0], li = lbase + v[1];
        while (a) {
            int j = __ffs((int)a) - 1;
            a &= a - 1;
            sep_pos[si] = g + j;
            if (b & (1u << j)) nl_idx[li++] = si;
            si++;
        }
        sbase += tot[0];
        lbase += tot[1];
    }
    if (threadIdx.x == 0 && tile == gridDim.x - 1 && in_len > 0 && in[in_len - 1] != '\n') {
        sep_pos[sbase] = in_len;
        nl_idx[lbase] = sbase;
    }
}

/*
 * The separator index in ONE pass over the text (round 3; k_sep_count / k_scan_tiles / k_sep_write above read it twice and are kept for
 * the first batch of a context, whose separator density is not known yet). A workgroup takes the next 64 KiB tile from a ticket
 * counter, keeps the tab / newline masks of its sixteen rounds in registers (two 16-bit masks per round and thread), turns the counts
 * into positions inside the tile with ONE workgroup scan (the per-round counts are laid out in LDS in text order, every thread sums
 * sixteen consecutive entries; the two-pass version ran a workgroup scan per round), learns the number of separators and lines in
 * front of its tile by decoupled look-back over the tiles' published counts (a tile publishes its own counts at once and the running
 * totals as soon as it knows them; tiles are handed out in dispatch order, so a tile only ever waits for tiles that are running), and
 * writes the positions. Capacities are the caller's guess: nothing is written past them, the totals tell the host whether to repeat.
 */
#define SEP_AGG (1ull << 62)
#define SEP_INC (2ull << 62)
__device__ __forceinline__ unsigned long long sep_pack(uint32_t seps, uint32_t lines) { return (unsigned long long)seps | ((unsigned long long)lines << 31); }
__global__ __launch_bounds__(PAFFY_NT) void k_sep_index(const uint8_t *in, uint32_t in_len, uint32_t n_tiles, unsigned long long *state, uint32_t *sep_pos,
                                                         uint32_t cap_seps, uint32_t *nl_idx, uint32_t cap_lines, DevInfo *info, uint16_t *nd) {
    __shared__ int64_t scratch_mem[2 * PAFFY_NWAVE * 4];
    /* per round and thread, in text order (entry e = round * 256 + thread): separators | newlines << 16 -- first the counts, then the
       exclusive prefix inside the tile. One spare word per sixteen entries: a thread's sixteen consecutive entries are then 17 words from
       its neighbour's, not 16 (sixteen lanes on four banks) */
    __shared__ uint32_t pref[16 * PAFFY_NT + PAFFY_NT];
#define SEP_PREF(e) pref[(e) + ((e) >> 4)]
    __shared__ uint32_t s_tile, s_base[2];
    BlockComm scratch{scratch_mem, 0};
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_tile = atomicAdd(reinterpret_cast<unsigned int *>(state), 1u);
    __syncthreads();
    const uint32_t tile = s_tile, tile0 = tile * SEP_TILE;
    unsigned long long *status = state + 1;
    uint32_t m[16];
    uint4 txt[16]; /* the tile's sixteen loads in flight together: one at a time, each waited for, was most of the kernel's time */
#pragma unroll
    for (uint32_t it = 0; it < 16; it++) {
        const uint32_t g = tile0 + it * (PAFFY_NT * 16u) + tid * 16u;
        txt[it] = make_uint4(0, 0, 0, 0);
        if (g < in_len) txt[it] = *reinterpret_cast<const uint4 *>(in + g);
    }
#pragma unroll
    for (uint32_t it = 0; it < 16; it++) {
        uint32_t a, b, c;
        sep_masks_nd(txt[it], in_len, tile0 + it * (PAFFY_NT * 16u) + tid * 16u, a, b, c);
        c = wave_sum_u32(c); /* a wave's 64 x 16 bytes are one 1 KiB tile */
        if (lane == 0 && nd && tile0 + it * (PAFFY_NT * 16u) + tid * 16u < in_len) nd[(tile0 + it * (PAFFY_NT * 16u) + tid * 16u) >> FLAT_TILE_SHIFT] = (uint16_t)c;
        m[it] = a | (b << 16);
        SEP_PREF(it * PAFFY_NT + tid) = (uint32_t)__popc(a) | ((uint32_t)__popc(b) << 16);
    }
    __syncthreads();
    /* entries in text order: e = round * 256 + thread; this thread sums entries [16 tid, 16 tid + 16) (at most 256 per field: no carry) */
    uint32_t loc[16], run = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        loc[k] = run;
        run += pref[17u * tid + k]; /* = SEP_PREF(16 tid + k) */
    }
    uint32_t v[2] = {run & 0xffffu, run >> 16}, tot[2];
    block_excl_scan_u32<2>(v, tot, scratch);
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) pref[17u * tid + k] = (v[0] + (loc[k] & 0xffffu)) | ((v[1] + (loc[k] >> 16)) << 16); /* below 65 536 each */
    /* a final line without '\n' still is a record (impl/paf.c:213): virtual newline at in_len */
    const bool virt = tile == n_tiles - 1 && in_len > 0 && in[in_len - 1] != '\n';
    const uint32_t t_seps = tot[0] + (virt ? 1u : 0u), t_lines = tot[1] + (virt ? 1u : 0u);
    if (wave == 0) {
        uint32_t e_seps = 0, e_lines = 0;
        if (tile > 0) {
            if (lane == 0) __hip_atomic_store(&status[tile], SEP_AGG | sep_pack(t_seps, t_lines), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t look = (int64_t)tile - 1;
            for (;;) {
                const int64_t idx = look - (int64_t)lane;
                unsigned long long sv = SEP_INC; /* in front of tile 0: nothing */
                if (idx >= 0) sv = __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__any((sv >> 62) == 0)) continue; /* a tile in the window has not published yet: it is running, ask again */
                const unsigned long long inc = __ballot((sv >> 62) == 2);
                const uint32_t first = inc ? (uint32_t)__ffsll((long long)inc) - 1u : 63u; /* nearest tile that knows its running totals */
                const bool use = lane <= first;
                uint32_t a = use ? (uint32_t)(sv & 0x7fffffffull) : 0u, b = use ? (uint32_t)((sv >> 31) & 0x7fffffffull) : 0u;
                a = wave_last_u32(wave_incl_scan_u32(a));
                b = wave_last_u32(wave_incl_scan_u32(b));
                e_seps += a;
                e_lines += b;
                if (inc) break;
                look -= 64;
            }
        }
        if (lane == 0) {
            __hip_atomic_store(&status[tile], SEP_INC | sep_pack(e_seps + t_seps, e_lines + t_lines), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_base[0] = e_seps;
            s_base[1] = e_lines;
            if (tile == n_tiles - 1) {
                info->n_seps = e_seps + t_seps;
                info->n_lines = e_lines + t_lines;
            }
        }
    }
    __syncthreads();
    const uint32_t e_seps = s_base[0], e_lines = s_base[1];
#pragma unroll
    for (uint32_t it = 0; it < 16; it++) {
        uint32_t a = m[it] & 0xffffu;
        const uint32_t b = m[it] >> 16, g = tile0 + it * (PAFFY_NT * 16u) + tid * 16u, pp = SEP_PREF(it * PAFFY_NT + tid);
        uint32_t si = e_seps + (pp & 0xffffu), li = e_lines + (pp >> 16);
        while (a) {
            const int j = __ffs((int)a) - 1;
            a &= a - 1;
            if (si < cap_seps) sep_pos[si] = g + j;
            if (b & (1u << j)) {
                if (li < cap_lines) nl_idx[li] = si;
                li++;
            }
            si++;
        }
    }
    if (virt && tid == 0) {
        const uint32_t si = e_seps + tot[0], li = e_lines + tot[1];
        if (si < cap_seps) sep_pos[si] = in_len;
        if (li < cap_lines) nl_idx[li] = si;
    }
#undef SEP_PREF
}

/* ------------------------------------------------------------------ */
/* header fields                                                        */
/* ------------------------------------------------------------------ */

/* str_to_int64, impl/paf.c:37-48 */
__device__ int64_t parse_i64_dev(const uint8_t *in, uint32_t p, uint32_t e) {
    uint64_t v = 0;
    bool neg = false;
    if (p < e && in[p] == '-') {
        neg = true;
        p++;
    }
    while (p < e) {
        uint32_t d = (uint32_t)in[p] - '0';
        if (d > 9u) break;
        v = v * 10 + d;
        p++;
    }
    return (int64_t)(neg ? (uint64_t)0 - v : v);
}

/* the same for a token of at most 20 bytes with its text in registers: three aligned 8-byte words that hold bytes of the token are loaded at
   once (a word is only read when it starts in front of the token's end: nothing beyond the text is touched), where parse_i64_dev waits
   for one byte load per digit -- a line's twelve columns were most of k_header's time */
__device__ __forceinline__ int64_t parse_i64_words(const uint8_t *in, uint32_t p, uint32_t e) {
    if (e - p > 20u) return parse_i64_dev(in, p, e);
    const uintptr_t a = reinterpret_cast<uintptr_t>(in + p);
    const uint64_t *w = reinterpret_cast<const uint64_t *>(a & ~(uintptr_t)7);
    const uint32_t sh = (uint32_t)(a & 7u) * 8u, n = e - p;
    const uint32_t span = (uint32_t)(a & 7u) + n; /* bytes from the first word's start to the token's end: <= 27 */
    const uint64_t w0 = w[0], w1 = span > 8u ? w[1] : 0ull, w2 = span > 16u ? w[2] : 0ull, w3 = span > 24u ? w[3] : 0ull;
    uint64_t t[3];
    if (sh) {
        t[0] = (w0 >> sh) | (w1 << (64u - sh));
        t[1] = (w1 >> sh) | (w2 << (64u - sh));
        t[2] = (w2 >> sh) | (w3 << (64u - sh));
    } else {
        t[0] = w0; t[1] = w1; t[2] = w2;
    }
    uint64_t v = 0;
    uint32_t i = 0;
    const bool neg = (uint32_t)(t[0] & 0xffu) == (uint32_t)'-'; /* n >= 1: the token is not empty */
    if (neg) i = 1;
    for (; i < n; i++) {
        const uint64_t word = i < 8u ? t[0] : (i < 16u ? t[1] : t[2]);
        const uint32_t d = ((uint32_t)(word >> (8u * (i & 7u))) & 0xffu) - (uint32_t)'0';
        if (d > 9u) break;
        v = v * 10 + d;
    }
    return (int64_t)(neg ? (uint64_t)0 - v : v);
}

/*
 * paf_parse, impl/paf.c:137-209: tokens are the non-empty gaps between consecutive separators of
 * the line (strtok_r collapses runs of tabs). Tag tokens shorter than 5 bytes are never
 * recognised (documented deviation: the reference reads past the token there).
 *
 * 32 lanes per record, one separator (= one token) per lane and round: a token's field number is the count of non-empty tokens in
 * front of it (ballot + popcount), every lane parses its own token and drops the result into the record's RecMeta image in LDS, the
 * image leaves as 36 coalesced words. The reference stops at the first token it aborts on (strand, tp): tokens behind the first
 * failing one are ignored; of several tags of one kind the last one wins. (The one-lane-per-record version of rounds 1-2 needed 256
 * registers -- one wave per SIMD -- and 0.16 ms per 131 072 records.)
 */
#define HDR_GROUP 32u
__global__ __launch_bounds__(PAFFY_NT) void k_header(const uint8_t *in, const uint32_t *sep_pos, const uint32_t *nl_idx, uint32_t n_lines,
                                                      RecMeta *meta, uint32_t *big_list, DevInfo *info, uint32_t lvl0_max, uint32_t *chunk_rec) {
    constexpr uint32_t kWords = sizeof(RecMeta) / 4; /* 36 */
    static_assert(sizeof(RecMeta) % 4 == 0 && kWords > 32 && kWords <= 64, "the image is written as two words per lane at most");
    __shared__ __attribute__((aligned(16))) RecMeta image[PAFFY_NT / HDR_GROUP];
    const uint32_t g = threadIdx.x / HDR_GROUP, gl = threadIdx.x % HDR_GROUP;
    const uint32_t r = blockIdx.x * (PAFFY_NT / HDR_GROUP) + g;
    const bool live = r < n_lines;
    const uint32_t shift = (threadIdx.x & 32u); /* this group's half of the wave's 64-bit ballots */
    RecMeta *m = &image[g];
    uint32_t *mw = reinterpret_cast<uint32_t *>(m);
    mw[gl] = 0;
    if (gl + 32 < kWords) mw[32 + gl] = 0;
    __builtin_amdgcn_wave_barrier();
    if (gl == 0) {
        m->tile_level = -1;
        m->chain_id = -1;
        m->chain_score = -1;
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t s_end = 0, s_begin = 1;
    if (live) {
        s_end = nl_idx[r];
        s_begin = r == 0 ? 0 : nl_idx[r - 1] + 1;
    }
    uint32_t n_fields = 0; /* non-empty tokens taken so far (group-uniform) */
    int32_t err = 0;       /* group-uniform */
    for (uint32_t c = s_begin; c <= s_end && err == 0; c += HDR_GROUP) { /* s_end - s_begin < 2^31: no wrap */
        const uint32_t si = c + gl;
        const bool valid = live && si <= s_end && si >= c;
        uint32_t te = 0, t = 0;
        if (valid) {
            te = sep_pos[si];
            t = si == 0 ? 0u : sep_pos[si - 1] + 1u; /* the separator in front of a line's first token is the newline of the line before */
        }
        bool on = valid && te > t;
        const uint32_t ne = (uint32_t)(__ballot(on) >> shift);
        const uint32_t field = n_fields + (uint32_t)__popc(ne & ((1u << gl) - 1u));
        /* what this token is */
        int kind = -1; /* 0..5: tp AS cg tl cn s1 */
        int32_t my_err = 0, my_aux = 0;
        int64_t val = 0;
        uint32_t v_off = 0;
        uint8_t c0 = 0;
        if (on) {
            if (field < 12) {
                if (field == 4) {
                    c0 = in[t];
                    if (c0 != '+' && c0 != '-') {
                        my_err = PAFFY_ERR_STRAND;
                        my_aux = c0;
                    }
                } else if (field != 0 && field != 5) {
                    val = parse_i64_words(in, t, te);
                }
            } else if (te - t >= 5 && in[t + 2] == ':' && in[t + 4] == ':') {
                const uint8_t t0 = in[t], t1 = in[t + 1];
                v_off = t + 5;
                if (t0 == 't' && t1 == 'p') {
                    kind = 0;
                    c0 = v_off < te ? in[v_off] : 0;
                    if (c0 != 'P' && c0 != 'S' && c0 != 'I') {
                        my_err = PAFFY_ERR_TP_ASSERT;
                        my_aux = c0;
                    }
                } else if (t0 == 'A' && t1 == 'S') {
                    kind = 1;
                } else if (t0 == 'c' && t1 == 'g') {
                    kind = 2;
                } else if (t0 == 't' && t1 == 'l') {
                    kind = 3;
                } else if (t0 == 'c' && t1 == 'n') {
                    kind = 4;
                } else if (t0 == 's' && t1 == '1') {
                    kind = 5;
                }
                if ((kind == 1 || kind >= 3) && v_off < te) val = parse_i64_words(in, v_off, te);
            }
        }
        /* the reference never sees a token behind the first one it aborts on */
        const uint32_t em = (uint32_t)(__ballot(my_err != 0) >> shift);
        if (em) {
            const uint32_t first = (uint32_t)__ffs((int)em) - 1u;
            on = on && gl <= first;
            err = __shfl(my_err, (int)(first + shift), 64);
            const int32_t aux = __shfl(my_aux, (int)(first + shift), 64);
            if (gl == first) {
                m->err = err;
                m->err_aux = aux;
            }
        }
        const uint32_t taken = (uint32_t)(__ballot(on) >> shift);
        n_fields += (uint32_t)__popc(taken);
        if (on && field < 12) {
            switch (field) {
                case 0: m->qname_off = t; m->qname_len = te - t; break;
                case 4: m->same_strand = c0 == '+'; break;
                case 5: m->tname_off = t; m->tname_len = te - t; break;
                default: (&m->qlen)[field <= 3 ? field - 1 : field - 3] = val; break; /* qlen qs qe | tlen ts te nmatch nbases mapq */
            }
        }
        /* of several tags of one kind the last one wins: the highest lane writes */
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const uint32_t km = (uint32_t)(__ballot(on && kind == k) >> shift);
            if (km && gl == 31u - (uint32_t)__clz((int)km)) {
                if (k == 0) m->type = c0;
                else if (k == 1) m->score = val;
                else if (k == 2) { m->has_cg = 1; m->cg_off = v_off; m->cg_len = te - v_off; } /* impl/paf.c:193-198 */
                else if (k == 3) m->tile_level = val;
                else if (k == 4) m->chain_id = val;
                else m->chain_score = val;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (live && err == 0 && n_fields < 12) {
        err = PAFFY_ERR_FEW_FIELDS;
        if (gl == 0) m->err = err;
    }
    __builtin_amdgcn_wave_barrier();
    if (live) {
        uint32_t *dst = reinterpret_cast<uint32_t *>(meta + r);
        dst[gl] = mw[gl];
        if (gl + 32 < kWords) dst[32 + gl] = mw[32 + gl];
        /* long cigars go straight to the sizing launch with the bigger LDS store (runs beside the main one) */
        if (gl == 0 && err == 0 && (m->cg_len >> 1) > lvl0_max) big_list[atomicAdd(&info->b_count[0], 1u)] = r;
    }
    if (chunk_rec && live && err == 0 && m->has_cg && m->cg_len > 0) {
        /* the flat sizing pass (flat_kernel.h): the record's cigar is pieces (its text cut at the 1 KiB boundaries of the batch) and chunks of
           four pieces; chunk c of record r stands at slot (cg_off >> 12) + r + c of the chunk list (records are in text order: no two
           chunks share a slot, no scan or atomic hands the slots out) */
        const uint32_t tf = m->cg_off >> FLAT_TILE_SHIFT;
        const uint32_t np = ((m->cg_off + m->cg_len - 1u) >> FLAT_TILE_SHIFT) - tf + 1u;
        const uint32_t nc = (np + FLAT_CHUNK_PIECES - 1u) / FLAT_CHUNK_PIECES;
        for (uint32_t j = gl; j < nc; j += HDR_GROUP) chunk_rec[(tf >> 2) + r + j] = r;
    }
}

/* ------------------------------------------------------------------ */
/* dechunk (impl/paf_dechunk.c)                                         */
/* ------------------------------------------------------------------ */

/* sscanf(token, "%" PRIi64) of glibc x86-64 ("%li": strtol with base 0 on what the scanner took): white space, a sign, a 0x / 0X or 0
   prefix, the digits of the base; a value outside int64 saturates. false: nothing converted (the reference's assert) */
__device__ bool scan_li_dev(const uint8_t *in, uint32_t p, uint32_t e, int64_t &out) {
    while (p < e && (in[p] == ' ' || (in[p] >= 9 && in[p] <= 13))) p++;
    if (p == e) return false; /* sscanf's EOF */
    bool neg = false;
    if (in[p] == '+' || in[p] == '-') {
        neg = in[p] == '-';
        p++;
    }
    uint32_t base = 10;
    bool any = false; /* a digit (the 0 of a prefix counts) */
    if (p < e && in[p] == '0') {
        any = true;
        p++;
        if (p < e && (in[p] | 0x20u) == 'x') {
            base = 16;
            p++;
        } else {
            base = 8;
        }
    }
    uint64_t v = 0;
    bool over = false;
    for (; p < e; p++) {
        const uint32_t ch = in[p], lc = ch | 0x20u;
        uint32_t d;
        if (ch - '0' < 10u) d = ch - '0';
        else if (lc - 'a' < 6u) d = lc - 'a' + 10u;
        else break;
        if (d >= base) break;
        any = true;
        if (v > (~0ull - d) / base) over = true;
        else v = v * base + d;
    }
    if (!any) return false;
    if (neg) out = (over || v > (1ull << 63)) ? INT64_MIN : (int64_t)(0ull - v);
    else out = (over || v > (uint64_t)INT64_MAX) ? INT64_MAX : (int64_t)v;
    return true;
}

/* decode_fasta_header (impl/paf.c:716-731) of one name and the shift of impl/paf_dechunk.c:24-29: the last '|'-token is the chunk's start, the
   one before it the sequence length, the rest (joined by '|' again: the text in front of the second-to-last '|') the new name -- a prefix
   of the old one, so the record keeps addressing its name in the input text. The int64 sums wrap as the reference's do. */
__device__ bool dechunk_side(const uint8_t *in, uint32_t off, uint32_t &len, int64_t &start, int64_t &end, int64_t &length) {
    const uint32_t e = off + len;
    uint32_t c1 = e, c2 = e; /* the last and the second-to-last '|' */
    for (uint32_t i = e; i > off; i--)
        if (in[i - 1] == '|') {
            if (c1 == e) c1 = i - 1;
            else {
                c2 = i - 1;
                break;
            }
        }
    if (c1 == e) return false; /* one token: its start converts or not, the length then peeks an empty list */
    int64_t cs, cl;
    if (!scan_li_dev(in, c1 + 1, e, cs)) return false;
    if (!scan_li_dev(in, c2 == e ? off : c2 + 1, c1, cl)) return false;
    len = c2 == e ? 0u : c2 - off; /* two tokens: fastaEncodeHeader of an empty list */
    start = (int64_t)((uint64_t)start + (uint64_t)cs);
    end = (int64_t)((uint64_t)end + (uint64_t)cs);
    length = cl;
    return true;
}

/*
 * One lane per record, between k_header and the sizing kernels: the fixed sides' names and coordinates of RecMeta rewritten in place,
 * so that everything after (sizes, digit counts, the flat pass, the writers) sees the dechunked record. A name that does not decode is
 * PAFFY_ERR_DECHUNK_HEADER -- unless the cigar, which the reference parses while reading (impl/paf_dechunk.c:114), fails first.
 */
__global__ __launch_bounds__(PAFFY_NT) void k_dechunk(const uint8_t *in, RecMeta *meta, uint32_t n_lines, uint32_t fix_query, uint32_t fix_target) {
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n_lines) return;
    RecMeta &m = meta[r];
    if (m.err) return;
    bool ok = true;
    if (fix_query) ok = dechunk_side(in, m.qname_off, m.qname_len, m.qs, m.qe, m.qlen);
    if (ok && fix_target) ok = dechunk_side(in, m.tname_off, m.tname_len, m.ts, m.te, m.tlen);
    if (ok) return;
    int32_t err = PAFFY_ERR_DECHUNK_HEADER, aux = 0;
    if (m.has_cg && m.cg_len > 0) { /* cigar_parse, impl/paf.c:70-110: the first byte that is neither a digit nor an op; '\0' after digits */
        bool digit_last = false;
        for (uint32_t i = m.cg_off; i < m.cg_off + m.cg_len; i++) {
            const uint32_t ch = in[i];
            digit_last = ch - '0' < 10u;
            if (digit_last || ch == 'M' || ch == 'I' || ch == 'D' || ch == '=' || ch == 'X') continue;
            err = PAFFY_ERR_CIGAR_CHAR;
            aux = (int32_t)ch;
            break;
        }
        if (err != PAFFY_ERR_CIGAR_CHAR && digit_last) err = PAFFY_ERR_CIGAR_CHAR;
    }
    m.err = err;
    m.err_aux = aux;
}

/* ------------------------------------------------------------------ */
/* upconvert (impl/paf_upconvert.c)                                     */
/* ------------------------------------------------------------------ */

/* One interval of paffy_hip_set_intervals, in cmp_intervals order (impl/paf.c:733-737): name and output name "name|length|start" are
   slices of one blob. */
struct UpInterval {
    int64_t start, end, length;
    uint32_t name_off, name_len, out_off, out_len;
};

/* strcmp of the record's name slice with an interval's name, bytes unsigned; only the sign is used */
__device__ int up_strcmp(const uint8_t *a, uint32_t alen, const uint8_t *b, uint32_t blen) {
    for (uint32_t i = 0;; i++) {
        const uint32_t x = i < alen ? a[i] : 0u, y = i < blen ? b[i] : 0u;
        if (x != y) return x < y ? -1 : 1;
        if (x == 0) return 0;
    }
}

/* stList_binarySearch(intervals, side, cmp_overlapping_intervals) (impl/paf_upconvert.c:26-44): glibc's bsearch probes, key first --
   idx = (l + u) / 2, < 0: u = idx, > 0: l = idx + 1. The end of an interval is inclusive, so which of two adjacent intervals a start on
   their common end meets first is this probe order's. Returns the interval, -1 for none, -2 for the comparator's assert. */
__device__ int32_t up_search(const uint8_t *name, uint32_t name_len, int64_t start, int64_t end, const UpInterval *iv, uint32_t n_iv, const uint8_t *names) {
    uint32_t l = 0, u = n_iv;
    while (l < u) {
        const uint32_t idx = (l + u) / 2u;
        const UpInterval y = iv[idx];
        int k = up_strcmp(name, name_len, names + y.name_off, y.name_len);
        if (k == 0) {
            if (start < y.start) k = -1;
            else if (start <= y.end) return end <= y.end ? (int32_t)idx : -2;
            else k = 1;
        }
        if (k < 0) u = idx;
        else l = idx + 1u;
    }
    return -1;
}

/*
 * One lane per record, after k_header: fix_interval of the query, then of the target (impl/paf_upconvert.c:46-66, 150-151), and paf_check
 * on the coordinates (the cigar is not parsed: impl/paf_upconvert.c:148). A renamed side addresses its new name in the interval table's
 * output names (RecMeta::pad0 bit 0 / bit 1, read by k_line_emit). The first failure in stream order goes to DevInfo::first_err_key;
 * order / level are the line writer's (every record, in input order).
 */
__global__ __launch_bounds__(PAFFY_NT) void k_upconvert(const uint8_t *in, RecMeta *meta, uint32_t n_lines, const UpInterval *iv, uint32_t n_iv,
                                                        const uint8_t *names, uint32_t check, uint32_t *order, int64_t *level, DevInfo *info) {
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n_lines) return;
    RecMeta &m = meta[r];
    order[r] = r;
    level[r] = m.tile_level;
    int32_t code = m.err, stage = -1;
    if (!code) {
        stage = 0;
        const int32_t qi = up_search(in + m.qname_off, m.qname_len, m.qs, m.qe, iv, n_iv, names);
        const int32_t ti = qi == -2 ? -1 : up_search(in + m.tname_off, m.tname_len, m.ts, m.te, iv, n_iv, names);
        if (qi == -2 || ti == -2) code = PAFFY_ERR_UPCONVERT_ASSERT;
        if (qi >= 0) {
            const UpInterval y = iv[qi];
            m.qname_off = y.out_off;
            m.qname_len = y.out_len;
            m.qs -= y.start;
            m.qe -= y.start;
            m.qlen = y.length;
            m.pad0 |= 1u;
        }
        if (ti >= 0) {
            const UpInterval y = iv[ti];
            m.tname_off = y.out_off;
            m.tname_len = y.out_len;
            m.ts -= y.start;
            m.te -= y.start;
            m.tlen = y.length;
            m.pad0 |= 2u;
        }
        if (!code && check) { /* paf_check without a cigar, impl/paf.c:427-439 */
            if (m.qs < 0 || m.qs >= m.qlen) code = PAFFY_ERR_CHECK_QSTART;
            else if (m.qs > m.qe || m.qe > m.qlen) code = PAFFY_ERR_CHECK_QEND;
            else if (m.ts < 0 || m.ts >= m.tlen) code = PAFFY_ERR_CHECK_TSTART;
            else if (m.ts > m.te || m.te > m.tlen) code = PAFFY_ERR_CHECK_TEND;
        }
    }
    if (code) atomicMin(&info->first_err_key, ((unsigned long long)r << 16) | ((unsigned long long)((stage + 1) & 0xff) << 8) | (unsigned long long)code);
}

/* ------------------------------------------------------------------ */
/* sequence lookup (add_mismatches)                                     */
/* ------------------------------------------------------------------ */

/* names sorted bytewise (memcmp, shorter first on a tie): binary search per record name; replaces the
 * stHash_search by name of impl/paf_add_mismatches.c:116,123 */
__device__ int32_t find_seq(const uint8_t *in, uint32_t off, uint32_t len, const uint8_t *names, const uint32_t *name_off, int32_t n) {
    int32_t lo = 0, hi = n - 1;
    while (lo <= hi) {
        int32_t mid = (lo + hi) >> 1;
        const uint8_t *nm = names + name_off[mid];
        uint32_t nl = name_off[mid + 1] - name_off[mid];
        uint32_t k = 0, m = len < nl ? len : nl;
        int cmp = 0;
        for (; k < m; k++) {
            int d = (int)in[off + k] - (int)nm[k];
            if (d) {
                cmp = d;
                break;
            }
        }
        if (cmp == 0) cmp = len < nl ? -1 : (len > nl ? 1 : 0);
        if (cmp == 0) return mid;
        if (cmp < 0) hi = mid - 1;
        else lo = mid + 1;
    }
    return -1;
}
__global__ __launch_bounds__(PAFFY_NT) void k_seq_lookup(const uint8_t *in, const RecMeta *meta, uint32_t n_rec, const uint8_t *names,
                                                          const uint32_t *name_off, int32_t n_seqs, int32_t *rec_qseq, int32_t *rec_tseq) {
    uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n_rec) return;
    const RecMeta &m = meta[r];
    rec_qseq[r] = m.err ? -1 : find_seq(in, m.qname_off, m.qname_len, names, name_off, n_seqs);
    rec_tseq[r] = m.err ? -1 : find_seq(in, m.tname_off, m.tname_len, names, name_off, n_seqs);
}

/* ------------------------------------------------------------------ */
/* record sizes -> offsets                                              */
/* ------------------------------------------------------------------ */

/*
 * Exclusive prefix sum of the record sizes up to the first failing record (records at or after it contribute
 * nothing), two levels: k_scan_part sums and scans blocks of SCAN_BLOCK records, k_scan_fix adds the block bases
 * (at most a few hundred of them, re-added by every workgroup) and leaves the totals in DevInfo.
 */
#define SCAN_PER 8
#define SCAN_BLOCK (PAFFY_NT * SCAN_PER)
__global__ __launch_bounds__(PAFFY_NT) void k_scan_part(const int64_t *out_len, const int64_t *out_rows, uint32_t n, int64_t *out_off, int64_t *part,
                                                         const DevInfo *info) {
    __shared__ int64_t scratch_mem[2 * PAFFY_NWAVE * 4];
    BlockComm scratch{scratch_mem, 0};
    const uint32_t first_err = (uint32_t)(info->first_err_key >> 16);
    const uint32_t live_n = n < first_err ? n : first_err;
    const uint32_t i0 = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER;
    int64_t len[SCAN_PER];
    int64_t v[2] = {0, 0}, tot[2];
#pragma unroll
    for (int j = 0; j < SCAN_PER; j++) {
        const uint32_t i = i0 + j;
        len[j] = i < live_n ? out_len[i] : 0;
        v[0] += len[j];
        v[1] += i < live_n ? out_rows[i] : 0;
    }
    block_excl_scan<2>(v, tot, scratch);
    int64_t run = v[0];
#pragma unroll
    for (int j = 0; j < SCAN_PER; j++) {
        const uint32_t i = i0 + j;
        if (i < n) out_off[i] = run; /* block-local; k_scan_fix adds the base */
        run += len[j];
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = tot[0];
        part[2 * blockIdx.x + 1] = tot[1];
    }
}
__global__ __launch_bounds__(PAFFY_NT) void k_scan_fix(uint32_t n, uint32_t n_blocks, int64_t *out_off, const int64_t *part, DevInfo *info) {
    __shared__ int64_t scratch_mem[2 * PAFFY_NWAVE * 4];
    BlockComm scratch{scratch_mem, 0};
    /* base of this block = sum of the totals of the blocks before it; the last workgroup also sees the grand totals */
    int64_t v[2] = {0, 0};
    for (uint32_t b = threadIdx.x; b < n_blocks; b += PAFFY_NT) {
        if (b < blockIdx.x) v[0] += part[2 * b];
    }
    int64_t t[2] = {0, 0};
    if (blockIdx.x == n_blocks - 1)
        for (uint32_t b = threadIdx.x; b < n_blocks; b += PAFFY_NT) {
            t[0] += part[2 * b];
            t[1] += part[2 * b + 1];
        }
    int64_t s[3] = {v[0], t[0], t[1]};
    block_sum<3>(s, scratch);
    const uint32_t i0 = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER;
#pragma unroll
    for (int j = 0; j < SCAN_PER; j++)
        if (i0 + j < n) out_off[i0 + j] += s[0];
    if (blockIdx.x == n_blocks - 1 && threadIdx.x == 0) {
        info->out_bytes = (unsigned long long)s[1];
        info->out_rows = (unsigned long long)s[2];
    }
}

/*
 * Launch order of the record kernels: records in 64 classes of size (the sizing pass: 512 bytes of cigar text per class,
 * the writers: 16 KiB of output), largest class first, so that the long records do not start last and stretch the kernel's tail (longest-processing-time-first, coarse).
 * k_order_count histograms the classes, k_order_scatter gives every record its slot.
 */
#define ORDER_CLASSES 64u
__device__ __forceinline__ uint32_t order_class(int64_t out_len, uint32_t shift) {
    const uint64_t c = (uint64_t)(out_len < 0 ? 0 : out_len) >> shift;
    return c < ORDER_CLASSES ? (uint32_t)c : ORDER_CLASSES - 1;
}
__global__ __launch_bounds__(PAFFY_NT) void k_cigar_bytes(const RecMeta *meta, uint32_t n, int64_t *out) {
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r < n) out[r] = meta[r].has_cg ? (int64_t)meta[r].cg_len : 0;
}
__global__ __launch_bounds__(PAFFY_NT) void k_order_count(const int64_t *out_len, uint32_t n, uint32_t shift, uint32_t *counts) {
    __shared__ uint32_t h[ORDER_CLASSES];
    if (threadIdx.x < ORDER_CLASSES) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r < n) atomicAdd(&h[order_class(out_len[r], shift)], 1u);
    __syncthreads();
    if (threadIdx.x < ORDER_CLASSES && h[threadIdx.x]) atomicAdd(&counts[threadIdx.x], h[threadIdx.x]);
}
__global__ __launch_bounds__(PAFFY_NT) void k_order_scatter(const int64_t *out_len, uint32_t n, uint32_t shift, const uint32_t *counts, uint32_t *cursor,
                                                             uint32_t *order) {
    __shared__ uint32_t base[ORDER_CLASSES], mine[ORDER_CLASSES], got[ORDER_CLASSES];
    if (threadIdx.x < ORDER_CLASSES) mine[threadIdx.x] = 0;
    if (threadIdx.x == 0) { /* classes in descending order */
        uint32_t run = 0;
        for (int c = (int)ORDER_CLASSES - 1; c >= 0; c--) {
            base[c] = run;
            run += counts[c];
        }
    }
    __syncthreads();
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    uint32_t c = 0, local = 0;
    if (r < n) {
        c = order_class(out_len[r], shift);
        local = atomicAdd(&mine[c], 1u); /* slot inside this workgroup's share of the class */
    }
    __syncthreads();
    if (threadIdx.x < ORDER_CLASSES && mine[threadIdx.x]) got[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], mine[threadIdx.x]); /* one global atomic per class */
    __syncthreads();
    if (r < n) order[base[c] + got[c] + local] = r;
}

/* ------------------------------------------------------------------ */
/* tile: keys for the host ordering, sizes and the verbatim writer       */
/* ------------------------------------------------------------------ */

/* dedupe: 128-bit key of (query name, target name, strand, four coordinates), the same for the swapped record, the
 * coordinate part of paf_check (impl/paf.c:427-438; the cigar is not parsed here) and the record's own tile level */
struct DedupeKey {
    uint64_t a, b;   /* key */
    uint64_t ia, ib; /* key of the record with query and target swapped */
    int32_t err;     /* parse error (PAFFY_ERR_*) */
    int32_t check;   /* paf_check code on the coordinates, 0 = fine */
};
__device__ __forceinline__ void dedupe_mix(uint64_t &h1, uint64_t &h2, uint64_t x) {
    h1 = (h1 ^ x) * 0x100000001b3ull;
    h1 ^= h1 >> 29;
    h2 = (h2 + x) * 0x9e3779b97f4a7c15ull;
    h2 ^= h2 >> 32;
}
__device__ __forceinline__ void dedupe_name(const uint8_t *in, uint32_t off, uint32_t len, uint64_t &h1, uint64_t &h2) {
    h1 = 0xcbf29ce484222325ull;
    h2 = 0x6a09e667f3bcc909ull;
    for (uint32_t i = 0; i < len; i++) dedupe_mix(h1, h2, in[off + i]);
    dedupe_mix(h1, h2, 0x100u + len);
}
__global__ __launch_bounds__(PAFFY_NT) void k_dedupe_keys(const uint8_t *in, const RecMeta *meta, uint32_t n, DedupeKey *keys, int64_t *level) {
    uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n) return;
    const RecMeta &m = meta[r];
    DedupeKey k;
    k.err = m.err;
    uint64_t q1, q2, t1, t2;
    dedupe_name(in, m.qname_off, m.qname_len, q1, q2);
    dedupe_name(in, m.tname_off, m.tname_len, t1, t2);
    uint64_t a = q1, b = q2, ia = t1, ib = t2;
    dedupe_mix(a, b, t1); dedupe_mix(a, b, t2);
    dedupe_mix(ia, ib, q1); dedupe_mix(ia, ib, q2);
    const uint64_t strand = m.same_strand ? 1 : 2;
    const uint64_t f[4] = {(uint64_t)m.qs, (uint64_t)m.qe, (uint64_t)m.ts, (uint64_t)m.te};
    dedupe_mix(a, b, strand); dedupe_mix(ia, ib, strand);
    for (int i = 0; i < 4; i++) {
        dedupe_mix(a, b, f[i]);
        dedupe_mix(ia, ib, f[i ^ 2]); /* the swapped record's query coordinates are this one's target coordinates */
    }
    k.a = a; k.b = b; k.ia = ia; k.ib = ib;
    int chk = 0;
    if (m.qs < 0 || m.qs >= m.qlen) chk = PAFFY_ERR_CHECK_QSTART;
    else if (m.qs > m.qe || m.qe > m.qlen) chk = PAFFY_ERR_CHECK_QEND;
    else if (m.ts < 0 || m.ts >= m.tlen) chk = PAFFY_ERR_CHECK_TSTART;
    else if (m.ts > m.te || m.te > m.tlen) chk = PAFFY_ERR_CHECK_TEND;
    k.check = chk;
    keys[r] = k;
    level[r] = m.tile_level;
}

/* PAFFY_STATS: the batch's six sums from the records' (rec_stats[6 n], zero for records that stopped in front of the stage) */
__global__ __launch_bounds__(PAFFY_NT) void k_stats_reduce(const int64_t *rec_stats, uint32_t n, unsigned long long *sums) {
    __shared__ unsigned long long part[PAFFY_NT / 64][6];
    unsigned long long a[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x; i < n; i += gridDim.x * PAFFY_NT) {
#pragma unroll
        for (int k = 0; k < 6; k++) a[k] += (unsigned long long)rec_stats[6ull * i + k];
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        for (int d = 32; d; d >>= 1) a[k] += __shfl_down(a[k], d, 64);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < 6; k++) part[wave][k] = a[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < PAFFY_NT / 64; w++) t += part[w][threadIdx.x];
        if (t) atomicAdd(&sums[threadIdx.x], t);
    }
}

__device__ __forceinline__ void tile_state(const RecMeta &m, int64_t level, RecState &s) {
    load_state(m, s);
    s.has_cigar = false; /* the cigar is written verbatim from the text, impl/paf.c:381-385 */
    s.tile_level = level;
}

/* ------------------------------------------------------------------ */
/* synthetic workload, one lane per record                   */
/* ------------------------------------------------------------------ */

__global__ __launch_bounds__(PAFFY_NT) void k_synth_size(psynth_cfg cfg, uint64_t r0, uint32_t n, int64_t *sizes) {
    uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n) sizes[i] = psynth_emit_record(&cfg, r0 + i, nullptr);
}
__global__ __launch_bounds__(PAFFY_NT) void k_synth_fill(psynth_cfg cfg, uint64_t r0, uint32_t n, const int64_t *off, uint8_t *out) {
    uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n) psynth_emit_record(&cfg, r0 + i, reinterpret_cast<char *>(out) + off[i]);
}
__global__ __launch_bounds__(PAFFY_NT) void k_scan_i64(const int64_t *in, uint32_t n, int64_t *out_excl, int64_t *total) {
    __shared__ int64_t scratch_mem[2 * PAFFY_NWAVE * 4];
    BlockComm scratch{scratch_mem, 0};
    int64_t carry = 0;
    for (uint32_t base = 0; base < n; base += PAFFY_NT) {
        uint32_t i = base + threadIdx.x;
        int64_t v[1] = {i < n ? in[i] : 0}, tot[1];
        block_excl_scan<1>(v, tot, scratch);
        if (i < n) out_excl[i] = carry + v[0];
        carry += tot[0];
    }
    if (threadIdx.x == 0) *total = carry;
}

/* Sequences are kept in the form they are compared in (impl/paf.c:752-757: toupper of both bases, the query base complemented
 * on the - strand): seq upper-cased in place, comp = its complement. 16 bytes per lane. */
__global__ __launch_bounds__(PAFFY_NT) void k_seq_canon(uint8_t *seq, uint8_t *comp, uint64_t n16) {
    const uint64_t i = (uint64_t)blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n16) return;
    uint4 w = reinterpret_cast<uint4 *>(seq)[i];
    w.x = upper4(w.x); w.y = upper4(w.y); w.z = upper4(w.z); w.w = upper4(w.w);
    reinterpret_cast<uint4 *>(seq)[i] = w;
    w.x = comp4(w.x); w.y = comp4(w.y); w.z = comp4(w.z); w.w = comp4(w.w);
    reinterpret_cast<uint4 *>(comp)[i] = w;
}

/* ---- cfg4 workload: master alignments, genomes, records (paf_synth_core.h; host twin in tools/paf_synth.c) ---- */

/* one wave per contig pair walks the master ops 64 at a time: op count, query length, checkpoints */
__global__ __launch_bounds__(64) void k_synth4_master(psynth4_cfg cfg, psynth4_contig *contigs, int64_t *ckpt_q, int64_t *ckpt_t) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    psynth4_contig ct = contigs[c];
    const uint64_t mkey = psynth4_mkey(cfg.seed, c);
    int64_t q = 0, t = 0, best_q = 0;
    uint64_t best_n = 0;
    for (uint64_t base = 0; base < ct.ckpt_cap * PSYNTH4_G; base += 64) {
        if (base % PSYNTH4_G == 0 && lane == 0) {
            ckpt_q[ct.ckpt_base + base / PSYNTH4_G] = q;
            ckpt_t[ct.ckpt_base + base / PSYNTH4_G] = t;
        }
        int op;
        const int64_t len = psynth_op(mkey, base + lane, &op);
        const int64_t qi = q + wave_incl_scan(op != 2 ? len : 0), ti = t + wave_incl_scan(op != 1 ? len : 0);
        const uint64_t ok = __ballot(ti <= ct.tlen); /* a prefix of the lanes: the offsets only grow */
        const uint64_t even_ok = ok & 0x5555555555555555ull;
        if (even_ok) {
            const int top = 63 - __clzll((long long)even_ok);
            best_n = base + (uint64_t)top + 1;
            best_q = __shfl(qi, top);
        }
        if (ok != ~0ull) break;
        q = wave_last(qi);
        t = wave_last(ti);
    }
    if (lane == 0) {
        contigs[c].n_ops = best_n;
        contigs[c].qlen = best_q;
    }
}

/* target genome: one thread per 32 bases */
__global__ __launch_bounds__(PAFFY_NT) void k_synth4_target(psynth4_cfg cfg, uint32_t c, int64_t tlen, uint8_t *out) {
    const int64_t p0 = ((int64_t)blockIdx.x * PAFFY_NT + threadIdx.x) * 32;
    for (int64_t p = p0; p < p0 + 32 && p < tlen; p++) {
        int lower;
        const uint32_t b = psynth4_tbase(cfg.seed, c, p, &lower);
        out[p] = (uint8_t)psynth4_letter(b, lower, 0);
    }
}

/* query genome: one wave per checkpoint block of master ops, one lane per op */
__global__ __launch_bounds__(64) void k_synth4_query(psynth4_cfg cfg, uint32_t c, psynth4_tab tab, uint8_t *out) {
    const psynth4_contig ct = tab.contigs[c];
    const uint64_t mkey = psynth4_mkey(cfg.seed, c);
    const int minus = psynth4_minus(c);
    int64_t q = tab.ckpt_q[ct.ckpt_base + blockIdx.x], t = tab.ckpt_t[ct.ckpt_base + blockIdx.x];
    for (uint64_t base = (uint64_t)blockIdx.x * PSYNTH4_G; base < ((uint64_t)blockIdx.x + 1) * PSYNTH4_G && base < ct.n_ops; base += 64) {
        const uint64_t j = base + threadIdx.x;
        int op;
        int64_t len = psynth_op(mkey, j, &op);
        const int64_t dq = op != 2 ? len : 0, dt = op != 1 ? len : 0;
        const int64_t qi = wave_incl_scan(dq), ti = wave_incl_scan(dt);
        if (j < ct.n_ops && op != 2) {
            const int64_t q0 = q + qi - dq, t0 = t + ti - dt;
            for (int64_t i = 0; i < len; i++) {
                int lower;
                const uint32_t b = psynth4_qbase(cfg.seed, c, q0 + i, op == 0 ? t0 + i : -1, &lower);
                out[minus ? ct.qlen - 1 - (q0 + i) : q0 + i] = (uint8_t)psynth4_letter(b, lower, minus);
            }
        }
        q += wave_last(qi);
        t += wave_last(ti);
    }
}

__global__ __launch_bounds__(PAFFY_NT) void k_synth4_size(psynth4_cfg cfg, psynth4_tab tab, uint64_t r0, uint32_t n, int64_t *sizes) {
    uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n) sizes[i] = psynth4_emit_record(&cfg, &tab, r0 + i, nullptr);
}
__global__ __launch_bounds__(PAFFY_NT) void k_synth4_fill(psynth4_cfg cfg, psynth4_tab tab, uint64_t r0, uint32_t n, const int64_t *off, uint8_t *out) {
    uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n) psynth4_emit_record(&cfg, &tab, r0 + i, reinterpret_cast<char *>(out) + off[i]);
}

/* ------------------------------------------------------------------ */
/* host side                                                            */
/* ------------------------------------------------------------------ */

struct ProfEntry {
    std::string name;
    double ms = 0;
    int64_t launches = 0;
};

/* what the current plan is, and so what paffy_hip_emit writes and which getters answer */
enum PlanKind {
    PLAN_NONE,
    PLAN_RECORDS, /* paffy_hip_plan: the stage list's output through the record writers */
    PLAN_LINES,   /* tile, chain, dedupe, upconvert: a line table (header + the cigar text as it was read) */
    PLAN_BED      /* paffy to_bed: the run lines */
};

/* the command states the context owns: complete where the context's destructor is defined, at the end of this file */
struct DedupeState;
struct DedupeParts;
struct SplitState;
struct BedParams;
struct ChainState;
struct FastaState;
struct CovState;

struct paffy_hip_ctx {
    ~paffy_hip_ctx(); /* teardown order: DESIGN "Who owns device memory" */
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr; /* sizing launches of the long-cigar records run here, beside the main launch */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string last_error;
    double sep_guess_per_mib = 0, line_guess_per_mib = 0; /* separators / lines per MiB of the last batch indexed: sizes the one-pass index of the next */
    DevBuf tile_counts, sep_pos, nl_idx, meta, out_len, out_rows, status, err_aux, n_ops, arena_off, out_off, w_list, b_list, b_list1, arena, info, synth_sizes, rec_plan, ops_mirror, seq_blob, seq_table, seq_names, seq_name_off, rec_qseq, rec_tseq, seq_comp;
    int32_t n_seqs = 0;
    DevBuf synth4_contigs, synth4_q, synth4_t; /* cfg4 workload tables (paffy_hip_synth4_setup) */
    psynth4_cfg synth4_cfg = {0, 0, 0, 0, 0};
    paffy_filter filter = {-1, -1, -1.0, -1.0, -1, 0};
    DevBuf dedupe_keys;
    std::unique_ptr<DedupeState> dedupe; /* dedupe_host.h: keys of the records written so far (sorted, on the device) and scratch */
    /* dedupe in parts (dedupe_parts_kernel.h): how far the round of this context's batch has come -- 0 none, 1 keys sent, 2 verdicts in; any
       planner and anything that indexes another batch puts it back to 0 (the round's state lies in the index buffers) -- and whether a
       round reported a failure since the last paffy_hip_dedupe_reset */
    int dd_part_stage = 0;
    bool dd_part_failed = false;
    std::unique_ptr<DedupeParts> dd_parts; /* the round's entry map and verdicts; the owner's memory */
    std::unique_ptr<SplitState> split; /* `paffy split_file` (split_host.h): grouping scratch and the files of the run */
    DevBuf scan_part, emit_order, order_cnt, tile_keys, tile_order, tile_rank, tile_coff, tile_cbase, tile_cov, tile_level, tile_len, tile_items, tile_slots, tile_parts;
    bool keep_raw = false;    /* paffy_hip_keep_raw_sequences: seq_raw holds the bases as loaded (paf_pretty_print shows their case) */
    bool plan_seq_lookup = false; /* rec_qseq / rec_tseq belong to the current plan */
    DevBuf seq_raw, pretty_off, pretty_out, pretty_err, host_in, host_out;
    DevBuf rec_stats; /* six sums per record of the PAFFY_STATS stage */
    DevBuf flat_nd, flat_rec, flat_chunks, flat_sums, flat_done, flat_items, flat_pieces; /* the flat sizing pass (flat_kernel.h) */
    DevBuf add_pieces, add_scr_cnt, add_scr_off, add_new_cnt, add_new_off, add_text, add_bad, add_part, add_scratch, add_new_ops; /* flat_add_kernel.h */
    uint32_t flat_piece_slots = 0;
    DevBuf bed_keys; /* paffy_hip_bed_sequence_keys: the first entry of every sequence, staged for k_bed_seq_keys */
    DevBuf bed_tab, bed_starts, bed_len, bed_off, bed_tiles;
    std::unique_ptr<BedParams> bed_params; /* host copy */
    uint64_t bed_runs = 0;
    const uint8_t *tile_in = nullptr;
    std::unique_ptr<ChainState> chain; /* `paffy chain` (chain_host.h) */
    std::unique_ptr<FastaState> fasta; /* `faffy chunk | extract | merge`: FASTA index and item plan (fasta_host.h) */
    int64_t name_sort_stats[4] = {0, 0, 0, 0}; /* the last name sort (name_sort_host.h): records, rounds, records tied after the first round, distinct names */
    std::unique_ptr<CovState> cov; /* `paffy tile` / `paffy to_bed` over any number of batches (coverage_host.h) */
    /* the batch paffy_hip_query_names indexed last: paffy_hip_split_by_owner on the same batch reuses the index (one use) */
    const void *indexed_in = nullptr;
    int64_t indexed_len = 0;
    uint32_t indexed_n = 0;
    /* the index of batches whose names were asked for (paffy_hip_query_names), kept until the batch is split: a sharded tile asks
       for the names of all its batches before it splits the first one */
    struct KeptIndex {
        const void *in = nullptr;
        int64_t len = 0;
        uint32_t n = 0, n_seps = 0;
        DevBuf meta, sep_pos, nl_idx;
    };
    std::vector<KeptIndex> kept_index;
    std::vector<KeptIndex> index_pool; /* buffers of dropped entries, reused by the next kept index (no hipMalloc / hipFree per batch) */
    DevBuf one_batch;               /* table with the single text pointer of a one-batch plan (dedupe / split_file lines) */
    /* what emit writes for a line plan (tile, dedupe): record order, levels, offsets */
    const uint8_t *const *line_batches = nullptr;
    const RecMeta *line_meta = nullptr;
    const uint32_t *line_order = nullptr;
    const int64_t *line_level = nullptr;
    const uint64_t *line_off = nullptr;
    uint64_t line_n = 0;
    const uint8_t *line_names2 = nullptr; /* upconvert: the interval table's output names (k_line_emit) */
    /* upconvert (paffy_hip_set_intervals): the FASTA intervals sorted by (name, start), their names and output names in one blob */
    DevBuf up_table, up_names;
    uint32_t n_intervals = 0;
    /* paffy_hip_intervals_info: the bytes of up_names in use, whether the device built the table (upconvert_build_host.h) and the rounds
       of that build's name sort */
    uint64_t up_blob_bytes = 0;
    bool up_on_device = false;
    int64_t up_rounds = 0;
    DevInfo *h_info = nullptr; /* pinned */
    /* plan state (plan_begin clears it) */
    bool planned = false;
    PlanKind plan_kind = PLAN_NONE;
    KParams kp;
    paffy_plan_info plan;
    /* profiling */
    bool profile = false;
    int64_t flat_left = -1, flat_reasons[16] = {0}; /* paffy_hip_flat_stats */
    bool stats_only = false;      /* paffy_hip_stats_only: the caller will only ask a plan for its sums */
    bool chain_fresh = false;     /* paffy_hip_chain_fresh_walk: chain_run restates the reference's walk from a fresh iterator */
    bool plan_stats_only = false; /* the last plan took FLAT_MODE_VIEW: it has sums, no ops and no line plan */
    bool plan_split = false;      /* the last plan is paffy_hip_split_plan's: a line plan with a group table (paffy_hip_split_groups) */
    DevBuf view_sums;             /* flat_view_kernel.h: six sums per piece slot */
    DevBuf add_nsums;             /* flat_add_pipe_kernel.h: a PieceSum of the new ops per piece slot */
    DevBuf view_work;             /* view_line_kernel.h: sizes, row offsets and the offsets' verdict of a paffy_hip_plan_view_* call */
    /* paffy_hip_plan_view_layout: the sizes of the batch's blocks, their running sums, the rows' bytes and offsets and the verdict of a range
       (view_layout), the ranges the cut kernel wrote (view_ranges_dev) and their copy on the host (view_tab: n_ranges + 1 entries) */
    DevBuf view_layout, view_ranges_dev;
    std::vector<int64_t> view_tab; /* {first record, first byte} per range */
    bool view_laid = false; /* the layout belongs to the current plan (plan_begin clears it) */
    bool view_laid_rows = false;
    uint32_t flat_chunk_slots = 0;
    bool lvl0_long_ok = false, lvl0_long_off = false; /* the longer first store level: shown safe by the batch before / overflowed once */
    /* device buffers of the two slots of a closed stream (paffy_hip_stream_close), taken again by the next paffy_hip_stream_open: a
       hipMalloc of the tens of GB a slot's output needs takes 16 ms most of the time and 0.5-2.6 s right behind the hipFree of the stream
       before (tools/probes/d2h_pieces.py) */
    DevBuf kept_slot[2][2]; /* [slot][0 = input, 1 = output] */
    std::vector<struct paffy_hip_stream *> open_streams; /* streams of this context that are open: the destructor detaches them (a stream closed later frees
                                                           its buffers itself instead of leaving them with a context that is gone) */
    std::string profile_only; /* when not empty: only launches of this kernel are bracketed (paffy_hip_profile_only) */
    std::vector<hipEvent_t> event_pool;
    std::vector<ProfEntry> prof;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
    std::vector<std::string> name_store;
};

#define HIPCHK(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);          \
            return PAFFY_E_HIP;                                                             \
        }                                                                                   \
    } while (0)

static int ensure(paffy_hip_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    HIPCHK(c, b.release());
    /* room to grow: a batch a little larger than the last must not cost a free and an allocation */
    if (b.alloc(bytes + bytes / 2 + 256) != hipSuccess) { /* no room for the slack: an input that fits HBM at its exact size must not fail here */
        (void)hipGetLastError();
        HIPCHK(c, b.alloc(bytes));
    }
    return 0;
}

static int prof_slot(paffy_hip_ctx *c, const char *name) {
    for (size_t i = 0; i < c->prof.size(); i++)
        if (c->prof[i].name == name) return (int)i;
    ProfEntry e;
    e.name = name;
    c->prof.push_back(e);
    return (int)c->prof.size() - 1;
}
static void prof_collect(paffy_hip_ctx *c) {
    for (auto &p : c->pending) {
        float ms = 0;
        (void)hipEventSynchronize(p.second.second);
        (void)hipEventElapsedTime(&ms, p.second.first, p.second.second);
        c->prof[p.first].ms += ms;
        c->prof[p.first].launches += 1;
        c->event_pool.push_back(p.second.first);
        c->event_pool.push_back(p.second.second);
    }
    c->pending.clear();
}
static hipEvent_t prof_event(paffy_hip_ctx *c) {
    hipEvent_t e = nullptr;
    if (!c->event_pool.empty()) {
        e = c->event_pool.back();
        c->event_pool.pop_back();
    } else {
        (void)hipEventCreate(&e);
    }
    return e;
}
static bool prof_wants(const paffy_hip_ctx *c, const char *name) { return c->profile && (c->profile_only.empty() || c->profile_only == name); }

/* launch wrapper: optional HIP events on the context's stream around each kernel */
#define LAUNCH(ctx, name, kernel, grid, block, shmem, ...)                                  \
    do {                                                                                    \
        hipEvent_t e0_ = nullptr, e1_ = nullptr;                                            \
        const bool prof_ = prof_wants(ctx, name);                                           \
        if (prof_) {                                                                        \
            e0_ = prof_event(ctx);                                                          \
            e1_ = prof_event(ctx);                                                          \
            (void)hipEventRecord(e0_, (ctx)->stream);                                             \
        }                                                                                   \
        hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->stream, __VA_ARGS__);         \
        if (prof_) {                                                                        \
            (void)hipEventRecord(e1_, (ctx)->stream);                                             \
            (ctx)->pending.push_back({prof_slot(ctx, name), {e0_, e1_}});                   \
        }                                                                                   \
        HIPCHK(ctx, hipGetLastError());                                                     \
    } while (0)

/* the dynamic LDS of one stage-mask instantiation of the sizing kernels (more than the default 64 KiB) */
template <uint32_t MASK>
static void size_lds_attributes() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_size_lds<MASK>), hipFuncAttributeMaxDynamicSharedMemorySize, PAFFY_SIZE_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_size_lds_long<MASK>), hipFuncAttributeMaxDynamicSharedMemorySize, PAFFY_SIZE_LDS_BYTES_FOR(PAFFY_OPS_CAP_BIG));
}

/* One sizing pass of the record kernels: levels 1 and 2 (long cigars, queued by k_header) on the side stream, level 0 on the main one
   -- one wave per record for the cigars of at most kp.wave_max_bytes (0: none), four waves for the rest -- then the join. */
template <uint32_t MASK>
static int size_records(paffy_hip_ctx *c, const KParams &kp, uint32_t n_lines) {
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
    KParams k1 = kp;
    k1.ops_cap = PAFFY_OPS_CAP_MID;
    k1.next_cap = PAFFY_OPS_CAP_BIG;
    k1.level = 1;
    hipLaunchKernelGGL(k_size_lds_long<MASK>, dim3(768), dim3(PAFFY_NT), PAFFY_SIZE_LDS_BYTES_FOR(PAFFY_OPS_CAP_MID), c->side, k1);
    k1.ops_cap = PAFFY_OPS_CAP_BIG;
    k1.next_cap = 0;
    k1.level = 2;
    hipLaunchKernelGGL(k_size_lds_long<MASK>, dim3(256), dim3(PAFFY_NT), PAFFY_SIZE_LDS_BYTES_FOR(PAFFY_OPS_CAP_BIG), c->side, k1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_join, c->side));
    if (kp.wave_max_bytes) { /* short cigars: one wave per record, sixteen records in flight per CU */
        KParams kw = kp;
        kw.ops_cap = WAVE_OPS_CAP;
        const size_t wlds = (size_t)WAVE_OPS_CAP * 4 + PAFFY_HALO + 64 * 16 + 64 * 8 + 64;
        LAUNCH(c, "k_size_wave", g64::k_size_lds<MASK>, dim3(n_lines), dim3(64), wlds, kw);
    }
    LAUNCH(c, "k_size_lds", k_size_lds<MASK>, dim3(n_lines), dim3(PAFFY_NT), PAFFY_SIZE_LDS_BYTES, kp);
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0)); /* join */
    return 0;
}
static int size_records_for(paffy_hip_ctx *c, uint32_t mask, const KParams &kp, uint32_t n_lines) {
    switch (mask) {
    case PAFFY_MASK_LEAN: return size_records<PAFFY_MASK_LEAN>(c, kp, n_lines);
    case PAFFY_MASK_ADD: return size_records<PAFFY_MASK_ADD>(c, kp, n_lines);
    case PAFFY_MASK_SEL: return size_records<PAFFY_MASK_SEL>(c, kp, n_lines);
    case PAFFY_MASK_PLAIN: return size_records<PAFFY_MASK_PLAIN>(c, kp, n_lines);
    default: return size_records<PAFFY_MASK_ALL>(c, kp, n_lines);
    }
}

extern "C" {

int paffy_hip_create(paffy_hip_ctx **out, int device) {
    if (!out) return PAFFY_E_ARG;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return PAFFY_E_HIP;
    paffy_hip_ctx *c = new paffy_hip_ctx();
    if (hipHostMalloc(reinterpret_cast<void **>(&c->h_info), sizeof(DevInfo)) != hipSuccess) {
        delete c;
        return PAFFY_E_HIP;
    }
    if (ensure(c, c->info, sizeof(DevInfo))) {
        delete c;
        return PAFFY_E_HIP;
    }
    (void)hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
    (void)hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    (void)hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    /* the record kernels use more than the default 64 KiB of LDS */
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cov_walk<true>), hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(CovWalkLds));
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cov_walk<false>), hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(CovWalkLds));
    size_lds_attributes<PAFFY_MASK_LEAN>();
    size_lds_attributes<PAFFY_MASK_ADD>();
    size_lds_attributes<PAFFY_MASK_SEL>();
    size_lds_attributes<PAFFY_MASK_PLAIN>();
    size_lds_attributes<PAFFY_MASK_ALL>();
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_emit_lds<true>), hipFuncAttributeMaxDynamicSharedMemorySize, PAFFY_EMIT_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_emit_lds<false>), hipFuncAttributeMaxDynamicSharedMemorySize, PAFFY_EMIT_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_arena_size), hipFuncAttributeMaxDynamicSharedMemorySize, PAFFY_SIZE_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_arena_emit<true>), hipFuncAttributeMaxDynamicSharedMemorySize, PAFFY_EMIT_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_arena_emit<false>), hipFuncAttributeMaxDynamicSharedMemorySize, PAFFY_EMIT_LDS_BYTES);
    *out = c;
    return 0;
}

void paffy_hip_destroy(paffy_hip_ctx *c) {
    if (!c) return;
    delete c;
}

int paffy_hip_set_stream(paffy_hip_ctx *c, void *s) {
    if (!c) return PAFFY_E_ARG;
    c->stream = reinterpret_cast<hipStream_t>(s);
    return 0;
}

const char *paffy_hip_last_error(paffy_hip_ctx *c) { return c ? c->last_error.c_str() : "null context"; }

static int fetch_info(paffy_hip_ctx *c) {
    HIPCHK(c, hipMemcpyAsync(c->h_info, c->info.p, sizeof(DevInfo), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* Every planner starts here: nothing that describes the plan before survives (what emit writes, what the getters report). */
static void plan_begin(paffy_hip_ctx *c, PlanKind kind, int64_t in_bytes, paffy_plan_info *info) {
    c->planned = false;
    c->plan_kind = kind;
    c->dd_part_stage = 0;
    memset(info, 0, sizeof(*info));
    info->in_bytes = in_bytes;
    memset(&c->plan, 0, sizeof(c->plan));
    c->plan.in_bytes = in_bytes;
    memset(&c->kp, 0, sizeof(c->kp));
    c->flat_left = -1;
    memset(c->flat_reasons, 0, sizeof(c->flat_reasons));
    c->plan_stats_only = false;
    c->plan_split = false;
    c->line_n = 0;
    c->bed_runs = 0;
    c->plan_seq_lookup = false;
    c->view_laid = false;
}

/* the kept indexes (defined with index_keep, behind the kernels they need) */
static void index_drop(paffy_hip_ctx *c, const void *d_in);
static void index_drop_all(paffy_hip_ctx *c) {
    while (!c->kept_index.empty()) index_drop(c, c->kept_index.back().in);
    c->indexed_in = nullptr;
}

/* Separator index + header parse shared by plan and tile_plan. */
static int index_and_parse(paffy_hip_ctx *c, const uint8_t *in, uint32_t len, uint32_t *n_lines_out, uint32_t lvl0_max = PAFFY_OPS_CAP, bool flat = false) {
    index_drop(c, in); /* a kept index of this buffer describes what it held before */
    c->dd_part_stage = 0;
    const uint32_t n_tiles = (len + SEP_TILE - 1) / SEP_TILE;
    c->indexed_in = nullptr; /* the index buffers are about to describe another batch */

    DevInfo zero;
    memset(&zero, 0, sizeof(zero));
    zero.first_err_key = ~0ull;
    HIPCHK(c, hipMemcpyAsync(c->info.p, &zero, sizeof(zero), hipMemcpyHostToDevice, c->stream));
    /* One pass (k_sep_index) when the separator density of this context's batches is known from the batch before: the index buffers are
       sized by that guess, the kernel writes nothing past them and reports the true counts; a batch that needs more is indexed again
       with exact sizes. The first batch of a context (no guess) takes the two-pass form, which sizes the buffers exactly. */
    uint32_t n_seps = 0, n_lines = 0;
    bool indexed = false;
    /* the flat sizing pass wants the non-digit bytes of every 1 KiB tile of the text: the index kernels count them on their way */
    uint16_t *nd = nullptr;
    if (flat) {
        if (ensure(c, c->flat_nd, sizeof(uint16_t) * (((size_t)len >> FLAT_TILE_SHIFT) + 2))) return PAFFY_E_HIP;
        nd = static_cast<uint16_t *>(c->flat_nd.p);
    }
    if (c->sep_guess_per_mib > 0) {
        const double mib = (double)len / (1 << 20) + 1.0;
        const size_t want_seps = (size_t)(c->sep_guess_per_mib * mib * 1.25) + 4096, want_lines = (size_t)(c->line_guess_per_mib * mib * 1.25) + 4096;
        if (ensure(c, c->sep_pos, sizeof(uint32_t) * (want_seps + 1)) || ensure(c, c->nl_idx, sizeof(uint32_t) * (want_lines + 1)) ||
            ensure(c, c->tile_counts, sizeof(unsigned long long) * ((size_t)n_tiles + 1)))
            return PAFFY_E_HIP;
        const uint32_t cap_seps = (uint32_t)std::min<size_t>(c->sep_pos.cap / sizeof(uint32_t), 0x7fffffffu), cap_lines = (uint32_t)std::min<size_t>(c->nl_idx.cap / sizeof(uint32_t), 0x7fffffffu);
        HIPCHK(c, hipMemsetAsync(c->tile_counts.p, 0, sizeof(unsigned long long) * ((size_t)n_tiles + 1), c->stream));
        LAUNCH(c, "k_sep_index", k_sep_index, dim3(n_tiles), dim3(PAFFY_NT), 0, in, len, n_tiles, static_cast<unsigned long long *>(c->tile_counts.p),
               static_cast<uint32_t *>(c->sep_pos.p), cap_seps, static_cast<uint32_t *>(c->nl_idx.p), cap_lines, static_cast<DevInfo *>(c->info.p), nd);
        if (fetch_info(c)) return PAFFY_E_HIP;
        n_seps = c->h_info->n_seps;
        n_lines = c->h_info->n_lines;
        indexed = n_seps <= cap_seps && n_lines <= cap_lines; /* otherwise: denser than the guess, once more below with exact sizes */
    }
    if (!indexed) {
        if (ensure(c, c->tile_counts, sizeof(uint2) * n_tiles)) return PAFFY_E_HIP;
        LAUNCH(c, "k_sep_count", k_sep_count, dim3(n_tiles), dim3(PAFFY_NT), 0, in, len, static_cast<uint2 *>(c->tile_counts.p), nd);
        LAUNCH(c, "k_scan_tiles", k_scan_tiles, dim3(1), dim3(PAFFY_NT), 0, static_cast<uint2 *>(c->tile_counts.p), n_tiles,
               static_cast<DevInfo *>(c->info.p));
        if (fetch_info(c)) return PAFFY_E_HIP;
        n_seps = c->h_info->n_seps;
        n_lines = c->h_info->n_lines;
        if (ensure(c, c->sep_pos, sizeof(uint32_t) * (size_t)(n_seps + 1))) return PAFFY_E_HIP;
        if (ensure(c, c->nl_idx, sizeof(uint32_t) * (size_t)(n_lines + 1))) return PAFFY_E_HIP;
    }
    *n_lines_out = n_lines;
    {
        const double mib = (double)len / (1 << 20) + 1.0;
        c->sep_guess_per_mib = (double)n_seps / mib + 1.0;
        c->line_guess_per_mib = (double)n_lines / mib + 1.0;
    }

    const struct {
        DevBuf *buf;
        size_t entry;
    } per_record[] = {{&c->meta, sizeof(RecMeta)},     {&c->b_list, sizeof(uint32_t)},    {&c->out_len, sizeof(int64_t)}, {&c->out_rows, sizeof(int64_t)},
                      {&c->out_off, sizeof(int64_t)},  {&c->status, sizeof(uint32_t)},    {&c->err_aux, sizeof(int32_t)}, {&c->n_ops, sizeof(uint32_t)},
                      {&c->arena_off, sizeof(uint64_t)}, {&c->w_list, sizeof(uint32_t)}, {&c->b_list1, sizeof(uint32_t)}, {&c->rec_plan, sizeof(RecPlan)}};
    for (const auto &r : per_record)
        if (ensure(c, *r.buf, r.entry * (size_t)(n_lines + 1))) return PAFFY_E_HIP;
    if (ensure(c, c->ops_mirror, sizeof(uint32_t) * ((size_t)len / 2 + 64))) return PAFFY_E_HIP;
    if (c->arena.cap == 0 && ensure(c, c->arena, (size_t)8 << 20)) return PAFFY_E_HIP;

    if (!indexed)
        LAUNCH(c, "k_sep_write", k_sep_write, dim3(n_tiles), dim3(PAFFY_NT), 0, in, len, static_cast<const uint2 *>(c->tile_counts.p),
               static_cast<uint32_t *>(c->sep_pos.p), static_cast<uint32_t *>(c->nl_idx.p));
    if (flat && n_lines > 0) {
        /* summary slot of piece p of record r: (cg_off >> 10) + r + p; chunk slot of its chunk c: (cg_off >> 12) + r + c (flat_kernel.h) */
        const size_t piece_slots = ((size_t)len >> FLAT_TILE_SHIFT) + (size_t)n_lines + 8, chunk_slots = ((size_t)len >> (FLAT_TILE_SHIFT + 2)) + (size_t)n_lines + 8;
        if (ensure(c, c->flat_chunks, sizeof(uint32_t) * chunk_slots) || ensure(c, c->flat_sums, sizeof(PieceSum) * piece_slots) ||
            ensure(c, c->flat_done, (size_t)n_lines + 16))
            return PAFFY_E_HIP;
        HIPCHK(c, hipMemsetAsync(c->flat_chunks.p, 0xff, sizeof(uint32_t) * chunk_slots, c->stream)); /* FLAT_NO_CHUNK */
        c->flat_chunk_slots = (uint32_t)chunk_slots;
        c->flat_piece_slots = (uint32_t)piece_slots;
    }
    if (n_lines > 0)
        LAUNCH(c, "k_header", k_header, dim3((n_lines + PAFFY_NT / HDR_GROUP - 1) / (PAFFY_NT / HDR_GROUP)), dim3(PAFFY_NT), 0, in,
               static_cast<const uint32_t *>(c->sep_pos.p), static_cast<const uint32_t *>(c->nl_idx.p), n_lines,
               static_cast<RecMeta *>(c->meta.p), static_cast<uint32_t *>(c->b_list.p), static_cast<DevInfo *>(c->info.p), lvl0_max,
               flat ? static_cast<uint32_t *>(c->flat_chunks.p) : static_cast<uint32_t *>(nullptr));

    return 0;
}

static int upconvert_plan(paffy_hip_ctx *c, const void *d_in, int64_t in_len, bool check, paffy_plan_info *info);

/* what a stage list asks of paffy_hip_plan, worked out once */
enum FlatMode {
    FLAT_MODE_NONE, /* the record kernels size every record */
    FLAT_MODE_PASS, /* the flat pass (flat_kernel.h); what it leaves goes to the record kernels */
    FLAT_MODE_ADD,  /* `paffy add_mismatches` alone: the flat parse and the encoder on its pieces (flat_add_kernel.h) */
    FLAT_MODE_REMOVE, /* `paffy add_mismatches -a` alone: the flat parse and the merge of the M/=/X runs on its pieces (flat_remove_kernel.h) */
    FLAT_MODE_VIEW, /* `paffy view` without rows, under paffy_hip_stats_only: the flat parse and the count walk alone (flat_view_kernel.h) */
    FLAT_MODE_ADD_PIPE /* `paffy add_mismatches` in front of an identity trim, a filter or both: the encoder on the pieces, then trim and filter
                          on the summaries of the new ops (flat_add_pipe_kernel.h) */
};
struct StageClass {
    paffy_stage stages[PAFFY_MAX_STAGES]; /* kinds without the PAFFY_NO_CHECK flag; a leading dechunk is its paf_check */
    int32_t n_stages;
    uint32_t nocheck_mask, fix_query, fix_target;
    bool upconvert; /* `paffy upconvert`: a plan of its own */
    bool need_seqs, add_not_last, has_stats, has_shatter;
    bool has_fixed;   /* FLAT_MODE_PASS with a fixed trim at any place: every record takes the wave kernel (k_flat_size<1> or <2>) */
    bool fixed_inner; /* ... and a stage behind a fixed trim: the instantiation whose stages know the shortened end ops */
    FlatMode flat;
    uint32_t size_mask; /* the instantiation of the sizing kernels: PAFFY_MASK_LEAN / ADD / SEL / PLAIN / ALL */
};

static int classify_stages(paffy_hip_ctx *c, const paffy_stage *stages, int32_t n_stages, StageClass &s) {
    s = StageClass{};
    s.n_stages = n_stages;
    paffy_stage *norm = s.stages;
    for (int32_t i = 0; i < n_stages; i++) {
        norm[i] = stages[i];
        if (stages[i].kind & PAFFY_NO_CHECK) s.nocheck_mask |= 1u << i;
        norm[i].kind = stages[i].kind & ~PAFFY_NO_CHECK;
    }
    /* `paffy dechunk` in front: k_dechunk rewrites the parsed names and coordinates, and what is left of the stage is its paf_check */
    const bool dechunk = n_stages > 0 && norm[0].kind == PAFFY_DECHUNK;
    s.fix_query = dechunk && norm[0].p0 != 0.0f;
    s.fix_target = dechunk && norm[0].p1 != 0.0f;
    if (dechunk) {
        norm[0].kind = (s.nocheck_mask & 1u) ? PAFFY_PASS : PAFFY_CHECK;
        norm[0].p0 = norm[0].p1 = 0.0f;
        s.nocheck_mask &= ~1u;
    }
    if (n_stages > 0 && norm[0].kind == PAFFY_UPCONVERT) { /* its read differs (no cigar parse): a plan of its own */
        if (n_stages != 1) {
            c->last_error = "upconvert is a stage list of its own";
            return PAFFY_E_UNSUPPORTED;
        }
        s.upconvert = true;
        return 0;
    }
    uint32_t kinds = 0;
    for (int32_t i = 0; i < n_stages; i++) {
        int k = norm[i].kind;
        bool ok = k == PAFFY_CHECK || k == PAFFY_INVERT || k == PAFFY_TRIM_IDENTITY || k == PAFFY_TRIM_FIXED || k == PAFFY_TRIM_ENDS || k == PAFFY_PASS || k == PAFFY_FILTER || k == PAFFY_STATS ||
                  k == PAFFY_REMOVE_MISMATCHES || (k == PAFFY_ADD_MISMATCHES && c->n_seqs > 0) ||
                  (k == PAFFY_SHATTER && i == n_stages - 1);
        if (!ok) {
            c->last_error = "stage list not fusable in this build";
            return PAFFY_E_UNSUPPORTED;
        }
        kinds |= 1u << k;
        /* add_mismatches makes more ops of a cigar (about 1.8 x at 2 % substitutions, 1.45 per two cigar bytes): when a stage follows
           it, its records start one store level up at 5/8 of the usual length, so that the rebuilt array usually fits the level the
           record was parsed at */
        if (k == PAFFY_ADD_MISMATCHES && i + 1 < n_stages) s.add_not_last = true;
    }
    s.need_seqs = (kinds >> PAFFY_ADD_MISMATCHES) & 1u;
    s.has_stats = (kinds >> PAFFY_STATS) & 1u;
    s.has_shatter = (kinds >> PAFFY_SHATTER) & 1u;
    /* the lean pipes are sized by the flat pass (flat_kernel.h): the text parsed in chunks whatever record they belong to, one wave per
       record on the chunks' summaries; what it leaves (FLAT_F_IRREG and friends) goes through the record kernels as before. It also
       knows `paffy filter` (a predicate on the sums it keeps anyway), the stats stage of `paffy view -s` (paf_stats_calc,
       impl/paf.c:236-260: sums the pieces' summaries hold, with the I ops counted where a shatter pipe counts the digits of its rows --
       so not both in one pipe), and a fixed trim (`paffy trim -f`) at any place and any number of times in a pipe without a shatter: the
       wave kernel finds the two ops it stops at (flat_find_aligned), and the stages behind it count those ops with their shortened
       lengths (FlatCuts). A pipe with a fixed trim and a shatter stays with the record kernels: the one-wave row writer does not
       write shortened end ops */
    s.has_fixed = ((kinds >> PAFFY_TRIM_FIXED) & 1u) && !s.has_shatter;
    const uint32_t flat_kinds = PAFFY_MASK_LEAN | (1u << PAFFY_FILTER) | (s.has_shatter ? 0u : 1u << PAFFY_STATS) | (dechunk ? 1u << PAFFY_CHECK : 0u) |
                                (s.has_fixed ? 1u << PAFFY_TRIM_FIXED : 0u);
    bool lean_or_filter = n_stages > 0;
    for (int32_t i = 0; i < n_stages; i++) lean_or_filter = lean_or_filter && ((flat_kinds >> norm[i].kind) & 1u);
    static const bool flat_off = getenv("PAFFY_NO_FLAT") != nullptr;
    /* `paffy add_mismatches` alone (BASELINE cfg4): the same parse, the encoder on the pieces (flat_add_kernel.h) */
    if (n_stages == 1 && norm[0].kind == PAFFY_ADD_MISMATCHES && s.nocheck_mask == 0 && !flat_off && c->n_seqs > 0) s.flat = FLAT_MODE_ADD;
    /* `paffy add_mismatches -a` alone, with its paf_check: the same parse, the runs merged across the pieces (flat_remove_kernel.h) */
    else if (n_stages == 1 && norm[0].kind == PAFFY_REMOVE_MISMATCHES && s.nocheck_mask == 0 && !flat_off) s.flat = FLAT_MODE_REMOVE;
    /* `paffy view` when it prints no rows: the sums of the encoded records, nothing else (flat_view_kernel.h); only for a caller that
       has said so -- without the setting [ADD, STATS] leaves ops and a line plan behind, and goes through the record kernels */
    else if (c->stats_only && n_stages == 2 && norm[0].kind == PAFFY_ADD_MISMATCHES && norm[1].kind == PAFFY_STATS && s.nocheck_mask == 0 && !flat_off && c->n_seqs > 0)
        s.flat = FLAT_MODE_VIEW;
    /* [ADD, TRIM_IDENTITY], [ADD, FILTER], [ADD, TRIM_IDENTITY, FILTER] (`paffy add_mismatches | paffy trim -r | paffy filter`): the encoder on
       the pieces, the trim and the filter on the summaries of the new ops (flat_add_pipe_kernel.h); every other list with add_mismatches and
       a further stage stays with the record kernels */
    else if (norm[0].kind == PAFFY_ADD_MISMATCHES && s.nocheck_mask == 0 && !flat_off && c->n_seqs > 0 &&
             ((n_stages == 2 && (norm[1].kind == PAFFY_TRIM_IDENTITY || norm[1].kind == PAFFY_FILTER)) ||
              (n_stages == 3 && norm[1].kind == PAFFY_TRIM_IDENTITY && norm[2].kind == PAFFY_FILTER)))
        s.flat = FLAT_MODE_ADD_PIPE;
    else if (lean_or_filter && s.nocheck_mask == 0 && !flat_off) s.flat = FLAT_MODE_PASS;
    s.has_fixed = s.has_fixed && s.flat == FLAT_MODE_PASS;
    for (int32_t i = 0; i + 1 < n_stages; i++) s.fixed_inner = s.fixed_inner || (s.has_fixed && norm[i].kind == PAFFY_TRIM_FIXED);
    /* the first instantiation that knows every stage kind: the lean kinds; them and add_mismatches (the encoder wants the registers); them
       with filter / trim -f / stats / check; no stage of the kinds that came with the encoder; all */
    s.size_mask = PAFFY_MASK_ALL;
    for (uint32_t m : {PAFFY_MASK_LEAN, PAFFY_MASK_ADD, PAFFY_MASK_SEL, PAFFY_MASK_PLAIN})
        if ((kinds & ~m) == 0) {
            s.size_mask = m;
            break;
        }
    return 0;
}

/* the record kernels' parameters for the batch at in (c->kp), with the sequence lookup of add_mismatches and the stats stage's sums */
static int record_params(paffy_hip_ctx *c, const StageClass &s, const uint8_t *in, uint32_t len, uint32_t n_lines) {
    KParams &kp = c->kp;
    kp.in = in;
    kp.in_len = len;
    kp.n_rec = n_lines;
    kp.meta = static_cast<const RecMeta *>(c->meta.p);
    for (int32_t i = 0; i < s.n_stages; i++) kp.stages[i] = s.stages[i];
    kp.n_stages = s.n_stages;
    kp.nocheck_mask = s.nocheck_mask;
    kp.out_len = static_cast<int64_t *>(c->out_len.p);
    kp.out_rows = static_cast<int64_t *>(c->out_rows.p);
    kp.status = static_cast<uint32_t *>(c->status.p);
    kp.err_aux = static_cast<int32_t *>(c->err_aux.p);
    kp.n_ops = static_cast<uint32_t *>(c->n_ops.p);
    kp.arena_off = static_cast<uint64_t *>(c->arena_off.p);
    kp.rec_plan = c->rec_plan.p;
    kp.ops_mirror = static_cast<uint32_t *>(c->ops_mirror.p);
    c->plan_seq_lookup = s.need_seqs && n_lines > 0;
    if (s.need_seqs && n_lines > 0) {
        if (ensure(c, c->rec_qseq, sizeof(int32_t) * (size_t)(n_lines + 1))) return PAFFY_E_HIP;
        if (ensure(c, c->rec_tseq, sizeof(int32_t) * (size_t)(n_lines + 1))) return PAFFY_E_HIP;
        LAUNCH(c, "k_seq_lookup", k_seq_lookup, dim3((n_lines + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, in,
               static_cast<const RecMeta *>(c->meta.p), n_lines, static_cast<const uint8_t *>(c->seq_names.p),
               static_cast<const uint32_t *>(c->seq_name_off.p), c->n_seqs, static_cast<int32_t *>(c->rec_qseq.p),
               static_cast<int32_t *>(c->rec_tseq.p));
        kp.seq_base = static_cast<const uint8_t *>(c->seq_blob.p);
        kp.seq_comp = static_cast<const uint8_t *>(c->seq_comp.p);
        kp.seqs = static_cast<const SeqEntry *>(c->seq_table.p);
        kp.rec_qseq = static_cast<const int32_t *>(c->rec_qseq.p);
        kp.rec_tseq = static_cast<const int32_t *>(c->rec_tseq.p);
    }
    kp.out_off = static_cast<const int64_t *>(c->out_off.p);
    kp.w_list = static_cast<uint32_t *>(c->w_list.p);
    kp.b_list[0] = static_cast<uint32_t *>(c->b_list.p);
    kp.b_list[1] = static_cast<uint32_t *>(c->b_list1.p);
    kp.info = static_cast<DevInfo *>(c->info.p);
    kp.filter = c->filter;
    for (int32_t i = 0; i < s.n_stages; i++)
        if (s.stages[i].kind == PAFFY_STATS && n_lines > 0) {
            if (ensure(c, c->rec_stats, sizeof(int64_t) * 6 * (size_t)n_lines)) return PAFFY_E_HIP;
            kp.rec_stats = static_cast<int64_t *>(c->rec_stats.p);
            HIPCHK(c, hipMemsetAsync(c->rec_stats.p, 0, sizeof(int64_t) * 6 * (size_t)n_lines, c->stream)); /* records that stop before the stage */
        }
    return 0;
}

/* the offsets of the lines and the emit order (long lines first): the scan rides along, one host synchronisation per plan in the usual case */
static int post_scans(paffy_hip_ctx *c, uint32_t n_lines) {
    KParams &kp = c->kp;
    const uint32_t n_blocks = (n_lines + SCAN_BLOCK - 1) / SCAN_BLOCK;
    if (ensure(c, c->scan_part, sizeof(int64_t) * 2 * (size_t)n_blocks)) return PAFFY_E_HIP;
    LAUNCH(c, "k_scan_part", k_scan_part, dim3(n_blocks), dim3(PAFFY_NT), 0, kp.out_len, kp.out_rows, n_lines,
           static_cast<int64_t *>(c->out_off.p), static_cast<int64_t *>(c->scan_part.p), kp.info);
    LAUNCH(c, "k_scan_fix", k_scan_fix, dim3(n_blocks), dim3(PAFFY_NT), 0, n_lines, n_blocks, static_cast<int64_t *>(c->out_off.p),
           static_cast<const int64_t *>(c->scan_part.p), kp.info);
    if (ensure(c, c->emit_order, sizeof(uint32_t) * (size_t)n_lines)) return PAFFY_E_HIP;
    if (ensure(c, c->order_cnt, sizeof(uint32_t) * 2 * ORDER_CLASSES)) return PAFFY_E_HIP;
    uint32_t *cnt = static_cast<uint32_t *>(c->order_cnt.p);
    HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(uint32_t) * 2 * ORDER_CLASSES, c->stream));
    const uint32_t g = (n_lines + PAFFY_NT - 1) / PAFFY_NT;
    LAUNCH(c, "k_order_count", k_order_count, dim3(g), dim3(PAFFY_NT), 0, kp.out_len, n_lines, 14u, cnt);
    LAUNCH(c, "k_order_scatter", k_order_scatter, dim3(g), dim3(PAFFY_NT), 0, kp.out_len, n_lines, 14u, cnt, cnt + ORDER_CLASSES,
           static_cast<uint32_t *>(c->emit_order.p));
    kp.emit_order = static_cast<const uint32_t *>(c->emit_order.p);
    return 0;
}

static FlatParams flat_params(const paffy_hip_ctx *c, uint32_t items_mode) {
    const KParams &kp = c->kp;
    FlatParams fp;
    fp.in = kp.in;
    fp.in_len = kp.in_len;
    fp.meta = kp.meta;
    fp.chunk_rec = static_cast<const uint32_t *>(c->flat_chunks.p);
    fp.n_chunk_slots = c->flat_chunk_slots;
    fp.nd = static_cast<const uint16_t *>(c->flat_nd.p);
    fp.sums = static_cast<PieceSum *>(c->flat_sums.p);
    fp.ops_mirror = kp.ops_mirror;
    fp.info = kp.info;
    fp.items_mode = items_mode;
    return fp;
}

/* `paffy add_mismatches` alone: the flat parse, then the encoder on its pieces, repeated with more scratch while a batch asks for more.
   pipe: stages stand behind it (FLAT_MODE_ADD_PIPE) -- the same tries, with the two kernels of flat_add_pipe_kernel.h in the place of
   k_add_fill and k_add_final. *need_records: the encoder left records to the record kernels. */
static int plan_flat_add(paffy_hip_ctx *c, uint32_t n_lines, bool *need_records, bool pipe = false) {
    KParams &kp = c->kp;
    const uint32_t len = kp.in_len;
    const FlatParams fp = flat_params(c, 1u);
    LAUNCH(c, "k_flat_parse", k_flat_parse<1u>, dim3(2048), dim3(64 * FLAT_PARSE_WAVES), 0, fp);
    const uint32_t n_slots = c->flat_piece_slots, n_sblocks = (n_slots + SCAN32_BLOCK - 1) / SCAN32_BLOCK;
    if (ensure(c, c->add_pieces, sizeof(AddPiece) * (size_t)n_slots) || ensure(c, c->add_scr_cnt, sizeof(uint32_t) * (size_t)n_slots) ||
        ensure(c, c->add_scr_off, sizeof(uint64_t) * (size_t)n_slots) || ensure(c, c->add_new_cnt, sizeof(uint32_t) * (size_t)n_slots) ||
        ensure(c, c->add_new_off, sizeof(uint64_t) * (size_t)n_slots) || ensure(c, c->add_text, sizeof(uint32_t) * (size_t)n_slots) ||
        ensure(c, c->add_bad, sizeof(uint32_t) * (size_t)(n_lines + 1)) || ensure(c, c->add_part, sizeof(uint64_t) * (size_t)(n_sblocks + 1)))
        return PAFFY_E_HIP;
    if (pipe && ensure(c, c->add_nsums, sizeof(PieceSum) * (size_t)n_slots)) return PAFFY_E_HIP;
    /* item words + passed-through ops, and the new 4-byte ops: about 2.4 and 2.9 bytes per byte of text for 2 %-divergent sequences; a
       batch that needs more is encoded again with what it asked for (the totals come back with the plan's one synchronisation) */
    size_t scr_words = std::max<size_t>(c->add_scratch.cap / 4, (size_t)len + ((size_t)1 << 20)), new_words = std::max<size_t>(c->add_new_ops.cap / 4, (size_t)len + ((size_t)1 << 20));
    for (int attempt = 0;; attempt++) {
        if (ensure(c, c->add_scratch, 4 * scr_words) || ensure(c, c->add_new_ops, 4 * new_words)) return PAFFY_E_HIP;
        AddParams ap;
        ap.P = kp;
        ap.sums = fp.sums;
        ap.pieces = static_cast<AddPiece *>(c->add_pieces.p);
        ap.n_piece_slots = n_slots;
        ap.scr_cnt = static_cast<uint32_t *>(c->add_scr_cnt.p);
        ap.scr_off = static_cast<const uint64_t *>(c->add_scr_off.p);
        ap.scratch = static_cast<uint32_t *>(c->add_scratch.p);
        ap.scr_cap = c->add_scratch.cap / 4;
        ap.new_cnt = static_cast<uint32_t *>(c->add_new_cnt.p);
        ap.new_off = static_cast<const uint64_t *>(c->add_new_off.p);
        ap.new_ops = static_cast<uint32_t *>(c->add_new_ops.p);
        ap.new_cap = c->add_new_ops.cap / 4;
        ap.text_cnt = static_cast<uint32_t *>(c->add_text.p);
        ap.rec_bad = static_cast<uint32_t *>(c->add_bad.p);
        ap.flat_done = static_cast<uint8_t *>(c->flat_done.p);
        { /* segments of the lines that become more than PAFFY_ROWS_MAX_OPS ops. A segment closes only when the next piece would take it
             past ADD_SEG_OPS (16 384), so two neighbouring segments hold more than 16 384 new ops and a line of T new ops has at most
             T / 8192 + 1 segments. new_words / 8192 covers the first term of every line; the list runs out only when more lines than
             len / 16 384 + 64 + (new_words - total) / 8192 use their "+ 1". A line does that with five segments over a little more than
             32 768 new ops (pieces of about 0, 16 400, 200, 16 400, 200 new ops), which takes 3 KiB of text: 4.03 x 1.125 + 0.19 < 5
             once the second try has sized new_words to 1.125 x total, so some 250 such lines in a batch overflow it. That is left so:
             k_add_final gives the lines that find no room to the record kernels, marks the slots they reserved inside the list, and
             n_items is cut to the list below (test_gpu_flat_edges.py::test_add_item_list_overflow_goes_to_the_record_kernels). */
            const size_t items_cap = new_words / (PAFFY_ROWS_MAX_OPS / 4u) + ((size_t)len >> 14) + 64;
            if (ensure(c, c->flat_items, sizeof(EmitItem) * items_cap)) return PAFFY_E_HIP;
            kp.items = static_cast<EmitItem *>(c->flat_items.p);
            kp.items_cap = (uint32_t)items_cap;
            ap.P = kp;
        }
        HIPCHK(c, hipMemsetAsync(c->add_pieces.p, 0xff, sizeof(AddPiece) * (size_t)n_slots, c->stream)); /* rec = FLAT_NO_CHUNK */
        HIPCHK(c, hipMemsetAsync(c->add_scr_cnt.p, 0, sizeof(uint32_t) * (size_t)n_slots, c->stream));
        HIPCHK(c, hipMemsetAsync(c->add_new_cnt.p, 0, sizeof(uint32_t) * (size_t)n_slots, c->stream));
        LAUNCH(c, "k_add_prep", k_add_prep, dim3((n_lines + 255) / 256), dim3(256), 0, ap);
        LAUNCH(c, "k_scan32_part", k_scan32_part, dim3(n_sblocks), dim3(256), 0, ap.scr_cnt, n_slots, static_cast<uint64_t *>(c->add_scr_off.p), static_cast<uint64_t *>(c->add_part.p));
        LAUNCH(c, "k_scan32_fix", k_scan32_fix, dim3(n_sblocks), dim3(256), 0, n_slots, n_sblocks, static_cast<uint64_t *>(c->add_scr_off.p), static_cast<const uint64_t *>(c->add_part.p),
               reinterpret_cast<uint64_t *>(&static_cast<DevInfo *>(c->info.p)->add_scr_total));
        LAUNCH(c, "k_add_count", k_add_count, dim3(2048), dim3(64 * ADD_WAVES), 0, ap);
        LAUNCH(c, "k_scan32_part", k_scan32_part, dim3(n_sblocks), dim3(256), 0, ap.new_cnt, n_slots, static_cast<uint64_t *>(c->add_new_off.p), static_cast<uint64_t *>(c->add_part.p));
        LAUNCH(c, "k_scan32_fix", k_scan32_fix, dim3(n_sblocks), dim3(256), 0, n_slots, n_sblocks, static_cast<uint64_t *>(c->add_new_off.p), static_cast<const uint64_t *>(c->add_part.p),
               reinterpret_cast<uint64_t *>(&static_cast<DevInfo *>(c->info.p)->add_new_total));
        if (pipe) {
            AddPipeParams pp;
            pp.A = ap;
            pp.nsums = static_cast<PieceSum *>(c->add_nsums.p);
            LAUNCH(c, "k_addp_fill", k_addp_fill, dim3(2048), dim3(64 * ADD_WAVES), 0, pp);
            LAUNCH(c, "k_addp_size", k_addp_size, dim3(std::min<uint32_t>(2048u, (n_lines + ADDP_SIZE_WAVES - 1) / ADDP_SIZE_WAVES)), dim3(64 * ADDP_SIZE_WAVES), 0, pp);
        } else {
            LAUNCH(c, "k_add_fill", k_add_fill, dim3(2048), dim3(64 * ADD_WAVES), 0, ap);
            LAUNCH(c, "k_add_final", k_add_final, dim3((n_lines + 255) / 256), dim3(256), 0, ap);
        }
        kp.new_ops = ap.new_ops;
        if (post_scans(c, n_lines)) return PAFFY_E_HIP;
        if (fetch_info(c)) return PAFFY_E_HIP;
        kp.n_items = std::min(c->h_info->n_items, kp.items_cap); /* reservations past the list's end were not written (k_add_final) */
        if (c->h_info->add_scr_total <= ap.scr_cap && c->h_info->add_new_total <= ap.new_cap) break;
        if (attempt == 2) {
            c->last_error = "add_mismatches: the scratch demand kept growing";
            return PAFFY_E_HIP;
        }
        scr_words = std::max<size_t>(scr_words, (size_t)c->h_info->add_scr_total + ((size_t)c->h_info->add_scr_total >> 3) + 1024);
        new_words = std::max<size_t>(new_words, (size_t)c->h_info->add_new_total + ((size_t)c->h_info->add_new_total >> 3) + 1024);
        DevInfo z = *c->h_info; /* once more: nothing of the first try counts */
        z.flat_legacy = 0;
        z.n_items = 0;
        z.out_bytes = z.out_rows = 0;
        HIPCHK(c, hipMemcpyAsync(c->info.p, &z, sizeof(z), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    *need_records = c->h_info->flat_legacy > 0;
    c->flat_left = c->h_info->flat_legacy;
    if (pipe)
        for (int k = 0; k < 16; k++) c->flat_reasons[k] = c->h_info->flat_reason[k];
    kp.flat_done = static_cast<const uint8_t *>(c->flat_done.p);
    return 0;
}

/* `paffy add_mismatches -a` alone: the flat parse, then the merge of the M/=/X runs on its pieces. One pass: the new cigar never has more
   ops than the old one and an op takes two bytes of text at least, so len / 2 words always hold the new ops of a batch.
   *need_records: records were left to the record kernels. */
static int plan_flat_remove(paffy_hip_ctx *c, uint32_t n_lines, bool *need_records) {
    KParams &kp = c->kp;
    const uint32_t len = kp.in_len;
    const FlatParams fp = flat_params(c, 0u);
    LAUNCH(c, "k_flat_parse", k_flat_parse<0u>, dim3(2048), dim3(64 * FLAT_PARSE_WAVES), 0, fp);
    const uint32_t n_slots = c->flat_piece_slots, n_sblocks = (n_slots + SCAN32_BLOCK - 1) / SCAN32_BLOCK;
    static_assert(sizeof(RmEdge) == sizeof(uint64_t), "the edges take the encoder's scratch offsets");
    if (ensure(c, c->add_pieces, sizeof(AddPiece) * (size_t)n_slots) || ensure(c, c->add_scr_cnt, sizeof(uint32_t) * (size_t)n_slots) ||
        ensure(c, c->add_scr_off, sizeof(RmEdge) * (size_t)n_slots) || ensure(c, c->add_new_cnt, sizeof(uint32_t) * (size_t)n_slots) ||
        ensure(c, c->add_new_off, sizeof(uint64_t) * (size_t)n_slots) || ensure(c, c->add_text, sizeof(uint32_t) * (size_t)n_slots) ||
        ensure(c, c->add_bad, sizeof(uint32_t) * (size_t)(n_lines + 1)) || ensure(c, c->add_part, sizeof(uint64_t) * (size_t)(n_sblocks + 1)) ||
        ensure(c, c->add_new_ops, 4 * ((size_t)len / 2 + 1024)))
        return PAFFY_E_HIP;
    /* segments of the lines of more than PAFFY_ROWS_MAX_OPS new ops. As in plan_flat_add two neighbouring segments hold more than
       ADD_SEG_OPS (16 384) new ops, so a line of T new ops has at most T / 8192 + 1 segments. Here the bounds are hard: all lines
       together have at most len / 2 new ops (len >> 14 segments), and a line with segments has more than 32 768 ops, 64 KiB of text,
       so at most len >> 16 lines add their "+ 1". The list cannot run out; n_items is clamped all the same. */
    const size_t items_cap = ((size_t)len >> 14) + ((size_t)len >> 16) + 16;
    if (ensure(c, c->flat_items, sizeof(EmitItem) * items_cap)) return PAFFY_E_HIP;
    kp.items = static_cast<EmitItem *>(c->flat_items.p);
    kp.items_cap = (uint32_t)items_cap;
    RmParams rp;
    memset(&rp, 0, sizeof(rp));
    AddParams &ap = rp.A;
    ap.P = kp;
    ap.sums = fp.sums;
    ap.pieces = static_cast<AddPiece *>(c->add_pieces.p);
    ap.n_piece_slots = n_slots;
    ap.new_cnt = static_cast<uint32_t *>(c->add_new_cnt.p);
    ap.new_off = static_cast<const uint64_t *>(c->add_new_off.p);
    ap.new_ops = static_cast<uint32_t *>(c->add_new_ops.p);
    ap.new_cap = c->add_new_ops.cap / 4;
    ap.text_cnt = static_cast<uint32_t *>(c->add_text.p);
    ap.rec_bad = static_cast<uint32_t *>(c->add_bad.p);
    ap.flat_done = static_cast<uint8_t *>(c->flat_done.p);
    rp.edges = static_cast<RmEdge *>(c->add_scr_off.p);
    rp.carry = static_cast<uint32_t *>(c->add_scr_cnt.p);
    HIPCHK(c, hipMemsetAsync(c->add_pieces.p, 0xff, sizeof(AddPiece) * (size_t)n_slots, c->stream)); /* rec = FLAT_NO_CHUNK */
    HIPCHK(c, hipMemsetAsync(c->add_new_cnt.p, 0, sizeof(uint32_t) * (size_t)n_slots, c->stream));
    LAUNCH(c, "k_rm_prep", k_rm_prep, dim3((n_lines + 255) / 256), dim3(256), 0, rp);
    LAUNCH(c, "k_rm_edges", k_rm_edges, dim3(2048), dim3(64 * ADD_WAVES), 0, rp);
    LAUNCH(c, "k_rm_carry", k_rm_carry, dim3((n_lines + 255) / 256), dim3(256), 0, rp);
    LAUNCH(c, "k_scan32_part", k_scan32_part, dim3(n_sblocks), dim3(256), 0, ap.new_cnt, n_slots, static_cast<uint64_t *>(c->add_new_off.p), static_cast<uint64_t *>(c->add_part.p));
    LAUNCH(c, "k_scan32_fix", k_scan32_fix, dim3(n_sblocks), dim3(256), 0, n_slots, n_sblocks, static_cast<uint64_t *>(c->add_new_off.p), static_cast<const uint64_t *>(c->add_part.p),
           static_cast<uint64_t *>(nullptr));
    LAUNCH(c, "k_rm_fill", k_rm_fill, dim3(2048), dim3(64 * ADD_WAVES), 0, rp);
    LAUNCH(c, "k_add_final", k_add_final, dim3((n_lines + 255) / 256), dim3(256), 0, ap);
    kp.new_ops = ap.new_ops;
    if (post_scans(c, n_lines)) return PAFFY_E_HIP;
    if (fetch_info(c)) return PAFFY_E_HIP;
    kp.n_items = std::min(c->h_info->n_items, kp.items_cap);
    *need_records = c->h_info->flat_legacy > 0;
    c->flat_left = c->h_info->flat_legacy;
    kp.flat_done = static_cast<const uint8_t *>(c->flat_done.p);
    return 0;
}

/* [ADD_MISMATCHES, STATS] under paffy_hip_stats_only: the flat parse, then the count walk on its pieces. No scratch and no new ops, so
   no capacity to run out of and one pass. *need_records: records were left to the record kernels (which then also reduce the sums). */
static int plan_flat_view(paffy_hip_ctx *c, uint32_t n_lines, bool *need_records) {
    KParams &kp = c->kp;
    const FlatParams fp = flat_params(c, 0u);
    LAUNCH(c, "k_flat_parse", k_flat_parse<0u>, dim3(2048), dim3(64 * FLAT_PARSE_WAVES), 0, fp);
    const uint32_t n_slots = c->flat_piece_slots;
    if (ensure(c, c->add_pieces, sizeof(AddPiece) * (size_t)n_slots) || ensure(c, c->view_sums, sizeof(ViewSum) * (size_t)n_slots) ||
        ensure(c, c->add_bad, sizeof(uint32_t) * (size_t)(n_lines + 1)))
        return PAFFY_E_HIP;
    ViewParams vp;
    memset(&vp, 0, sizeof(vp));
    AddParams &ap = vp.A;
    ap.P = kp;
    ap.sums = fp.sums;
    ap.pieces = static_cast<AddPiece *>(c->add_pieces.p);
    ap.n_piece_slots = n_slots;
    ap.rec_bad = static_cast<uint32_t *>(c->add_bad.p);
    ap.flat_done = static_cast<uint8_t *>(c->flat_done.p);
    vp.vsum = static_cast<ViewSum *>(c->view_sums.p);
    HIPCHK(c, hipMemsetAsync(c->add_pieces.p, 0xff, sizeof(AddPiece) * (size_t)n_slots, c->stream)); /* rec = FLAT_NO_CHUNK */
    LAUNCH(c, "k_view_prep", k_view_prep, dim3((n_lines + 255) / 256), dim3(256), 0, vp);
    LAUNCH(c, "k_view_count", k_view_count, dim3(2048), dim3(64 * ADD_WAVES), 0, vp);
    LAUNCH(c, "k_view_final", k_view_final, dim3((n_lines + 255) / 256), dim3(256), 0, vp);
    if (post_scans(c, n_lines)) return PAFFY_E_HIP;
    if (fetch_info(c)) return PAFFY_E_HIP;
    *need_records = c->h_info->flat_legacy > 0;
    c->flat_left = c->h_info->flat_legacy;
    kp.flat_done = static_cast<const uint8_t *>(c->flat_done.p);
    if (!*need_records) { /* the batch's sums (the record kernels' launch chain does this when it runs) */
        LAUNCH(c, "k_stats_reduce", k_stats_reduce, dim3(std::min<uint32_t>(512u, (n_lines + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, kp.rec_stats, n_lines,
               static_cast<DevInfo *>(c->info.p)->stats);
        if (fetch_info(c)) return PAFFY_E_HIP;
    }
    return 0;
}

/* the flat pass: *need_records as above; *g_count = the records it left to the four-wave writers */
static int plan_flat(paffy_hip_ctx *c, const StageClass &s, uint32_t n_lines, bool *need_records, uint32_t *g_count) {
    KParams &kp = c->kp;
    const uint32_t len = kp.in_len;
    const FlatParams fp = flat_params(c, s.has_stats ? 2u : 0u);
    /* persistent waves over the chunks: eight workgroups of four waves per CU */
    if (s.has_stats) LAUNCH(c, "k_flat_parse", k_flat_parse<2u>, dim3(2048), dim3(64 * FLAT_PARSE_WAVES), 0, fp);
    else LAUNCH(c, "k_flat_parse", k_flat_parse<0u>, dim3(2048), dim3(64 * FLAT_PARSE_WAVES), 0, fp);
    /* segments of the shatter records too long for one wave of the row writer: a record of more than PAFFY_ROWS_MAX_OPS ops has
       2 x that many cigar bytes at least, a segment holds half that many ops */
    const size_t items_cap = ((size_t)len >> 15) + ((size_t)len >> 16) + 16;
    if (ensure(c, c->flat_items, sizeof(EmitItem) * items_cap)) return PAFFY_E_HIP;
    kp.items = static_cast<EmitItem *>(c->flat_items.p);
    kp.items_cap = (uint32_t)items_cap;
    if (s.has_shatter) { /* the constant pieces of a shatter record's rows, 144 bytes per record (lane_row_pieces, flat_kernel.h) */
        if (ensure(c, c->flat_pieces, FLAT_ROW_PIECES_BYTES * (size_t)(n_lines + 1))) return PAFFY_E_HIP;
        kp.row_pieces = static_cast<uint8_t *>(c->flat_pieces.p);
    }
    FlatSizeParams fs;
    fs.P = kp;
    fs.sums = fp.sums;
    fs.flat_done = static_cast<uint8_t *>(c->flat_done.p);
    if (ensure(c, c->flat_rec, sizeof(uint32_t) * (size_t)(n_lines + 1))) return PAFFY_E_HIP;
    fs.defer = static_cast<uint32_t *>(c->flat_rec.p);
    /* one lane per record for the records that need little, one wave per record for the rest (a list whose length only the device knows) */
    if (s.has_fixed) { /* one wave per record for all of them */
        if (s.fixed_inner) LAUNCH(c, "k_flat_size", k_flat_size<2>, dim3(std::min<uint32_t>(2048u, (n_lines + FLAT_SIZE_WAVES - 1) / FLAT_SIZE_WAVES)), dim3(64 * FLAT_SIZE_WAVES), 0, fs);
        else LAUNCH(c, "k_flat_size", k_flat_size<1>, dim3(std::min<uint32_t>(2048u, (n_lines + FLAT_SIZE_WAVES - 1) / FLAT_SIZE_WAVES)), dim3(64 * FLAT_SIZE_WAVES), 0, fs);
    } else {
        LAUNCH(c, "k_flat_lane", k_flat_lane, dim3((n_lines + 255) / 256), dim3(256), 0, fs);
        LAUNCH(c, "k_flat_size", k_flat_size<0>, dim3(std::min<uint32_t>(2048u, (n_lines + FLAT_SIZE_WAVES - 1) / FLAT_SIZE_WAVES)), dim3(64 * FLAT_SIZE_WAVES), 0, fs);
    }
    if (post_scans(c, n_lines)) return PAFFY_E_HIP;
    if (fetch_info(c)) return PAFFY_E_HIP;
    *g_count = c->h_info->g_count;
    kp.n_items = std::min(c->h_info->n_items, kp.items_cap);
    *need_records = c->h_info->flat_legacy > 0;
    c->flat_left = c->h_info->flat_legacy;
    for (int k = 0; k < 16; k++) c->flat_reasons[k] = c->h_info->flat_reason[k];
    kp.flat_done = static_cast<const uint8_t *>(c->flat_done.p);
    if (kp.rec_stats && !*need_records) { /* the batch's sums (the record kernels' launch chain does this when it runs) */
        LAUNCH(c, "k_stats_reduce", k_stats_reduce, dim3(std::min<uint32_t>(512u, (n_lines + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, kp.rec_stats, n_lines,
               static_cast<DevInfo *>(c->info.p)->stats);
        if (fetch_info(c)) return PAFFY_E_HIP;
    }
    return 0;
}

/* the record kernels, sizing again with a larger arena while a batch asks for more; lvl0_long: the batch started at the longer first
   store level; flat_g_count: the records the flat pass left to the four-wave writers */
static int plan_records(paffy_hip_ctx *c, const StageClass &s, uint32_t n_lines, bool lvl0_long, uint32_t flat_g_count) {
    KParams &kp = c->kp;
    if (s.flat == FLAT_MODE_NONE) { /* launch order of the sizing workgroups: long cigars first (out_len is scratch until the sizing pass fills it) */
        if (ensure(c, c->emit_order, sizeof(uint32_t) * (size_t)n_lines)) return PAFFY_E_HIP;
        if (ensure(c, c->order_cnt, sizeof(uint32_t) * 2 * ORDER_CLASSES)) return PAFFY_E_HIP;
        uint32_t *cnt = static_cast<uint32_t *>(c->order_cnt.p);
        HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(uint32_t) * 2 * ORDER_CLASSES, c->stream));
        const uint32_t g = (n_lines + PAFFY_NT - 1) / PAFFY_NT;
        LAUNCH(c, "k_cigar_bytes", k_cigar_bytes, dim3(g), dim3(PAFFY_NT), 0, kp.meta, n_lines, kp.out_len);
        LAUNCH(c, "k_order_count", k_order_count, dim3(g), dim3(PAFFY_NT), 0, kp.out_len, n_lines, 9u, cnt);
        LAUNCH(c, "k_order_scatter", k_order_scatter, dim3(g), dim3(PAFFY_NT), 0, kp.out_len, n_lines, 9u, cnt, cnt + ORDER_CLASSES,
               static_cast<uint32_t *>(c->emit_order.p));
        kp.size_order = static_cast<const uint32_t *>(c->emit_order.p); /* any permutation serves a repeated sizing pass too */
    }
    /* add_mismatches keeps one word per 16 columns and the new 4-byte ops of every record in the arena: about eight times
       the text for 2 %-divergent sequences; start there instead of finding out through repeated passes */
    if (s.need_seqs && ensure(c, c->arena, (size_t)kp.in_len * 8 + ((size_t)8 << 20))) return PAFFY_E_HIP;
    const int max_attempts = 6;
    for (int attempt = 0; attempt < max_attempts; attempt++) {
        kp.arena = static_cast<uint64_t *>(c->arena.p);
        kp.arena_cap = c->arena.cap / 8;
        kp.ops_cap = PAFFY_OPS_CAP;
        kp.next_cap = 0;
        kp.level = 0;
        /* records with at most WAVE_MAX_BYTES cigar bytes (about WAVE_OPS_CAP ops at three bytes per op) are sized one wave per record;
           denser cigars of that length overflow the wave's store and are redone by the four-wave build. add_mismatches rebuilds the op
           array: when a stage follows it the new array must fit the store, so only pipes that end with it take the one-wave build. */
        kp.wave_max_bytes = s.add_not_last ? 0u : WAVE_MAX_BYTES;
        {
            int rc = size_records_for(c, s.size_mask, kp, n_lines);
            if (rc) return rc;
        }
        LAUNCH(c, "k_arena_size", k_arena_size, dim3(2048), dim3(PAFFY_NT), PAFFY_SIZE_LDS_BYTES, kp);
        if (kp.rec_stats)
            LAUNCH(c, "k_stats_reduce", k_stats_reduce, dim3(std::min<uint32_t>(512u, (n_lines + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, kp.rec_stats, n_lines,
                   static_cast<DevInfo *>(c->info.p)->stats);
        if (post_scans(c, n_lines)) return PAFFY_E_HIP;
        if (fetch_info(c)) return PAFFY_E_HIP;
        if (c->h_info->arena_used <= kp.arena_cap) {
            if (lvl0_long && c->h_info->lvl0_over > 0) { /* denser cigars than the longer first level takes: back to the safe bound, for good */
                c->lvl0_long_ok = false;
                c->lvl0_long_off = true;
            } else if (kp.lvl0_long_bytes) { /* the safe bound was in force and the second level kept count */
                c->lvl0_long_ok = c->h_info->lvl0_probe_dense == 0;
            }
            return 0;
        }
        /* arena too small: grow to the demand seen so far and redo the sizing pass */
        /* a record that found no room stopped asking, so the demand seen is a lower bound: at least double what there was */
        size_t need = (size_t)c->h_info->arena_used * 8 * 2;
        if (need < c->arena.cap * 2) need = c->arena.cap * 2;
        if (ensure(c, c->arena, need)) return PAFFY_E_HIP;
        DevInfo z = *c->h_info;
        z.arena_used = 0;
        z.w_count = 0;
        z.g_count = flat_g_count; /* the records the flat pass left to the four-wave writers stay counted */
        z.b_count[1] = 0; /* b_count[0] was filled by k_header and stays */
        for (int k = 0; k < 6; k++) z.stats[k] = 0;
        z.first_err_key = ~0ull;
        z.out_bytes = z.out_rows = 0;
        HIPCHK(c, hipMemcpyAsync(c->info.p, &z, sizeof(z), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->last_error = "arena demand kept growing";
    return PAFFY_E_HIP;
}

/* the plan's totals and its first failing record, from the DevInfo fetched last */
static int plan_finish(paffy_hip_ctx *c, uint32_t n_lines, paffy_plan_info *info) {
    if (c->profile) prof_collect(c);
    if (c->h_info->internal) {
        char buf[128];
        snprintf(buf, sizeof(buf), "internal limit hit (flags 0x%x): record pieces longer than the LDS staging area", c->h_info->internal);
        c->last_error = buf;
        return PAFFY_E_UNSUPPORTED;
    }
    paffy_plan_info &pl = c->plan;
    pl.n_records = n_lines;
    pl.n_rows = (int64_t)c->h_info->out_rows;
    pl.out_bytes = (int64_t)c->h_info->out_bytes;
    if (c->h_info->first_err_key != ~0ull) {
        unsigned long long k = c->h_info->first_err_key;
        pl.error.code = (int32_t)(k & 0xff);
        pl.error.stage = (int32_t)((k >> 8) & 0xff) - 1;
        pl.error.record = (int64_t)(k >> 16);
        if (pl.error.code == PAFFY_ERR_DECHUNK_HEADER) pl.error.stage = 0; /* k_dechunk's verdict travels with the parse's (RecMeta::err) */
        int32_t aux = 0;
        HIPCHK(c, hipMemcpy(&aux, static_cast<int32_t *>(c->err_aux.p) + pl.error.record, sizeof(aux), hipMemcpyDeviceToHost));
        pl.error.aux = aux;
    }
    *info = pl;
    c->planned = true;
    return 0;
}

int paffy_hip_plan(paffy_hip_ctx *c, const paffy_stage *stages, int32_t n_stages, const void *d_in, int64_t in_len,
                   paffy_plan_info *info) {
    if (!c || !info || (n_stages > 0 && !stages) || n_stages < 0 || n_stages > PAFFY_MAX_STAGES) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    StageClass s;
    int rc = classify_stages(c, stages, n_stages, s);
    if (rc) return rc;
    if (s.upconvert) return upconvert_plan(c, d_in, in_len, (s.nocheck_mask & 1u) == 0, info);
    plan_begin(c, PLAN_RECORDS, in_len, info);
    if (in_len == 0) {
        c->planned = true;
        return 0;
    }
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    const uint32_t len = (uint32_t)in_len;
    /* Cigars of more than 2 x lvl0_max bytes start at the second store level (k_header queues them), whose 64 KB of ops leave a CU two
       workgroups: on cfg3 / cfg4 the 7 % of the records there cost as much kernel time as all the others. Two bytes per op is the bound
       that can never overflow the first level's 8 192-op store, but a cigar of the usual density (2.5-3 bytes per op) fits it up to about
       LVL0_LONG_BYTES. So a context starts with the safe bound and lets the second level count the records that would have overflowed the
       longer one (DevInfo::lvl0_probe_dense); a batch without any switches the following batches to the longer first level (cfg4 12.23 ->
       11.72 ms per step, cfg3 -1.2 to -1.6 %), and the first record that does overflow there (it goes to the arena class: slow, correct)
       switches the context back for good. */
    static_assert(LVL0_LONG_BYTES > 2u * PAFFY_OPS_CAP, "the longer first level must be longer than the safe bound");
    const bool lvl0_long = !s.add_not_last && c->lvl0_long_ok;
    const uint32_t lvl0_max = s.add_not_last ? PAFFY_OPS_CAP * 5 / 8 : (lvl0_long ? LVL0_LONG_BYTES / 2u : PAFFY_OPS_CAP);
    uint32_t n_lines = 0;
    rc = index_and_parse(c, in, len, &n_lines, lvl0_max, s.flat != FLAT_MODE_NONE);
    if (rc) return rc;
    if ((s.fix_query || s.fix_target) && n_lines > 0)
        LAUNCH(c, "k_dechunk", k_dechunk, dim3((n_lines + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, in, static_cast<RecMeta *>(c->meta.p), n_lines,
               s.fix_query, s.fix_target);
    c->kp.lvl0_max = lvl0_max;
    c->kp.lvl0_long_bytes = (!s.add_not_last && !lvl0_long && !c->lvl0_long_off) ? LVL0_LONG_BYTES : 0u;
    rc = record_params(c, s, in, len, n_lines);
    if (rc) return rc;
    if (n_lines == 0) {
        rc = fetch_info(c);
    } else {
        bool need_records = true;
        uint32_t flat_g_count = 0;
        if (s.flat == FLAT_MODE_ADD) rc = plan_flat_add(c, n_lines, &need_records);
        else if (s.flat == FLAT_MODE_ADD_PIPE) rc = plan_flat_add(c, n_lines, &need_records, true);
        else if (s.flat == FLAT_MODE_REMOVE) rc = plan_flat_remove(c, n_lines, &need_records);
        else if (s.flat == FLAT_MODE_VIEW) rc = plan_flat_view(c, n_lines, &need_records);
        else if (s.flat == FLAT_MODE_PASS) rc = plan_flat(c, s, n_lines, &need_records, &flat_g_count);
        if (!rc && need_records) rc = plan_records(c, s, n_lines, lvl0_long, flat_g_count);
    }
    if (rc) return rc;
    rc = plan_finish(c, n_lines, info);
    if (!rc && s.flat == FLAT_MODE_VIEW) { /* sums only: the records the record kernels took were sized there, but nothing of this plan is emitted */
        c->plan_stats_only = true;
        c->plan.out_bytes = info->out_bytes = 0;
        c->plan.n_rows = info->n_rows = 0;
    }
    return rc;
}

} /* extern "C" */

#include "coverage_host.h"
#include "dedupe_host.h"
#include "chain_host.h"
#include "pretty_kernel.h"
#include "view_line_kernel.h"
#include "fasta_host.h"

static CovState &cov_state(paffy_hip_ctx *c) {
    if (!c->cov) c->cov.reset(new CovState());
    return *c->cov;
}
static int64_t cov_in_bytes(const CovState &S) {
    int64_t n = 0;
    for (const CovBatch &b : S.batches) n += b.len;
    return n;
}
static ChainState &chain_state(paffy_hip_ctx *c) {
    if (!c->chain) c->chain.reset(new ChainState());
    return *c->chain;
}

extern "C" {

/* the lines of S.order (records) with the levels of S.level: sizes, offsets, and the line table emit reads */
static int lines_plan(paffy_hip_ctx *c, CovState &S, uint64_t n) {
    if (ensure(c, S.out_len, sizeof(uint64_t) * (size_t)(n + 1))) return PAFFY_E_HIP;
    if (ensure(c, S.out_off, sizeof(uint64_t) * (size_t)(n + 1))) return PAFFY_E_HIP;
    LAUNCH(c, "k_line_size", k_line_size, dim3((unsigned)((n + 1 + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(S.meta.p),
           static_cast<const uint32_t *>(S.order.p), static_cast<const int64_t *>(S.level.p), n, static_cast<uint64_t *>(S.out_len.p));
    if (cov_excl_scan64(c, S, static_cast<uint64_t *>(S.out_len.p), static_cast<uint64_t *>(S.out_off.p), (size_t)n)) return PAFFY_E_HIP;
    uint64_t total = 0;
    if (cov_fetch(c, &total, static_cast<uint64_t *>(S.out_off.p) + n, sizeof(total))) return PAFFY_E_HIP;
    c->plan.out_bytes = (int64_t)total;
    c->plan.n_rows = (int64_t)n;
    c->line_batches = static_cast<const uint8_t *const *>(S.batch_ptrs.p);
    c->line_meta = static_cast<const RecMeta *>(S.meta.p);
    c->line_names2 = nullptr;
    c->line_order = static_cast<const uint32_t *>(S.order.p);
    c->line_level = static_cast<const int64_t *>(S.level.p);
    c->line_off = static_cast<const uint64_t *>(S.out_off.p);
    c->line_n = n;
    return 0;
}

/*
 * `paffy tile` (impl/paf_tile.c:156-178) over any number of text batches: begin, add every batch (the text stays where it is until
 * the output has been emitted), run. The visiting order (chain_score desc, score desc, input order) and the grouping by query name
 * are radix sorts on the device; the per-base walk keeps the counters of a 32 Ki-base slice in LDS (coverage_kernel.h).
 * Any failing record means nothing is written (the reference writes only after the last record).
 */
int paffy_hip_tile_begin(paffy_hip_ctx *c) {
    if (c) (void)paffy_hip_stream_trim(c); /* a closed stream's slot buffers (tens of GB) are this command's to use */
    if (!c) return PAFFY_E_ARG;
    c->planned = false;
    index_drop_all(c); /* indexes kept by paffy_hip_query_names for batches that were never split */
    return cov_begin(c, 1);
}
int paffy_hip_tile_add(paffy_hip_ctx *c, const void *d_in, int64_t in_len) {
    if (!c) return PAFFY_E_ARG;
    return cov_add(c, d_in, in_len, true);
}
int paffy_hip_tile_run(paffy_hip_ctx *c, paffy_plan_info *info) {
    if (!c || !info) return PAFFY_E_ARG;
    CovState &S = cov_state(c);
    plan_begin(c, PLAN_LINES, cov_in_bytes(S), info);
    c->plan.n_records = (int64_t)S.n_rec;
    const uint64_t n = S.n_rec;
    if (n > 0) {
        int rc = cov_run(c, 0, &c->plan.error);
        if (rc) return rc;
        if (c->plan.error.code == 0) {
            int rl = lines_plan(c, S, n);
            if (rl) return rl;
        }
        if (c->profile) prof_collect(c);
    }
    *info = c->plan;
    c->planned = true;
    return 0;
}
/* the one-batch form */
int paffy_hip_tile_plan(paffy_hip_ctx *c, const void *d_in, int64_t in_len, paffy_plan_info *info) {
    if (!c || !info) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    int rc = paffy_hip_tile_begin(c);
    if (!rc) rc = paffy_hip_tile_add(c, d_in, in_len);
    if (!rc) rc = paffy_hip_tile_run(c, info);
    return rc;
}

/*
 * `paffy chain` (impl/paf_chain.c:123-127, impl/chaining.c:266-343) over any number of text batches, like tile: begin, add, run;
 * the output lines (cn / s1 tags set, cigar text verbatim) are written by paffy_hip_emit or paffy_hip_emit_lines.
 */
int paffy_hip_chain_begin(paffy_hip_ctx *c) {
    if (c) (void)paffy_hip_stream_trim(c); /* a closed stream's slot buffers (tens of GB) are this command's to use */
    if (!c) return PAFFY_E_ARG;
    c->planned = false;
    index_drop_all(c); /* indexes kept by paffy_hip_query_names for batches that were never split */
    ChainState &H = chain_state(c);
    H.indexed = H.part_ready = false;
    H.n_chains = 0;
    return cov_begin(c, 1);
}
/* records [first, first + n) of the chain state get their global input numbers: the caller's (d_gidx), or the running local index */
static int chain_number_records(paffy_hip_ctx *c, uint64_t first, uint64_t n, const void *d_gidx) {
    ChainState &H = chain_state(c);
    if (n == 0 || (!d_gidx && !H.indexed)) return 0;
    if (ensure_keep(c, H.gidx, sizeof(int64_t) * (first + n), H.indexed ? sizeof(int64_t) * first : 0)) return PAFFY_E_HIP;
    int64_t *g = static_cast<int64_t *>(H.gidx.p);
    if (!H.indexed && first) /* the batches before this one were added without numbers */
        LAUNCH(c, "k_iota64", k_iota64, dim3((unsigned)((first + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, g, (int64_t)0, (uint32_t)first);
    if (d_gidx) {
        HIPCHK(c, hipMemcpyAsync(g + first, d_gidx, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* d_gidx is the caller's again */
    } else LAUNCH(c, "k_iota64", k_iota64, dim3((unsigned)((n + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, g + first, (int64_t)first, (uint32_t)n);
    H.indexed = true;
    return 0;
}
int paffy_hip_chain_add(paffy_hip_ctx *c, const void *d_in, int64_t in_len) {
    if (!c) return PAFFY_E_ARG;
    const uint64_t first = cov_state(c).n_rec;
    int rc = cov_add(c, d_in, in_len, false);
    return rc ? rc : chain_number_records(c, first, cov_state(c).n_rec - first, nullptr);
}
int paffy_hip_chain_add_indexed(paffy_hip_ctx *c, const void *d_in, int64_t in_len, const void *d_gidx) {
    if (!c || !d_gidx) return PAFFY_E_ARG;
    const uint64_t first = cov_state(c).n_rec;
    int rc = cov_add(c, d_in, in_len, false);
    return rc ? rc : chain_number_records(c, first, cov_state(c).n_rec - first, d_gidx);
}
int paffy_hip_chain_run(paffy_hip_ctx *c, const paffy_chain_opts *opts, paffy_plan_info *info) {
    if (!c || !info || !opts) return PAFFY_E_ARG;
    CovState &S = cov_state(c);
    plan_begin(c, PLAN_LINES, cov_in_bytes(S), info); /* the output is a line table, as for tile */
    c->plan.n_records = (int64_t)S.n_rec;
    const uint64_t n = S.n_rec;
    if (n > 0) {
        const ChainOpts o{opts->gap_open, opts->gap_extend, opts->max_gap_length, opts->trim_fraction};
        int rc = chain_run(c, o, &c->plan.error, c->chain_fresh);
        if (rc) return rc;
        if (c->plan.error.code == 0) {
            int rl = lines_plan(c, S, n);
            if (rl) return rl;
        }
        if (c->profile) prof_collect(c);
    }
    *info = c->plan;
    c->planned = true;
    return 0;
}
/*
 * Chain in parts: paffy_hip_chain_run cut where its global decisions begin (chain_host.h). A context that holds the records of some
 * query sequences runs the part, hands out four numbers per chain, takes the chains' numbers in the whole input, and finishes.
 */
int paffy_hip_chain_run_part(paffy_hip_ctx *c, const paffy_chain_opts *opts, paffy_plan_info *info) {
    if (!c || !info || !opts) return PAFFY_E_ARG;
    if (c->chain_fresh) { /* a strand's leading run is a property of the whole input, not of a part */
        c->last_error = "paffy_hip_chain_run_part: not built under paffy_hip_chain_fresh_walk (a strand's leading run spans the parts)";
        return PAFFY_E_UNSUPPORTED;
    }
    CovState &S = cov_state(c);
    plan_begin(c, PLAN_LINES, cov_in_bytes(S), info);
    c->plan.n_records = (int64_t)S.n_rec;
    const ChainOpts o{opts->gap_open, opts->gap_extend, opts->max_gap_length, opts->trim_fraction};
    int rc = chain_part(c, o, true, &c->plan.error);
    if (rc) return rc;
    if (c->profile) prof_collect(c);
    *info = c->plan; /* no lines planned: c->planned stays false until paffy_hip_chain_renumber */
    return 0;
}
int paffy_hip_chain_fresh_walk(paffy_hip_ctx *c, int on) {
    if (!c) return PAFFY_E_ARG;
    c->chain_fresh = on != 0;
    return 0;
}
int paffy_hip_chain_fresh_stats(paffy_hip_ctx *c, int64_t out[4]) {
    if (!c || !out) return PAFFY_E_ARG;
    if (!c->chain) return PAFFY_E_STATE;
    memcpy(out, c->chain->fresh_stats, sizeof(c->chain->fresh_stats));
    return 0;
}
int64_t paffy_hip_chain_tail_keys(paffy_hip_ctx *c, int64_t cap_chains, void *d_keys) {
    if (!c) return PAFFY_E_ARG;
    if (!c->chain || !c->chain->part_ready || c->plan.error.code) return PAFFY_E_STATE;
    ChainState &H = *c->chain;
    const uint32_t n = H.n_chains;
    if (cap_chains < (int64_t)n) return PAFFY_E_CAPACITY;
    if (n == 0) return 0;
    if (!d_keys) return PAFFY_E_ARG;
    LAUNCH(c, "k_chain_tail_keys", k_chain_tail_keys, dim3((n + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(H.tails.p), chain_pos(H),
           H.indexed ? static_cast<const int64_t *>(H.gidx.p) : nullptr, n, static_cast<int64_t *>(d_keys));
    return (int64_t)n;
}
int paffy_hip_chain_renumber(paffy_hip_ctx *c, const void *d_global_id, paffy_plan_info *info, int64_t fail_key[3]) {
    if (!c || !info) return PAFFY_E_ARG;
    if (!c->chain || !c->chain->part_ready || c->plan.error.code) return PAFFY_E_STATE;
    CovState &S = cov_state(c);
    ChainState &H = *c->chain;
    const uint64_t n = S.n_rec;
    if (H.n_chains && !d_global_id) return PAFFY_E_ARG;
    c->planned = false;
    c->line_n = 0; /* a renumber before this one may have planned lines */
    c->plan.n_rows = c->plan.out_bytes = 0;
    if (n > 0) {
        uint32_t *bad = reinterpret_cast<uint32_t *>(static_cast<unsigned long long *>(H.words.p) + 2), hit = 0;
        HIPCHK(c, hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
        LAUNCH(c, "k_chain_renumber", k_chain_renumber, dim3((H.n_chains + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(H.tails.p),
               static_cast<const int64_t *>(d_global_id), H.n_chains, static_cast<uint32_t *>(H.chain_of_tail.p), bad);
        if (cov_fetch(c, &hit, bad, sizeof(hit))) return PAFFY_E_HIP;
        if (hit) {
            c->last_error = "a chain number outside [0, 2^31)";
            H.part_ready = false;
            return PAFFY_E_ARG;
        }
        int rc = chain_finish(c, &c->plan.error);
        if (rc) return rc;
        if (c->plan.error.code) {
            if (fail_key) memcpy(fail_key, H.fail_key, sizeof(H.fail_key));
        } else {
            int rl = lines_plan(c, S, n);
            if (rl) return rl;
        }
        if (c->profile) prof_collect(c);
    }
    *info = c->plan;
    c->planned = true;
    return 0;
}
int64_t paffy_hip_chain_line_keys(paffy_hip_ctx *c, int64_t cap_lines, void *d_keys) {
    if (!c) return PAFFY_E_ARG;
    if (!c->planned || c->plan_kind != PLAN_LINES || !c->chain || !c->cov || c->plan.error.code) return PAFFY_E_STATE;
    CovState &S = cov_state(c);
    ChainState &H = *c->chain;
    const uint64_t n = H.n_out;
    if (n == 0 && c->line_n == 0) return 0; /* a part without records */
    if (n != c->line_n || c->line_meta != static_cast<const RecMeta *>(S.meta.p)) return PAFFY_E_STATE; /* the last plan was not a chain */
    if ((uint64_t)cap_lines < n) return PAFFY_E_CAPACITY;
    if (!d_keys) return PAFFY_E_ARG;
    LAUNCH(c, "k_chain_line_keys", k_chain_line_keys, dim3((unsigned)((n + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(H.o3.p), chain_pos(H),
           static_cast<const uint32_t *>(H.chain_id.p), static_cast<const uint32_t *>(H.link.p), static_cast<const uint64_t *>(S.out_len.p), (uint32_t)n,
           static_cast<int64_t *>(d_keys));
    return (int64_t)n;
}
int64_t paffy_hip_chain_tags(paffy_hip_ctx *c, int64_t cap, int64_t *chain_id, int64_t *chain_score) {
    if (!c || cap < 0 || !chain_id || !chain_score) return PAFFY_E_ARG;
    if (!c->planned || !c->chain || c->plan.error.code) return PAFFY_E_STATE;
    const int64_t n = (int64_t)c->chain->n_out;
    if (cap < n) return PAFFY_E_CAPACITY;
    if (n > 0) {
        HIPCHK(c, hipMemcpy(chain_id, c->chain->tag_chain.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(chain_score, c->chain->tag_score.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return n;
}

/*
 * Sharding `paffy tile` by query sequence (the reference pipeline's `split_file -q`, tests/paf_pipeline_test.sh:42):
 *   paffy_hip_query_names    the distinct query names of a batch as 64-bit hashes with the bytes of their lines (the weights a
 *                            partitioner balances)
 *   paffy_hip_split_by_owner the lines of a batch regrouped by the owner of their query name (owner table: hash -> part), input order
 *                            kept inside a part: what an all-to-all over the ranks sends
 *   paffy_hip_scatter_lines  lines to given offsets of an output (the ordered write once every line's place is known)
 */
__global__ __launch_bounds__(PAFFY_NT) void k_query_hash(const uint8_t *in, const RecMeta *meta, const uint32_t *sep_pos, const uint32_t *nl_idx, uint32_t n, uint32_t in_len,
                                                          uint64_t *hash, uint64_t *line_len, uint32_t *idx) {
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n) return;
    const RecMeta &m = meta[r];
    hash[r] = cov_name_hash(in, m.qname_off, m.qname_len);
    const uint32_t start = r == 0 ? 0u : sep_pos[nl_idx[r - 1]] + 1u, end = sep_pos[nl_idx[r]];
    (void)in_len;
    line_len[r] = (uint64_t)(end - start) + 1u; /* with its newline (a last line without one gets one) */
    idx[r] = r;
}
/* sorted by hash: line bytes in sorted order (for a scan), and at the head of every run of equal hashes its hash */
__global__ __launch_bounds__(PAFFY_NT) void k_run_lens(const uint32_t *sorted_idx, const uint64_t *line_len, uint32_t n, uint64_t *out) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n) out[i] = line_len[sorted_idx[i]];
    if (i == 0) out[n] = 0;
}
/* weight of run c = (bytes in front of the next run) - (bytes in front of this one): no atomics on a handful of addresses */
__global__ __launch_bounds__(PAFFY_NT) void k_run_heads_out(const uint64_t *sorted_hash, const uint32_t *flag, const uint32_t *scan, const uint64_t *byte_off, uint32_t n,
                                                             uint64_t *out_hash, uint64_t *out_start, uint64_t *out_first) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) {
        out_hash[scan[i] - 1u] = sorted_hash[i];
        out_start[scan[i] - 1u] = byte_off[i];
        out_first[scan[i] - 1u] = i; /* lines in front of the run: run lengths are differences */
    }
    if (i == n - 1) {
        out_start[scan[i]] = byte_off[n];
        out_first[scan[i]] = n;
    }
}
__global__ __launch_bounds__(PAFFY_NT) void k_owner_keys(const uint64_t *hash, uint32_t n, const uint64_t *tab_hash, const uint32_t *tab_owner, uint32_t n_tab, uint32_t n_parts,
                                                          uint64_t *key) {
    const uint32_t r = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (r >= n) return;
    uint32_t lo = 0, hi = n_tab; /* first entry >= hash */
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab_hash[mid] < hash[r]) lo = mid + 1;
        else hi = mid;
    }
    uint32_t owner = (lo < n_tab && tab_hash[lo] == hash[r]) ? tab_owner[lo] : (uint32_t)(hash[r] % n_parts); /* a name the table does not know */
    if (owner >= n_parts) owner = n_parts - 1;
    key[r] = ((uint64_t)owner << 32) | r;
}
__global__ __launch_bounds__(PAFFY_NT) void k_gather_len(const uint64_t *sorted_key, const uint64_t *line_len, uint32_t n, uint64_t *out) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n) out[i] = line_len[(uint32_t)sorted_key[i]];
    if (i == 0) out[n] = 0;
}
/* where every part starts in the sorted order: first[p] = index of its first line, start[p] = its first byte (parts without lines keep -1) */
__global__ __launch_bounds__(PAFFY_NT) void k_part_bounds(const uint64_t *sorted_key, const uint64_t *off, uint32_t n, int64_t *first, int64_t *start) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = (uint32_t)(sorted_key[i] >> 32);
    if (i == 0 || (uint32_t)(sorted_key[i - 1] >> 32) != p) {
        first[p] = i;
        start[p] = (int64_t)off[i];
    }
}
/* one workgroup per line: bytes [src_off, src_off + len) of src to dst + dst_off; a source line that ends without newline gets one */
__device__ __forceinline__ void copy_line(const uint8_t *src, uint64_t len, uint8_t *dst, bool add_nl) {
    const uint64_t body = add_nl ? len - 1 : len;
    const uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    if (head >= body) {
        for (uint64_t x = threadIdx.x; x < body; x += PAFFY_NT) dst[x] = src[x];
    } else {
        for (uint32_t x = threadIdx.x; x < head; x += PAFFY_NT) dst[x] = src[x];
        const uint64_t n_ch = (body - head) >> 4;
        for (uint64_t ch = threadIdx.x; ch < n_ch; ch += PAFFY_NT)
            *reinterpret_cast<u32x4 *>(dst + head + 16 * ch) = *reinterpret_cast<const u32x4_unaligned *>(src + head + 16 * ch);
        for (uint64_t x = head + 16 * n_ch + threadIdx.x; x < body; x += PAFFY_NT) dst[x] = src[x];
    }
    if (add_nl && threadIdx.x == 0) dst[body] = '\n';
}
/* line blockIdx.x of the (part, input index) order. Without part_dst the parts follow each other in `out` and in rec_index; with it
   part p's lines start at out + part_dst[p] and its record indices at rec_index + part_dst[n_parts + p] (the caller's send buffer, in
   which the parts of several batches stand behind each other per destination). rec_base is added to every index. */
__global__ __launch_bounds__(PAFFY_NT) void k_split_copy(const uint8_t *in, uint32_t in_len, const uint32_t *sep_pos, const uint32_t *nl_idx, const uint64_t *sorted_key,
                                                          const uint64_t *off, uint8_t *out, const int64_t *part_first, const int64_t *part_start, const int64_t *part_dst,
                                                          uint32_t n_parts, int64_t *rec_index, int64_t rec_base) {
    const uint64_t key = sorted_key[blockIdx.x];
    const uint32_t r = (uint32_t)key, p = (uint32_t)(key >> 32);
    const uint32_t start = r == 0 ? 0u : sep_pos[nl_idx[r - 1]] + 1u, end = sep_pos[nl_idx[r]];
    uint64_t at = off[blockIdx.x];
    int64_t slot = (int64_t)blockIdx.x;
    if (part_dst) {
        at = (uint64_t)part_dst[p] + (at - (uint64_t)part_start[p]);
        slot = part_dst[n_parts + p] + ((int64_t)blockIdx.x - part_first[p]);
    }
    if (rec_index && threadIdx.x == 0) rec_index[slot] = (int64_t)r + rec_base;
    copy_line(in + start, (uint64_t)(end - start) + 1u, out + at, end >= in_len);
}
__global__ __launch_bounds__(PAFFY_NT) void k_scatter_lines(const uint8_t *src, const int64_t *src_off, const int64_t *dst_off, uint8_t *dst) {
    const uint64_t k = blockIdx.x;
    copy_line(src + src_off[k], (uint64_t)(src_off[k + 1] - src_off[k]), dst + dst_off[k], false);
}

#include "bed_parts_kernel.h"

/* the kept indexes (see paffy_hip_ctx::kept_index): copy out after query_names, copy back for split_by_owner; an entry owns its buffers
   and moves between kept_index and index_pool */
static void index_drop(paffy_hip_ctx *c, const void *d_in) {
    for (size_t i = 0; i < c->kept_index.size(); i++)
        if (c->kept_index[i].in == d_in) {
            c->index_pool.push_back(std::move(c->kept_index[i])); /* the buffers stay allocated for the next batch */
            c->kept_index.erase(c->kept_index.begin() + (long)i);
            return;
        }
}
static int index_keep(paffy_hip_ctx *c, const void *d_in, int64_t in_len, uint32_t n) {
    index_drop(c, d_in);
    if (c->kept_index.size() >= 64) return 0; /* a caller that never splits: stop keeping */
    paffy_hip_ctx::KeptIndex k;
    if (!c->index_pool.empty()) {
        k = std::move(c->index_pool.back());
        c->index_pool.pop_back();
    }
    k.in = d_in;
    k.len = in_len;
    k.n = n;
    k.n_seps = c->h_info->n_seps;
    const size_t mb = sizeof(RecMeta) * (size_t)n, sb = sizeof(uint32_t) * ((size_t)k.n_seps + 1), nb = sizeof(uint32_t) * ((size_t)n + 1);
    if (ensure(c, k.meta, mb) || ensure(c, k.sep_pos, sb) || ensure(c, k.nl_idx, nb)) return PAFFY_E_HIP;
    HIPCHK(c, hipMemcpyAsync(k.meta.p, c->meta.p, mb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(k.sep_pos.p, c->sep_pos.p, sb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(k.nl_idx.p, c->nl_idx.p, nb, hipMemcpyDeviceToDevice, c->stream));
    c->kept_index.push_back(std::move(k));
    return 0;
}
/* 0: the index buffers describe d_in again; 1: nothing kept for it */
static int index_restore(paffy_hip_ctx *c, const void *d_in, int64_t in_len, uint32_t *n, bool keep = false) {
    for (size_t i = 0; i < c->kept_index.size(); i++) {
        paffy_hip_ctx::KeptIndex &k = c->kept_index[i];
        if (k.in != d_in || k.len != in_len) continue;
        const size_t mb = sizeof(RecMeta) * (size_t)k.n, sb = sizeof(uint32_t) * ((size_t)k.n_seps + 1), nb = sizeof(uint32_t) * ((size_t)k.n + 1);
        c->dd_part_stage = 0;
        if (ensure(c, c->meta, mb) || ensure(c, c->sep_pos, sb) || ensure(c, c->nl_idx, nb)) return 1;
        if (hipMemcpyAsync(c->meta.p, k.meta.p, mb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->sep_pos.p, k.sep_pos.p, sb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->nl_idx.p, k.nl_idx.p, nb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) /* the kept copy is freed below */
            return 1;
        *n = k.n;
        if (!keep) index_drop(c, d_in);
        return 0;
    }
    return 1;
}

static int64_t query_names_impl(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int64_t cap, uint64_t *hashes, int64_t *weights, int64_t *records, bool with_target = false) {
    if (!c || !hashes || !weights || cap < 0) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    if (in_len == 0) return 0;
    CovState &S = cov_state(c);
    uint32_t n = 0;
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    c->indexed_in = nullptr;
    int rc = index_and_parse(c, in, (uint32_t)in_len, &n);
    if (rc) return rc;
    if (n == 0) return 0;
    c->indexed_in = d_in;
    c->indexed_len = in_len;
    c->indexed_n = n;
    if (index_keep(c, d_in, in_len, n)) return PAFFY_E_HIP;
    const uint32_t n_lines = n, g_lines = (n + PAFFY_NT - 1) / PAFFY_NT;
    if (with_target) n = 2 * n_lines; /* an item per side (n_lines < 2^31) */
    const uint32_t g = (n + PAFFY_NT - 1) / PAFFY_NT;
    if (ensure(c, S.k64a, sizeof(uint64_t) * ((size_t)n + 1)) || ensure(c, S.k64b, sizeof(uint64_t) * ((size_t)n + 1)) || ensure(c, S.name_hash, sizeof(uint64_t) * ((size_t)n + 1)) ||
        ensure(c, S.v32a, sizeof(uint32_t) * ((size_t)n + 1)) || ensure(c, S.v32b, sizeof(uint32_t) * ((size_t)n + 1)) || ensure(c, S.flags, sizeof(uint32_t) * ((size_t)n + 1)) ||
        ensure(c, S.scan32, sizeof(uint32_t) * ((size_t)n + 1)))
        return PAFFY_E_HIP;
    uint64_t *hash = static_cast<uint64_t *>(S.name_hash.p), *len = static_cast<uint64_t *>(S.k64b.p), *sorted = static_cast<uint64_t *>(S.k64a.p);
    uint32_t *idx = static_cast<uint32_t *>(S.v32a.p), *sidx = static_cast<uint32_t *>(S.v32b.p), *flags = static_cast<uint32_t *>(S.flags.p), *scan = static_cast<uint32_t *>(S.scan32.p);
    if (with_target)
        LAUNCH(c, "k_side_hash", k_side_hash, dim3(g_lines), dim3(PAFFY_NT), 0, in, static_cast<const RecMeta *>(c->meta.p), static_cast<const uint32_t *>(c->sep_pos.p),
               static_cast<const uint32_t *>(c->nl_idx.p), n_lines, hash, len, idx);
    else
        LAUNCH(c, "k_query_hash", k_query_hash, dim3(g), dim3(PAFFY_NT), 0, in, static_cast<const RecMeta *>(c->meta.p), static_cast<const uint32_t *>(c->sep_pos.p),
               static_cast<const uint32_t *>(c->nl_idx.p), n, (uint32_t)in_len, hash, len, idx);
    if (cov_sort_pairs(c, S, hash, sorted, idx, sidx, n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_cov_run_heads", k_cov_run_heads, dim3(g), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(sorted), n, flags);
    if (cov_incl_scan32(c, S, flags, scan, n)) return PAFFY_E_HIP;
    uint32_t n_names = 0;
    if (cov_fetch(c, &n_names, scan + (n - 1), sizeof(uint32_t))) return PAFFY_E_HIP;
    if ((int64_t)n_names > cap) return PAFFY_E_CAPACITY;
    if (ensure(c, S.pairs, sizeof(uint64_t) * (size_t)n_names) || ensure(c, S.pairs2, sizeof(uint64_t) * 2 * ((size_t)n_names + 1)) || ensure(c, S.bm_words, sizeof(uint64_t) * ((size_t)n + 1)) ||
        ensure(c, S.bm_off, sizeof(uint64_t) * ((size_t)n + 2)))
        return PAFFY_E_HIP;
    uint64_t *slen = static_cast<uint64_t *>(S.bm_words.p), *soff = static_cast<uint64_t *>(S.bm_off.p);
    LAUNCH(c, "k_run_lens", k_run_lens, dim3(g), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(sidx), static_cast<const uint64_t *>(len), n, slen);
    if (cov_excl_scan64(c, S, slen, soff, n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_run_heads_out", k_run_heads_out, dim3(g), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(sorted), static_cast<const uint32_t *>(flags), static_cast<const uint32_t *>(scan),
           static_cast<const uint64_t *>(soff), n, static_cast<uint64_t *>(S.pairs.p), static_cast<uint64_t *>(S.pairs2.p), static_cast<uint64_t *>(S.pairs2.p) + n_names + 1);
    std::vector<uint64_t> starts(2 * ((size_t)n_names + 1));
    HIPCHK(c, hipMemcpyAsync(hashes, S.pairs.p, sizeof(uint64_t) * (size_t)n_names, hipMemcpyDeviceToHost, c->stream));
    if (cov_fetch(c, starts.data(), S.pairs2.p, sizeof(uint64_t) * 2 * ((size_t)n_names + 1))) return PAFFY_E_HIP;
    for (uint32_t k = 0; k < n_names; k++) weights[k] = (int64_t)(starts[k + 1] - starts[k]);
    if (records)
        for (uint32_t k = 0; k < n_names; k++) records[k] = (int64_t)(starts[(size_t)n_names + 1 + k + 1] - starts[(size_t)n_names + 1 + k]);
    return (int64_t)n_names;
}

static int split_impl0(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner, int64_t n_table,
                       void *d_out, int64_t out_cap, const int64_t *part_dst, const int64_t *rec_dst, int64_t rec_base, int64_t *part_bytes, int64_t *part_records,
                       void *d_rec_index, int64_t rec_index_cap, int64_t *n_records) {
    if (!c || n_parts < 1 || n_table < 0 || (n_table > 0 && (!table_hash || !table_owner)) || !part_bytes || !part_records || !n_records) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    if ((part_dst != nullptr) != (rec_dst != nullptr)) return PAFFY_E_ARG;
    for (int32_t p = 0; p < n_parts; p++) part_bytes[p] = part_records[p] = 0;
    *n_records = 0;
    if (in_len == 0) return 0;
    if (!d_out || (!part_dst && out_cap < in_len + 1)) return PAFFY_E_CAPACITY;
    CovState &S = cov_state(c);
    uint32_t n = 0;
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    if (c->indexed_in == d_in && c->indexed_len == in_len) { /* indexed by paffy_hip_query_names just before */
        n = c->indexed_n;
        index_drop(c, d_in);
    } else if (index_restore(c, d_in, in_len, &n) != 0) { /* ... or some batches ago: its index comes back from the kept copy */
        int rc = index_and_parse(c, in, (uint32_t)in_len, &n);
        if (rc) return rc;
    }
    c->indexed_in = nullptr;
    *n_records = n;
    if (n == 0) return 0;
    if (d_rec_index && !part_dst && rec_index_cap < (int64_t)n) return PAFFY_E_CAPACITY;
    const uint32_t g = (n + PAFFY_NT - 1) / PAFFY_NT;
    if (ensure(c, S.k64a, sizeof(uint64_t) * ((size_t)n + 1)) || ensure(c, S.k64b, sizeof(uint64_t) * ((size_t)n + 1)) || ensure(c, S.name_hash, sizeof(uint64_t) * ((size_t)n + 1)) ||
        ensure(c, S.v32a, sizeof(uint32_t) * ((size_t)n + 1)) || ensure(c, S.bm_words, sizeof(uint64_t) * ((size_t)n + 1)) || ensure(c, S.bm_off, sizeof(uint64_t) * ((size_t)n + 2)) ||
        ensure(c, S.pairs, (sizeof(uint64_t) + sizeof(uint32_t)) * ((size_t)n_table + 1)) || ensure(c, S.pairs2, sizeof(int64_t) * 4 * (size_t)n_parts))
        return PAFFY_E_HIP;
    uint64_t *hash = static_cast<uint64_t *>(S.name_hash.p), *len = static_cast<uint64_t *>(S.k64b.p), *key = static_cast<uint64_t *>(S.k64a.p), *skey = static_cast<uint64_t *>(S.bm_words.p);
    uint64_t *off = static_cast<uint64_t *>(S.bm_off.p);
    uint64_t *d_th = static_cast<uint64_t *>(S.pairs.p);
    uint32_t *d_to = reinterpret_cast<uint32_t *>(d_th + n_table + 1);
    if (n_table) {
        HIPCHK(c, hipMemcpyAsync(d_th, table_hash, sizeof(uint64_t) * (size_t)n_table, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_to, table_owner, sizeof(uint32_t) * (size_t)n_table, hipMemcpyHostToDevice, c->stream));
    }
    LAUNCH(c, "k_query_hash", k_query_hash, dim3(g), dim3(PAFFY_NT), 0, in, static_cast<const RecMeta *>(c->meta.p), static_cast<const uint32_t *>(c->sep_pos.p),
           static_cast<const uint32_t *>(c->nl_idx.p), n, (uint32_t)in_len, hash, len, static_cast<uint32_t *>(S.v32a.p));
    LAUNCH(c, "k_owner_keys", k_owner_keys, dim3(g), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(hash), n, static_cast<const uint64_t *>(d_th), static_cast<const uint32_t *>(d_to),
           (uint32_t)n_table, (uint32_t)n_parts, key);
    if (cov_sort_keys(c, S, key, skey, n)) return PAFFY_E_HIP; /* (owner, input index): input order inside a part */
    LAUNCH(c, "k_gather_len", k_gather_len, dim3(g), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(skey), static_cast<const uint64_t *>(len), n, key);
    if (cov_excl_scan64(c, S, key, off, n)) return PAFFY_E_HIP;
    int64_t *d_tot = static_cast<int64_t *>(S.pairs2.p);
    HIPCHK(c, hipMemsetAsync(d_tot, 0xff, sizeof(int64_t) * 2 * (size_t)n_parts, c->stream));
    LAUNCH(c, "k_part_bounds", k_part_bounds, dim3(g), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(skey), static_cast<const uint64_t *>(off), n, d_tot, d_tot + n_parts);
    /* the sizes of the parts first: a caller's destinations are checked against them before a byte is written */
    std::vector<int64_t> tot(2 * (size_t)n_parts);
    uint64_t all_bytes = 0;
    HIPCHK(c, hipMemcpyAsync(&all_bytes, off + n, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (cov_fetch(c, tot.data(), d_tot, sizeof(int64_t) * 2 * (size_t)n_parts)) return PAFFY_E_HIP;
    int64_t next_first = (int64_t)n, next_start = (int64_t)all_bytes; /* a part ends where the next non-empty one starts */
    for (int32_t p = n_parts - 1; p >= 0; p--) {
        const int64_t first = tot[(size_t)p], start = tot[(size_t)n_parts + p];
        if (first < 0) continue;
        part_records[p] = next_first - first;
        part_bytes[p] = next_start - start;
        next_first = first;
        next_start = start;
    }
    const int64_t *d_dst = nullptr;
    if (part_dst) {
        std::vector<int64_t> dst(2 * (size_t)n_parts);
        for (int32_t p = 0; p < n_parts; p++) {
            if (part_dst[p] < 0 || rec_dst[p] < 0 || part_dst[p] + part_bytes[p] > out_cap || (d_rec_index && rec_dst[p] + part_records[p] > rec_index_cap)) {
                for (int32_t q = 0; q < n_parts; q++) part_bytes[q] = part_records[q] = 0;
                return PAFFY_E_CAPACITY;
            }
            dst[(size_t)p] = part_dst[p];
            dst[(size_t)n_parts + p] = rec_dst[p];
        }
        HIPCHK(c, hipMemcpyAsync(d_tot + 2 * n_parts, dst.data(), sizeof(int64_t) * 2 * (size_t)n_parts, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream)); /* `dst` is a local */
        d_dst = d_tot + 2 * n_parts;
    }
    LAUNCH(c, "k_split_copy", k_split_copy, dim3(n), dim3(PAFFY_NT), 0, in, (uint32_t)in_len, static_cast<const uint32_t *>(c->sep_pos.p), static_cast<const uint32_t *>(c->nl_idx.p),
           static_cast<const uint64_t *>(skey), static_cast<const uint64_t *>(off), static_cast<uint8_t *>(d_out), static_cast<const int64_t *>(d_tot),
           static_cast<const int64_t *>(d_tot + n_parts), d_dst, (uint32_t)n_parts, static_cast<int64_t *>(d_rec_index), rec_base);
    return 0;
}

/* A failing call leaves no kept index behind: whatever the caller does next starts from the text. */
int64_t paffy_hip_query_names(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int64_t cap, uint64_t *hashes, int64_t *weights) {
    const int64_t n = query_names_impl(c, d_in, in_len, cap, hashes, weights, nullptr);
    if (n < 0 && c) index_drop_all(c);
    return n;
}
int64_t paffy_hip_query_names_counts(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int64_t cap, uint64_t *hashes, int64_t *weights, int64_t *records) {
    if (!records) return PAFFY_E_ARG;
    const int64_t n = query_names_impl(c, d_in, in_len, cap, hashes, weights, records);
    if (n < 0 && c) index_drop_all(c);
    return n;
}
static int split_impl(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner, int64_t n_table,
                      void *d_out, int64_t out_cap, const int64_t *part_dst, const int64_t *rec_dst, int64_t rec_base, int64_t *part_bytes, int64_t *part_records,
                      void *d_rec_index, int64_t rec_index_cap, int64_t *n_records) {
    const int rc = split_impl0(c, d_in, in_len, n_parts, table_hash, table_owner, n_table, d_out, out_cap, part_dst, rec_dst, rec_base, part_bytes, part_records, d_rec_index,
                               rec_index_cap, n_records);
    if (rc && c) index_drop_all(c);
    return rc;
}
int paffy_hip_split_by_owner(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner, int64_t n_table,
                             void *d_out, int64_t out_cap, int64_t *part_bytes, int64_t *part_records, void *d_rec_index, int64_t rec_index_cap, int64_t *n_records) {
    return split_impl(c, d_in, in_len, n_parts, table_hash, table_owner, n_table, d_out, out_cap, nullptr, nullptr, 0, part_bytes, part_records, d_rec_index, rec_index_cap,
                      n_records);
}
int paffy_hip_split_to(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner, int64_t n_table,
                       void *d_out, int64_t out_cap, const int64_t *part_dst, const int64_t *rec_dst, int64_t rec_base, int64_t *part_bytes, int64_t *part_records,
                       void *d_rec_index, int64_t rec_index_cap, int64_t *n_records) {
    if (!part_dst || !rec_dst) return PAFFY_E_ARG;
    return split_impl(c, d_in, in_len, n_parts, table_hash, table_owner, n_table, d_out, out_cap, part_dst, rec_dst, rec_base, part_bytes, part_records, d_rec_index,
                      rec_index_cap, n_records);
}
int64_t paffy_hip_side_names_counts(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int include_inverted, int64_t cap, uint64_t *hashes, int64_t *weights, int64_t *records) {
    if (!records) return PAFFY_E_ARG;
    const int64_t n = query_names_impl(c, d_in, in_len, cap, hashes, weights, records, include_inverted != 0);
    if (n < 0 && c) index_drop_all(c);
    return n;
}

/* the partition by the names of both sides: sizes only (d_out NULL; the batch's kept index stays) or the copy */
static int split_sides_impl0(paffy_hip_ctx *c, const void *d_in, int64_t in_len, bool with_target, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner,
                             int64_t n_table, bool count_only, void *d_out, int64_t out_cap, const int64_t *part_dst, const int64_t *rec_dst, int64_t rec_base,
                             int64_t *part_bytes, int64_t *part_records, void *d_rec_index, void *d_sides, int64_t rec_index_cap, int64_t *n_records) {
    if (!c || n_parts < 1 || n_table < 0 || (n_table > 0 && (!table_hash || !table_owner)) || !part_bytes || !part_records || !n_records) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    if (!count_only && (!part_dst || !rec_dst)) return PAFFY_E_ARG;
    for (int32_t p = 0; p < n_parts; p++) part_bytes[p] = part_records[p] = 0;
    *n_records = 0;
    if (in_len == 0) return 0;
    if (!count_only && (!d_out || !d_sides)) return PAFFY_E_ARG;
    CovState &S = cov_state(c);
    uint32_t n = 0;
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    if (c->indexed_in == d_in && c->indexed_len == in_len) { /* the index buffers describe this batch */
        n = c->indexed_n;
        if (!count_only) index_drop(c, d_in);
    } else if (index_restore(c, d_in, in_len, &n, count_only) != 0) {
        int rc = index_and_parse(c, in, (uint32_t)in_len, &n);
        if (rc) return rc;
    }
    c->indexed_in = nullptr;
    *n_records = n;
    if (n == 0) return 0;
    if (count_only) { /* the split of the same batch may follow at once */
        c->indexed_in = d_in;
        c->indexed_len = in_len;
        c->indexed_n = n;
    }
    const uint32_t n_items = with_target ? 2 * n : n, np1 = (uint32_t)n_parts + 1u;
    const uint32_t g = (n + PAFFY_NT - 1) / PAFFY_NT, gi = (n_items + PAFFY_NT - 1) / PAFFY_NT;
    if (ensure(c, S.k64a, sizeof(uint64_t) * ((size_t)n_items + 1)) || ensure(c, S.k64b, sizeof(uint64_t) * ((size_t)n_items + 1)) || ensure(c, S.name_hash, sizeof(uint64_t) * ((size_t)n + 1)) ||
        ensure(c, S.v32a, sizeof(uint32_t) * ((size_t)n + 1)) || ensure(c, S.v32b, (size_t)n_items + 16) || ensure(c, S.bm_words, sizeof(uint64_t) * ((size_t)n_items + 1)) ||
        ensure(c, S.bm_off, sizeof(uint64_t) * ((size_t)n_items + 2)) || ensure(c, S.pairs, (sizeof(uint64_t) + sizeof(uint32_t)) * ((size_t)n_table + 1)) ||
        ensure(c, S.pairs2, sizeof(int64_t) * 4 * (size_t)np1) || ensure(c, S.seq_len, sizeof(uint64_t) * ((size_t)n + 1)))
        return PAFFY_E_HIP;
    uint64_t *hash = static_cast<uint64_t *>(S.name_hash.p), *len = static_cast<uint64_t *>(S.seq_len.p), *key = static_cast<uint64_t *>(S.k64a.p), *skey = static_cast<uint64_t *>(S.bm_words.p);
    uint64_t *lens = static_cast<uint64_t *>(S.k64b.p), *off = static_cast<uint64_t *>(S.bm_off.p);
    uint8_t *item_mask = static_cast<uint8_t *>(S.v32b.p);
    uint64_t *d_th = static_cast<uint64_t *>(S.pairs.p);
    uint32_t *d_to = reinterpret_cast<uint32_t *>(d_th + n_table + 1);
    if (n_table) {
        HIPCHK(c, hipMemcpyAsync(d_th, table_hash, sizeof(uint64_t) * (size_t)n_table, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_to, table_owner, sizeof(uint32_t) * (size_t)n_table, hipMemcpyHostToDevice, c->stream));
    }
    LAUNCH(c, "k_query_hash", k_query_hash, dim3(g), dim3(PAFFY_NT), 0, in, static_cast<const RecMeta *>(c->meta.p), static_cast<const uint32_t *>(c->sep_pos.p),
           static_cast<const uint32_t *>(c->nl_idx.p), n, (uint32_t)in_len, hash, len, static_cast<uint32_t *>(S.v32a.p));
    LAUNCH(c, "k_side_owner_keys", k_side_owner_keys, dim3(g), dim3(PAFFY_NT), 0, in, static_cast<const RecMeta *>(c->meta.p), n, with_target ? 1u : 0u,
           static_cast<const uint64_t *>(d_th), static_cast<const uint32_t *>(d_to), (uint32_t)n_table, (uint32_t)n_parts, key, item_mask);
    if (cov_sort_keys(c, S, key, skey, n_items)) return PAFFY_E_HIP; /* (part, record, side): input order inside a part */
    LAUNCH(c, "k_side_gather_len", k_side_gather_len, dim3(gi), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(skey), static_cast<const uint64_t *>(len), n_items, (uint32_t)n_parts, lens);
    if (cov_excl_scan64(c, S, lens, off, n_items)) return PAFFY_E_HIP;
    int64_t *d_tot = static_cast<int64_t *>(S.pairs2.p);
    HIPCHK(c, hipMemsetAsync(d_tot, 0xff, sizeof(int64_t) * 2 * (size_t)np1, c->stream));
    LAUNCH(c, "k_side_part_bounds", k_side_part_bounds, dim3(gi), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(skey), static_cast<const uint64_t *>(off), n_items, d_tot, d_tot + np1);
    std::vector<int64_t> tot(2 * (size_t)np1);
    uint64_t all_bytes = 0;
    HIPCHK(c, hipMemcpyAsync(&all_bytes, off + n_items, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (cov_fetch(c, tot.data(), d_tot, sizeof(int64_t) * 2 * (size_t)np1)) return PAFFY_E_HIP;
    int64_t next_first = (int64_t)n_items, next_start = (int64_t)all_bytes; /* a part ends where the next non-empty one starts */
    for (int32_t p = n_parts; p >= 0; p--) {
        const int64_t first = tot[(size_t)p], start = tot[(size_t)np1 + p];
        if (first < 0) continue;
        if (p < n_parts) {
            part_records[p] = next_first - first;
            part_bytes[p] = next_start - start;
        }
        next_first = first;
        next_start = start;
    }
    if (count_only) return 0;
    const int64_t n_sent = tot[(size_t)n_parts] >= 0 ? tot[(size_t)n_parts] : (int64_t)n_items;
    std::vector<int64_t> dst(2 * (size_t)n_parts);
    for (int32_t p = 0; p < n_parts; p++) {
        if (part_dst[p] < 0 || rec_dst[p] < 0 || part_dst[p] + part_bytes[p] > out_cap || rec_dst[p] + part_records[p] > rec_index_cap) {
            for (int32_t q = 0; q < n_parts; q++) part_bytes[q] = part_records[q] = 0;
            return PAFFY_E_CAPACITY;
        }
        dst[(size_t)p] = part_dst[p];
        dst[(size_t)n_parts + p] = rec_dst[p];
    }
    HIPCHK(c, hipMemcpyAsync(d_tot + 2 * np1, dst.data(), sizeof(int64_t) * 2 * (size_t)n_parts, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* `dst` is a local */
    if (n_sent > 0)
        LAUNCH(c, "k_split_sides_copy", k_split_sides_copy, dim3((unsigned)n_sent), dim3(PAFFY_NT), 0, in, (uint32_t)in_len, static_cast<const uint32_t *>(c->sep_pos.p),
               static_cast<const uint32_t *>(c->nl_idx.p), static_cast<const uint64_t *>(skey), static_cast<const uint64_t *>(off), static_cast<uint8_t *>(d_out),
               static_cast<const int64_t *>(d_tot), static_cast<const int64_t *>(d_tot + np1), static_cast<const int64_t *>(d_tot + 2 * np1),
               static_cast<const int64_t *>(d_tot + 2 * np1 + n_parts), n, static_cast<const uint8_t *>(item_mask), static_cast<int64_t *>(d_rec_index),
               static_cast<uint8_t *>(d_sides), rec_base);
    return 0;
}
int paffy_hip_split_sides_count(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int include_inverted, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner,
                                int64_t n_table, int64_t *part_bytes, int64_t *part_records, int64_t *n_records) {
    const int rc = split_sides_impl0(c, d_in, in_len, include_inverted != 0, n_parts, table_hash, table_owner, n_table, true, nullptr, 0, nullptr, nullptr, 0, part_bytes,
                                     part_records, nullptr, nullptr, 0, n_records);
    if (rc && c) index_drop_all(c);
    return rc;
}
int paffy_hip_split_sides_to(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int include_inverted, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner,
                             int64_t n_table, void *d_out, int64_t out_cap, const int64_t *part_dst, const int64_t *rec_dst, int64_t rec_base, int64_t *part_bytes,
                             int64_t *part_records, void *d_rec_index, void *d_sides, int64_t rec_index_cap, int64_t *n_records) {
    const int rc = split_sides_impl0(c, d_in, in_len, include_inverted != 0, n_parts, table_hash, table_owner, n_table, false, d_out, out_cap, part_dst, rec_dst, rec_base,
                                     part_bytes, part_records, d_rec_index, d_sides, rec_index_cap, n_records);
    if (rc && c) index_drop_all(c);
    return rc;
}
int paffy_hip_drop_index(paffy_hip_ctx *c, const void *d_in) {
    if (!c) return PAFFY_E_ARG;
    if (d_in) {
        index_drop(c, d_in);
        if (c->indexed_in == d_in) c->indexed_in = nullptr;
    } else {
        index_drop_all(c);
    }
    return 0;
}

int paffy_hip_scatter_lines(paffy_hip_ctx *c, const void *d_src, const void *d_src_off, const void *d_dst_off, int64_t n_lines, void *d_dst) {
    if (!c || n_lines < 0 || n_lines >= (1ll << 31)) return PAFFY_E_ARG;
    if (n_lines == 0) return 0;
    if (!d_src || !d_src_off || !d_dst_off || !d_dst) return PAFFY_E_ARG;
    LAUNCH(c, "k_scatter_lines", k_scatter_lines, dim3((unsigned)n_lines), dim3(PAFFY_NT), 0, static_cast<const uint8_t *>(d_src), static_cast<const int64_t *>(d_src_off),
           static_cast<const int64_t *>(d_dst_off), static_cast<uint8_t *>(d_dst));
    return 0;
}

/* After a tile run: (chain_score, score, input record, line bytes, tile level) of the lines emit writes, in output order -- what ranks
 * exchange to merge their shares of a `paffy tile` sharded by query sequence. Returns the line count. */
__global__ __launch_bounds__(PAFFY_NT) void k_tile_keys_out(const RecMeta *meta, const uint32_t *order, const int64_t *level, const uint64_t *out_len, uint64_t n,
                                                             int64_t *keys) {
    const uint64_t k = (uint64_t)blockIdx.x * PAFFY_NT + threadIdx.x;
    if (k >= n) return;
    const RecMeta &m = meta[order[k]];
    keys[5 * k + 0] = m.chain_score;
    keys[5 * k + 1] = m.score;
    keys[5 * k + 2] = order[k];
    keys[5 * k + 3] = (int64_t)out_len[k];
    keys[5 * k + 4] = level[order[k]];
}
int64_t paffy_hip_tile_keys(paffy_hip_ctx *c, int64_t cap_lines, void *d_keys) {
    if (!c || !d_keys) return PAFFY_E_ARG;
    if (!c->planned || c->plan_kind != PLAN_LINES || !c->cov) return PAFFY_E_STATE;
    CovState &S = cov_state(c);
    const uint64_t n = c->line_n;
    if (c->line_meta != static_cast<const RecMeta *>(S.meta.p)) return PAFFY_E_STATE; /* a dedupe plan */
    if ((uint64_t)cap_lines < n) return PAFFY_E_CAPACITY;
    if (n) LAUNCH(c, "k_tile_keys_out", k_tile_keys_out, dim3((unsigned)((n + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, c->line_meta, c->line_order, c->line_level,
                  static_cast<const uint64_t *>(S.out_len.p), n, static_cast<int64_t *>(d_keys));
    return (int64_t)n;
}

/* `paffy upconvert` (impl/paf_upconvert.c:144-156): index, header parse, k_upconvert, then the line writer of tile / dedupe (header + the
   cigar text as it was read) for every record in front of the first failing one */
static int upconvert_plan(paffy_hip_ctx *c, const void *d_in, int64_t in_len, bool check, paffy_plan_info *info) {
    plan_begin(c, PLAN_LINES, in_len, info);
    if (in_len == 0) {
        c->planned = true;
        return 0;
    }
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint32_t n = 0;
    {
        int rc = index_and_parse(c, in, (uint32_t)in_len, &n);
        if (rc) return rc;
    }
    c->plan.n_records = n;
    if (n == 0) {
        if (fetch_info(c)) return PAFFY_E_HIP;
        *info = c->plan;
        c->planned = true;
        return 0;
    }
    if (ensure(c, c->tile_level, sizeof(int64_t) * (size_t)n) || ensure(c, c->tile_order, sizeof(uint32_t) * (size_t)n) ||
        ensure(c, c->tile_len, sizeof(int64_t) * (size_t)(n + 2)))
        return PAFFY_E_HIP;
    RecMeta *meta = static_cast<RecMeta *>(c->meta.p);
    LAUNCH(c, "k_upconvert", k_upconvert, dim3((n + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, in, meta, n, static_cast<const UpInterval *>(c->up_table.p),
           c->n_intervals, static_cast<const uint8_t *>(c->up_names.p), check ? 1u : 0u, static_cast<uint32_t *>(c->tile_order.p),
           static_cast<int64_t *>(c->tile_level.p), static_cast<DevInfo *>(c->info.p));
    if (fetch_info(c)) return PAFFY_E_HIP;
    uint32_t nk = n;
    if (c->h_info->first_err_key != ~0ull) {
        const unsigned long long k = c->h_info->first_err_key;
        nk = (uint32_t)(k >> 16);
        c->plan.error.code = (int32_t)(k & 0xff);
        c->plan.error.stage = (int32_t)((k >> 8) & 0xff) - 1;
        c->plan.error.record = nk;
        if (c->plan.error.stage < 0) {
            RecMeta m;
            HIPCHK(c, hipMemcpy(&m, meta + nk, sizeof(m), hipMemcpyDeviceToHost));
            c->plan.error.aux = m.err_aux;
        }
    }
    int64_t total = 0;
    if (nk > 0) {
        int64_t *lens = static_cast<int64_t *>(c->tile_len.p);
        LAUNCH(c, "k_line_size", k_line_size, dim3((nk + 1 + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(meta),
               static_cast<const uint32_t *>(c->tile_order.p), static_cast<const int64_t *>(c->tile_level.p), (uint64_t)nk, reinterpret_cast<uint64_t *>(lens));
        if (ensure(c, c->out_off, sizeof(int64_t) * ((size_t)nk + 1))) return PAFFY_E_HIP;
        if (!c->dedupe) c->dedupe.reset(new DedupeState());
        DedupeState &D = *c->dedupe; /* its scratch for the scan */
        size_t bytes = 0;
        RPCHK(c, rocprim::exclusive_scan(nullptr, bytes, lens, static_cast<int64_t *>(c->out_off.p), (int64_t)0, (size_t)nk + 1, rocprim::plus<int64_t>(), c->stream));
        if (ensure(c, D.tmp, bytes + 16)) return PAFFY_E_HIP;
        RPCHK(c, rocprim::exclusive_scan(D.tmp.p, bytes, lens, static_cast<int64_t *>(c->out_off.p), (int64_t)0, (size_t)nk + 1, rocprim::plus<int64_t>(), c->stream));
        HIPCHK(c, hipMemcpyAsync(&total, static_cast<int64_t *>(c->out_off.p) + nk, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        if (ensure(c, c->one_batch, sizeof(void *))) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(c->one_batch.p, &in, sizeof(void *), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (c->profile) prof_collect(c);
    c->plan.out_bytes = total;
    c->plan.n_rows = nk;
    c->line_batches = static_cast<const uint8_t *const *>(c->one_batch.p);
    c->line_meta = meta;
    c->line_names2 = static_cast<const uint8_t *>(c->up_names.p);
    c->line_order = static_cast<const uint32_t *>(c->tile_order.p);
    c->line_level = static_cast<const int64_t *>(c->tile_level.p);
    c->line_off = static_cast<const uint64_t *>(c->out_off.p);
    c->line_n = total ? nk : 0;
    *info = c->plan;
    c->planned = true;
    return 0;
}

/* decode_fasta_header (impl/paf.c:716-731) of a FASTA header: false when the reference's asserts would fire */
static bool up_decode(const char *h, std::string &name, int64_t &start, int64_t &length) {
    const size_t n = strlen(h);
    size_t c1 = n, c2 = n; /* the last and the second-to-last '|' */
    for (size_t i = n; i > 0; i--)
        if (h[i - 1] == '|') {
            if (c1 == n) c1 = i - 1;
            else {
                c2 = i - 1;
                break;
            }
        }
    if (c1 == n) return false;
    int64_t a = 0, b = 0;
    const std::string ts(h + c1 + 1), tl(c2 == n ? std::string(h, c1) : std::string(h + c2 + 1, c1 - c2 - 1));
    if (sscanf(ts.c_str(), "%" SCNi64, &a) != 1 || sscanf(tl.c_str(), "%" SCNi64, &b) != 1) return false;
    name.assign(h, c2 == n ? 0 : c2);
    start = a;
    length = b;
    return true;
}

struct UpHost {
    std::string name;
    int64_t start, end, length;
};
static int up_cmp_intervals(const void *i, const void *j) { /* cmp_intervals, impl/paf.c:733-737 */
    const UpHost *x = *static_cast<const UpHost *const *>(i), *y = *static_cast<const UpHost *const *>(j);
    const int k = strcmp(x->name.c_str(), y->name.c_str());
    return k == 0 ? (x->start < y->start ? -1 : (x->start > y->start ? 1 : 0)) : k;
}

int paffy_hip_set_intervals(paffy_hip_ctx *c, const char *const *headers, const int64_t *seq_lens, int64_t n) {
    if (!c || n < 0 || n >= (1ll << 31) || (n > 0 && (!headers || !seq_lens))) return PAFFY_E_ARG;
    c->n_intervals = 0;
    c->up_blob_bytes = 0;
    c->up_on_device = false;
    c->up_rounds = 0;
    std::vector<UpHost> iv((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (!headers[i] || !up_decode(headers[i], iv[(size_t)i].name, iv[(size_t)i].start, iv[(size_t)i].length)) {
            c->last_error = "upconvert: a FASTA header does not end in |length|start";
            return PAFFY_E_HEADER;
        }
        iv[(size_t)i].end = (int64_t)((uint64_t)iv[(size_t)i].start + (uint64_t)seq_lens[i]); /* i->start + strlen(sequence) */
    }
    /* stList_sort: qsort of the list's pointer array */
    std::vector<UpHost *> ptr((size_t)n);
    for (int64_t i = 0; i < n; i++) ptr[(size_t)i] = &iv[(size_t)i];
    if (n > 1) qsort(ptr.data(), (size_t)n, sizeof(UpHost *), up_cmp_intervals);
    std::vector<UpInterval> tab((size_t)n);
    std::string blob;
    char num[64];
    for (int64_t i = 0; i < n; i++) {
        const UpHost &h = *ptr[(size_t)i];
        UpInterval &t = tab[(size_t)i];
        t.start = h.start;
        t.end = h.end;
        t.length = h.length;
        t.name_off = (uint32_t)blob.size();
        t.name_len = (uint32_t)h.name.size();
        blob += h.name;
        snprintf(num, sizeof(num), "|%lld|%lld", (long long)h.length, (long long)h.start); /* "%s|%" PRIi64 "|%" PRIi64, impl/paf_upconvert.c:55 */
        t.out_off = (uint32_t)blob.size();
        t.out_len = t.name_len + (uint32_t)strlen(num);
        blob += h.name;
        blob += num;
        if (blob.size() >= 0xffffffffull) return PAFFY_E_ARG;
    }
    if (n > 0) {
        if (ensure(c, c->up_table, sizeof(UpInterval) * (size_t)n) || ensure(c, c->up_names, blob.size() + 16)) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpy(c->up_table.p, tab.data(), sizeof(UpInterval) * (size_t)n, hipMemcpyHostToDevice));
        if (!blob.empty()) HIPCHK(c, hipMemcpy(c->up_names.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    }
    c->n_intervals = (uint32_t)n;
    c->up_blob_bytes = blob.size();
    return 0;
}

static void dedupe_parts_reset(paffy_hip_ctx *c); /* dedupe_parts_kernel.h */
int paffy_hip_dedupe_reset(paffy_hip_ctx *c) {
    if (!c) return PAFFY_E_ARG;
    if (c->dedupe) c->dedupe->seen_n = 0;
    dedupe_parts_reset(c);
    return 0;
}

/* the tail of a dedupe plan: the nk records listed in tile_order (input order) become the plan's lines -- sizes, offsets, the table emit
   reads. The verbatim writer of tile: header + the cigar text as it was read. Shared with the plan of a part (dedupe_parts_kernel.h). */
static int dedupe_plan_lines(paffy_hip_ctx *c, const uint8_t *in, uint32_t nk, paffy_plan_info *info) {
    int64_t total = 0;
    if (nk > 0) {
        int64_t *lens = static_cast<int64_t *>(c->tile_len.p);
        LAUNCH(c, "k_line_size", k_line_size, dim3((nk + 1 + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(c->meta.p),
               static_cast<const uint32_t *>(c->tile_order.p), static_cast<const int64_t *>(c->tile_level.p), (uint64_t)nk, reinterpret_cast<uint64_t *>(lens));
        { /* offsets of the lines: exclusive scan of nk + 1 lengths (the last one zero, k_line_size), so that entry nk is the total */
            if (ensure(c, c->out_off, sizeof(int64_t) * ((size_t)nk + 1))) return PAFFY_E_HIP;
            DedupeState &D = *c->dedupe;
            size_t bytes = 0;
            RPCHK(c, rocprim::exclusive_scan(nullptr, bytes, lens, static_cast<int64_t *>(c->out_off.p), (int64_t)0, (size_t)nk + 1, rocprim::plus<int64_t>(), c->stream));
            if (ensure(c, D.tmp, bytes + 16)) return PAFFY_E_HIP;
            RPCHK(c, rocprim::exclusive_scan(D.tmp.p, bytes, lens, static_cast<int64_t *>(c->out_off.p), (int64_t)0, (size_t)nk + 1, rocprim::plus<int64_t>(), c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(&total, static_cast<int64_t *>(c->out_off.p) + nk, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        if (ensure(c, c->one_batch, sizeof(void *))) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(c->one_batch.p, &in, sizeof(void *), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (c->profile) prof_collect(c);
    c->plan.out_bytes = total;
    c->plan.n_rows = nk;
    c->line_batches = static_cast<const uint8_t *const *>(c->one_batch.p);
    c->line_meta = static_cast<const RecMeta *>(c->meta.p);
    c->line_names2 = nullptr;
    c->line_order = static_cast<const uint32_t *>(c->tile_order.p);
    c->line_level = static_cast<const int64_t *>(c->tile_level.p);
    c->line_off = static_cast<const uint64_t *>(c->out_off.p);
    c->line_n = total ? nk : 0;
    *info = c->plan;
    c->planned = true;
    return 0;
}

/* the head of a dedupe plan (plan_begin has run): index, header parse, keys, the selection and the record that ends the run. *n = the
   batch's records, tile_order[0 .. *nk) = the records written, in input order. Shared with the plan of split_file (split_host.h). */
static int dedupe_plan_select(paffy_hip_ctx *c, const uint8_t *in, int64_t in_len, int check_inverse, uint32_t *n_out, uint32_t *nk_out) {
    uint32_t n = 0;
    *n_out = 0;
    *nk_out = 0;
    {
        int rc = index_and_parse(c, in, (uint32_t)in_len, &n);
        if (rc) return rc;
    }
    c->plan.n_records = n;
    if (n == 0) return 0;
    const uint32_t grid = (n + PAFFY_NT - 1) / PAFFY_NT;
    if (ensure(c, c->dedupe_keys, sizeof(DedupeKey) * (size_t)n)) return PAFFY_E_HIP;
    if (ensure(c, c->tile_level, sizeof(int64_t) * (size_t)n)) return PAFFY_E_HIP;
    if (ensure(c, c->tile_order, sizeof(uint32_t) * (size_t)n)) return PAFFY_E_HIP;
    if (ensure(c, c->tile_len, sizeof(int64_t) * (size_t)(n + 2))) return PAFFY_E_HIP;
    LAUNCH(c, "k_dedupe_keys", k_dedupe_keys, dim3(grid), dim3(PAFFY_NT), 0, in, static_cast<const RecMeta *>(c->meta.p), n,
           static_cast<DedupeKey *>(c->dedupe_keys.p), static_cast<int64_t *>(c->tile_level.p));
    /* the reference's loop, record by record (impl/paf_dedupe.c:117-143): first seen wins -- on the device, dedupe_host.h */
    if (!c->dedupe) c->dedupe.reset(new DedupeState());
    uint32_t nk = 0, first_bad = n;
    {
        int rc = dedupe_select(c, *c->dedupe, static_cast<const DedupeKey *>(c->dedupe_keys.p), n, check_inverse, static_cast<uint32_t *>(c->tile_order.p), &nk, &first_bad);
        if (rc) return rc;
    }
    if (first_bad < n) { /* the record that ends the run: a parse error, or paf_check (impl/paf_dedupe.c:126) */
        DedupeKey k;
        HIPCHK(c, hipMemcpy(&k, static_cast<const DedupeKey *>(c->dedupe_keys.p) + first_bad, sizeof(k), hipMemcpyDeviceToHost));
        c->plan.error.record = first_bad;
        if (k.err) {
            c->plan.error.code = k.err;
            c->plan.error.stage = -1;
            RecMeta m;
            HIPCHK(c, hipMemcpy(&m, static_cast<RecMeta *>(c->meta.p) + first_bad, sizeof(m), hipMemcpyDeviceToHost));
            c->plan.error.aux = m.err_aux;
        } else {
            c->plan.error.code = k.check;
            c->plan.error.stage = 0;
        }
    }
    *n_out = n;
    *nk_out = nk;
    return 0;
}

int paffy_hip_dedupe_plan(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int check_inverse, paffy_plan_info *info) {
    if (!c || !info) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    plan_begin(c, PLAN_LINES, in_len, info); /* same writer as tile: header + the cigar text as it was read */
    if (in_len == 0) {
        c->planned = true;
        return 0;
    }
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint32_t n = 0, nk = 0;
    {
        int rc = dedupe_plan_select(c, in, in_len, check_inverse, &n, &nk);
        if (rc) return rc;
    }
    if (n == 0) {
        *info = c->plan;
        c->planned = true;
        return 0;
    }
    return dedupe_plan_lines(c, in, nk, info);
}

#include "split_host.h"

#include "dedupe_parts_kernel.h"

/* a plan made under paffy_hip_stats_only has sums and nothing else: what reads ops, rows or a line plan is refused */
static bool stats_only_refuses(paffy_hip_ctx *c, const char *what) {
    if (!c->planned || !c->plan_stats_only) return false;
    c->last_error = std::string(what) + ": the plan was made under paffy_hip_stats_only (sums only: no ops, rows or lines were built)";
    return true;
}

int64_t paffy_hip_plan_rows(paffy_hip_ctx *c, int64_t cap, uint32_t *record, int64_t *out_off) {
    if (!c || !record || !out_off) return PAFFY_E_ARG;
    if (stats_only_refuses(c, "paffy_hip_plan_rows")) return PAFFY_E_STATE;
    if (!c->planned || c->plan_kind != PLAN_LINES) return PAFFY_E_STATE;
    const int64_t n = (int64_t)c->line_n;
    if (cap < n + 1) return PAFFY_E_CAPACITY;
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(record, c->line_order, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_off, c->line_off, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    out_off[n] = c->plan.out_bytes;
    return n;
}

int paffy_hip_emit(paffy_hip_ctx *c, void *d_out, int64_t out_cap) {
    if (!c) return PAFFY_E_ARG;
    if (!c->planned) return PAFFY_E_STATE;
    if (stats_only_refuses(c, "paffy_hip_emit")) return PAFFY_E_STATE;
    if (c->plan.out_bytes == 0 || (c->plan_kind == PLAN_RECORDS && c->kp.n_rec == 0)) return 0;
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 15)) return PAFFY_E_ARG;
    if (out_cap < c->plan.out_bytes) return PAFFY_E_CAPACITY;
    if (c->plan_kind == PLAN_BED) {
        const uint64_t n_runs = c->bed_runs;
        LAUNCH(c, "k_bed_lines", k_bed_lines, dim3((unsigned)((n_runs + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, *c->bed_params,
               static_cast<const uint64_t *>(c->bed_starts.p), n_runs, static_cast<int64_t *>(c->bed_len.p), static_cast<const int64_t *>(c->bed_off.p),
               static_cast<uint8_t *>(d_out));
        return 0;
    }
    if (c->plan_kind == PLAN_LINES) {
        if (c->line_n) LAUNCH(c, "k_tile_emit", k_line_emit, dim3((unsigned)((c->line_n + PAFFY_NWAVE - 1) / PAFFY_NWAVE)), dim3(PAFFY_NT), 0, c->line_batches, c->line_meta,
                              c->line_order, c->line_level, c->line_off, (uint64_t)0, c->line_n, (uint64_t)0, static_cast<uint8_t *>(d_out), c->line_names2);
        return 0;
    }
    KParams kp = c->kp;
    kp.out = static_cast<uint8_t *>(d_out);
    const bool shatter = kp.n_stages > 0 && kp.stages[kp.n_stages - 1].kind == PAFFY_SHATTER;
    if (shatter) {
        LAUNCH(c, "k_emit_rows", k_emit_rows, dim3(kp.n_rec + kp.n_items), dim3(64), PAFFY_ROWS_LDS_BYTES, kp);
        /* the records whose first row piece is shorter than 16 bytes (names like chr1): none in most batches */
        if (c->h_info->s_count > 0) LAUNCH(c, "k_emit_rows_short", k_emit_rows_short, dim3(kp.n_rec), dim3(64), PAFFY_ROWS_LDS_BYTES, kp);
        if (c->h_info->g_count > 0) LAUNCH(c, "k_emit_lds", k_emit_lds<true>, dim3(kp.n_rec), dim3(PAFFY_NT), PAFFY_EMIT_LDS_BYTES, kp);
        if (c->h_info->w_count > 0) LAUNCH(c, "k_arena_emit", k_arena_emit<true>, dim3(2048), dim3(PAFFY_NT), PAFFY_EMIT_LDS_BYTES, kp);
    } else {
        LAUNCH(c, "k_emit_line", k_emit_line, dim3(kp.n_rec + kp.n_items), dim3(64), PAFFY_LINE_LDS_BYTES, kp);
        /* the lines of the flat pass whose cigar is a stretch of the input's (a workgroup without such a record ends at once) */
        if (kp.flat_done && !kp.new_ops) LAUNCH(c, "k_emit_copy", k_emit_copy, dim3(kp.n_rec), dim3(64), PAFFY_COPY_LDS_BYTES, kp);
        if (c->h_info->g_count > 0) LAUNCH(c, "k_emit_lds<line>", k_emit_lds<false>, dim3(kp.n_rec), dim3(PAFFY_NT), PAFFY_EMIT_LDS_BYTES, kp);
        if (c->h_info->w_count > 0) LAUNCH(c, "k_arena_emit<line>", k_arena_emit<false>, dim3(2048), dim3(PAFFY_NT), PAFFY_EMIT_LDS_BYTES, kp);
    }
    return 0;
}

/* lines [first, first + n) of a line plan (tile, dedupe) into d_out, the first of them at d_out[0]: for hosts that drain a
 * large output through a bounded staging buffer. *bytes = what was written. */
int paffy_hip_emit_lines(paffy_hip_ctx *c, int64_t first, int64_t n, void *d_out, int64_t out_cap, int64_t *bytes) {
    if (!c || !bytes || first < 0 || n < 0) return PAFFY_E_ARG;
    if (stats_only_refuses(c, "paffy_hip_emit_lines")) return PAFFY_E_STATE;
    if (!c->planned || c->plan_kind != PLAN_LINES) return PAFFY_E_STATE;
    *bytes = 0;
    if ((uint64_t)(first + n) > c->line_n) return PAFFY_E_ARG;
    if (n == 0) return 0;
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 15)) return PAFFY_E_ARG;
    uint64_t lo = 0, hi = (uint64_t)c->plan.out_bytes;
    HIPCHK(c, hipMemcpyAsync(&lo, c->line_off + first, sizeof(lo), hipMemcpyDeviceToHost, c->stream));
    if ((uint64_t)(first + n) < c->line_n) HIPCHK(c, hipMemcpyAsync(&hi, c->line_off + first + n, sizeof(hi), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((int64_t)(hi - lo) > out_cap) return PAFFY_E_CAPACITY;
    LAUNCH(c, "k_tile_emit", k_line_emit, dim3((unsigned)((n + PAFFY_NWAVE - 1) / PAFFY_NWAVE)), dim3(PAFFY_NT), 0, c->line_batches, c->line_meta, c->line_order, c->line_level,
           c->line_off, (uint64_t)first, (uint64_t)n, lo, static_cast<uint8_t *>(d_out), c->line_names2);
    *bytes = (int64_t)(hi - lo);
    return 0;
}

int paffy_hip_sync(paffy_hip_ctx *c) {
    if (!c) return PAFFY_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->profile) prof_collect(c);
    return 0;
}

int paffy_hip_run_host(paffy_hip_ctx *c, const paffy_stage *stages, int32_t n_stages, const char *h_in, int64_t in_len, char **h_out,
                       int64_t *out_len, paffy_plan_info *info) {
    if (!c || !h_out || !out_len || !info) return PAFFY_E_ARG;
    *h_out = nullptr;
    *out_len = 0;
    /* the device buffers stay with the context: the record API (host/paf_api.c) makes one such call per record */
    void *d_in = nullptr, *d_out = nullptr;
    int rc = 0;
    if (in_len > 0) {
        if (ensure(c, c->host_in, (size_t)in_len + 64)) return PAFFY_E_HIP;
        d_in = c->host_in.p;
        if (hipMemcpyAsync(d_in, h_in, (size_t)in_len, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = PAFFY_E_HIP;
    }
    if (!rc) rc = paffy_hip_plan(c, stages, n_stages, d_in, in_len, info);
    if (!rc && info->out_bytes > 0) {
        if (ensure(c, c->host_out, (size_t)info->out_bytes + 64)) return PAFFY_E_HIP;
        d_out = c->host_out.p;
        rc = paffy_hip_emit(c, d_out, info->out_bytes + 64);
        if (!rc) {
            *h_out = static_cast<char *>(malloc((size_t)info->out_bytes));
            if (!*h_out || hipMemcpyAsync(*h_out, d_out, (size_t)info->out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = PAFFY_E_HIP;
            *out_len = info->out_bytes;
        }
        if (!rc) rc = paffy_hip_sync(c);
    }
    c->planned = false; /* the input buffer will be overwritten by the next call */
    return rc;
}

/*
 * Streaming through host buffers (the loop of impl/paf_invert.c:84-89 and friends with the GPU in the middle): two slots, each a
 * pinned input buffer and device in / out buffers; the output returns through two pinned pieces. Chunk k + 1 is copied in, planned
 * and written on the GPU while the host still drains chunk k: H2D, kernels and D2H run on three streams.
 */
struct StreamSlot {
    char *h_in = nullptr;
    size_t h_cap = 0;
    DevBuf d_in, d_out;
    hipEvent_t ev_in = nullptr, ev_emit = nullptr;
    int64_t out_len = 0, read_at = 0; /* bytes of output, bytes already handed to the host */
    bool busy = false;
    /* view mode: the chunk's ranges, the one in d_out, the verdict of that range (pinned) and whether read has looked at it */
    int64_t view_ranges = 0, view_range_at = 0;
    int64_t *h_verdict = nullptr;
    bool verdict_seen = false, view_open = false; /* view_open: this chunk has more than one range */
};
struct paffy_hip_stream {
    paffy_hip_ctx *c = nullptr;
    paffy_stage stages[PAFFY_MAX_STAGES];
    int32_t n_stages = 0;
    StreamSlot slot[2];
    int fill = 0, drain = 0; /* slot the next chunk goes to, slot being read */
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    /* three output pieces: the one handed out, the one handed out before it (still the caller's until the next read) and the one in flight */
    char *piece[3] = {nullptr, nullptr, nullptr};
    size_t piece_cap = 0;
    hipEvent_t ev_piece[3] = {nullptr, nullptr, nullptr};
    int64_t piece_len[3] = {0, 0, 0};
    int64_t issued_at = 0; /* bytes of the draining chunk whose copy has been issued */
    int n_issued = 0, n_returned = 0;
    /* paffy_hip_stream_open_view: -1 a stream of stage lists; 0 sums only, 1 stats lines, 2 lines and base-level rows */
    int view_text = -1;
    int64_t view_range_bytes = 0;
    int64_t view_sums[6] = {0, 0, 0, 0, 0, 0}, view_records = 0;
    bool view_open = false; /* the chunk submitted last has ranges still to be written: the plan stays until it is read out */
    paffy_error view_rows_err = {0, 0, 0, 0};
    bool view_failed = false;
};
static int view_stream_submit(paffy_hip_stream *s, int64_t in_len, paffy_plan_info *info);
static int view_stream_read(paffy_hip_stream *s, const char **piece, int64_t *len);

static void stream_detach(paffy_hip_stream *s) { s->c = nullptr; }

int paffy_hip_stream_trim(paffy_hip_ctx *c) {
    if (!c) return PAFFY_E_ARG;
    for (int k = 0; k < 2; k++)
        for (int b = 0; b < 2; b++) (void)c->kept_slot[k][b].release();
    return 0;
}

int paffy_hip_stream_open(paffy_hip_ctx *c, const paffy_stage *stages, int32_t n_stages, int64_t chunk_bytes, int64_t piece_bytes, paffy_hip_stream **out) {
    if (!c || !out || n_stages < 0 || n_stages > PAFFY_MAX_STAGES || (n_stages > 0 && !stages) || chunk_bytes < 4096 || chunk_bytes >= (1ll << 31) - 64 || piece_bytes < 4096)
        return PAFFY_E_ARG;
    paffy_hip_stream *s = new paffy_hip_stream();
    s->c = c;
    c->open_streams.push_back(s);
    s->n_stages = n_stages;
    for (int32_t i = 0; i < n_stages; i++) s->stages[i] = stages[i];
    bool ok = hipStreamCreateWithFlags(&s->s_h2d, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&s->s_d2h, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < 2; k++) { /* the device buffers the stream before left with the context */
        s->slot[k].d_in = std::move(c->kept_slot[k][0]);
        s->slot[k].d_out = std::move(c->kept_slot[k][1]);
    }
    for (int k = 0; k < 2 && ok; k++) {
        StreamSlot &sl = s->slot[k];
        sl.h_cap = (size_t)chunk_bytes;
        ok = hipHostMalloc(reinterpret_cast<void **>(&sl.h_in), sl.h_cap + 64) == hipSuccess && hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sl.ev_emit, hipEventDisableTiming) == hipSuccess;
    }
    for (int k = 0; k < 3 && ok; k++)
        ok = hipHostMalloc(reinterpret_cast<void **>(&s->piece[k]), (size_t)piece_bytes) == hipSuccess && hipEventCreateWithFlags(&s->ev_piece[k], hipEventDisableTiming) == hipSuccess;
    s->piece_cap = (size_t)piece_bytes;
    if (!ok) {
        c->last_error = "paffy_hip_stream_open: pinned buffers / streams";
        paffy_hip_stream_close(s);
        return PAFFY_E_HIP;
    }
    *out = s;
    return 0;
}

void paffy_hip_stream_close(paffy_hip_stream *s) {
    if (s && s->c) { /* no longer an open stream of its context */
        auto &v = s->c->open_streams;
        for (size_t k = 0; k < v.size(); k++)
            if (v[k] == s) {
                v.erase(v.begin() + (long)k);
                break;
            }
    }
    if (!s) return;
    (void)hipDeviceSynchronize();
    for (int k = 0; k < 2; k++) {
        StreamSlot &sl = s->slot[k];
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        /* the device buffers stay with the context for its next stream (freed with it or by paffy_hip_stream_trim); where the context
           is gone or holds one already, they go with the stream */
        if (s->c) {
            DevBuf(&kept)[2] = s->c->kept_slot[k];
            if (!kept[0].p) kept[0] = std::move(sl.d_in);
            if (!kept[1].p) kept[1] = std::move(sl.d_out);
        }
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_emit) (void)hipEventDestroy(sl.ev_emit);
        if (sl.h_verdict) (void)hipHostFree(sl.h_verdict);
    }
    for (int k = 0; k < 3; k++) {
        if (s->piece[k]) (void)hipHostFree(s->piece[k]);
        if (s->ev_piece[k]) (void)hipEventDestroy(s->ev_piece[k]);
    }
    if (s->s_h2d) (void)hipStreamDestroy(s->s_h2d);
    if (s->s_d2h) (void)hipStreamDestroy(s->s_d2h);
    delete s;
}

/* the pinned buffer the next chunk is to be written into (NULL while both slots hold unread output); with want > its capacity it is
   enlarged, keeping the first `keep` bytes (a line longer than the chunk) */
char *paffy_hip_stream_input(paffy_hip_stream *s, int64_t want, int64_t keep, int64_t *cap) {
    if (!s || !cap) return nullptr;
    StreamSlot &sl = s->slot[s->fill];
    if (sl.busy || s->view_open) return nullptr;
    if (want > (int64_t)sl.h_cap) {
        if (want >= (1ll << 31) - 64) return nullptr;
        char *nb = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&nb), (size_t)want + 64) != hipSuccess) return nullptr;
        if (keep > 0) memcpy(nb, sl.h_in, (size_t)keep);
        (void)hipHostFree(sl.h_in);
        sl.h_in = nb;
        sl.h_cap = (size_t)want;
    }
    *cap = (int64_t)sl.h_cap;
    return sl.h_in;
}

/* ---- what both kinds of stream (stage lists, view mode) do alike ---- */
/* stage-in: room for the chunk on the device, its copy on the H2D stream, and the kernels wait for it */
static int stream_stage_in(paffy_hip_stream *s, StreamSlot &sl, int64_t in_len) {
    paffy_hip_ctx *c = s->c;
    if ((size_t)in_len + 64 > sl.d_in.cap) {
        HIPCHK(c, sl.d_in.release());
        HIPCHK(c, sl.d_in.alloc((size_t)in_len + (size_t)in_len / 4 + 4096));
    }
    if (in_len > 0) HIPCHK(c, hipMemcpyAsync(sl.d_in.p, sl.h_in, (size_t)in_len, hipMemcpyHostToDevice, s->s_h2d));
    HIPCHK(c, hipEventRecord(sl.ev_in, s->s_h2d));
    HIPCHK(c, hipStreamWaitEvent(c->stream, sl.ev_in, 0));
    return 0;
}
/* room for `bytes` of output in the slot; slack: a quarter more, so that a chunk a little longer than the last costs no allocation */
static int stream_out_room(paffy_hip_ctx *c, StreamSlot &sl, int64_t bytes, bool slack) {
    if ((size_t)bytes + 64 <= sl.d_out.cap) return 0;
    HIPCHK(c, sl.d_out.release());
    HIPCHK(c, sl.d_out.alloc((size_t)bytes + (slack ? (size_t)bytes / 4 : 0) + 4096));
    return 0;
}
/* the writers of the slot's output are enqueued: the chunk is the stream's */
static int stream_submitted(paffy_hip_stream *s, StreamSlot &sl) {
    HIPCHK(s->c, hipEventRecord(sl.ev_emit, s->c->stream));
    sl.busy = true;
    s->fill ^= 1;
    return 0;
}
/* keep two copies in flight: the piece handed out now and the one after it, of the sl.out_len bytes in the slot's output */
static int stream_issue_pieces(paffy_hip_stream *s, StreamSlot &sl) {
    paffy_hip_ctx *c = s->c;
    while (s->n_issued < s->n_returned + 2 && s->issued_at < sl.out_len) {
        const int k = s->n_issued % 3;
        const int64_t n = sl.out_len - s->issued_at < (int64_t)s->piece_cap ? sl.out_len - s->issued_at : (int64_t)s->piece_cap;
        HIPCHK(c, hipMemcpyAsync(s->piece[k], static_cast<char *>(sl.d_out.p) + s->issued_at, (size_t)n, hipMemcpyDeviceToHost, s->s_d2h));
        HIPCHK(c, hipEventRecord(s->ev_piece[k], s->s_d2h));
        s->piece_len[k] = n;
        s->issued_at += n;
        s->n_issued++;
    }
    return 0;
}
/* everything of the draining chunk has been handed out: the next chunk's turn */
static void stream_chunk_done(paffy_hip_stream *s, StreamSlot &sl) {
    sl.busy = false;
    s->drain ^= 1;
    s->issued_at = 0;
    s->n_issued = s->n_returned = 0;
}
/* the oldest piece in flight, once it has arrived */
static int stream_hand_out(paffy_hip_stream *s, const char **piece, int64_t *len) {
    const int k = s->n_returned % 3;
    HIPCHK(s->c, hipEventSynchronize(s->ev_piece[k]));
    *piece = s->piece[k];
    *len = s->piece_len[k];
    s->n_returned++;
    return 0;
}

/* the first in_len bytes of the current input buffer (whole lines) go through the stage list; *info is complete on return (the
   plan is synchronous), the output is drained with paffy_hip_stream_read */
int paffy_hip_stream_submit(paffy_hip_stream *s, int64_t in_len, paffy_plan_info *info) {
    if (!s || !info || in_len < 0) return PAFFY_E_ARG;
    if (s->view_text >= 0) return view_stream_submit(s, in_len, info);
    paffy_hip_ctx *c = s->c;
    StreamSlot &sl = s->slot[s->fill];
    if (sl.busy || in_len > (int64_t)sl.h_cap) return PAFFY_E_STATE;
    int rc = stream_stage_in(s, sl, in_len);
    if (!rc) rc = paffy_hip_plan(c, s->stages, s->n_stages, sl.d_in.p, in_len, info);
    if (rc) return rc;
    sl.out_len = info->out_bytes;
    sl.read_at = 0;
    if (sl.out_len > 0) {
        rc = stream_out_room(c, sl, sl.out_len, true);
        if (!rc) rc = paffy_hip_emit(c, sl.d_out.p, (int64_t)sl.d_out.cap);
        if (rc) return rc;
    }
    return stream_submitted(s, sl);
}

/* the next piece of the oldest submitted chunk's output: *len bytes at *piece, valid until the call after next (three pinned pieces
   rotate: this call starts the copy that follows the piece it hands out, into the buffer handed out two calls ago); *len = 0: that
   chunk has been read completely (or nothing was submitted) */
int paffy_hip_stream_read(paffy_hip_stream *s, const char **piece, int64_t *len) {
    if (!s || !piece || !len) return PAFFY_E_ARG;
    if (s->view_text >= 0) return view_stream_read(s, piece, len);
    paffy_hip_ctx *c = s->c;
    *piece = nullptr;
    *len = 0;
    StreamSlot &sl = s->slot[s->drain];
    if (!sl.busy) return 0;
    if (s->n_issued == 0) HIPCHK(c, hipStreamWaitEvent(s->s_d2h, sl.ev_emit, 0)); /* first piece of this chunk */
    int rc = stream_issue_pieces(s, sl);
    if (rc) return rc;
    if (s->n_returned == s->n_issued) { /* everything of this chunk has been handed out */
        stream_chunk_done(s, sl);
        return 0;
    }
    return stream_hand_out(s, piece, len);
}

/* exclusive scan of n int64 values on the device (two levels); *total on the host */
static int scan64(paffy_hip_ctx *c, const int64_t *in, uint64_t n, int64_t *out, int64_t *total) {
    const uint64_t tiles = (n + PAFFY_NT * 16 - 1) / (PAFFY_NT * 16);
    if (ensure(c, c->bed_tiles, sizeof(int64_t) * (size_t)(2 * tiles + 2))) return PAFFY_E_HIP;
    int64_t *sums = static_cast<int64_t *>(c->bed_tiles.p), *offs = sums + tiles, *tot = offs + tiles;
    LAUNCH(c, "k_scan64_tiles", k_scan64_tiles, dim3((unsigned)tiles), dim3(PAFFY_NT), 0, in, n, sums);
    LAUNCH(c, "k_scan_i64", k_scan_i64, dim3(1), dim3(PAFFY_NT), 0, sums, (uint32_t)tiles, offs, tot);
    LAUNCH(c, "k_scan64_fix", k_scan64_fix, dim3((unsigned)tiles), dim3(PAFFY_NT), 0, in, n, static_cast<const int64_t *>(offs), out);
    HIPCHK(c, hipMemcpyAsync(total, tot, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/*
 * `paffy to_bed` (impl/paf_to_bed.c:166-190) over any number of text batches: coverage counters per sequence as in `paffy tile`
 * (every record bumps the counters of its query range; with include_inverted also those of its target range, as the inverted
 * record would), then each sequence's counters as maximal runs. Sequences are written in order of first appearance (the
 * reference iterates a sonLib hash: its order is not defined). Any failing record means no output.
 */
int paffy_hip_bed_begin(paffy_hip_ctx *c, const paffy_bed_opts *opts) {
    if (c) (void)paffy_hip_stream_trim(c); /* a closed stream's slot buffers (tens of GB) are this command's to use */
    if (!c || !opts) return PAFFY_E_ARG;
    c->planned = false;
    index_drop_all(c);
    return cov_begin(c, opts->include_inverted ? 2 : 1);
}
int paffy_hip_bed_add(paffy_hip_ctx *c, const void *d_in, int64_t in_len) {
    if (!c) return PAFFY_E_ARG;
    return cov_add(c, d_in, in_len, false);
}
int paffy_hip_bed_add_sides(paffy_hip_ctx *c, const void *d_in, int64_t in_len, const void *d_sides) {
    if (!c) return PAFFY_E_ARG;
    return cov_add_sides(c, d_in, in_len, d_sides);
}
int paffy_hip_bed_run(paffy_hip_ctx *c, const paffy_bed_opts *opts, paffy_plan_info *info) {
    if (!c || !info || !opts) return PAFFY_E_ARG;
    CovState &S = cov_state(c);
    if (S.sides != (opts->include_inverted ? 2u : 1u)) return PAFFY_E_STATE;
    plan_begin(c, PLAN_BED, cov_in_bytes(S), info);
    c->plan.n_records = (int64_t)S.n_rec;
    if (S.n_rec == 0) {
        *info = c->plan;
        c->planned = true;
        return 0;
    }
    int rc = cov_run(c, 1, &c->plan.error);
    if (rc) return rc;
    if (c->plan.error.code) {
        if (c->plan.error.code == PAFFY_ERR_CIGAR_CHAR) c->plan.error.stage = -1; /* the read loop parses the cigar (paf_read(.., 1)) */
        *info = c->plan;
        c->planned = true;
        return 0;
    }
    /* the runs: sequences in order of first appearance = ascending counter bases */
    const size_t ns = S.n_contigs;
    std::vector<uint64_t> cbase(ns + 1);
    std::vector<int64_t> clen(ns);
    std::vector<uint32_t> name_off(ns), name_len(ns);
    {
        std::vector<CovName> cname(ns);
        if (cov_fetch(c, cname.data(), S.name_tab.p, sizeof(CovName) * ns)) return PAFFY_E_HIP;
        std::vector<uint32_t> boff(ns + 1);
        uint32_t at = 0;
        for (size_t ci = 0; ci < ns; ci++) {
            boff[ci] = at;
            at += cname[ci].len;
        }
        for (size_t k = 0; k < ns; k++) {
            const uint32_t ci = S.appearance[k];
            cbase[k] = S.h_contig_cov[ci];
            clen[k] = S.h_contig_len[ci];
            name_off[k] = boff[ci];
            name_len[k] = cname[ci].len;
        }
        cbase[ns] = S.cov_total;
    }
    if (ensure(c, c->bed_tab, 8 * (2 * ns + 1) + 4 * 2 * ns + 64)) return PAFFY_E_HIP;
    uint64_t *d_cbase = static_cast<uint64_t *>(c->bed_tab.p);
    int64_t *d_clen = reinterpret_cast<int64_t *>(d_cbase + ns + 1);
    uint32_t *d_noff = reinterpret_cast<uint32_t *>(d_clen + ns), *d_nlen = d_noff + ns;
    HIPCHK(c, hipMemcpyAsync(d_cbase, cbase.data(), 8 * (ns + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_clen, clen.data(), 8 * ns, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_noff, name_off.data(), 4 * ns, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_nlen, name_len.data(), 4 * ns, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t cov_total = S.cov_total;
    if (!c->bed_params) c->bed_params.reset(new BedParams);
    BedParams &B = *c->bed_params;
    memset(&B, 0, sizeof(B));
    B.counts = static_cast<const uint16_t *>(S.cov.p);
    B.n_counts = cov_total;
    B.contig_base = d_cbase;
    B.contig_len = d_clen;
    B.name_off = d_noff;
    B.name_len = d_nlen;
    B.n_contigs = (uint32_t)ns;
    B.in = static_cast<const uint8_t *>(S.names.p);
    B.binary = opts->binary;
    B.exclude_unaligned = opts->exclude_unaligned;
    B.exclude_aligned = opts->exclude_aligned;
    B.min_size = opts->min_size;
    if (ns == 0 || cov_total == 0) {
        *info = c->plan;
        c->planned = true;
        return 0;
    }
    const uint64_t rtiles = (cov_total + (uint64_t)PAFFY_NT * BED_PER - 1) / ((uint64_t)PAFFY_NT * BED_PER);
    if (ensure(c, c->bed_len, sizeof(int64_t) * (size_t)(2 * rtiles + 2))) return PAFFY_E_HIP;
    int64_t *tile_cnt = static_cast<int64_t *>(c->bed_len.p), *tile_off = tile_cnt + rtiles;
    LAUNCH(c, "k_bed_runs", k_bed_runs, dim3((unsigned)rtiles), dim3(PAFFY_NT), 0, B, static_cast<const int64_t *>(nullptr), tile_cnt, static_cast<uint64_t *>(nullptr));
    int64_t n_runs = 0;
    if (scan64(c, tile_cnt, rtiles, tile_off, &n_runs)) return PAFFY_E_HIP;
    if (ensure(c, c->bed_starts, sizeof(uint64_t) * (size_t)(n_runs + 1))) return PAFFY_E_HIP;
    LAUNCH(c, "k_bed_runs", k_bed_runs, dim3((unsigned)rtiles), dim3(PAFFY_NT), 0, B, static_cast<const int64_t *>(tile_off), tile_cnt, static_cast<uint64_t *>(c->bed_starts.p));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* bed_len is reused below */
    if (ensure(c, c->bed_len, sizeof(int64_t) * (size_t)(n_runs + 1))) return PAFFY_E_HIP;
    if (ensure(c, c->bed_off, sizeof(int64_t) * (size_t)(n_runs + 1))) return PAFFY_E_HIP;
    const unsigned lgrid = (unsigned)(((uint64_t)n_runs + PAFFY_NT - 1) / PAFFY_NT);
    LAUNCH(c, "k_bed_lines", k_bed_lines, dim3(lgrid), dim3(PAFFY_NT), 0, B, static_cast<const uint64_t *>(c->bed_starts.p), (uint64_t)n_runs,
           static_cast<int64_t *>(c->bed_len.p), static_cast<const int64_t *>(nullptr), static_cast<uint8_t *>(nullptr));
    int64_t total = 0;
    if (scan64(c, static_cast<const int64_t *>(c->bed_len.p), (uint64_t)n_runs, static_cast<int64_t *>(c->bed_off.p), &total)) return PAFFY_E_HIP;
    if (c->profile) prof_collect(c);
    c->bed_runs = (uint64_t)n_runs;
    c->plan.out_bytes = total;
    c->plan.n_rows = 0; /* lines: counted by the caller if wanted */
    *info = c->plan;
    c->planned = true;
    return 0;
}
int paffy_hip_bed_plan(paffy_hip_ctx *c, const void *d_in, int64_t in_len, const paffy_bed_opts *opts, paffy_plan_info *info) {
    if (!c || !info || !opts) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15)) return PAFFY_E_ARG;
    int rc = paffy_hip_bed_begin(c, opts);
    if (!rc) rc = paffy_hip_bed_add(c, d_in, in_len);
    if (!rc) rc = paffy_hip_bed_run(c, opts, info);
    return rc;
}

int paffy_hip_flat_stats(paffy_hip_ctx *c, int64_t *left, int64_t reasons[16]) {
    if (!c || !left) return PAFFY_E_ARG;
    *left = c->flat_left;
    if (reasons)
        for (int k = 0; k < 16; k++) reasons[k] = c->flat_left >= 0 ? c->flat_reasons[k] : 0;
    return 0;
}

int paffy_hip_plan_stats(paffy_hip_ctx *c, int64_t sums[6]) {
    if (!c || !sums) return PAFFY_E_ARG;
    if (!c->planned || c->plan_kind == PLAN_LINES) return PAFFY_E_STATE;
    for (int k = 0; k < 6; k++) sums[k] = c->plan.in_bytes > 0 ? (int64_t)c->h_info->stats[k] : 0;
    return 0;
}

int64_t paffy_hip_plan_record_stats(paffy_hip_ctx *c, int64_t cap_records, int64_t *sums) {
    if (!c || !sums || cap_records < 0) return PAFFY_E_ARG;
    if (!c->planned || c->plan_kind != PLAN_RECORDS) return PAFFY_E_STATE;
    const int64_t n = c->plan.n_records;
    if (n == 0) return 0;
    if (!c->kp.rec_stats) return PAFFY_E_STATE; /* no PAFFY_STATS stage in the plan */
    if (cap_records < n) return PAFFY_E_CAPACITY;
    HIPCHK(c, hipMemcpy(sums, c->kp.rec_stats, sizeof(int64_t) * 6 * (size_t)n, hipMemcpyDeviceToHost));
    return n;
}

int paffy_hip_plan_record_layout(paffy_hip_ctx *c, int64_t first, int64_t count, uint32_t *flags, uint32_t *klass) {
    if (!c || (count > 0 && (!flags || !klass))) return PAFFY_E_ARG;
    if (stats_only_refuses(c, "paffy_hip_plan_record_layout")) return PAFFY_E_STATE;
    if (!c->planned || c->plan_kind != PLAN_RECORDS) return PAFFY_E_STATE;
    if (first < 0 || count < 0 || first + count > c->plan.n_records) return PAFFY_E_ARG;
    if (count == 0) return 0;
    std::vector<RecPlan> pl((size_t)count);
    HIPCHK(c, hipMemcpyAsync(pl.data(), static_cast<const RecPlan *>(c->rec_plan.p) + first, sizeof(RecPlan) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(klass, c->kp.status + first, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < count; i++) {
        flags[i] = pl[(size_t)i].flags;
        klass[i] >>= 16;
    }
    return 0;
}

/* ---- the counters of a to_bed run, for hosts that keep SequenceCountArray objects (inc/paf.h:214-233) ---- */
__global__ __launch_bounds__(PAFFY_NT) void k_counts_add_sat(uint16_t *acc, const uint16_t *add, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = (uint32_t)acc[i] + add[i]; /* one record at a time stops at INT16_MAX - 1 (impl/paf.c:701); so does the sum */
    acc[i] = acc[i] >= 32766 ? acc[i] : (uint16_t)(s < 32766u ? s : 32766u);
}
int paffy_hip_bed_failure_side(paffy_hip_ctx *c) {
    if (!c || !c->planned || c->plan_kind != PLAN_BED || !c->cov || !c->plan.error.code) return -1;
    return c->cov->fail_side;
}
int64_t paffy_hip_bed_sequence_keys(paffy_hip_ctx *c, int64_t cap_sequences, void *d_keys) {
    if (!c || cap_sequences < 0) return PAFFY_E_ARG;
    if (!c->planned || c->plan_kind != PLAN_BED || !c->cov || c->plan.error.code) return PAFFY_E_STATE;
    CovState &S = *c->cov;
    const size_t ns = S.appearance.size();
    if (S.n_rec == 0 || ns == 0) return 0;
    if (!d_keys) return PAFFY_E_ARG;
    if ((size_t)cap_sequences < ns) return PAFFY_E_CAPACITY;
    /* A run that wrote nothing (every line excluded) returned before the run finder: bed_starts / bed_len / bed_off are an earlier run's, but
       plan_begin has set bed_runs to 0, so k_bed_seq_keys reads none of them and gives every sequence 0 bytes (b0 = b1 = out_bytes = 0)
       and 0 lines. */
    std::vector<int64_t> first(ns);
    for (size_t k = 0; k < ns; k++) first[k] = S.sides == 2 ? (int64_t)S.h_first_entry[k] : 2 * (int64_t)S.h_first_entry[k]; /* 2 * record + side */
    if (ensure(c, c->bed_keys, sizeof(int64_t) * ns)) return PAFFY_E_HIP;
    HIPCHK(c, hipMemcpyAsync(c->bed_keys.p, first.data(), sizeof(int64_t) * ns, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* `first` is a local */
    LAUNCH(c, "k_bed_seq_keys", k_bed_seq_keys, dim3((unsigned)ns), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(c->bed_starts.p), c->bed_runs,
           static_cast<const int64_t *>(c->bed_len.p), static_cast<const int64_t *>(c->bed_off.p), c->plan.out_bytes, c->bed_params->contig_base, (uint32_t)ns,
           static_cast<const int64_t *>(c->bed_keys.p), static_cast<int64_t *>(d_keys));
    return (int64_t)ns;
}
int64_t paffy_hip_bed_sequences(paffy_hip_ctx *c) {
    if (!c) return PAFFY_E_ARG;
    if (!c->planned || c->plan_kind != PLAN_BED || !c->cov) return PAFFY_E_STATE;
    return (int64_t)c->cov->appearance.size();
}
int paffy_hip_bed_counts(paffy_hip_ctx *c, int64_t sequence, int64_t start, int64_t end, uint16_t *h_counts, int accumulate) {
    if (!c || !h_counts || sequence < 0 || start < 0 || end < start) return PAFFY_E_ARG;
    if (!c->planned || c->plan_kind != PLAN_BED || !c->cov) return PAFFY_E_STATE;
    CovState &S = *c->cov;
    if ((size_t)sequence >= S.appearance.size()) return PAFFY_E_ARG;
    const uint32_t ci = S.appearance[(size_t)sequence];
    if (end > S.h_contig_len[ci]) return PAFFY_E_ARG;
    const uint64_t n = (uint64_t)(end - start);
    if (n == 0) return 0;
    const uint16_t *src = static_cast<const uint16_t *>(S.cov.p) + S.h_contig_cov[ci] + start;
    if (!accumulate) {
        HIPCHK(c, hipMemcpyAsync(h_counts, src, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
    if (ensure(c, c->pretty_out, sizeof(uint16_t) * n + 64)) return PAFFY_E_HIP;
    uint16_t *acc = static_cast<uint16_t *>(c->pretty_out.p);
    HIPCHK(c, hipMemcpyAsync(acc, h_counts, sizeof(uint16_t) * n, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_counts_add_sat", k_counts_add_sat, dim3((unsigned)((n + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, acc, src, n);
    HIPCHK(c, hipMemcpyAsync(h_counts, acc, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

/* ---- paf_pretty_print's base-level rows (pretty_kernel.h) ---- */
int paffy_hip_stats_only(paffy_hip_ctx *c, int on) {
    if (!c) return PAFFY_E_ARG;
    c->stats_only = on != 0;
    return 0;
}

int paffy_hip_keep_raw_sequences(paffy_hip_ctx *c, int on) {
    if (!c) return PAFFY_E_ARG;
    c->keep_raw = on != 0;
    return 0;
}

static int pretty_params(paffy_hip_ctx *c, int64_t first, int64_t count, PrettyParams *pp) {
    if (stats_only_refuses(c, "alignment rows")) return PAFFY_E_STATE;
    if (!c->planned || c->plan_kind != PLAN_RECORDS) return PAFFY_E_STATE;
    if (first < 0 || count < 0 || first + count > c->plan.n_records) return PAFFY_E_ARG;
    if (c->n_seqs <= 0 || !c->seq_raw.p) {
        c->last_error = "alignment rows: no sequences loaded with paffy_hip_keep_raw_sequences on";
        return PAFFY_E_STATE;
    }
    const uint32_t n = c->kp.n_rec;
    if (!c->plan_seq_lookup && n > 0) { /* a plan without the mismatch encoder did not look the names up */
        if (ensure(c, c->rec_qseq, sizeof(int32_t) * (size_t)(n + 1))) return PAFFY_E_HIP;
        if (ensure(c, c->rec_tseq, sizeof(int32_t) * (size_t)(n + 1))) return PAFFY_E_HIP;
        LAUNCH(c, "k_seq_lookup", k_seq_lookup, dim3((n + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, c->kp.in, c->kp.meta, n,
               static_cast<const uint8_t *>(c->seq_names.p), static_cast<const uint32_t *>(c->seq_name_off.p), c->n_seqs,
               static_cast<int32_t *>(c->rec_qseq.p), static_cast<int32_t *>(c->rec_tseq.p));
        c->plan_seq_lookup = true;
    }
    memset(pp, 0, sizeof(*pp));
    pp->meta = c->kp.meta;
    pp->plan = static_cast<const RecPlan *>(c->rec_plan.p);
    pp->status = c->kp.status;
    pp->arena = c->kp.arena;
    pp->arena_off = c->kp.arena_off;
    pp->ops_mirror = c->kp.ops_mirror;
    pp->new_ops = c->kp.new_ops;
    pp->seq_raw = static_cast<const uint8_t *>(c->seq_raw.p);
    pp->seqs = static_cast<const SeqEntry *>(c->seq_table.p);
    pp->rec_qseq = static_cast<const int32_t *>(c->rec_qseq.p);
    pp->rec_tseq = static_cast<const int32_t *>(c->rec_tseq.p);
    pp->first = (uint32_t)first;
    return 0;
}

int paffy_hip_plan_alignment_sizes(paffy_hip_ctx *c, int64_t first, int64_t count, int64_t *h_bytes) {
    if (!c || (count > 0 && !h_bytes)) return PAFFY_E_ARG;
    PrettyParams pp;
    int rc = pretty_params(c, first, count, &pp);
    if (rc || count == 0) return rc;
    if (ensure(c, c->pretty_off, sizeof(int64_t) * (size_t)(count + 1))) return PAFFY_E_HIP;
    LAUNCH(c, "k_pretty_size", k_pretty_size, dim3((unsigned)count), dim3(PRETTY_NT), 0, pp, static_cast<int64_t *>(c->pretty_off.p));
    HIPCHK(c, hipMemcpyAsync(h_bytes, c->pretty_off.p, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int paffy_hip_plan_alignment_rows(paffy_hip_ctx *c, int64_t first, int64_t count, const int64_t *h_off, char *h_out, paffy_error *err) {
    if (!c || !err || (count > 0 && (!h_off || !h_out))) return PAFFY_E_ARG;
    memset(err, 0, sizeof(*err));
    PrettyParams pp;
    int rc = pretty_params(c, first, count, &pp);
    if (rc || count == 0) return rc;
    const int64_t total = h_off[count] - h_off[0];
    if (total < 0) return PAFFY_E_ARG;
    if (ensure(c, c->pretty_off, sizeof(int64_t) * (size_t)(count + 1))) return PAFFY_E_HIP;
    if (ensure(c, c->pretty_out, (size_t)total + 64)) return PAFFY_E_HIP;
    if (ensure(c, c->pretty_err, sizeof(unsigned long long))) return PAFFY_E_HIP;
    std::vector<int64_t> off((size_t)count + 1);
    for (int64_t i = 0; i <= count; i++) off[(size_t)i] = h_off[i] - h_off[0];
    HIPCHK(c, hipMemcpyAsync(c->pretty_off.p, off.data(), sizeof(int64_t) * (size_t)(count + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->pretty_err.p, 0xff, sizeof(unsigned long long), c->stream));
    pp.row_off = static_cast<const int64_t *>(c->pretty_off.p);
    pp.out = static_cast<uint8_t *>(c->pretty_out.p);
    pp.err = static_cast<unsigned long long *>(c->pretty_err.p);
    LAUNCH(c, "k_pretty_rows", k_pretty_rows, dim3((unsigned)count), dim3(PRETTY_NT), 0, pp);
    unsigned long long e = 0;
    HIPCHK(c, hipMemcpyAsync(&e, c->pretty_err.p, sizeof(e), hipMemcpyDeviceToHost, c->stream));
    if (total > 0) HIPCHK(c, hipMemcpyAsync(h_out, c->pretty_out.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (e != ~0ull) {
        err->code = (int32_t)(e & 0xff);
        err->record = (int64_t)(e >> 8);
        err->stage = -1;
    }
    return 0;
}

/* ---- paf_pretty_print's text in device memory: the stats line (view_line_kernel.h), with the rows behind it on demand ---- */
static int view_params(paffy_hip_ctx *c, const char *what, int64_t first, int64_t count, int with_rows, ViewLineParams *vp, PrettyParams *pp) {
    if (!c->planned || c->plan_kind != PLAN_RECORDS) {
        c->last_error = std::string(what) + ": the last plan is not a record plan (paffy_hip_plan)";
        return PAFFY_E_STATE;
    }
    if (first < 0 || count < 0 || first + count > c->plan.n_records) return PAFFY_E_ARG;
    if (c->plan.n_records > 0 && !c->kp.rec_stats) {
        c->last_error = std::string(what) + ": the plan has no PAFFY_STATS stage";
        return PAFFY_E_STATE;
    }
    if (c->plan.error.code) {
        c->last_error = std::string(what) + ": the plan reported a failing record";
        return PAFFY_E_STATE;
    }
    if (with_rows) { /* as for paffy_hip_plan_alignment_*: raw sequences, and a plan that kept its ops */
        int rc = pretty_params(c, first, count, pp);
        if (rc) return rc;
    }
    memset(vp, 0, sizeof(*vp));
    vp->in = c->kp.in;
    vp->meta = c->kp.meta;
    vp->rec_stats = c->kp.rec_stats;
    vp->first = (uint32_t)first;
    vp->count = (uint32_t)count;
    return 0;
}

/* view_work: count sizes (the rows' bytes, then the blocks'), count + 1 row offsets, the verdict on the offsets */
static int view_work(paffy_hip_ctx *c, int64_t count, int64_t **bytes, int64_t **rows_off, uint32_t **bad) {
    if (ensure(c, c->view_work, sizeof(int64_t) * (size_t)(2 * count + 2))) return PAFFY_E_HIP;
    *bytes = static_cast<int64_t *>(c->view_work.p);
    *rows_off = *bytes + count;
    *bad = reinterpret_cast<uint32_t *>(*rows_off + count + 1);
    return 0;
}

int paffy_hip_plan_view_sizes(paffy_hip_ctx *c, int64_t first, int64_t count, int with_rows, int64_t *h_bytes) {
    if (!c || (count > 0 && !h_bytes)) return PAFFY_E_ARG;
    ViewLineParams vp;
    PrettyParams pp;
    int rc = view_params(c, "paffy_hip_plan_view_sizes", first, count, with_rows, &vp, &pp);
    if (rc || count == 0) return rc;
    int64_t *bytes, *rows_off;
    uint32_t *bad;
    if (view_work(c, count, &bytes, &rows_off, &bad)) return PAFFY_E_HIP;
    if (with_rows) LAUNCH(c, "k_pretty_size", k_pretty_size, dim3((unsigned)count), dim3(PRETTY_NT), 0, pp, bytes);
    LAUNCH(c, "k_view_line_size", k_view_line_size, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, vp, bytes, with_rows ? 1 : 0);
    HIPCHK(c, hipMemcpyAsync(h_bytes, bytes, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int paffy_hip_plan_view_text(paffy_hip_ctx *c, int64_t first, int64_t count, int with_rows, const int64_t *h_off, void *d_out, int64_t out_cap,
                             paffy_error *err) {
    if (!c || !err || out_cap < 0 || (count > 0 && !h_off)) return PAFFY_E_ARG;
    memset(err, 0, sizeof(*err));
    ViewLineParams vp;
    PrettyParams pp;
    int rc = view_params(c, "paffy_hip_plan_view_text", first, count, with_rows, &vp, &pp);
    if (rc || count == 0) return rc;
    const int64_t total = h_off[count] - h_off[0];
    if (total < 0 || total > out_cap || !d_out) return PAFFY_E_ARG;
    int64_t *bytes, *rows_off;
    uint32_t *bad;
    if (view_work(c, count, &bytes, &rows_off, &bad)) return PAFFY_E_HIP;
    if (ensure(c, c->pretty_off, sizeof(int64_t) * (size_t)(count + 1))) return PAFFY_E_HIP;
    if (ensure(c, c->pretty_err, sizeof(unsigned long long))) return PAFFY_E_HIP;
    std::vector<int64_t> off((size_t)count + 1);
    for (int64_t i = 0; i <= count; i++) off[(size_t)i] = h_off[i] - h_off[0];
    HIPCHK(c, hipMemcpyAsync(c->pretty_off.p, off.data(), sizeof(int64_t) * (size_t)(count + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(bad, 0, sizeof(uint32_t), c->stream));
    if (with_rows) LAUNCH(c, "k_pretty_size", k_pretty_size, dim3((unsigned)count), dim3(PRETTY_NT), 0, pp, bytes);
    vp.off = static_cast<const int64_t *>(c->pretty_off.p);
    vp.rows_bytes = with_rows ? bytes : nullptr;
    vp.rows_off = with_rows ? rows_off : nullptr;
    vp.out = static_cast<uint8_t *>(d_out);
    vp.out_cap = total;
    vp.bad = bad;
    LAUNCH(c, "k_view_line_emit", k_view_line_emit, dim3((unsigned)((count + VIEW_LINE_WAVES - 1) / VIEW_LINE_WAVES)), dim3(64 * VIEW_LINE_WAVES), 0, vp);
    uint32_t h_bad = 0;
    HIPCHK(c, hipMemcpyAsync(&h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); /* `off` is a local; the rows are written only where the lines' offsets held */
    if (h_bad) {
        c->last_error = "paffy_hip_plan_view_text: the offsets are not the running sums of paffy_hip_plan_view_sizes";
        return PAFFY_E_ARG;
    }
    if (!with_rows) return 0;
    HIPCHK(c, hipMemsetAsync(c->pretty_err.p, 0xff, sizeof(unsigned long long), c->stream));
    pp.row_off = rows_off;
    pp.out = static_cast<uint8_t *>(d_out);
    pp.err = static_cast<unsigned long long *>(c->pretty_err.p);
    LAUNCH(c, "k_pretty_rows", k_pretty_rows, dim3((unsigned)count), dim3(PRETTY_NT), 0, pp);
    unsigned long long e = 0;
    HIPCHK(c, hipMemcpyAsync(&e, c->pretty_err.p, sizeof(e), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (e != ~0ull) {
        err->code = (int32_t)(e & 0xff);
        err->record = (int64_t)(e >> 8);
        err->stage = -1;
    }
    return 0;
}

/*
 * ---- the layout of a planned batch's view text, kept on the device ----
 * view_layout: size[n + 1] (the blocks' bytes and a closing 0, so that the scan leaves the total in off[n]), off[n + 1], rows_bytes[n + 1],
 * rows_off[n + 1], then verdict[3], the rows' failure, *bad and the number of ranges.
 */
struct ViewLayout {
    int64_t *size, *off, *rows_bytes, *rows_off, *verdict;
    unsigned long long *err;
    uint32_t *bad, *n_ranges;
};
static ViewLayout view_layout_of(paffy_hip_ctx *c, int64_t n) {
    ViewLayout L;
    int64_t *p = static_cast<int64_t *>(c->view_layout.p);
    L.size = p;
    L.off = p + (n + 1);
    L.rows_bytes = p + 2 * (n + 1);
    L.rows_off = p + 3 * (n + 1);
    L.verdict = p + 4 * (n + 1);
    L.err = reinterpret_cast<unsigned long long *>(L.verdict + 3);
    L.bad = reinterpret_cast<uint32_t *>(L.verdict + 4);
    L.n_ranges = L.bad + 1;
    return L;
}

int paffy_hip_plan_view_layout(paffy_hip_ctx *c, int with_rows, int64_t range_bytes, int64_t *total_bytes, int64_t *n_ranges) {
    if (!c || !total_bytes || !n_ranges || range_bytes < 1) return PAFFY_E_ARG;
    *total_bytes = 0;
    *n_ranges = 0;
    c->view_laid = false;
    if (range_bytes > (1ll << 61)) range_bytes = 1ll << 61;
    ViewLineParams vp;
    PrettyParams pp;
    const int64_t n = c->planned ? c->plan.n_records : 0;
    int rc = view_params(c, "paffy_hip_plan_view_layout", 0, n, with_rows, &vp, &pp);
    if (rc) return rc;
    c->view_laid_rows = with_rows != 0;
    c->view_tab.assign(2, 0);
    if (n == 0) {
        c->view_laid = true;
        return 0;
    }
    if (ensure(c, c->view_layout, sizeof(int64_t) * (size_t)(4 * (n + 1) + 8))) return PAFFY_E_HIP;
    const ViewLayout L = view_layout_of(c, n);
    HIPCHK(c, hipMemsetAsync(L.size + n, 0, sizeof(int64_t), c->stream));
    if (with_rows) {
        LAUNCH(c, "k_pretty_size", k_pretty_size, dim3((unsigned)n), dim3(PRETTY_NT), 0, pp, L.rows_bytes);
        HIPCHK(c, hipMemcpyAsync(L.size, L.rows_bytes, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    }
    LAUNCH(c, "k_view_line_size", k_view_line_size, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, vp, L.size, with_rows ? 1 : 0);
    int64_t total = 0;
    rc = scan64(c, L.size, (uint64_t)n + 1, L.off, &total); /* the total comes to the host; off[n] holds it on the device */
    if (rc) return rc;
    if (total <= range_bytes) { /* one range: nothing to cut */
        c->view_tab.assign({0, 0, n, total});
    } else {
        /* two ranges in a row hold more than range_bytes, or they would be one */
        int64_t cap = 2 * (total / range_bytes) + 3;
        if (cap > n) cap = n;
        if (ensure(c, c->view_ranges_dev, sizeof(ViewRange) * (size_t)(cap + 1))) return PAFFY_E_HIP;
        ViewRange *tab = static_cast<ViewRange *>(c->view_ranges_dev.p);
        LAUNCH(c, "k_view_range_cut", k_view_range_cut, dim3(1), dim3(64), 0, static_cast<const int64_t *>(L.off), (uint32_t)n, range_bytes, tab, (uint32_t)cap, L.n_ranges);
        uint32_t nr = 0;
        HIPCHK(c, hipMemcpyAsync(&nr, L.n_ranges, sizeof(nr), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nr == 0 || (int64_t)nr > cap) {
            c->last_error = "paffy_hip_plan_view_layout: more ranges than the sizes allow";
            return PAFFY_E_STATE;
        }
        static_assert(sizeof(ViewRange) == 2 * sizeof(int64_t), "the range table is pairs of int64");
        c->view_tab.assign(2 * ((size_t)nr + 1), 0);
        HIPCHK(c, hipMemcpyAsync(c->view_tab.data(), tab, sizeof(ViewRange) * ((size_t)nr + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->view_tab[2 * (size_t)nr] != n || c->view_tab[2 * (size_t)nr + 1] != total) {
            c->last_error = "paffy_hip_plan_view_layout: the ranges do not end with the batch";
            return PAFFY_E_STATE;
        }
    }
    c->view_laid = true;
    *total_bytes = total;
    *n_ranges = (int64_t)(c->view_tab.size() / 2) - 1;
    return 0;
}

int64_t paffy_hip_plan_view_ranges(paffy_hip_ctx *c, int64_t cap_ranges, int64_t *first_record, int64_t *first_byte) {
    if (!c || cap_ranges < 0 || !first_record || !first_byte) return PAFFY_E_ARG;
    if (!c->planned || !c->view_laid) return PAFFY_E_STATE;
    const int64_t nr = (int64_t)(c->view_tab.size() / 2) - 1;
    if (cap_ranges < nr + 1) return PAFFY_E_CAPACITY;
    for (int64_t r = 0; r <= nr; r++) {
        first_record[r] = c->view_tab[2 * (size_t)r];
        first_byte[r] = c->view_tab[2 * (size_t)r + 1];
    }
    return nr;
}

/* range `range` of the layout into d_out, enqueued: *bytes = the range's bytes; h_verdict[3] (k_view_range_verdict) is written when the
   context's stream gets there */
static int view_emit_range(paffy_hip_ctx *c, int64_t range, void *d_out, int64_t out_cap, int64_t *bytes, int64_t *h_verdict) {
    if (!c->planned || !c->view_laid) {
        c->last_error = "paffy_hip_plan_view_emit_range: no paffy_hip_plan_view_layout of the current plan";
        return PAFFY_E_STATE;
    }
    const int64_t nr = (int64_t)(c->view_tab.size() / 2) - 1;
    if (range < 0 || range >= nr) return PAFFY_E_ARG;
    const int64_t first = c->view_tab[2 * (size_t)range], count = c->view_tab[2 * (size_t)range + 2] - first;
    const int64_t base = c->view_tab[2 * (size_t)range + 1], len = c->view_tab[2 * (size_t)range + 3] - base;
    if (!d_out) return PAFFY_E_ARG;
    if (len > out_cap) return PAFFY_E_CAPACITY;
    const bool with_rows = c->view_laid_rows;
    ViewLineParams vp;
    PrettyParams pp;
    int rc = view_params(c, "paffy_hip_plan_view_emit_range", first, count, with_rows, &vp, &pp);
    if (rc) return rc;
    const ViewLayout L = view_layout_of(c, c->plan.n_records);
    HIPCHK(c, hipMemsetAsync(L.bad, 0, sizeof(uint32_t), c->stream));
    vp.off = L.off + first;
    vp.off_base = base;
    vp.rows_bytes = with_rows ? L.rows_bytes + first : nullptr;
    vp.rows_off = with_rows ? L.rows_off + first : nullptr;
    vp.out = static_cast<uint8_t *>(d_out);
    vp.out_cap = len;
    vp.bad = L.bad;
    LAUNCH(c, "k_view_line_emit", k_view_line_emit, dim3((unsigned)((count + VIEW_LINE_WAVES - 1) / VIEW_LINE_WAVES)), dim3(64 * VIEW_LINE_WAVES), 0, vp);
    if (with_rows) { /* the offsets are the layout's own: the rows go where the lines left them room */
        HIPCHK(c, hipMemsetAsync(L.err, 0xff, sizeof(unsigned long long), c->stream));
        pp.row_off = L.rows_off + first;
        pp.out = static_cast<uint8_t *>(d_out);
        pp.err = L.err;
        LAUNCH(c, "k_pretty_rows", k_pretty_rows, dim3((unsigned)count), dim3(PRETTY_NT), 0, pp);
    }
    LAUNCH(c, "k_view_range_verdict", k_view_range_verdict, dim3(1), dim3(64), 0, with_rows ? L.err : nullptr, static_cast<const uint32_t *>(L.bad),
           static_cast<const int64_t *>(L.off), static_cast<const int64_t *>(L.size), static_cast<const int64_t *>(L.rows_bytes), base, L.verdict);
    HIPCHK(c, hipMemcpyAsync(h_verdict, L.verdict, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    *bytes = len;
    return 0;
}

/* what a verdict says: PAFFY_E_STATE for refused offsets; a rows failure in *err with *bytes = what the reference had printed of the range */
static int view_verdict(paffy_hip_ctx *c, const int64_t *h_verdict, int64_t *bytes, paffy_error *err) {
    memset(err, 0, sizeof(*err));
    if (h_verdict[2]) {
        c->last_error = "paffy_hip_plan_view_emit_range: a record's offsets are not the running sums of its size";
        return PAFFY_E_STATE;
    }
    if (h_verdict[0] != -1) {
        const unsigned long long e = (unsigned long long)h_verdict[0];
        err->code = (int32_t)(e & 0xff);
        err->record = (int64_t)(e >> 8);
        err->stage = -1;
        *bytes = h_verdict[1];
    }
    return 0;
}

int paffy_hip_plan_view_emit_range(paffy_hip_ctx *c, int64_t range, void *d_out, int64_t out_cap, int64_t *bytes, paffy_error *err) {
    if (!c || !bytes || !err) return PAFFY_E_ARG;
    memset(err, 0, sizeof(*err));
    *bytes = 0;
    int64_t verdict[3] = {-1, -1, 0};
    int rc = view_emit_range(c, range, d_out, out_cap, bytes, verdict);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return view_verdict(c, verdict, bytes, err);
}

/*
 * ---- a stream in view mode: the chunks go through [PAFFY_ADD_MISMATCHES, PAFFY_STATS], what comes back is the view text ----
 * A chunk of one range (the common case) pipelines like any other chunk. A chunk of more ranges is "open": its later ranges are written into
 * the slot's output buffer by paffy_hip_stream_read, each once the pieces of the range before it have arrived, and the plan they are written
 * from must stay -- paffy_hip_stream_input answers NULL until the chunk is read out.
 */
int paffy_hip_stream_open_view(paffy_hip_ctx *c, int text, int64_t chunk_bytes, int64_t piece_bytes, int64_t range_bytes, paffy_hip_stream **out) {
    if (!c || !out || text < 0 || text > 2 || range_bytes < 1) return PAFFY_E_ARG;
    const paffy_stage st[2] = {{PAFFY_ADD_MISMATCHES, 0.05f, 1.0f}, {PAFFY_STATS, 0.0f, 0.0f}};
    paffy_hip_stream *s = nullptr;
    int rc = paffy_hip_stream_open(c, st, 2, chunk_bytes, piece_bytes, &s);
    if (rc) return rc;
    s->view_text = text;
    s->view_range_bytes = range_bytes;
    for (int k = 0; k < 2; k++)
        if (hipHostMalloc(reinterpret_cast<void **>(&s->slot[k].h_verdict), 4 * sizeof(int64_t)) != hipSuccess) {
            c->last_error = "paffy_hip_stream_open_view: pinned buffers";
            paffy_hip_stream_close(s);
            return PAFFY_E_HIP;
        }
    *out = s;
    return 0;
}

int paffy_hip_stream_view_status(paffy_hip_stream *s, int64_t sums[6], int64_t *n_records, paffy_error *rows_err) {
    if (!s || !sums || !n_records || !rows_err) return PAFFY_E_ARG;
    if (s->view_text < 0) return PAFFY_E_STATE;
    for (int k = 0; k < 6; k++) sums[k] = s->view_sums[k];
    *n_records = s->view_records;
    *rows_err = s->view_rows_err;
    return 0;
}

static int view_stream_submit(paffy_hip_stream *s, int64_t in_len, paffy_plan_info *info) {
    paffy_hip_ctx *c = s->c;
    if (!c) return PAFFY_E_STATE;
    StreamSlot &sl = s->slot[s->fill];
    if (s->view_failed) {
        c->last_error = "paffy_hip_stream_submit: the rows of an earlier chunk failed (paffy_hip_stream_view_status)";
        return PAFFY_E_STATE;
    }
    if (sl.busy || s->view_open || in_len > (int64_t)sl.h_cap) return PAFFY_E_STATE;
    int rc = stream_stage_in(s, sl, in_len);
    if (!rc) rc = paffy_hip_plan(c, s->stages, s->n_stages, sl.d_in.p, in_len, info);
    if (rc) return rc;
    sl.out_len = sl.read_at = 0;
    sl.view_ranges = sl.view_range_at = 0;
    sl.verdict_seen = sl.view_open = false;
    info->out_bytes = 0;
    info->n_rows = 0;
    if (info->error.code == 0) {
        int64_t sums[6];
        rc = paffy_hip_plan_stats(c, sums);
        if (rc) return rc;
        for (int k = 0; k < 6; k++) s->view_sums[k] += sums[k];
        s->view_records += info->n_records;
        if (s->view_text > 0 && info->n_records > 0) {
            int64_t total = 0, nr = 0, longest = 0;
            rc = paffy_hip_plan_view_layout(c, s->view_text == 2, s->view_range_bytes, &total, &nr);
            if (rc) return rc;
            for (int64_t r = 0; r < nr; r++) longest = std::max(longest, c->view_tab[2 * (size_t)r + 3] - c->view_tab[2 * (size_t)r + 1]);
            rc = stream_out_room(c, sl, longest, nr == 1);
            if (!rc) rc = view_emit_range(c, 0, sl.d_out.p, (int64_t)sl.d_out.cap, &sl.out_len, sl.h_verdict);
            if (rc) return rc;
            sl.view_ranges = nr;
            info->out_bytes = total;
            info->n_rows = info->n_records;
            sl.view_open = s->view_open = nr > 1;
        }
    } else if (s->view_text > 0) {
        /* a chunk with a failing record writes nothing. What is reported is the first line that does not parse, if there is one, before
           the first record the stages fail on -- the order the reference reads and works in: a plan of the parse alone tells */
        const paffy_stage pass = {PAFFY_PASS, 0.0f, 0.0f};
        paffy_plan_info parsed;
        if (paffy_hip_plan(c, &pass, 1, sl.d_in.p, in_len, &parsed) == 0 && parsed.error.code) {
            *info = parsed;
            info->out_bytes = 0;
            info->n_rows = 0;
        }
    }
    return stream_submitted(s, sl);
}

static int view_stream_read(paffy_hip_stream *s, const char **piece, int64_t *len) {
    paffy_hip_ctx *c = s->c;
    *piece = nullptr;
    *len = 0;
    if (!c) return PAFFY_E_STATE;
    StreamSlot &sl = s->slot[s->drain];
    if (!sl.busy) return 0;
    for (;;) {
        if (sl.view_ranges > 0 && !sl.verdict_seen) { /* the range in d_out is written: what its writers found */
            HIPCHK(c, hipStreamWaitEvent(s->s_d2h, sl.ev_emit, 0));
            HIPCHK(c, hipEventSynchronize(sl.ev_emit));
            sl.verdict_seen = true;
            paffy_error e;
            int rc = view_verdict(c, sl.h_verdict, &sl.out_len, &e);
            if (rc) return rc;
            if (e.code) { /* the text ends with the failing record's stats line; no later range is written */
                s->view_rows_err = e;
                s->view_failed = true;
                sl.view_ranges = sl.view_range_at + 1;
            }
        }
        int rc = stream_issue_pieces(s, sl);
        if (rc) return rc;
        if (s->n_returned < s->n_issued) break;
        /* every piece of the range has arrived: the next range may take its place in d_out */
        if (sl.view_range_at + 1 < sl.view_ranges) {
            sl.view_range_at++;
            s->issued_at = 0;
            sl.verdict_seen = false;
            rc = view_emit_range(c, sl.view_range_at, sl.d_out.p, (int64_t)sl.d_out.cap, &sl.out_len, sl.h_verdict);
            if (rc) return rc;
            HIPCHK(c, hipEventRecord(sl.ev_emit, c->stream));
            continue;
        }
        if (sl.view_open) sl.view_open = s->view_open = false; /* the chunk has been read out */
        stream_chunk_done(s, sl);
        return 0;
    }
    return stream_hand_out(s, piece, len);
}

int paffy_hip_parse_host(paffy_hip_ctx *c, const char *h_in, int64_t in_len, paffy_record **recs, uint64_t **ops, int64_t *n_ops_total,
                         paffy_plan_info *info) {
    if (!c || !recs || !ops || !n_ops_total || !info || in_len < 0 || (in_len > 0 && !h_in)) return PAFFY_E_ARG;
    *recs = nullptr;
    *ops = nullptr;
    *n_ops_total = 0;
    void *d_in = nullptr;
    int rc = 0;
    if (in_len > 0) { /* the context's own input buffer, like paffy_hip_run_host */
        if (ensure(c, c->host_in, (size_t)in_len + 64)) return PAFFY_E_HIP;
        d_in = c->host_in.p;
        if (hipMemcpy(d_in, h_in, (size_t)in_len, hipMemcpyHostToDevice) != hipSuccess) rc = PAFFY_E_HIP;
    }
    const paffy_stage pass = {PAFFY_PASS, 0.0f, 0.0f};
    if (!rc) rc = paffy_hip_plan(c, &pass, 1, d_in, in_len, info); /* index, header parse, cigar parse: the ops are in the mirror / arena */
    const size_t n = (size_t)info->n_records;
    if (!rc && info->error.code == 0 && n > 0) {
        std::vector<RecMeta> meta(n);
        std::vector<RecPlan> plan(n);
        std::vector<uint32_t> status(n), mirror((size_t)in_len / 2 + 64);
        std::vector<uint64_t> arena_off(n), arena((size_t)c->h_info->arena_used);
        if (hipMemcpy(meta.data(), c->meta.p, sizeof(RecMeta) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(plan.data(), c->rec_plan.p, sizeof(RecPlan) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(status.data(), c->status.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(arena_off.data(), c->arena_off.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(mirror.data(), c->ops_mirror.p, sizeof(uint32_t) * mirror.size(), hipMemcpyDeviceToHost) != hipSuccess ||
            (!arena.empty() && hipMemcpy(arena.data(), c->arena.p, sizeof(uint64_t) * arena.size(), hipMemcpyDeviceToHost) != hipSuccess)) {
            c->last_error = "paffy_hip_parse_host: copy back failed";
            rc = PAFFY_E_HIP;
        } else {
            int64_t total = 0;
            for (size_t r = 0; r < n; r++)
                if (plan[r].flags & 8u) total += plan[r].n;
            paffy_record *out = static_cast<paffy_record *>(calloc(n, sizeof(paffy_record)));
            uint64_t *oo = static_cast<uint64_t *>(malloc(sizeof(uint64_t) * (size_t)(total > 0 ? total : 1)));
            int64_t at = 0;
            for (size_t r = 0; r < n; r++) {
                const RecMeta &m = meta[r];
                paffy_record &o = out[r];
                o.query_length = m.qlen; o.query_start = m.qs; o.query_end = m.qe;
                o.target_length = m.tlen; o.target_start = m.ts; o.target_end = m.te;
                o.score = m.score; o.mapping_quality = m.mapq; o.num_matches = m.nmatch; o.num_bases = m.nbases;
                o.tile_level = m.tile_level; o.chain_id = m.chain_id; o.chain_score = m.chain_score;
                o.query_name_off = m.qname_off; o.query_name_len = m.qname_len; o.target_name_off = m.tname_off; o.target_name_len = m.tname_len;
                o.cigar_off = m.has_cg ? m.cg_off : 0; o.cigar_len = m.has_cg ? m.cg_len : 0;
                o.same_strand = m.same_strand; o.type = m.type;
                o.ops_first = at;
                o.n_ops = -1;
                if (plan[r].flags & 8u) { /* has a cigar: the ops as parsed (a pass stage leaves the view on the whole array) */
                    o.n_ops = plan[r].n;
                    if ((status[r] >> 16) == KLASS_ARENA) {
                        const uint64_t *src = arena.data() + arena_off[r];
                        for (uint32_t i = 0; i < plan[r].n; i++) oo[at++] = (((uint64_t)((int64_t)src[i] >> 8)) & 0x00ffffffffffffffull) | ((src[i] & 0xffull) << 56);
                    } else {
                        const uint32_t *src = mirror.data() + (m.cg_off >> 1);
                        const uint16_t *src16 = reinterpret_cast<const uint16_t *>(src);
                        const bool half = (plan[r].flags & 0x60000u) == 0x40000u; /* 2-byte words (every length below 8192): emit_ops_half() */
                        for (uint32_t i = 0; i < plan[r].n; i++) {
                            const uint32_t w = half ? (uint32_t)src16[i] : src[i];
                            oo[at++] = (uint64_t)(w >> 3) | ((uint64_t)(w & 7u) << 56);
                        }
                    }
                }
            }
            *recs = out;
            *ops = oo;
            *n_ops_total = at;
        }
    }
    c->planned = false; /* the input buffer will be overwritten by the next call */
    return rc;
}

/* Lays the sequence store out for n named sequences (sorted by name for the lookup kernel) and uploads the name tables;
 * blob_off[i] = where sequence i starts in seq_blob. The bases are written by the caller. fixed_off: sequence i starts at fixed_off[i]
 * of a seq_blob the caller provides (nothing is allocated for it); nullptr: back to back in name order in a seq_blob allocated here. */
static int seq_store_layout(paffy_hip_ctx *c, int64_t n, const char *const *names, const int64_t *lens, std::vector<uint64_t> &blob_off,
                            const int64_t *fixed_off = nullptr) {
    c->n_seqs = 0;
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
    std::vector<size_t> nlen((size_t)n);
    for (int64_t i = 0; i < n; i++) nlen[(size_t)i] = strlen(names[i]);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        size_t m = nlen[(size_t)a] < nlen[(size_t)b] ? nlen[(size_t)a] : nlen[(size_t)b];
        int d = memcmp(names[a], names[b], m);
        if (d) return d < 0;
        return nlen[(size_t)a] < nlen[(size_t)b];
    });
    std::vector<uint32_t> name_off((size_t)n + 1);
    std::string blob;
    std::vector<SeqEntry> table((size_t)n);
    blob_off.assign((size_t)n, 0);
    uint64_t total = 0;
    for (int64_t k = 0; k < n; k++) {
        int64_t i = order[(size_t)k];
        name_off[(size_t)k] = (uint32_t)blob.size();
        blob.append(names[i], nlen[(size_t)i]);
        const uint64_t at = fixed_off ? (uint64_t)fixed_off[i] : total;
        table[(size_t)k].off = at;
        table[(size_t)k].len = lens[i];
        blob_off[(size_t)i] = at;
        total += (uint64_t)lens[i];
    }
    name_off[(size_t)n] = (uint32_t)blob.size();
    if (blob.size() >= 0xffffffffull) { /* name_off is 32-bit */
        c->last_error = "sequence store: the names pass 4 GiB";
        return PAFFY_E_ARG;
    }
    if (!fixed_off && ensure(c, c->seq_blob, total + 64)) return PAFFY_E_HIP;
    if (ensure(c, c->seq_table, sizeof(SeqEntry) * (size_t)n)) return PAFFY_E_HIP;
    if (ensure(c, c->seq_names, blob.size() + 16)) return PAFFY_E_HIP;
    if (ensure(c, c->seq_name_off, sizeof(uint32_t) * ((size_t)n + 1))) return PAFFY_E_HIP;
    HIPCHK(c, hipMemcpy(c->seq_table.p, table.data(), sizeof(SeqEntry) * (size_t)n, hipMemcpyHostToDevice));
    if (!blob.empty()) HIPCHK(c, hipMemcpy(c->seq_names.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->seq_name_off.p, name_off.data(), sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
    return 0;
}

/* After the bases are in seq_blob: upper-case them and build the complemented copy. */
static int seq_store_canon(paffy_hip_ctx *c) {
    const size_t bytes = c->seq_blob.cap & ~(size_t)15; /* the whole allocation, whole 16-byte words */
    if (c->keep_raw) {
        if (ensure(c, c->seq_raw, c->seq_blob.cap)) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(c->seq_raw.p, c->seq_blob.p, c->seq_blob.cap, hipMemcpyDeviceToDevice, c->stream));
    }
    if (ensure(c, c->seq_comp, c->seq_blob.cap)) return PAFFY_E_HIP;
    const uint64_t n16 = bytes / 16;
    if (n16) {
        LAUNCH(c, "k_seq_canon", k_seq_canon, dim3((unsigned)((n16 + PAFFY_NT - 1) / PAFFY_NT)), dim3(PAFFY_NT), 0, static_cast<uint8_t *>(c->seq_blob.p),
               static_cast<uint8_t *>(c->seq_comp.p), n16);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

int paffy_hip_set_sequences(paffy_hip_ctx *c, int64_t n, const char *const *names, const char *const *seqs, const int64_t *lens) {
    if (!c || n < 0 || (n > 0 && (!names || !seqs || !lens))) return PAFFY_E_ARG;
    c->n_seqs = 0;
    if (n == 0) return 0;
    std::vector<uint64_t> blob_off;
    int rc = seq_store_layout(c, n, names, lens, blob_off);
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++)
        if (lens[i] > 0)
            HIPCHK(c, hipMemcpy(static_cast<uint8_t *>(c->seq_blob.p) + blob_off[(size_t)i], seqs[i], (size_t)lens[i], hipMemcpyHostToDevice));
    if (seq_store_canon(c)) return PAFFY_E_HIP;
    c->n_seqs = (int32_t)n;
    return 0;
}

int paffy_hip_set_filter(paffy_hip_ctx *c, const paffy_filter *f) {
    if (!c) return PAFFY_E_ARG;
    const paffy_filter d = {-1, -1, -1.0, -1.0, -1, 0};
    c->filter = f ? *f : d;
    return 0;
}

int paffy_hip_error_exit_status(int32_t code) {
    switch (code) {
        case PAFFY_OK: return 0;
        case PAFFY_ERR_STRAND: case PAFFY_ERR_CIGAR_CHAR:
        case PAFFY_ERR_CHECK_QSTART: case PAFFY_ERR_CHECK_QEND: case PAFFY_ERR_CHECK_TSTART: case PAFFY_ERR_CHECK_TEND:
        case PAFFY_ERR_CHECK_CIGAR_Q: case PAFFY_ERR_CHECK_CIGAR_T:
        case PAFFY_ERR_MISSING_QUERY_SEQ: case PAFFY_ERR_MISSING_TARGET_SEQ: case PAFFY_ERR_FAFFY_MISSING_SEQ:
            return 1; /* st_errAbort / exit(1) */
        case PAFFY_ERR_FEW_FIELDS: case PAFFY_ERR_NULL_CIGAR: case PAFFY_ERR_SEQ_RANGE:
            return 139; /* the reference dereferences NULL / reads out of bounds */
        default:
            return 134; /* assert -> abort() */
    }
}

const char *paffy_hip_error_string(int32_t code) {
    switch (code) {
        case PAFFY_OK: return "ok";
        case PAFFY_ERR_FEW_FIELDS: return "Paf line has fewer than 12 fields";
        case PAFFY_ERR_STRAND: return "Got an unexpected strand character in a paf string";
        case PAFFY_ERR_TP_ASSERT: return "tp tag is not P, S or I";
        case PAFFY_ERR_CIGAR_CHAR: return "Got an unexpected character paf cigar string";
        case PAFFY_ERR_CHECK_QSTART: return "Paf query start coordinates are invalid";
        case PAFFY_ERR_CHECK_QEND: return "Paf query end coordinates are invalid";
        case PAFFY_ERR_CHECK_TSTART: return "Paf target start coordinates are invalid";
        case PAFFY_ERR_CHECK_TEND: return "Paf target end coordinates are invalid";
        case PAFFY_ERR_CHECK_CIGAR_Q: return "Paf cigar alignment does not match query length";
        case PAFFY_ERR_CHECK_CIGAR_T: return "Paf cigar alignment does not match target length";
        case PAFFY_ERR_SHATTER_ZERO_LEN: return "shatter: cigar op of length < 1";
        case PAFFY_ERR_SHATTER_BAD_OP: return "shatter: cigar op other than M, I or D";
        case PAFFY_ERR_SHATTER_END: return "shatter: cigar does not end on the record's end coordinates";
        case PAFFY_ERR_TRIM_IDENTITY_ASSERT: return "trim: final identity below the starting identity";
        case PAFFY_ERR_TRIM_FIXED_ASSERT: return "trim: fraction outside [0, 1]";
        case PAFFY_ERR_NULL_CIGAR: return "record has no cigar";
        case PAFFY_ERR_MISSING_QUERY_SEQ: return "No query sequence found";
        case PAFFY_ERR_MISSING_TARGET_SEQ: return "No target sequence found";
        case PAFFY_ERR_TILE_ASSERT: return "tile: coverage assertion failed";
        case PAFFY_ERR_SEQ_RANGE: return "alignment reaches outside a sequence";
        case PAFFY_ERR_CHAIN_ASSERT: return "chain: trim fraction outside [0, 1] or a negative alignment length";
        case PAFFY_ERR_DECHUNK_HEADER: return "dechunk: a name does not end in |length|start";
        case PAFFY_ERR_UPCONVERT_ASSERT: return "upconvert: an alignment starts inside an interval and ends beyond it";
        case PAFFY_ERR_FAFFY_ASSERT: return "faffy: assertion failed (chunk size, interval bounds, or merge order)";
        case PAFFY_ERR_FAFFY_BASE: return "faffy: a base other than a, c, g, t or n";
        case PAFFY_ERR_FAFFY_MISSING_SEQ: return "Missing sequence";
        default: return "unknown error";
    }
}

int paffy_hip_profile_enable(paffy_hip_ctx *c, int on) {
    if (!c) return PAFFY_E_ARG;
    c->profile = on != 0;
    return 0;
}
int paffy_hip_profile_only(paffy_hip_ctx *c, const char *kernel) {
    if (!c) return PAFFY_E_ARG;
    c->profile_only = kernel ? kernel : "";
    return 0;
}
int paffy_hip_profile_reset(paffy_hip_ctx *c) {
    if (!c) return PAFFY_E_ARG;
    prof_collect(c);
    for (auto &e : c->prof) {
        e.ms = 0;
        e.launches = 0;
    }
    return 0;
}
int paffy_hip_profile_read(paffy_hip_ctx *c, const char **names, double *total_ms, int64_t *launches, int cap) {
    if (!c) return PAFFY_E_ARG;
    prof_collect(c);
    int n = (int)c->prof.size();
    for (int i = 0; i < n && i < cap; i++) {
        if (names) names[i] = c->prof[i].name.c_str();
        if (total_ms) total_ms[i] = c->prof[i].ms;
        if (launches) launches[i] = c->prof[i].launches;
    }
    return n;
}

int paffy_hip_malloc(void **p, int64_t bytes) { return hipMalloc(p, (size_t)bytes + 64) == hipSuccess ? 0 : PAFFY_E_HIP; }
int paffy_hip_free(void *p) { return hipFree(p) == hipSuccess ? 0 : PAFFY_E_HIP; }
int paffy_hip_device_buffers(int64_t *buffers, int64_t *bytes) {
    if (!buffers || !bytes) return PAFFY_E_ARG;
    *buffers = devbuf_held_buffers.load(std::memory_order_relaxed);
    *bytes = devbuf_held_bytes.load(std::memory_order_relaxed);
    return 0;
}
int paffy_hip_memcpy_h2d(void *d, const void *h, int64_t n) { return hipMemcpy(d, h, (size_t)n, hipMemcpyHostToDevice) == hipSuccess ? 0 : PAFFY_E_HIP; }
int paffy_hip_memcpy_d2h(void *h, const void *d, int64_t n) { return hipMemcpy(h, d, (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : PAFFY_E_HIP; }
int paffy_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int paffy_hip_synth_contigs(paffy_hip_ctx *c, uint64_t seed, uint32_t mean_ops, uint32_t n_contigs, uint64_t r0, uint64_t n, void *d_out, int64_t out_cap,
                            int64_t *bytes);
int paffy_hip_synth(paffy_hip_ctx *c, uint64_t seed, uint32_t mean_ops, uint64_t r0, uint64_t n, void *d_out, int64_t out_cap,
                    int64_t *bytes) {
    return paffy_hip_synth_contigs(c, seed, mean_ops, 24, r0, n, d_out, out_cap, bytes);
}
int paffy_hip_synth_contigs(paffy_hip_ctx *c, uint64_t seed, uint32_t mean_ops, uint32_t n_contigs, uint64_t r0, uint64_t n, void *d_out, int64_t out_cap,
                            int64_t *bytes) {
    if (!c || !bytes || n >= (1ull << 31) || n_contigs < 1) return PAFFY_E_ARG;
    *bytes = 0;
    if (n == 0) return 0;
    psynth_cfg cfg;
    cfg.seed = seed;
    cfg.mean_ops = mean_ops;
    cfg.n_contigs = n_contigs;
    if (ensure(c, c->synth_sizes, sizeof(int64_t) * (size_t)(2 * n + 2))) return PAFFY_E_HIP;
    int64_t *sizes = static_cast<int64_t *>(c->synth_sizes.p), *offs = sizes + n, *total = offs + n;
    const uint32_t nn = (uint32_t)n, grid = (nn + PAFFY_NT - 1) / PAFFY_NT;
    LAUNCH(c, "k_synth_size", k_synth_size, dim3(grid), dim3(PAFFY_NT), 0, cfg, r0, nn, sizes);
    LAUNCH(c, "k_scan_i64", k_scan_i64, dim3(1), dim3(PAFFY_NT), 0, sizes, nn, offs, total);
    int64_t h_total = 0;
    HIPCHK(c, hipMemcpyAsync(&h_total, total, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *bytes = h_total;
    if (!d_out) return 0;
    if (out_cap < h_total) return PAFFY_E_CAPACITY;
    LAUNCH(c, "k_synth_fill", k_synth_fill, dim3(grid), dim3(PAFFY_NT), 0, cfg, r0, nn, offs, static_cast<uint8_t *>(d_out));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static psynth4_tab synth4_tab(paffy_hip_ctx *c) {
    psynth4_tab t;
    t.contigs = static_cast<const psynth4_contig *>(c->synth4_contigs.p);
    t.ckpt_q = static_cast<const int64_t *>(c->synth4_q.p);
    t.ckpt_t = static_cast<const int64_t *>(c->synth4_t.p);
    return t;
}

int paffy_hip_synth4_setup(paffy_hip_ctx *c, uint64_t seed, uint32_t mean_ops, uint32_t n_contigs, int64_t tlen_min, int64_t tlen_span,
                           int with_genomes) {
    if (!c || n_contigs < 1 || n_contigs > 4096 || tlen_min < 2048 || tlen_span < 0) return PAFFY_E_ARG;
    psynth4_cfg cfg;
    cfg.seed = seed;
    cfg.mean_ops = mean_ops;
    cfg.n_contigs = n_contigs;
    cfg.tlen_min = tlen_min;
    cfg.tlen_span = tlen_span;
    c->synth4_cfg.n_contigs = 0;
    std::vector<psynth4_contig> ct(n_contigs);
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_contigs; k++) {
        memset(&ct[k], 0, sizeof(psynth4_contig));
        ct[k].tlen = psynth4_tlen(&cfg, k);
        ct[k].ckpt_cap = psynth4_ckpt_cap(ct[k].tlen);
        ct[k].ckpt_base = total;
        total += ct[k].ckpt_cap;
    }
    if (ensure(c, c->synth4_contigs, sizeof(psynth4_contig) * n_contigs)) return PAFFY_E_HIP;
    if (ensure(c, c->synth4_q, sizeof(int64_t) * total)) return PAFFY_E_HIP;
    if (ensure(c, c->synth4_t, sizeof(int64_t) * total)) return PAFFY_E_HIP;
    HIPCHK(c, hipMemcpyAsync(c->synth4_contigs.p, ct.data(), sizeof(psynth4_contig) * n_contigs, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_synth4_master", k_synth4_master, dim3(n_contigs), dim3(64), 0, cfg, static_cast<psynth4_contig *>(c->synth4_contigs.p),
           static_cast<int64_t *>(c->synth4_q.p), static_cast<int64_t *>(c->synth4_t.p));
    HIPCHK(c, hipMemcpyAsync(ct.data(), c->synth4_contigs.p, sizeof(psynth4_contig) * n_contigs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->synth4_cfg = cfg;
    if (!with_genomes) return 0;
    std::vector<std::string> names;
    std::vector<int64_t> lens;
    for (int g = 0; g < 2; g++)
        for (uint32_t k = 0; k < n_contigs; k++) {
            names.push_back(std::string(g ? "pt.chr" : "hs.chr") + std::to_string(k + 1));
            lens.push_back(g ? ct[k].tlen : ct[k].qlen);
        }
    std::vector<const char *> name_ptr;
    for (const std::string &s : names) name_ptr.push_back(s.c_str());
    std::vector<uint64_t> blob_off;
    int rc = seq_store_layout(c, (int64_t)names.size(), name_ptr.data(), lens.data(), blob_off);
    if (rc) return rc;
    uint8_t *blob = static_cast<uint8_t *>(c->seq_blob.p);
    const psynth4_tab tab = synth4_tab(c);
    for (uint32_t k = 0; k < n_contigs; k++) {
        const uint32_t q_blocks = (uint32_t)((ct[k].n_ops + PSYNTH4_G - 1) / PSYNTH4_G);
        LAUNCH(c, "k_synth4_query", k_synth4_query, dim3(q_blocks), dim3(64), 0, cfg, k, tab, blob + blob_off[k]);
        const uint32_t t_blocks = (uint32_t)((ct[k].tlen + 32ll * PAFFY_NT - 1) / (32ll * PAFFY_NT));
        LAUNCH(c, "k_synth4_target", k_synth4_target, dim3(t_blocks), dim3(PAFFY_NT), 0, cfg, k, ct[k].tlen, blob + blob_off[n_contigs + k]);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (seq_store_canon(c)) return PAFFY_E_HIP;
    c->n_seqs = (int32_t)names.size();
    return 0;
}

int paffy_hip_synth4(paffy_hip_ctx *c, uint64_t r0, uint64_t n, void *d_out, int64_t out_cap, int64_t *bytes) {
    if (!c || !bytes || n >= (1ull << 31)) return PAFFY_E_ARG;
    if (c->synth4_cfg.n_contigs == 0) return PAFFY_E_STATE;
    *bytes = 0;
    if (n == 0) return 0;
    const psynth4_cfg cfg = c->synth4_cfg;
    const psynth4_tab tab = synth4_tab(c);
    if (ensure(c, c->synth_sizes, sizeof(int64_t) * (size_t)(2 * n + 2))) return PAFFY_E_HIP;
    int64_t *sizes = static_cast<int64_t *>(c->synth_sizes.p), *offs = sizes + n, *total = offs + n;
    const uint32_t nn = (uint32_t)n, grid = (nn + PAFFY_NT - 1) / PAFFY_NT;
    LAUNCH(c, "k_synth4_size", k_synth4_size, dim3(grid), dim3(PAFFY_NT), 0, cfg, tab, r0, nn, sizes);
    LAUNCH(c, "k_scan_i64", k_scan_i64, dim3(1), dim3(PAFFY_NT), 0, sizes, nn, offs, total);
    int64_t h_total = 0;
    HIPCHK(c, hipMemcpyAsync(&h_total, total, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *bytes = h_total;
    if (!d_out) return 0;
    if (out_cap < h_total) return PAFFY_E_CAPACITY;
    LAUNCH(c, "k_synth4_fill", k_synth4_fill, dim3(grid), dim3(PAFFY_NT), 0, cfg, tab, r0, nn, offs, static_cast<uint8_t *>(d_out));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

} /* extern "C" */

#include "seqload_kernel.h"
#include "seqload_host.h"

/* every command state is complete here. Nothing of this context may still be queued when its buffers go: they free themselves after
   this body, behind the one synchronise (teardown only, on no timed path) */
paffy_hip_ctx::~paffy_hip_ctx() {
    for (paffy_hip_stream *st : open_streams) stream_detach(st); /* streams still open: they close later without this context */
    open_streams.clear();
    prof_collect(this);
    for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
    event_pool.clear();
    (void)hipDeviceSynchronize();
    if (side) (void)hipStreamDestroy(side);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (h_info) (void)hipHostFree(h_info);
}

/*
 * dedupe_parts_kernel.h -- `paffy dedupe [-a]` sharded by KEY OWNER (include/paffy_hip.h, "Dedupe in parts"). Included by paffy_hip.hip
 * behind paffy_hip_dedupe_plan, whose keys (k_dedupe_keys), selection scratch and line tail (dedupe_plan_lines) it shares.
 *
 * "First seen wins" (dedupe_host.h) is a decision per CLASS of records -- a class is a key, with -a a key and its swapped key -- and
 * needs the class's records in one place, not the input. So a part (a context holding any share of the records, each with its global
 * input number) sends one 32-byte ENTRY per record to the part that owns the record's class key, the owner answers one VERDICT byte per
 * entry, and the text never moves:
 *   source  k_dd_count / k_dd_place   entries grouped by owner: counts per owner in LDS (wave-aggregated), one flush per workgroup,
 *                                     a scan over (owner, workgroup), then every workgroup places its entries from its own bases
 *   owner   k_dd_unpack .. k_dd_decide  the entries sorted by (class hi, class lo, global number); the head of every run is the class's
 *                                     first record; the owner's memory (classes it declared written in earlier rounds, sorted, each with
 *                                     the head's orientation) says whether the class was written before
 *   source  k_dd_verdicts, k_dd_keep  the bytes scattered back onto the local records, the records to write in input order
 * Orientation: flag bit 0 of an entry says that the record's own key is its class key. Two records of a class have the same own key iff
 * they have the same bit (a record that is its own swap has own key = swapped key = class key, and so has every record of its class:
 * all bits set), which is all "own key found" of impl/paf_dedupe.c:121-126 needs.
 */
#ifndef PAFFY_DEDUPE_PARTS_KERNEL_H_
#define PAFFY_DEDUPE_PARTS_KERNEL_H_

struct DdEntry {
    uint64_t chi, clo; /* class key */
    int64_t gnum;      /* global input number of the record */
    uint64_t flags;    /* bit 0: the own key is the class key, bit 1: the coordinates fail paf_check */
};
static_assert(sizeof(DdEntry) == 32, "an entry is two 16-byte words");

#define DD_WIN 1024u        /* owners counted per pass over a workgroup's records (LDS counters) */
#define DD_MAX_BLOCKS 512u  /* workgroups of the count / place kernels: each takes a contiguous stretch of the records */

/* The owner of a class key: a pure function of the key and the number of parts (shard.dedupe_owner is the same function). The keys are
   hashes already; the finalizer keeps related keys (a key and a near miss) from sharing high bits, the multiply-high maps to [0, n_parts). */
__device__ __forceinline__ uint32_t dd_owner(uint64_t chi, uint64_t clo, uint32_t n_parts) {
    uint64_t x = chi ^ clo;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return (uint32_t)__umul64hi(x, (uint64_t)n_parts);
}

/* cnt[slot] += 1 for every lane that is `on`, one LDS atomic per distinct slot of the wave; returns the lane's place: the counter's
   value before the wave plus the lane's rank among the wave's lanes of the same slot. Called by whole waves. */
__device__ __forceinline__ uint32_t dd_wave_add(uint32_t *cnt, bool on, uint32_t slot) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(on);
    uint32_t place = 0;
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t s = (uint32_t)__shfl((int)slot, lead);
        const unsigned long long same = __ballot(on && slot == s);
        uint32_t base = 0;
        if ((int)lane == lead) base = atomicAdd(&cnt[s], (uint32_t)__popcll(same));
        base = (uint32_t)__shfl((int)base, lead);
        if (on && slot == s) place = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return place;
}

__device__ __forceinline__ bool dd_class_of(const DedupeKey &k, int inverse, uint64_t &chi, uint64_t &clo) {
    const bool own_is_class = !inverse || !dd_less(k.ia, k.ib, k.a, k.b);
    chi = own_is_class ? k.a : k.ia;
    clo = own_is_class ? k.b : k.ib;
    return own_is_class;
}

/* Workgroup b takes records [b * per, (b + 1) * per). counts[owner * gridDim.x + b] = its records of that owner that parsed;
   *parse_bad = the lowest record that did not (one atomic per wave that has one). */
__global__ __launch_bounds__(PAFFY_NT) void k_dd_count(const DedupeKey *keys, uint32_t n, uint32_t per, int inverse, uint32_t n_parts, uint32_t *counts, uint32_t *parse_bad) {
    __shared__ uint32_t cnt[DD_WIN];
    const uint32_t b = blockIdx.x, lane = threadIdx.x & 63u;
    const uint32_t lo = b * per, hi = min(n, lo + per);
    for (uint32_t w0 = 0; w0 < n_parts; w0 += DD_WIN) {
        for (uint32_t s = threadIdx.x; s < DD_WIN; s += PAFFY_NT) cnt[s] = 0;
        __syncthreads();
        for (uint32_t base = lo; base < hi; base += PAFFY_NT) {
            const uint32_t i = base + threadIdx.x;
            bool on = false, bad = false;
            uint32_t slot = 0;
            if (i < hi) {
                const DedupeKey k = keys[i];
                if (k.err == 0) {
                    uint64_t chi, clo;
                    dd_class_of(k, inverse, chi, clo);
                    slot = dd_owner(chi, clo, n_parts) - w0;
                    on = slot < DD_WIN;
                } else {
                    bad = w0 == 0;
                }
            }
            const unsigned long long bm = __ballot(bad);
            if (bm && (int)lane == __ffsll((long long)bm) - 1) atomicMin(parse_bad, i); /* the wave's lowest lane = its lowest record */
            (void)dd_wave_add(cnt, on, slot);
        }
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < DD_WIN && w0 + s < n_parts; s += PAFFY_NT) counts[(size_t)(w0 + s) * gridDim.x + b] = cnt[s];
        __syncthreads();
    }
}
__global__ __launch_bounds__(PAFFY_NT) void k_dd_starts(const uint32_t *scanned, uint32_t n_blocks, uint32_t n_parts, uint32_t *starts) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p <= n_parts) starts[p] = scanned[(size_t)p * n_blocks];
}
/* scanned[owner * gridDim.x + b]: where workgroup b's entries of that owner begin. Order inside an owner's segment: by workgroup, free
   inside one (the entry carries its number). ent_rec[j] = the local record of entry j. */
__global__ __launch_bounds__(PAFFY_NT) void k_dd_place(const DedupeKey *keys, uint32_t n, uint32_t per, int inverse, uint32_t n_parts, const uint32_t *scanned, int64_t rec_base,
                                                     uint32_t n_entries, DdEntry *entries, uint32_t *ent_rec) {
    __shared__ uint32_t at[DD_WIN];
    const uint32_t b = blockIdx.x;
    const uint32_t lo = b * per, hi = min(n, lo + per);
    for (uint32_t w0 = 0; w0 < n_parts; w0 += DD_WIN) {
        for (uint32_t s = threadIdx.x; s < DD_WIN; s += PAFFY_NT) at[s] = w0 + s < n_parts ? scanned[(size_t)(w0 + s) * gridDim.x + b] : 0u;
        __syncthreads();
        for (uint32_t base = lo; base < hi; base += PAFFY_NT) {
            const uint32_t i = base + threadIdx.x;
            bool on = false;
            uint32_t slot = 0;
            uint64_t chi = 0, clo = 0, flags = 0;
            if (i < hi) {
                const DedupeKey k = keys[i];
                if (k.err == 0) {
                    flags = (dd_class_of(k, inverse, chi, clo) ? 1u : 0u) | (k.check != 0 ? 2u : 0u);
                    slot = dd_owner(chi, clo, n_parts) - w0;
                    on = slot < DD_WIN;
                }
            }
            const uint32_t j = dd_wave_add(at, on, slot);
            if (on && j < n_entries) {
                ulonglong2 *e = reinterpret_cast<ulonglong2 *>(entries + j);
                e[0] = make_ulonglong2(chi, clo);
                e[1] = make_ulonglong2((uint64_t)(rec_base + (int64_t)i), flags);
                ent_rec[j] = i;
            }
        }
        __syncthreads();
    }
}

/* ---- owner side ---- */
__global__ __launch_bounds__(PAFFY_NT) void k_dd_unpack(const DdEntry *entries, uint32_t n, uint64_t *khi, uint64_t *klo, uint64_t *kg, uint32_t *idx) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i >= n) return;
    const ulonglong2 *e = reinterpret_cast<const ulonglong2 *>(entries + i);
    const ulonglong2 k = e[0], g = e[1];
    khi[i] = k.x;
    klo[i] = k.y;
    kg[i] = g.x;
    idx[i] = i;
}
/* position p of the order by (class, number): head[p] = p where a class begins, else 0 (a running maximum gives every position its head) */
__global__ __launch_bounds__(PAFFY_NT) void k_dd_heads(const DdEntry *entries, const uint32_t *order, uint32_t n, uint32_t *head) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p >= n) return;
    bool h = p == 0;
    if (!h) {
        const ulonglong2 a = reinterpret_cast<const ulonglong2 *>(entries + order[p])[0], b = reinterpret_cast<const ulonglong2 *>(entries + order[p - 1])[0];
        h = a.x != b.x || a.y != b.y;
    }
    head[p] = h ? p : 0u;
}
/* verdict of the entry at position p: bit 0 written (the class's first record of the round, class not in the memory), bit 1 fails
   (-a, own key not found among the records written before it, coordinates fail paf_check); wflag[p] = the class enters the memory */
__global__ __launch_bounds__(PAFFY_NT) void k_dd_decide(const DdEntry *entries, const uint32_t *order, const uint32_t *head_of, uint32_t n, int inverse, const uint64_t *mem_hi,
                                                      const uint64_t *mem_lo, const uint32_t *mem_or, uint32_t mem_n, uint8_t *verdicts, uint32_t *wflag) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p >= n) return;
    const uint32_t hp = head_of[p], i = order[p], h = order[hp];
    const ulonglong2 *e = reinterpret_cast<const ulonglong2 *>(entries + i);
    const ulonglong2 k = e[0], g = e[1];
    const uint64_t head_flags = reinterpret_cast<const ulonglong2 *>(entries + h)[1].y;
    uint32_t lo = 0, hi = mem_n; /* first class of the memory not less than this one */
    while (lo < hi) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (dd_less(mem_hi[m], mem_lo[m], k.x, k.y)) lo = m + 1;
        else hi = m;
    }
    const bool in_mem = lo < mem_n && mem_hi[lo] == k.x && mem_lo[lo] == k.y;
    const uint32_t own_bit = (uint32_t)(g.y & 1u);
    const bool written = p == hp && !in_mem;
    /* the class's written record -- of an earlier round (memory) or this round's head -- has this record's orientation */
    const bool own_found = in_mem ? mem_or[lo] == own_bit : (p != hp && (uint32_t)(head_flags & 1u) == own_bit);
    const bool fails = inverse && !own_found && (g.y & 2u);
    verdicts[i] = (uint8_t)((written ? 1u : 0u) | (fails ? 2u : 0u));
    wflag[p] = written ? 1u : 0u;
}
__global__ __launch_bounds__(PAFFY_NT) void k_dd_remember(const DdEntry *entries, const uint32_t *order, const uint32_t *wflag, const uint32_t *wpos, uint32_t n, uint64_t *mem_hi,
                                                        uint64_t *mem_lo, uint32_t *mem_or) {
    const uint32_t p = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (p >= n || !wflag[p]) return;
    const ulonglong2 *e = reinterpret_cast<const ulonglong2 *>(entries + order[p]);
    const ulonglong2 k = e[0], g = e[1];
    const uint32_t q = wpos[p];
    mem_hi[q] = k.x;
    mem_lo[q] = k.y;
    mem_or[q] = (uint32_t)(g.y & 1u);
}
/* The memory's n_a classes [0, n_a) and the round's n_b new ones [n_a, n_a + n_b) of hi / lo / orient, each run sorted by (hi, lo) and
   the two disjoint (a new class is one the memory does not hold: no tie rule), merged into hi2 / lo2 / or2: element i of a run goes to
   i + the number of elements of the OTHER run that are less than it -- one binary search, and the orientation word moves with its key. */
__global__ __launch_bounds__(PAFFY_NT) void k_dd_merge(const uint64_t *hi, const uint64_t *lo, const uint32_t *orient, uint32_t n_a, uint32_t n_b, uint64_t *hi2, uint64_t *lo2,
                                                     uint32_t *or2) {
    const uint32_t t = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (t >= n_a + n_b) return;
    const bool mine_a = t < n_a;
    const uint64_t kh = hi[t], kl = lo[t];
    const uint32_t first = mine_a ? n_a : 0u; /* the other run is [first, first + len) */
    uint32_t b = 0, e = mine_a ? n_b : n_a;
    while (b < e) {
        const uint32_t m = b + ((e - b) >> 1);
        if (dd_less(hi[first + m], lo[first + m], kh, kl)) b = m + 1;
        else e = m;
    }
    const uint32_t q = (mine_a ? t : t - n_a) + b; /* < n_a + n_b: the place in its own run plus at most the other run's length */
    hi2[q] = kh;
    lo2[q] = kl;
    or2[q] = orient[t];
}

/* ---- source side, after the owners answered ---- */
/* vloc[record of entry j] = verdicts[j]; *first_bad = the lowest local record whose verdict has bit 1 (one atomic per wave that has one) */
__global__ __launch_bounds__(PAFFY_NT) void k_dd_verdicts(const uint8_t *verdicts, const uint32_t *ent_rec, uint32_t n_entries, uint32_t n, uint8_t *vloc, uint32_t *first_bad) {
    const uint32_t j = blockIdx.x * PAFFY_NT + threadIdx.x;
    uint32_t mine = 0xffffffffu;
    if (j < n_entries) {
        const uint32_t r = ent_rec[j], v = verdicts[j];
        if (r < n) {
            vloc[r] = (uint8_t)v;
            if (v & 2u) mine = r;
        }
    }
    if (__ballot(mine != 0xffffffffu)) {
        for (int off = 32; off > 0; off >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, off));
        if ((threadIdx.x & 63u) == 0) atomicMin(first_bad, mine);
    }
}
__global__ __launch_bounds__(PAFFY_NT) void k_dd_keep(const uint8_t *vloc, uint32_t n, uint32_t n_below, uint32_t *keep) {
    const uint32_t i = blockIdx.x * PAFFY_NT + threadIdx.x;
    if (i < n) keep[i] = (i < n_below && (vloc[i] & 1u)) ? 1u : 0u;
}

/* ---- host ---- */
struct DedupeParts {
    /* source side: the round of the batch in the index buffers (paffy_hip_ctx::dd_part_stage) */
    DevBuf counts, scanned, starts, first, ent_rec, vloc, keep, pos;
    const uint8_t *in = nullptr;
    int64_t in_len = 0, rec_base = 0;
    uint32_t n = 0, n_entries = 0;
    uint32_t parse_bad = 0xffffffffu, first_bad = 0xffffffffu; /* local records: the lowest that did not parse / the lowest failing one */
    /* owner side: the classes declared written since the last reset, sorted by (hi, lo), each with its head's orientation bit */
    DevBuf mem_hi, mem_lo, mem_or, mem_hi2, mem_lo2, mem_or2;
    size_t mem_n = 0;
    DevBuf khi, klo, kg, k64a, k64b, idx, va, vb, head, head_of, wflag, wpos, tmp;
};
static DedupeParts &dedupe_parts(paffy_hip_ctx *c) {
    if (!c->dd_parts) c->dd_parts.reset(new DedupeParts());
    return *c->dd_parts;
}
static void dedupe_parts_reset(paffy_hip_ctx *c) {
    c->dd_part_stage = 0;
    c->dd_part_failed = false;
    if (c->dd_parts) c->dd_parts->mem_n = 0;
}

static int dd_parts_sort(paffy_hip_ctx *c, DedupeParts &P, const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, size_t n) {
    size_t bytes = 0;
    RPCHK(c, rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0, 64, c->stream));
    if (ensure(c, P.tmp, bytes + 16)) return PAFFY_E_HIP;
    RPCHK(c, rocprim::radix_sort_pairs(P.tmp.p, bytes, kin, kout, vin, vout, n, 0, 64, c->stream));
    return 0;
}
static int dd_parts_excl_scan(paffy_hip_ctx *c, DedupeParts &P, const uint32_t *in, uint32_t *out, size_t n) {
    size_t bytes = 0;
    RPCHK(c, rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    if (ensure(c, P.tmp, bytes + 16)) return PAFFY_E_HIP;
    RPCHK(c, rocprim::exclusive_scan(P.tmp.p, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream));
    return 0;
}
/* the scratch of the owner's sorts, for m items */
static int dd_parts_scratch(paffy_hip_ctx *c, DedupeParts &P, size_t m) {
    if (ensure(c, P.k64a, sizeof(uint64_t) * m) || ensure(c, P.k64b, sizeof(uint64_t) * m) || ensure(c, P.idx, sizeof(uint32_t) * m) || ensure(c, P.va, sizeof(uint32_t) * m) ||
        ensure(c, P.vb, sizeof(uint32_t) * m))
        return PAFFY_E_HIP;
    return 0;
}

int paffy_hip_dedupe_part_keys(paffy_hip_ctx *c, const void *d_in, int64_t in_len, int check_inverse, int64_t rec_base, int32_t n_parts, void *d_entries, int64_t cap_entries,
                               int64_t *part_counts, int64_t *n_records) {
    if (!c || !part_counts || !n_records || n_parts < 1 || rec_base < 0 || cap_entries < 0 || (check_inverse != 0 && check_inverse != 1)) return PAFFY_E_ARG;
    if (in_len < 0 || in_len >= (1ll << 31) - 64 || (in_len > 0 && !d_in) || (reinterpret_cast<uintptr_t>(d_in) & 15) || (reinterpret_cast<uintptr_t>(d_entries) & 15)) return PAFFY_E_ARG;
    if (c->dd_part_failed) return PAFFY_E_STATE;
    paffy_plan_info unused;
    plan_begin(c, PLAN_LINES, in_len, &unused); /* whatever was planned is gone: the index buffers are this round's now */
    DedupeParts &P = dedupe_parts(c);
    P.in = static_cast<const uint8_t *>(d_in);
    P.in_len = in_len;
    P.rec_base = rec_base;
    P.n = P.n_entries = 0;
    P.parse_bad = P.first_bad = 0xffffffffu;
    for (int32_t p = 0; p < n_parts; p++) part_counts[p] = 0;
    *n_records = 0;
    uint32_t n = 0;
    if (in_len > 0) {
        int rc = index_and_parse(c, P.in, (uint32_t)in_len, &n);
        if (rc) return rc;
    }
    *n_records = n;
    if (n == 0) {
        c->dd_part_stage = 1;
        return 0;
    }
    const uint32_t grid = (n + PAFFY_NT - 1) / PAFFY_NT;
    if (ensure(c, c->dedupe_keys, sizeof(DedupeKey) * (size_t)n) || ensure(c, c->tile_level, sizeof(int64_t) * (size_t)n) || ensure(c, c->tile_order, sizeof(uint32_t) * (size_t)n) ||
        ensure(c, c->tile_len, sizeof(int64_t) * (size_t)(n + 2)))
        return PAFFY_E_HIP;
    const DedupeKey *keys = static_cast<const DedupeKey *>(c->dedupe_keys.p);
    LAUNCH(c, "k_dedupe_keys", k_dedupe_keys, dim3(grid), dim3(PAFFY_NT), 0, P.in, static_cast<const RecMeta *>(c->meta.p), n, static_cast<DedupeKey *>(c->dedupe_keys.p),
           static_cast<int64_t *>(c->tile_level.p));
    /* contiguous stretches of whole workgroup widths; few enough workgroups that the (owner, workgroup) table stays small */
    const uint32_t max_blocks = std::max<uint32_t>(1u, std::min<uint32_t>(DD_MAX_BLOCKS, (1u << 24) / (uint32_t)n_parts));
    const uint32_t per = ((grid + max_blocks - 1) / max_blocks) * PAFFY_NT, n_blocks = (n + per - 1) / per;
    const size_t n_counts = (size_t)n_parts * n_blocks;
    if (ensure(c, P.counts, sizeof(uint32_t) * (n_counts + 1)) || ensure(c, P.scanned, sizeof(uint32_t) * (n_counts + 1)) || ensure(c, P.starts, sizeof(uint32_t) * ((size_t)n_parts + 1)) ||
        ensure(c, P.first, 2 * sizeof(uint32_t)) || ensure(c, P.ent_rec, sizeof(uint32_t) * (size_t)n))
        return PAFFY_E_HIP;
    uint32_t *counts = static_cast<uint32_t *>(P.counts.p), *scanned = static_cast<uint32_t *>(P.scanned.p), *first = static_cast<uint32_t *>(P.first.p);
    HIPCHK(c, hipMemsetAsync(first, 0xff, 2 * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(counts + n_counts, 0, sizeof(uint32_t), c->stream)); /* so that the scan's last entry is the total */
    LAUNCH(c, "k_dd_count", k_dd_count, dim3(n_blocks), dim3(PAFFY_NT), 0, keys, n, per, check_inverse, (uint32_t)n_parts, counts, first);
    if (dd_parts_excl_scan(c, P, counts, scanned, n_counts + 1)) return PAFFY_E_HIP;
    LAUNCH(c, "k_dd_starts", k_dd_starts, dim3(((uint32_t)n_parts + 1 + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(scanned), n_blocks, (uint32_t)n_parts,
           static_cast<uint32_t *>(P.starts.p));
    std::vector<uint32_t> starts((size_t)n_parts + 1);
    HIPCHK(c, hipMemcpyAsync(starts.data(), P.starts.p, sizeof(uint32_t) * starts.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&P.parse_bad, first, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t n_entries = starts[(size_t)n_parts];
    if ((int64_t)n_entries > cap_entries) return PAFFY_E_CAPACITY; /* nothing was written to d_entries */
    if (n_entries > 0) {
        if (!d_entries) return PAFFY_E_ARG;
        LAUNCH(c, "k_dd_place", k_dd_place, dim3(n_blocks), dim3(PAFFY_NT), 0, keys, n, per, check_inverse, (uint32_t)n_parts, static_cast<const uint32_t *>(scanned), rec_base, n_entries,
               static_cast<DdEntry *>(d_entries), static_cast<uint32_t *>(P.ent_rec.p));
    }
    for (int32_t p = 0; p < n_parts; p++) part_counts[p] = (int64_t)(starts[(size_t)p + 1] - starts[(size_t)p]);
    if (c->profile) prof_collect(c);
    P.n = n;
    P.n_entries = n_entries;
    c->dd_part_stage = 1;
    return 0;
}

int paffy_hip_dedupe_part_decide(paffy_hip_ctx *c, const void *d_entries, int64_t n_entries, int check_inverse, void *d_verdicts) {
    if (!c || n_entries < 0 || n_entries >= (1ll << 31) || (check_inverse != 0 && check_inverse != 1) || (reinterpret_cast<uintptr_t>(d_entries) & 15)) return PAFFY_E_ARG;
    if (c->dd_part_failed) return PAFFY_E_STATE;
    if (n_entries == 0) return 0;
    if (!d_entries || !d_verdicts) return PAFFY_E_ARG;
    DedupeParts &P = dedupe_parts(c);
    const uint32_t n = (uint32_t)n_entries, grid = (n + PAFFY_NT - 1) / PAFFY_NT;
    const DdEntry *entries = static_cast<const DdEntry *>(d_entries);
    if (dd_parts_scratch(c, P, n) || ensure(c, P.khi, sizeof(uint64_t) * (size_t)n) || ensure(c, P.klo, sizeof(uint64_t) * (size_t)n) || ensure(c, P.kg, sizeof(uint64_t) * (size_t)n) ||
        ensure(c, P.head, sizeof(uint32_t) * (size_t)n) || ensure(c, P.head_of, sizeof(uint32_t) * (size_t)n) || ensure(c, P.wflag, sizeof(uint32_t) * (size_t)n) ||
        ensure(c, P.wpos, sizeof(uint32_t) * (size_t)n))
        return PAFFY_E_HIP;
    uint64_t *khi = static_cast<uint64_t *>(P.khi.p), *klo = static_cast<uint64_t *>(P.klo.p), *kg = static_cast<uint64_t *>(P.kg.p);
    uint64_t *k64a = static_cast<uint64_t *>(P.k64a.p), *k64b = static_cast<uint64_t *>(P.k64b.p);
    uint32_t *idx = static_cast<uint32_t *>(P.idx.p), *va = static_cast<uint32_t *>(P.va.p), *vb = static_cast<uint32_t *>(P.vb.p);
    uint32_t *head = static_cast<uint32_t *>(P.head.p), *head_of = static_cast<uint32_t *>(P.head_of.p), *wflag = static_cast<uint32_t *>(P.wflag.p), *wpos = static_cast<uint32_t *>(P.wpos.p);
    /* stable sorts, least significant key first: global number, class lo, class hi */
    LAUNCH(c, "k_dd_unpack", k_dd_unpack, dim3(grid), dim3(PAFFY_NT), 0, entries, n, khi, klo, kg, idx);
    if (dd_parts_sort(c, P, kg, k64a, idx, va, n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_gather_u64_by", k_gather_u64_by, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(klo), static_cast<const uint32_t *>(va), n, k64b);
    if (dd_parts_sort(c, P, k64b, k64a, va, vb, n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_gather_u64_by", k_gather_u64_by, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(khi), static_cast<const uint32_t *>(vb), n, k64b);
    if (dd_parts_sort(c, P, k64b, k64a, vb, va, n)) return PAFFY_E_HIP;
    const uint32_t *order = va;
    LAUNCH(c, "k_dd_heads", k_dd_heads, dim3(grid), dim3(PAFFY_NT), 0, entries, order, n, head);
    {
        size_t bytes = 0;
        RPCHK(c, rocprim::inclusive_scan(nullptr, bytes, head, head_of, n, DdMax(), c->stream));
        if (ensure(c, P.tmp, bytes + 16)) return PAFFY_E_HIP;
        RPCHK(c, rocprim::inclusive_scan(P.tmp.p, bytes, head, head_of, n, DdMax(), c->stream));
    }
    LAUNCH(c, "k_dd_decide", k_dd_decide, dim3(grid), dim3(PAFFY_NT), 0, entries, order, static_cast<const uint32_t *>(head_of), n, check_inverse,
           static_cast<const uint64_t *>(P.mem_hi.p), static_cast<const uint64_t *>(P.mem_lo.p), static_cast<const uint32_t *>(P.mem_or.p), (uint32_t)P.mem_n, static_cast<uint8_t *>(d_verdicts),
           wflag);
    if (dd_parts_excl_scan(c, P, wflag, wpos, n)) return PAFFY_E_HIP;
    uint32_t last_pos = 0, last_flag = 0;
    HIPCHK(c, hipMemcpyAsync(&last_pos, wpos + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&last_flag, wflag + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t nw = last_pos + last_flag;
    if (nw > 0) { /* the new classes behind the memory's, then the two runs merged by (hi, lo) */
        const size_t m = P.mem_n + nw;
        if (m >= (1ull << 31)) {
            c->last_error = "dedupe in parts: more than 2^31 classes in one owner's memory";
            return PAFFY_E_ARG;
        }
        const size_t used = P.mem_n;
        if (ensure_keep(c, P.mem_hi, sizeof(uint64_t) * m, sizeof(uint64_t) * used) || ensure_keep(c, P.mem_lo, sizeof(uint64_t) * m, sizeof(uint64_t) * used) ||
            ensure_keep(c, P.mem_or, sizeof(uint32_t) * m, sizeof(uint32_t) * used) || ensure(c, P.mem_hi2, sizeof(uint64_t) * m) || ensure(c, P.mem_lo2, sizeof(uint64_t) * m) ||
            ensure(c, P.mem_or2, sizeof(uint32_t) * m))
            return PAFFY_E_HIP;
        uint64_t *mh = static_cast<uint64_t *>(P.mem_hi.p), *ml = static_cast<uint64_t *>(P.mem_lo.p);
        uint32_t *mo = static_cast<uint32_t *>(P.mem_or.p);
        LAUNCH(c, "k_dd_remember", k_dd_remember, dim3(grid), dim3(PAFFY_NT), 0, entries, order, static_cast<const uint32_t *>(wflag), static_cast<const uint32_t *>(wpos), n, mh + used,
               ml + used, mo + used);
        /* both runs are sorted -- the memory by construction, the new classes because wpos is a scan over entries in (hi, lo, number)
           order -- and disjoint: one merge in place of a sort of all m */
        const uint32_t gm = (uint32_t)((m + PAFFY_NT - 1) / PAFFY_NT);
        LAUNCH(c, "k_dd_merge", k_dd_merge, dim3(gm), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(mh), static_cast<const uint64_t *>(ml), static_cast<const uint32_t *>(mo),
               (uint32_t)used, nw, static_cast<uint64_t *>(P.mem_hi2.p), static_cast<uint64_t *>(P.mem_lo2.p), static_cast<uint32_t *>(P.mem_or2.p));
        std::swap(P.mem_hi, P.mem_hi2);
        std::swap(P.mem_lo, P.mem_lo2);
        std::swap(P.mem_or, P.mem_or2);
        P.mem_n = m;
    }
    if (c->profile) prof_collect(c);
    return 0;
}

int paffy_hip_dedupe_part_verdicts(paffy_hip_ctx *c, const void *d_verdicts, int64_t n_entries, int64_t *first_bad_global) {
    if (!c || !first_bad_global || n_entries < 0) return PAFFY_E_ARG;
    if (c->dd_part_failed || c->dd_part_stage != 1 || !c->dd_parts) return PAFFY_E_STATE;
    DedupeParts &P = *c->dd_parts;
    if (n_entries != (int64_t)P.n_entries || (n_entries > 0 && !d_verdicts)) return PAFFY_E_ARG;
    *first_bad_global = -1;
    P.first_bad = P.parse_bad;
    if (P.n > 0) {
        if (ensure(c, P.vloc, (size_t)P.n)) return PAFFY_E_HIP;
        HIPCHK(c, hipMemsetAsync(P.vloc.p, 0, (size_t)P.n, c->stream)); /* a record without an entry is not written */
    }
    if (P.n_entries > 0) {
        uint32_t *first = static_cast<uint32_t *>(P.first.p) + 1;
        uint32_t bad = 0xffffffffu;
        LAUNCH(c, "k_dd_verdicts", k_dd_verdicts, dim3((P.n_entries + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const uint8_t *>(d_verdicts),
               static_cast<const uint32_t *>(P.ent_rec.p), P.n_entries, P.n, static_cast<uint8_t *>(P.vloc.p), first);
        HIPCHK(c, hipMemcpyAsync(&bad, first, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        P.first_bad = std::min(P.first_bad, bad);
    }
    if (P.first_bad != 0xffffffffu) *first_bad_global = P.rec_base + (int64_t)P.first_bad;
    c->dd_part_stage = 2;
    return 0;
}

int paffy_hip_dedupe_part_plan(paffy_hip_ctx *c, int64_t first_bad_global, paffy_plan_info *info) {
    if (!c || !info) return PAFFY_E_ARG;
    if (c->dd_part_failed || c->dd_part_stage != 2 || !c->dd_parts) return PAFFY_E_STATE;
    DedupeParts &P = *c->dd_parts;
    const uint32_t n = P.n;
    plan_begin(c, PLAN_LINES, P.in_len, info);
    c->plan.n_records = n;
    if (first_bad_global >= 0) c->dd_part_failed = true; /* the run is over, here and in every other part, until the next reset */
    /* this part's records in front of the failing one */
    const uint32_t n_below = first_bad_global < 0 || first_bad_global >= P.rec_base + (int64_t)n ? n : first_bad_global <= P.rec_base ? 0u : (uint32_t)(first_bad_global - P.rec_base);
    if (first_bad_global >= P.rec_base && first_bad_global < P.rec_base + (int64_t)n) { /* the failing record is this part's */
        const uint32_t r = (uint32_t)(first_bad_global - P.rec_base);
        DedupeKey k;
        HIPCHK(c, hipMemcpy(&k, static_cast<const DedupeKey *>(c->dedupe_keys.p) + r, sizeof(k), hipMemcpyDeviceToHost));
        c->plan.error.record = first_bad_global;
        if (k.err) {
            c->plan.error.code = k.err;
            c->plan.error.stage = -1;
            RecMeta m;
            HIPCHK(c, hipMemcpy(&m, static_cast<RecMeta *>(c->meta.p) + r, sizeof(m), hipMemcpyDeviceToHost));
            c->plan.error.aux = m.err_aux;
        } else {
            c->plan.error.code = k.check;
            c->plan.error.stage = 0;
        }
    }
    uint32_t nk = 0;
    if (n > 0 && n_below > 0) {
        const uint32_t grid = (n + PAFFY_NT - 1) / PAFFY_NT;
        if (ensure(c, P.keep, sizeof(uint32_t) * (size_t)n) || ensure(c, P.pos, sizeof(uint32_t) * (size_t)n)) return PAFFY_E_HIP;
        uint32_t *keep = static_cast<uint32_t *>(P.keep.p), *pos = static_cast<uint32_t *>(P.pos.p);
        LAUNCH(c, "k_dd_keep", k_dd_keep, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint8_t *>(P.vloc.p), n, n_below, keep);
        if (dd_parts_excl_scan(c, P, keep, pos, n)) return PAFFY_E_HIP;
        uint32_t last_pos = 0, last_keep = 0;
        HIPCHK(c, hipMemcpyAsync(&last_pos, pos + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&last_keep, keep + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nk = last_pos + last_keep;
        if (nk > 0)
            LAUNCH(c, "k_dedupe_collect", k_dedupe_collect, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const DedupeKey *>(c->dedupe_keys.p), static_cast<const uint32_t *>(keep),
                   static_cast<const uint32_t *>(pos), n, n, 0, static_cast<uint32_t *>(c->tile_order.p), static_cast<uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), 0u);
    }
    if (!c->dedupe) c->dedupe.reset(new DedupeState()); /* the scan scratch of the line tail */
    return dedupe_plan_lines(c, P.in, nk, info);
}

#endif

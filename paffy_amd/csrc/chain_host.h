/*
 * chain_host.h -- host side of `paffy chain` (included by paffy_hip.hip after coverage_host.h, whose batch bookkeeping, radix sort
 * wrappers and line writer it shares). Every step runs on the device; the host sizes buffers and reads back three counters.
 */
#ifndef PAFFY_CHAIN_HOST_H_
#define PAFFY_CHAIN_HOST_H_

#include "chain_kernel.h"

struct ChainState {
    DevBuf i64[12]; /* per record: qs qe ts te sc (5), level (kept in CovState), per position: qs qe ts te sc mq best (7) */
    DevBuf qkey, ghash, ord1, ord2, rank, start, gid, idx, prank, pred, neg, taken, is_tail, tail_of, link, total, chain_of_tail, chain_id, score_key, o1, o2, o3, cls, big_list, n_big, rank_of, claim,
        tag_chain, tag_score, check_key, iota;
    /* chain in parts: the records' global input numbers (one int64 per record once a batch came with them), the records ordered and
       ranked by them (grank per record, ai per position), the chain ends in local chain order, a few words of counters */
    DevBuf gidx, gperm, grank, ai, tails, words;
    /* the walk from a fresh iterator (paffy_hip_chain_fresh_walk): the leading runs, one byte per position, the flag kernel's live lists */
    DevBuf lead, fresh, slots;
    int64_t fresh_stats[4] = {0, 0, 0, 0}; /* of the last run: records the flag kernel took, flagged fresh, links it gave, candidates skipped */
    bool indexed = false;    /* a batch was added with global numbers: gidx holds one per record */
    bool part_ready = false; /* chain_part ran without error: tail keys can be read, chain_finish may follow */
    uint32_t n_chains = 0;
    int64_t fail_key[3] = {0, 0, 0}; /* (own score, chain id, link) of the line whose paf_check failed in the last chain_finish */
    uint64_t n_out = 0;
    uint32_t group_salt = 0; /* salt the last run's grouping passed its name check with (0 unless group keys collided) */
};
static ChainState &chain_state(paffy_hip_ctx *c);

static ChainPos chain_pos(ChainState &H) {
    auto I64 = [&](int k) { return static_cast<int64_t *>(H.i64[k].p); };
    /* ai: without global numbers the address stand-in is the input index itself */
    return ChainPos{I64(5), I64(6), I64(7), I64(8), I64(9), I64(10), static_cast<uint32_t *>(H.idx.p), static_cast<uint32_t *>(H.prank.p),
                    static_cast<uint32_t *>(H.indexed ? H.ai.p : H.idx.p), I64(11), static_cast<uint32_t *>(H.pred.p), static_cast<uint8_t *>(H.neg.p)};
}
/* first_err_key -> *err; with global numbers the key's record is the global one and a parse error's record is looked up for its aux */
static int chain_report(paffy_hip_ctx *c, unsigned long long key, paffy_error *err) {
    CovState &S = cov_state(c);
    ChainState &H = chain_state(c);
    err->code = (int32_t)(key & 0xff);
    err->stage = (int32_t)((key >> 8) & 0xff) - 1;
    err->record = (int64_t)(key >> 16);
    err->aux = 0;
    if (err->stage < 0) {
        unsigned long long local = key >> 16;
        if (H.indexed) { /* k_cov_collect kept the lowest local record; the lowest global one is what one process reports */
            const uint32_t n = (uint32_t)S.n_rec, grid = (n + PAFFY_NT - 1) / PAFFY_NT;
            if (ensure(c, H.words, 4 * sizeof(unsigned long long))) return PAFFY_E_HIP;
            unsigned long long *w = static_cast<unsigned long long *>(H.words.p), got[2];
            HIPCHK(c, hipMemsetAsync(w, 0xff, 2 * sizeof(unsigned long long), c->stream));
            LAUNCH(c, "k_chain_parse_err_min", k_chain_parse_err_min, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(S.meta.p),
                   static_cast<const int64_t *>(H.gidx.p), n, w);
            LAUNCH(c, "k_chain_parse_err_rec", k_chain_parse_err_rec, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(S.meta.p),
                   static_cast<const int64_t *>(H.gidx.p), n, static_cast<const unsigned long long *>(w), w + 1);
            if (cov_fetch(c, got, w, sizeof(got))) return PAFFY_E_HIP;
            err->code = (int32_t)(got[0] & 0xff);
            err->record = (int64_t)(got[0] >> 16);
            local = got[1];
        }
        RecMeta m;
        if (cov_fetch(c, &m, static_cast<RecMeta *>(S.meta.p) + local, sizeof(m))) return PAFFY_E_HIP;
        err->aux = m.err_aux;
    }
    return 0;
}

/*
 * chain_run in two halves, cut where its global decisions begin. chain_part: keys, groups, the recurrence, the cut of the chains and
 * their numbering inside this context -- by (strand, chain-end score desc, processing key desc, input number desc). chain_finish: output
 * order, tags, paf_check, with the chain numbers chain_part gave or the ones a caller installed in between (paffy_hip_chain_renumber).
 */
static int chain_part(paffy_hip_ctx *c, const ChainOpts &o, bool count_chains, paffy_error *err, bool fresh_walk = false) {
    CovState &S = cov_state(c);
    ChainState &H = chain_state(c);
    memset(err, 0, sizeof(*err));
    memset(H.fresh_stats, 0, sizeof(H.fresh_stats));
    H.n_out = 0;
    H.n_chains = 0;
    H.part_ready = false;
    const uint32_t n = (uint32_t)S.n_rec;
    if (n == 0) {
        H.part_ready = true;
        return 0;
    }
    DevInfo hinfo;
    if (cov_fetch(c, &hinfo, S.info.p, sizeof(hinfo))) return PAFFY_E_HIP;
    auto report = [&](unsigned long long key) -> int { return chain_report(c, key, err); };
    if (hinfo.first_err_key != ~0ull) return report(hinfo.first_err_key); /* read_pafs parses every line first */
    {
        std::vector<const uint8_t *> ptrs;
        for (const CovBatch &b : S.batches) ptrs.push_back(b.in);
        if (ensure(c, S.batch_ptrs, sizeof(void *) * ptrs.size())) return PAFFY_E_HIP;
        HIPCHK(c, hipMemcpyAsync(S.batch_ptrs.p, ptrs.data(), sizeof(void *) * ptrs.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const size_t n1 = (size_t)n + 1;
    for (DevBuf &b : H.i64)
        if (ensure(c, b, sizeof(int64_t) * n1)) return PAFFY_E_HIP;
    DevBuf *u64s[] = {&H.qkey, &H.ghash, &H.score_key, &S.k64a, &S.k64b};
    for (DevBuf *b : u64s)
        if (ensure(c, *b, sizeof(uint64_t) * n1)) return PAFFY_E_HIP;
    DevBuf *u32s[] = {&H.ord1, &H.ord2, &H.rank, &H.start, &H.gid, &H.idx, &H.prank, &H.pred, &H.tail_of, &H.link, &H.chain_of_tail, &H.chain_id, &H.o1, &H.o2, &H.o3, &H.cls, &H.big_list, &H.rank_of, &H.claim,
                      &H.iota, &H.tails, &S.flags, &S.scan32, &S.v32a, &S.v32b, &S.order};
    for (DevBuf *b : u32s)
        if (ensure(c, *b, sizeof(uint32_t) * (n1 + 1))) return PAFFY_E_HIP;
    DevBuf *u8s[] = {&H.neg, &H.taken, &H.is_tail};
    for (DevBuf *b : u8s)
        if (ensure(c, *b, n1)) return PAFFY_E_HIP;
    if (ensure(c, H.total, sizeof(int64_t) * n1) || ensure(c, H.tag_chain, sizeof(int64_t) * n1) || ensure(c, H.tag_score, sizeof(int64_t) * n1) ||
        ensure(c, S.level, sizeof(int64_t) * n1) || ensure(c, H.check_key, sizeof(unsigned long long)) || ensure(c, H.n_big, sizeof(uint32_t)) ||
        ensure(c, H.words, 4 * sizeof(unsigned long long)))
        return PAFFY_E_HIP;
    if (H.indexed && (ensure(c, H.gperm, sizeof(uint32_t) * (n1 + 1)) || ensure(c, H.grank, sizeof(uint32_t) * (n1 + 1)) || ensure(c, H.ai, sizeof(uint32_t) * (n1 + 1)))) return PAFFY_E_HIP;
    auto I64 = [&](int k) { return static_cast<int64_t *>(H.i64[k].p); };
    auto U32 = [&](DevBuf &b) { return static_cast<uint32_t *>(b.p); };
    auto U64 = [&](DevBuf &b) { return static_cast<uint64_t *>(b.p); };
    auto U8 = [&](DevBuf &b) { return static_cast<uint8_t *>(b.p); };
    const uint32_t grid = (n + PAFFY_NT - 1) / PAFFY_NT;
    RecMeta *meta = static_cast<RecMeta *>(S.meta.p);
    ChainRecs R{I64(0), I64(1), I64(2), I64(3), I64(4), U64(H.qkey), U64(H.ghash), static_cast<int64_t *>(S.level.p)};
    const int64_t *gidx = H.indexed ? static_cast<const int64_t *>(H.gidx.p) : nullptr;
    if (gidx) { /* creation order = the global input numbers: the records sorted and ranked by them */
        LAUNCH(c, "k_iota32", k_iota32, dim3(grid), dim3(PAFFY_NT), 0, U32(H.iota), n);
        if (cov_sort_pairs(c, S, reinterpret_cast<const uint64_t *>(gidx), U64(S.k64a), U32(H.iota), U32(H.gperm), n)) return PAFFY_E_HIP;
        LAUNCH(c, "k_chain_rank", k_chain_rank, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.gperm)), n, U32(H.grank));
    }
    uint32_t n_groups = 0;
    for (uint32_t salt = 0;; salt++) {
        LAUNCH(c, "k_chain_keys", k_chain_keys, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint8_t *const *>(S.batch_ptrs.p), static_cast<const RecMeta *>(meta), n, o, R,
               static_cast<DevInfo *>(S.info.p), salt, gidx);
        if (cov_fetch(c, &hinfo, S.info.p, sizeof(hinfo))) return PAFFY_E_HIP;
        if (hinfo.first_err_key != ~0ull) return report(hinfo.first_err_key);
        /* processing order: query start, then input order (impl/chaining.c:14-21, 139) */
        LAUNCH(c, "k_iota32", k_iota32, dim3(grid), dim3(PAFFY_NT), 0, U32(H.iota), n);
        if (gidx) { /* the stable sort starts from the records in global input order */
            LAUNCH(c, "k_gather_u64", k_gather_u64, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(U64(H.qkey)), static_cast<const uint32_t *>(U32(H.gperm)), n,
                   U64(S.k64b));
            if (cov_sort_pairs(c, S, U64(S.k64b), U64(S.k64a), U32(H.gperm), U32(H.ord1), n)) return PAFFY_E_HIP;
        } else if (cov_sort_pairs(c, S, U64(H.qkey), U64(S.k64a), U32(H.iota), U32(H.ord1), n)) return PAFFY_E_HIP;
        LAUNCH(c, "k_chain_rank", k_chain_rank, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.ord1)), n, U32(H.rank));
        /* groups: (query name, target name, strand), members in processing order */
        LAUNCH(c, "k_gather_u64", k_gather_u64, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(U64(H.ghash)), static_cast<const uint32_t *>(U32(H.ord1)), n, U64(S.k64b));
        if (cov_sort_pairs(c, S, U64(S.k64b), U64(S.k64a), U32(H.ord1), U32(H.ord2), n)) return PAFFY_E_HIP;
        LAUNCH(c, "k_cov_run_heads", k_cov_run_heads, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(U64(S.k64a)), n, U32(S.flags));
        if (cov_incl_scan32(c, S, U32(S.flags), U32(S.scan32), n)) return PAFFY_E_HIP;
        if (cov_fetch(c, &n_groups, U32(S.scan32) + (n - 1), sizeof(uint32_t))) return PAFFY_E_HIP;
        LAUNCH(c, "k_chain_group_starts", k_chain_group_starts, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(S.flags)), static_cast<const uint32_t *>(U32(S.scan32)),
               n, U32(H.start), U32(H.gid));
        /* the names behind the hashes (impl/chaining.c:37-54 compares strings): a group holding two different keys is regrouped under the next salt */
        uint32_t *collide = U32(H.n_big), hit = 0;
        HIPCHK(c, hipMemsetAsync(collide, 0, sizeof(uint32_t), c->stream));
        LAUNCH(c, "k_chain_verify_groups", k_chain_verify_groups, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint8_t *const *>(S.batch_ptrs.p), static_cast<const RecMeta *>(meta),
               static_cast<const uint32_t *>(U32(H.ord2)), static_cast<const uint32_t *>(U32(H.start)), static_cast<const uint32_t *>(U32(H.gid)), n, collide);
        if (cov_fetch(c, &hit, collide, sizeof(uint32_t))) return PAFFY_E_HIP;
        H.group_salt = salt;
        if (!hit) break;
        if (salt == 7) {
            c->last_error = "chain groups keep colliding under eight differently salted 64-bit hashes";
            return PAFFY_E_UNSUPPORTED;
        }
    }
    ChainPos Q = chain_pos(H);
    LAUNCH(c, "k_chain_gather", k_chain_gather, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(meta), R, static_cast<const uint32_t *>(U32(H.ord2)),
           static_cast<const uint32_t *>(U32(H.rank)), static_cast<const uint32_t *>(gidx ? U32(H.grank) : nullptr), n, Q);
    const uint32_t wgrid = (n_groups + PAFFY_NWAVE - 1) / PAFFY_NWAVE;
    LAUNCH(c, "k_chain_prefix_max", k_chain_prefix_max, dim3(wgrid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.start)), n_groups, Q);
    HIPCHK(c, hipMemsetAsync(H.n_big.p, 0, sizeof(uint32_t), c->stream));
    LAUNCH(c, "k_chain_big_list", k_chain_big_list, dim3((n_groups + PAFFY_NT - 1) / PAFFY_NT), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.start)), n_groups,
           U32(H.big_list), U32(H.n_big));
    ChainLead *lead = nullptr;
    if (fresh_walk) { /* the strands' leading runs: the first recurrence counts what it skips inside them */
        if (ensure(c, H.lead, sizeof(ChainLead))) return PAFFY_E_HIP;
        lead = static_cast<ChainLead *>(H.lead.p);
        HIPCHK(c, hipMemsetAsync(lead, 0xff, sizeof(ChainLead), c->stream));
        const uint32_t ggrid = (n_groups + PAFFY_NT - 1) / PAFFY_NT;
        for (int phase = 0; phase < 3; phase++)
            LAUNCH(c, "k_chain_lead_runs", k_chain_lead_runs, dim3(phase < 2 ? ggrid : 1u), dim3(PAFFY_NT), 0, phase, static_cast<const uint32_t *>(U32(H.start)), n_groups, Q, lead);
    }
    LAUNCH(c, "k_chain_dp", k_chain_dp, dim3(wgrid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.start)), n_groups, o, Q, static_cast<const uint8_t *>(nullptr), lead);
    LAUNCH(c, "k_chain_dp_big", k_chain_dp_big, dim3(256), dim3(CHAIN_BIG_NT), 0, static_cast<const uint32_t *>(U32(H.start)), static_cast<const uint32_t *>(U32(H.big_list)),
           static_cast<const uint32_t *>(U32(H.n_big)), o, Q, static_cast<const uint8_t *>(nullptr), lead);
    bool flagged = false;
    if (fresh_walk) {
        ChainLead hl;
        if (cov_fetch(c, &hl, lead, sizeof(hl))) return PAFFY_E_HIP;
        H.fresh_stats[3] = (int64_t)(hl.skipped[0] + hl.skipped[1]);
        if (hl.skipped[0] + hl.skipped[1]) {
            /* some search of a leading run skipped a candidate: which searches were fresh, and those one or two groups again */
            const size_t per_run = ((size_t)n + 63) / 64 * 64 + 64;
            if (ensure(c, H.fresh, n1) || ensure(c, H.slots, (2 * sizeof(int64_t) + sizeof(uint32_t)) * 2 * per_run)) return PAFFY_E_HIP;
            HIPCHK(c, hipMemsetAsync(H.fresh.p, 0, n1, c->stream));
            int64_t *live = static_cast<int64_t *>(H.slots.p);
            const ChainLive V{live, live + 2 * per_run, reinterpret_cast<uint32_t *>(live + 4 * per_run), per_run};
            LAUNCH(c, "k_chain_fresh_flags", k_chain_fresh_flags, dim3(2), dim3(64), 0, o, Q, lead, V, U8(H.fresh));
            const uint8_t *fresh = U8(H.fresh);
            for (int s = 0; s < 2; s++) {
                if (!hl.skipped[s]) continue;
                H.fresh_stats[0] += (int64_t)(hl.last[s] - hl.g0[s]) + 1;
                uint32_t ends[2];
                if (cov_fetch(c, ends, U32(H.start) + hl.g[s], sizeof(ends))) return PAFFY_E_HIP;
                if (ends[1] - ends[0] > CHAIN_BIG_GROUP)
                    LAUNCH(c, "k_chain_dp_big", k_chain_dp_big, dim3(1), dim3(CHAIN_BIG_NT), 0, static_cast<const uint32_t *>(U32(H.start)), static_cast<const uint32_t *>(&lead->g[s]),
                           static_cast<const uint32_t *>(&lead->one), o, Q, fresh, static_cast<ChainLead *>(nullptr));
                else
                    LAUNCH(c, "k_chain_dp", k_chain_dp, dim3(1), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.start)) + hl.g[s], 1u, o, Q, fresh, static_cast<ChainLead *>(nullptr));
            }
            flagged = true;
        }
    }
    /* (chain score desc, processing index desc): least significant key first, stable sorts */
    LAUNCH(c, "k_chain_not", k_chain_not, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.prank)), n, U32(S.v32a));
    if (cov_sort_pairs32(c, S, U32(S.v32a), U32(S.v32b), U32(H.iota), U32(H.o1), n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_chain_desc_keys", k_chain_desc_keys, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const int64_t *>(I64(11)), static_cast<const uint32_t *>(U32(H.o1)), n, U64(S.k64b));
    if (cov_sort_pairs(c, S, U64(S.k64b), U64(S.k64a), U32(H.o1), U32(H.o2), n)) return PAFFY_E_HIP; /* o2: all positions by (score desc, index desc) */
    /* every chain end walks its chain (o2 gives the ranks) */
    HIPCHK(c, hipMemsetAsync(H.taken.p, 0, n1, c->stream));          /* has_child */
    HIPCHK(c, hipMemsetAsync(H.claim.p, 0xff, sizeof(uint32_t) * n1, c->stream));
    LAUNCH(c, "k_chain_rank_and_children", k_chain_rank_and_children, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.o2)), Q, n, U32(H.rank_of), U8(H.taken));
    LAUNCH(c, "k_chain_claim", k_chain_claim, dim3(grid), dim3(PAFFY_NT), 0, Q, static_cast<const uint32_t *>(U32(H.rank_of)), static_cast<const uint8_t *>(U8(H.taken)), n,
           U32(H.claim));
    LAUNCH(c, "k_chain_own", k_chain_own, dim3(grid), dim3(PAFFY_NT), 0, o, Q, static_cast<const uint32_t *>(U32(H.rank_of)), static_cast<const uint8_t *>(U8(H.taken)),
           static_cast<const uint32_t *>(U32(H.claim)), n, U32(H.tail_of), U32(H.link), static_cast<int64_t *>(H.total.p), U8(H.is_tail));
    /* chain ids: the tails by (strand, score desc, index desc) */
    LAUNCH(c, "k_chain_class", k_chain_class, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.o2)), static_cast<const uint8_t *>(U8(H.is_tail)),
           static_cast<const uint8_t *>(U8(H.neg)), n, U32(H.cls));
    if (cov_sort_pairs32(c, S, U32(H.cls), U32(S.v32b), U32(H.o2), U32(H.o1), n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_chain_number", k_chain_number, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.o1)), static_cast<const uint8_t *>(U8(H.is_tail)), n,
           U32(H.chain_of_tail), U32(H.tails));
    if (flagged) {
        ChainLead hl;
        LAUNCH(c, "k_chain_fresh_links", k_chain_fresh_links, dim3(grid), dim3(PAFFY_NT), 0, Q, n, lead);
        if (cov_fetch(c, &hl, lead, sizeof(hl))) return PAFFY_E_HIP;
        H.fresh_stats[1] = (int64_t)hl.n_fresh;
        H.fresh_stats[2] = (int64_t)hl.n_links;
    }
    if (count_chains) {
        uint32_t *n_chains = reinterpret_cast<uint32_t *>(static_cast<unsigned long long *>(H.words.p) + 2);
        HIPCHK(c, hipMemsetAsync(n_chains, 0, sizeof(uint32_t), c->stream));
        LAUNCH(c, "k_chain_count", k_chain_count, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(S.v32b)), n, n_chains);
        if (cov_fetch(c, &H.n_chains, n_chains, sizeof(uint32_t))) return PAFFY_E_HIP;
    }
    H.part_ready = true;
    return 0;
}

static int chain_finish(paffy_hip_ctx *c, paffy_error *err) {
    CovState &S = cov_state(c);
    ChainState &H = chain_state(c);
    memset(err, 0, sizeof(*err));
    H.n_out = 0;
    const uint32_t n = (uint32_t)S.n_rec;
    if (n == 0) return 0;
    auto U32 = [&](DevBuf &b) { return static_cast<uint32_t *>(b.p); };
    auto U64 = [&](DevBuf &b) { return static_cast<uint64_t *>(b.p); };
    const uint32_t grid = (n + PAFFY_NT - 1) / PAFFY_NT;
    RecMeta *meta = static_cast<RecMeta *>(S.meta.p);
    const int64_t *gidx = H.indexed ? static_cast<const int64_t *>(H.gidx.p) : nullptr;
    ChainPos Q = chain_pos(H);
    DevInfo hinfo;
    LAUNCH(c, "k_chain_out_keys", k_chain_out_keys, dim3(grid), dim3(PAFFY_NT), 0, Q, static_cast<const uint32_t *>(U32(H.tail_of)),
           static_cast<const uint32_t *>(U32(H.chain_of_tail)), n, U32(H.chain_id), U64(H.score_key));
    /* output order: own score desc; equal scores stay in the order the chains were written (chain, then link from the tail) */
    if (cov_sort_pairs32(c, S, U32(H.link), U32(S.v32b), U32(H.iota), U32(H.o1), n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_gather_u32", k_gather_u32, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint32_t *>(U32(H.chain_id)), static_cast<const uint32_t *>(U32(H.o1)), n, U32(S.v32a));
    if (cov_sort_pairs32(c, S, U32(S.v32a), U32(S.v32b), U32(H.o1), U32(H.o2), n)) return PAFFY_E_HIP;
    LAUNCH(c, "k_gather_u64", k_gather_u64, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const uint64_t *>(U64(H.score_key)), static_cast<const uint32_t *>(U32(H.o2)), n, U64(S.k64b));
    if (cov_sort_pairs(c, S, U64(S.k64b), U64(S.k64a), U32(H.o2), U32(H.o3), n)) return PAFFY_E_HIP;
    HIPCHK(c, hipMemsetAsync(H.check_key.p, 0xff, sizeof(unsigned long long), c->stream));
    LAUNCH(c, "k_chain_finish", k_chain_finish, dim3(grid), dim3(PAFFY_NT), 0, meta, Q, static_cast<const uint32_t *>(U32(H.o3)), static_cast<const uint32_t *>(U32(H.tail_of)),
           static_cast<const uint32_t *>(U32(H.chain_id)), static_cast<const uint32_t *>(U32(H.link)), static_cast<const int64_t *>(H.total.p), n, U32(S.order),
           static_cast<int64_t *>(H.tag_chain.p), static_cast<int64_t *>(H.tag_score.p), static_cast<unsigned long long *>(H.check_key.p));
    LAUNCH(c, "k_chain_find_failed", k_chain_find_failed, dim3(grid), dim3(PAFFY_NT), 0, static_cast<const RecMeta *>(meta), Q, static_cast<const uint32_t *>(U32(H.chain_id)),
           static_cast<const uint32_t *>(U32(H.link)), n, static_cast<const unsigned long long *>(H.check_key.p), gidx, static_cast<DevInfo *>(S.info.p),
           reinterpret_cast<int64_t *>(static_cast<unsigned long long *>(H.words.p) + 3));
    if (cov_fetch(c, &hinfo, S.info.p, sizeof(hinfo))) return PAFFY_E_HIP;
    if (c->profile) prof_collect(c);
    if (hinfo.first_err_key != ~0ull) {
        unsigned long long ck = 0;
        if (cov_fetch(c, &ck, H.check_key.p, sizeof(ck)) || cov_fetch(c, &H.fail_key[0], static_cast<unsigned long long *>(H.words.p) + 3, sizeof(int64_t))) return PAFFY_E_HIP;
        H.fail_key[1] = (int64_t)(ck >> 32);
        H.fail_key[2] = (int64_t)(ck & 0xffffffffull);
        H.part_ready = false; /* the check key is in the context's error word: a second finish would not start clean */
        return chain_report(c, hinfo.first_err_key, err);
    }
    H.n_out = n;
    return 0;
}

static int chain_run(paffy_hip_ctx *c, const ChainOpts &o, paffy_error *err, bool fresh_walk) {
    int rc = chain_part(c, o, false, err, fresh_walk);
    if (rc || err->code || (uint32_t)cov_state(c).n_rec == 0) return rc;
    return chain_finish(c, err);
}

#endif

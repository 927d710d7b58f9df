/*
 * flat_add_pipe_kernel.h -- `paffy add_mismatches | paffy trim -r` / `| paffy filter` (the reference's tests/paf_tools_test.sh:56, 100-106) as
 * the fused stage lists [ADD_MISMATCHES, TRIM_IDENTITY], [ADD_MISMATCHES, FILTER] and [ADD_MISMATCHES, TRIM_IDENTITY, FILTER] on the pieces of
 * the flat pass.
 *
 * The encoder of flat_add_kernel.h leaves every kept record's new cigar contiguous in new_ops[]. paf_trim_unreliable_tails
 * (impl/paf.c:811-953) only ever removes whole ops from the two ends, so the trimmed record is a window [lo, lo + n) over those ops plus
 * changed coordinates, and a filter behind it is a predicate on four sums of the window. Both need of the new ops what the flat pass
 * needs of the parsed ones: per piece the ops, the bases by kind and the bytes of text -- summed where the ops are written. The kernels,
 * in order:
 *
 *   k_flat_parse<1>, k_add_prep, (scan), k_add_count, (scan)     as flat_add_kernel.h
 *   k_addp_fill      k_add_fill with a PieceSum of the NEW ops per piece slot (add_fill_pieces<true>): 32 bytes written per piece
 *   k_addp_size      one wave per record, in place of k_add_final: the summaries become inclusive prefix sums (registers up to 64 pieces,
 *                    in place in HBM above), the trim runs on them as in k_flat_size (flat_trim_prefix on the 4-byte new ops: only the
 *                    pieces that can hold a hit are walked, one op per lane), the filter on the window's totals, then the line plan:
 *                    header with the trimmed coordinates, the window for k_emit_line (arena_off advanced to its first op), out_len from
 *                    the window's text (whole pieces from the summaries, the two edge pieces op by op: FlatRecT::raw_prefix), and for a
 *                    window of more than PAFFY_ROWS_MAX_OPS new ops the EmitItem segments cut at the piece boundaries inside it
 *
 * Every record is sized by a wave: the one-lane form of k_flat_lane for the short ones is not built here.
 *
 * Who leaves for the record kernels (flat_done = 0, counted in flat_legacy and by reason): what the encoder does not keep
 * (FLAT_WHY_ENCODER), a failing trim assert (FLAT_WHY_TRIM_ASSERT), a failing paf_check behind the trim (FLAT_WHY_CHECK), a window without
 * ops (FLAT_WHY_EMPTY), a header beyond the line writer's (FLAT_WHY_HEADER_LEN), one piece that becomes more new ops than a wave should
 * write or an item list without room (FLAT_WHY_ROW_SHAPE), sums beyond 31 bits (FLAT_WHY_SUMS). The counts are 32 bits wide, so a piece of
 * more than 65 535 new ops stays.
 */
#ifndef PAFFY_FLAT_ADD_PIPE_KERNEL_H_
#define PAFFY_FLAT_ADD_PIPE_KERNEL_H_

struct AddPipeParams {
    AddParams A;
    PieceSum *nsums; /* per piece slot: the summary of the piece's new ops (k_addp_fill); scanned in place by k_addp_size for records of more than 64 pieces */
};

typedef FlatRecT<uint32_t> AddRec; /* the walks read the 4-byte new ops where the encoder left them: no second mirror is written */

__global__ __launch_bounds__(64 * ADD_WAVES) void k_addp_fill(AddPipeParams Q) {
    __shared__ uint32_t s_slots[ADD_WAVES][PAFFY_FILL_SLOTS];
    add_fill_pieces<true>(Q.A, s_slots, Q.nsums);
}

__device__ __forceinline__ void addp_leave(const AddParams &A, uint32_t rec, int why) {
    if ((threadIdx.x & 63u) == 0) {
        if (why >= 0) atomicAdd(&A.P.info->flat_reason[why], 1u);
        A.flat_done[rec] = 0;
        A.P.out_len[rec] = 0;
        A.P.out_rows[rec] = 0;
        A.P.status[rec] = 0;
        atomicAdd(&A.P.info->flat_legacy, 1u);
    }
}

/* The segments of a window of more than PAFFY_ROWS_MAX_OPS new ops, by k_add_final's rule on the pieces' shares of the window: a segment
   closes where the next piece would take it past ADD_SEG_OPS. The first starts at the window's first op, the last ends at its last, wo
   counts from the window's first byte (a boundary between two pieces inside the window: the scanned text of the pieces in front of it).
   Sixty-four pieces' sums per load, then a scalar walk over them. WRITE: the items go to items[] (lane 0); returns their number, *fits =
   no piece holds more ops of the window than a wave should write. */
template <bool WRITE>
__device__ __forceinline__ uint32_t addp_segments(const AddRec &R, const FlatView &v, uint32_t rec, EmitItem *items, bool *fits) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w_end = v.lo + v.n;
    const uint32_t nb = (R.np + 63u) >> 6;
    uint32_t n_seg = 0, seg_ops = 0, seg_b = 0, seg_wo = 0;
    bool ok = true;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t p = b * 64u + lane;
        uint32_t e_cnt = 0, a_cnt = 0, a_text = 0;
        if (p < R.np) e_cnt = R.in_regs ? R.inc.cnt : flat_ld(&R.ps[p].cnt);
        if (R.in_regs) {
            a_cnt = dpp_mov_u32<0x138, 0xf, 0xf>(R.inc.cnt); /* wave_shr:1, lane 0 receives 0 */
            a_text = dpp_mov_u32<0x138, 0xf, 0xf>(R.inc.text);
        } else if (p > 0 && p < R.np) {
            a_cnt = flat_ld(&R.ps[p - 1u].cnt);
            a_text = flat_ld(&R.ps[p - 1u].text_end);
        }
        const uint32_t lo_c = a_cnt > v.lo ? a_cnt : v.lo, hi_c = e_cnt < w_end ? e_cnt : w_end;
        const uint32_t c = p < R.np && hi_c > lo_c ? hi_c - lo_c : 0u;
        unsigned long long live = __ballot(c != 0);
        while (live) {
            const uint32_t l = (uint32_t)__ffsll((long long)live) - 1u;
            live &= live - 1ull;
            const uint32_t cc = lane_val(c, l);
            if (seg_ops && seg_ops + cc > ADD_SEG_OPS) {
                if (WRITE && lane == 0) {
                    EmitItem it;
                    it.rec = rec; it.wb = seg_b; it.we = seg_b + seg_ops; it.pad = 0; it.cq0 = 0; it.ct0 = 0;
                    it.wo = (int64_t)seg_wo;
                    items[n_seg] = it;
                }
                n_seg++;
                seg_b += seg_ops;
                seg_wo = lane_val(a_text, l) - v.wlo.text; /* the piece starts inside the window: every op in front of it is a whole piece's or the cut's */
                seg_ops = 0;
            }
            seg_ops += cc;
            if (seg_ops > 4u * PAFFY_ROWS_MAX_OPS) ok = false;
        }
    }
    if (seg_ops) {
        if (WRITE && lane == 0) {
            EmitItem it;
            it.rec = rec; it.wb = seg_b; it.we = seg_b + seg_ops; it.pad = 0; it.cq0 = 0; it.ct0 = 0;
            it.wo = (int64_t)seg_wo;
            items[n_seg] = it;
        }
        n_seg++;
    }
    *fits = ok;
    return n_seg;
}

__device__ __forceinline__ void addp_size_one(const AddPipeParams &Q, uint32_t rec) {
    const AddParams &A = Q.A;
    const KParams &P = A.P;
    const uint32_t lane = threadIdx.x & 63u;
    if (uni(A.flat_done[rec]) != 2u || uni(A.rec_bad[rec])) return addp_leave(A, rec, FLAT_WHY_ENCODER);
    const RecMeta &m = P.meta[rec];
    const uint32_t cg_off = m.cg_off, cg_end = cg_off + m.cg_len;
    AddRec R;
    R.np = ((cg_end - 1u) >> FLAT_TILE_SHIFT) - (cg_off >> FLAT_TILE_SHIFT) + 1u;
    const uint32_t slot0 = (cg_off >> FLAT_TILE_SHIFT) + rec;
    PieceSum *const rec_sums = Q.nsums + slot0;
    const uint64_t at = A.new_off[slot0];
    R.ps = rec_sums;
    R.ops = A.new_ops + at;
    R.in_regs = R.np <= 64u;
    R.want_text = true;
    R.extra_icount = false;
    /* the pieces' sums become inclusive prefix sums, as in flat_size_one -- here the text too: a piece's own bytes were counted */
    unsigned long long tot_m = 0, tot_x = 0, tot_n = 0, tot_text = 0;
    {
        FlatPre carry;
        carry.cnt = carry.m = carry.x = carry.ins = carry.del = carry.rows = carry.extra = carry.text = 0;
        const uint32_t nb = (R.np + 63u) >> 6;
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t p = b * 64u + lane;
            uint4 qa = make_uint4(0, 0, 0, 0), qb = make_uint4(0, 0, 0, 0);
            if (p < R.np) {
                qa = reinterpret_cast<const uint4 *>(R.ps + p)[0];
                qb = reinterpret_cast<const uint4 *>(R.ps + p)[1];
            }
            FlatPre inc;
            inc.cnt = carry.cnt + wave_incl_scan_u32(qa.x);
            inc.m = carry.m + wave_incl_scan_u32(qa.y);
            inc.x = carry.x + wave_incl_scan_u32(qa.z);
            inc.ins = carry.ins + wave_incl_scan_u32(qa.w);
            inc.del = carry.del + wave_incl_scan_u32(qb.x);
            inc.rows = 0;
            inc.extra = 0;
            inc.text = carry.text + wave_incl_scan_u32(qb.w);
            /* 64 pieces of at most 8 191 x 512 bases, ops and bytes of text: a block's own sums stay below 2^32, the totals are kept in 64 bits */
            tot_m += wave_sum_u32(qa.y);
            tot_x += wave_sum_u32(qa.z);
            tot_n += wave_sum_u32(qa.x);
            tot_text += wave_sum_u32(qb.w);
            if (R.in_regs) {
                R.inc = inc;
            } else if (p < R.np) {
                uint4 *o = reinterpret_cast<uint4 *>(rec_sums + p);
                o[0] = make_uint4(inc.cnt, inc.m, inc.x, inc.ins);
                o[1] = make_uint4(inc.del, 0u, 0u, inc.text);
            }
            carry.cnt = lane_val(inc.cnt, 63); carry.m = lane_val(inc.m, 63); carry.x = lane_val(inc.x, 63); carry.ins = lane_val(inc.ins, 63);
            carry.del = lane_val(inc.del, 63); carry.text = lane_val(inc.text, 63);
        }
        R.n_ops = carry.cnt;
    }
    if (tot_n == 0 || tot_n >= (1ull << 31) || tot_text >= (1ull << 31) || tot_m + tot_x >= 0x7fffffffull) return addp_leave(A, rec, FLAT_WHY_SUMS);
    if (at + tot_n > A.new_cap) return addp_leave(A, rec, FLAT_WHY_ROW_SHAPE); /* (a try whose new_ops[] was too small: the host encodes the batch again) */
    if (!R.in_regs) __threadfence(); /* the scanned sums are read back below by this wave (other lanes' stores): past the L1, flat_ld() */
    FlatState s;
    s.qlen = m.qlen; s.qs = m.qs; s.qe = m.qe; s.tlen = m.tlen; s.ts = m.ts; s.te = m.te;
    s.same = m.same_strand != 0;
    FlatView v;
    v.lo = 0; v.n = R.n_ops; v.rev = false; v.swp = false;
    v.wlo = R.piece_prefix(0);
    v.whi = R.piece_prefix(R.np);
    /* stage 0 is the encoder, its paf_check passed in k_add_prep; what stands behind it sees the record as `paf_write | paf_parse` leaves it */
    for (int32_t si = 1; si < P.n_stages; si++) {
        const paffy_stage st = P.stages[si];
        if (v.n == 0) return addp_leave(A, rec, FLAT_WHY_EMPTY);
        if (st.kind == PAFFY_TRIM_IDENTITY) { /* paf_trim_unreliable_tails, impl/paf.c:906-953, as flat_size_one states it */
            const uint32_t mm = v.tm(), mx = v.tx();
            const double identity = ratio_f32((int64_t)mm, (int64_t)mm + (int64_t)mx);
            const double thr = __dsub_rn(identity, __dmul_rn(identity, (double)st.p0));
            const int64_t max_trim = __float2ll_rz(__fmul_rn(__ll2float_rn((int64_t)mm + (int64_t)mx), st.p1));
            const float thr_f = __double2float_rn(thr), id_f = __double2float_rn(identity);
            const uint32_t n_before = v.n;
#pragma unroll 1
            for (int pass = 0; pass < 2; pass++) {
                if (pass == 1) {
                    if (s.same && v.n == n_before) break;
                    flat_invert(s);
                    v.swp = !v.swp;
                    if (!s.same) v.rev = !v.rev;
                }
                flat_trim_prefix(R, s, v, thr_f, id_f, max_trim);
                if (pass == 1) {
                    flat_invert(s);
                    v.swp = !v.swp;
                    if (!s.same) v.rev = !v.rev;
                }
            }
            const uint32_t m2 = v.tm(), x2 = v.tx();
            const double final_identity = ratio_f32((int64_t)m2, (int64_t)m2 + (int64_t)x2);
            if (!(final_identity >= identity)) return addp_leave(A, rec, FLAT_WHY_TRIM_ASSERT);
            if (flat_check(s, v)) return addp_leave(A, rec, FLAT_WHY_CHECK);
        } else if (st.kind == PAFFY_FILTER) {
            if (flat_filter_pass(P, m, v) == (P.filter.invert != 0)) {
                if (lane == 0) flat_dropped(P, A.flat_done, rec);
                return;
            }
        } else {
            return addp_leave(A, rec, FLAT_WHY_STAGE); /* not reached: the host gives this mode to the three stage lists only */
        }
    }
    if (v.n == 0) return addp_leave(A, rec, FLAT_WHY_EMPTY);
    RecState rs;
    load_state(m, rs);
    rs.qs = s.qs; rs.qe = s.qe; rs.ts = s.ts; rs.te = s.te;
    if (rs.type == 0 && rs.tile_level != -1) rs.type = rs.tile_level > 1 ? 'S' : 'P'; /* written and parsed again behind the encoder */
    const uint32_t lenH = header_len(rs, false);
    if (lenH + 8 > PAFFY_TMPL_MAX) return addp_leave(A, rec, FLAT_WHY_HEADER_LEN);
    const FlatPre win = flat_sub(v.whi, v.wlo);
    const bool whole = v.n <= PAFFY_ROWS_MAX_OPS;
    uint32_t n_seg = 0, item0 = 0;
    if (!whole) {
        bool fits;
        n_seg = addp_segments<false>(R, v, rec, nullptr, &fits);
        if (!fits) return addp_leave(A, rec, FLAT_WHY_ROW_SHAPE);
        if (lane == 0) item0 = atomicAdd(&P.info->n_items, n_seg);
        item0 = uni(item0);
        if (item0 + n_seg > P.items_cap) { /* no room: the reserved slots inside the list name no record (the writers skip them) */
            if (lane == 0)
                for (uint32_t g = item0; g < P.items_cap && g < item0 + n_seg; g++) P.items[g].rec = FLAT_NO_CHUNK;
            return addp_leave(A, rec, FLAT_WHY_ROW_SHAPE);
        }
        addp_segments<true>(R, v, rec, P.items + item0, &fits);
    }
    if (lane == 0) {
        RecPlan *plan = static_cast<RecPlan *>(P.rec_plan) + rec;
        A.flat_done[rec] = 1;
        P.status[rec] = (uint32_t)KLASS_LDS << 16;
        P.err_aux[rec] = 0;
        P.n_ops[rec] = 0;
        P.out_len[rec] = (int64_t)lenH + (int64_t)win.text + 1;
        P.out_rows[rec] = 1;
        P.arena_off[rec] = at + v.lo; /* in 4-byte words of new_ops[] (flag bit 20): the window's first op */
        plan->qs = s.qs; plan->qe = s.qe; plan->ts = s.ts; plan->te = s.te; plan->sub_lo = 0; plan->sub_hi = 0;
        plan->lo = 0; plan->n = v.n;
        plan->flags = 8u | ((uint32_t)rs.type << 8) | (whole ? 0x10000u : 0x80000u) | 0x20000u | 0x100000u;
        plan->chunk = ((v.n + 63u) / 64u) | 1u;
        for (int w = 0; w < 4; w++) plan->wq[w] = plan->wt[w] = plan->wo[w] = 0;
    }
}

#define ADDP_SIZE_WAVES 4u
/* persistent waves over the records */
__global__ __launch_bounds__(64 * ADDP_SIZE_WAVES) void k_addp_size(AddPipeParams Q) {
    const KParams &P = Q.A.P;
    /* a try whose scratch or new_ops[] was too small (the scans left the demand in DevInfo): nothing of it counts, nothing is walked */
    const bool void_try = P.info->add_scr_total > Q.A.scr_cap || P.info->add_new_total > Q.A.new_cap;
    for (uint32_t rec = uni(blockIdx.x * ADDP_SIZE_WAVES + (threadIdx.x >> 6)); rec < P.n_rec; rec += gridDim.x * ADDP_SIZE_WAVES) {
        if (void_try) addp_leave(Q.A, rec, -1);
        else addp_size_one(Q, rec);
        __builtin_amdgcn_wave_barrier();
    }
}

#endif

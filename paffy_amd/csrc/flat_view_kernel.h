/*
 * flat_view_kernel.h -- the six sums of `paffy view` without `-a` (paf_stats_calc, impl/paf.c:236-260, on the record as
 * paf_encode_mismatches leaves it: impl/paf_view.c:166-178) on the pieces of the flat pass (flat_kernel.h), for the stage list
 * [ADD_MISMATCHES, STATS] of a context that has declared it will only ask for the sums (paffy_hip_stats_only).
 *
 * The sums of the encoded record need none of the encoder's products: an M op's matches are the set bits of the 16-column match masks
 * the count walk of the encoder computes anyway (mismatch_count_wave, record_kernel.h), its mismatches the other columns; = and X ops
 * pass through and count as what they say; I and D ops count as they do in the plain cigar. So there is one walk, no item scratch, no
 * new_ops[], no fill walk, no line plan -- and no limit on the ops other than M in a row (the item word's 62):
 *
 *   k_flat_parse     ops into the mirror, a summary per piece (any MODE: the walk counts what it needs itself)
 *   k_view_prep      one lane per record: k_add_prep without the scratch sizes -- the same records stay, the same AddPiece per piece
 *   k_view_count     one wave per piece: windows of 64 ops, the 16-column chunks of their M ops spread over the lanes; six sums per piece
 *   k_view_final     one lane per record: the pieces' sums into rec_stats[6 rec]; flat_done
 *
 * A record this does not take is left to the record kernels, which run the unchanged [ADD, STATS] code on it and report what there is
 * to report. Nothing here leaves ops or a line plan behind: the plan answers paffy_hip_plan_stats / _record_stats and nothing else.
 */
#ifndef PAFFY_FLAT_VIEW_KERNEL_H_
#define PAFFY_FLAT_VIEW_KERNEL_H_

struct ViewSum { /* per piece slot, written by k_view_count: the order of paf_stats_calc's arguments */
    uint32_t v[6]; /* matches, mismatches, I ops, D ops, I bases, D bases: a piece has at most 512 ops of at most 8 191 bases */
    uint32_t pad[2];
};
static_assert(sizeof(ViewSum) == 32, "two 16-byte stores");

struct ViewParams {
    AddParams A; /* pieces, sums, rec_bad, flat_done as the encoder uses them; no scratch, no new ops */
    ViewSum *vsum;
};

__global__ __launch_bounds__(256) void k_view_prep(ViewParams V) { add_prep_lane<false>(V.A); }

/* the count walk, one wave per piece: mismatch_count_wave's windows and item loop, with popcounts where that one stores item words */
__global__ __launch_bounds__(64 * ADD_WAVES) void k_view_count(ViewParams V) {
    const AddParams &A = V.A;
    const KParams &P = A.P;
    const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * ADD_WAVES;
    for (uint32_t slot = uni(blockIdx.x * ADD_WAVES + (threadIdx.x >> 6)); slot < A.n_piece_slots; slot += n_waves) {
        const AddPiece ap = A.pieces[slot];
        const uint32_t rec = uni(ap.rec);
        if (rec == FLAT_NO_CHUNK) continue;
        const RecMeta &m = P.meta[rec];
        uint32_t cnt = uni(A.sums[slot].cnt) & 0xffffu;
        if (cnt > FLAT_P_CAP) cnt = FLAT_P_CAP; /* never: such a piece is FLAT_F_IRREG */
        const uint16_t *ops = reinterpret_cast<const uint16_t *>(P.ops_mirror + (m.cg_off >> 1)) + uni(ap.op_base);
        const int32_t qi = P.rec_qseq[rec], ti = P.rec_tseq[rec];
        const int64_t qseq_len = P.seqs[qi].len, tseq_len = P.seqs[ti].len;
        const bool same = m.same_strand != 0;
        /* the - strand walks the complemented copy of the query downwards from qe - 1 */
        const uint8_t *T = P.seq_base + P.seqs[ti].off, *Q = (same ? P.seq_base : P.seq_comp) + P.seqs[qi].off;
        const int64_t ts = m.ts, q_first = same ? m.qs : m.qe - 1;
        uint32_t qpos = uni(ap.q_base), tpos = uni(ap.t_base); /* wave-uniform; below 2^30 (k_view_prep) */
        uint32_t acc[6] = {0, 0, 0, 0, 0, 0};
        bool bad = false;
        /* the op words of a window are requested a window ahead, as in mismatch_count_wave */
        uint32_t raw_ahead = lane < cnt ? ops[lane] : 0u;
        for (uint32_t base = 0; base < cnt; base += 64u) {
            const uint32_t i = base + lane;
            const uint32_t raw_now = raw_ahead;
            raw_ahead = 0;
            if (i + 64u < cnt) raw_ahead = ops[i + 64u];
            const bool valid = i < cnt;
            const uint32_t len = valid ? raw_now >> 3 : 0u, op = valid ? raw_now & 7u : (uint32_t)OP_I;
            const uint32_t dq = op != (uint32_t)OP_D ? len : 0u, dt = op != (uint32_t)OP_I ? len : 0u;
            const uint32_t qinc = wave_incl_scan_u32(dq), tinc = wave_incl_scan_u32(dt);
            const uint32_t qrel = qinc - dq, trel = tinc - dt; /* columns in front of this op, from the window's first */
            const int64_t tj0 = ts + (int64_t)tpos, qoff0 = same ? q_first + (int64_t)qpos : q_first - (int64_t)qpos;
            bool is_m = valid && op == (uint32_t)OP_M && len > 0;
            if (is_m) { /* the range test of mismatch_count_wave */
                const int64_t tj = tj0 + trel, qoff = same ? qoff0 + qrel : qoff0 - qrel;
                const bool in_range = tj >= 0 && tj + len <= tseq_len && (same ? (qoff >= 0 && qoff + len <= qseq_len) : (qoff < qseq_len && qoff - ((int64_t)len - 1) >= 0));
                if (!in_range) {
                    bad = true;
                    is_m = false;
                }
            }
            qpos += wave_last_u32(qinc);
            tpos += wave_last_u32(tinc);
            /* the ops that pass through the encoder: they count as what they say */
            acc[0] += op == (uint32_t)OP_EQ ? len : 0u;
            acc[1] += op == (uint32_t)OP_X ? len : 0u;
            acc[2] += valid && op == (uint32_t)OP_I ? 1u : 0u;
            acc[3] += op == (uint32_t)OP_D ? 1u : 0u;
            acc[4] += op == (uint32_t)OP_I ? len : 0u;
            acc[5] += op == (uint32_t)OP_D ? len : 0u;
            /* items: the chunks of 16 columns of the window's M ops, 64 at a time, lane = chunk */
            const uint32_t nch = is_m ? (len + 15u) >> 4 : 0u;
            const uint32_t iinc = wave_incl_scan_u32(nch);
            const uint32_t ioff = iinc - nch, n_items = wave_last_u32(iinc);
            const uint8_t *Tw = T + tj0, *Qw = Q + qoff0;
            for (uint32_t c0 = 0; c0 < n_items; c0 += 64u) {
                const uint32_t c = c0 + lane;
                uint32_t ol = 0; /* the op of item c: the last lane whose first item is <= c */
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1) {
                    const uint32_t cand = ol + step;
                    const uint32_t vv = __shfl(ioff, (int)(cand & 63u));
                    if (cand < 64 && vv <= c) ol = cand;
                }
                const uint32_t olen = __shfl(len, (int)ol), o_first = __shfl(ioff, (int)ol);
                const uint32_t oq = __shfl(qrel, (int)ol), ot = __shfl(trel, (int)ol); /* by every lane: the source lanes must be live */
                if (c < n_items) { /* every item is a chunk of an M op inside both sequences */
                    const uint32_t k = (c - o_first) << 4;
                    const uint32_t nb = olen - k < 16u ? olen - k : 16u;
                    const uint32_t mk = match_mask16(P.seq_comp, same ? Qw + (oq + k) : Qw - (oq + k), Tw + (ot + k), same) & ((1u << nb) - 1u);
                    const uint32_t eq = (uint32_t)__popc(mk);
                    acc[0] += eq;
                    acc[1] += nb - eq;
                }
            }
        }
        wave_sum6_u32(acc);
        const bool any_bad = __any(bad);
        if (lane == 0) {
            uint4 *o = reinterpret_cast<uint4 *>(V.vsum + slot);
            o[0] = make_uint4(acc[0], acc[1], acc[2], acc[3]);
            o[1] = make_uint4(acc[4], acc[5], 0u, 0u);
            if (any_bad) A.rec_bad[rec] = 1; /* bases outside a sequence: the record kernels report it */
        }
    }
}

/* one lane per record: the sums of its pieces; nothing to emit */
__global__ __launch_bounds__(256) void k_view_final(ViewParams V) {
    const AddParams &A = V.A;
    const KParams &P = A.P;
    const uint32_t rec = blockIdx.x * 256u + threadIdx.x;
    if (rec >= P.n_rec) return;
    const bool done = A.flat_done[rec] == 2 && !A.rec_bad[rec];
    if (done) {
        const RecMeta &m = P.meta[rec];
        const uint32_t cg_off = m.cg_off, cg_end = cg_off + m.cg_len;
        const uint32_t np = ((cg_end - 1u) >> FLAT_TILE_SHIFT) - (cg_off >> FLAT_TILE_SHIFT) + 1u;
        const uint32_t slot0 = (cg_off >> FLAT_TILE_SHIFT) + rec;
        int64_t s[6] = {0, 0, 0, 0, 0, 0};
        for (uint32_t p = 0; p < np; p++) {
            const uint4 a = reinterpret_cast<const uint4 *>(V.vsum + slot0 + p)[0], b = reinterpret_cast<const uint4 *>(V.vsum + slot0 + p)[1];
            s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w; s[4] += b.x; s[5] += b.y;
        }
        int64_t *o = P.rec_stats + 6ull * rec;
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = s[k];
        RecPlan *plan = static_cast<RecPlan *>(P.rec_plan) + rec; /* as for a record a filter dropped: nothing to write */
        P.status[rec] = (uint32_t)KLASS_LDS << 16;
        P.err_aux[rec] = 0;
        P.n_ops[rec] = 0;
        plan->flags = 128u;
        plan->n = 0;
    } else {
        P.status[rec] = 0;
        atomicAdd(&P.info->flat_legacy, 1u);
    }
    A.flat_done[rec] = done ? 1 : 0;
    P.out_len[rec] = 0;
    P.out_rows[rec] = 0;
}

#endif

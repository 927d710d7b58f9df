/*
 * flat_remove_kernel.h -- `paffy add_mismatches -a` (paf_remove_mismatches, impl/paf.c:786-809; the command loop impl/paf_add_mismatches.c:109-139)
 * on the pieces of the flat pass (flat_kernel.h), for the pipe that consists of that command alone.
 *
 * The record kernels (merge_match_runs, record_kernel.h) merge a record inside the workgroup that holds its ops in LDS, and a record whose
 * ops fit no LDS store in the arena class, one workgroup walking 8-byte ops in HBM. The command's input is the longest text of the
 * pipeline (whole alignment sets, every M op cut into = and X runs by add_mismatches), so here the work item is the piece, as in
 * flat_add_kernel.h. What is new against the encoder: a merged run does not stop at a piece boundary. Every piece therefore first says
 * what it looks like from outside (its edges), a lane per record passes the open runs along the pieces' edges, and only then the
 * pieces write: a run is written by the piece that holds its head, with the bases the later pieces add to it.
 *
 *   k_flat_parse<0>  ops into the mirror, a summary per piece (= and X are this command's normal input: FLAT_F_NONPLAIN is not looked at)
 *   k_rm_prep        one lane per record: what the flat pass keeps, paf_check on the parsed sums (merging changes neither sum), per
 *                    piece its record and the ops in front of it
 *   k_rm_edges       one wave per piece: does its first op continue a run (the op in front of it in the mirror is M, = or X), the
 *                    bases of its leading M/=/X ops up to its first I or D, whether it holds no I or D at all, the bases of the run
 *                    open at its end, its run heads (an op that is not "M/=/X behind M/=/X"): the ops it becomes
 *   k_rm_carry       one lane per record, over the edges only: the bases the run open at a piece's end gains from the pieces behind it
 *                    (a piece without I or D passes the run on)
 *   (scan)           places of the pieces' new ops: the new cigars of all records stand back to back in new_ops[]
 *   k_rm_fill        one wave per piece, windows of 64 ops taken from the piece's last to its first (so that a run's tail is known
 *                    when its head is met): a head of a run writes one M op of the whole run's length, I and D ops are copied
 *                    (3I4I stays two ops: the reference merges M/=/X only); the bytes of the new ops' text
 *   k_add_final      (flat_add_kernel.h, unchanged) one lane per record: the line's length, the plan for the line writers, the
 *                    segments of the lines of more than PAFFY_ROWS_MAX_OPS new ops; a piece that becomes no op at all adds nothing
 *                    to a segment
 *
 * A record this does not take (what the flat pass leaves, a failing check, sums beyond 2^30, a merged run of 2^29 bases or more -- the
 * 4-byte op holds 29 bits of length) is left to the record kernels, which report what there is to report.
 */
#ifndef PAFFY_FLAT_REMOVE_KERNEL_H_
#define PAFFY_FLAT_REMOVE_KERNEL_H_

#define RM_F_CONT 0x80000000u    /* the piece's first op continues a run begun in front of the piece */
#define RM_F_NOINDEL 0x40000000u /* the piece holds no I or D op */
#define RM_CARRY_MASK 0x3fffffffu
#define RM_WINDOWS (FLAT_P_CAP / 64u)

struct RmEdge {
    uint32_t lead;  /* bases of the piece's M/=/X ops in front of its first I or D */
    uint32_t trail; /* bases of its M/=/X ops behind its last I or D (all of them in a piece without) */
};

struct RmParams {
    AddParams A;     /* pieces, new_cnt / new_off / new_ops, text_cnt, rec_bad, flat_done as the encoder uses them (k_add_final reads them) */
    RmEdge *edges;   /* per piece slot, k_rm_edges */
    uint32_t *carry; /* per piece slot: RM_F_* of k_rm_edges | the bases the run open at the piece's end gains behind it (k_rm_carry; below 2^30) */
};

__device__ __forceinline__ bool rm_match_type(uint32_t code) { return ((0x19u >> code) & 1u) != 0; } /* M 0, = 3, X 4 */
/* the lanes of a window of a piece of cnt ops that hold an op (wave-uniform) */
__device__ __forceinline__ uint64_t rm_valid(uint32_t cnt, uint32_t i0) { return cnt - i0 >= 64u ? ~0ull : (1ull << (cnt - i0)) - 1ull; }
/* the run heads among them: M = the lanes with an M/=/X op, cin = the op in front of lane 0 is one */
__device__ __forceinline__ uint64_t rm_heads(uint64_t V, uint64_t M, uint32_t cin) { return V & ~(M & ((M << 1) | (uint64_t)cin)); }
__device__ __forceinline__ const uint16_t *rm_piece_ops(const KParams &P, uint32_t rec, uint32_t op_base) {
    return reinterpret_cast<const uint16_t *>(P.ops_mirror + (P.meta[rec].cg_off >> 1)) + op_base;
}

/* one lane per record: is the record this pass's, where do its pieces stand */
__global__ __launch_bounds__(256) void k_rm_prep(RmParams R) {
    const AddParams &A = R.A;
    const KParams &P = A.P;
    const uint32_t rec = blockIdx.x * 256u + threadIdx.x;
    if (rec >= P.n_rec) return;
    A.flat_done[rec] = 0;
    A.rec_bad[rec] = 0;
    const RecMeta &m = P.meta[rec];
    if (m.err || !m.has_cg || m.cg_len == 0) return;
    const uint32_t cg_off = m.cg_off, cg_end = cg_off + m.cg_len;
    const uint32_t np = ((cg_end - 1u) >> FLAT_TILE_SHIFT) - (cg_off >> FLAT_TILE_SHIFT) + 1u;
    const uint32_t slot0 = (cg_off >> FLAT_TILE_SHIFT) + rec;
    uint64_t n = 0, q = 0, t = 0;
    uint32_t flags = 0;
    for (uint32_t p = 0; p < np; p++) { /* first: may the record stay? */
        const FlatPre s = lane_piece(A.sums, slot0 + p);
        flags |= s.cnt >> 16;
        n += s.cnt & 0xffffu;
        q += (uint64_t)s.m + s.x - s.del;
        t += (uint64_t)s.m + s.x - s.ins;
    }
    if ((flags & FLAT_F_IRREG) || n == 0 || q >= (1ull << 30) || t >= (1ull << 30) || n >= (1ull << 31)) return;
    /* paf_check (impl/paf_add_mismatches.c:131) on the record as parsed: a merged run is as long as its ops together, so the merged
       record passes or fails with this one; a failing record is the record kernels' to report */
    if (m.qs < 0 || m.qs >= m.qlen || m.qs > m.qe || m.qe > m.qlen || m.ts < 0 || m.ts >= m.tlen || m.ts > m.te || m.te > m.tlen || (int64_t)q != m.qe - m.qs ||
        (int64_t)t != m.te - m.ts)
        return;
    uint32_t nb = 0;
    for (uint32_t p = 0; p < np; p++) {
        AddPiece ap;
        ap.op_base = nb; ap.q_base = 0; ap.t_base = 0; ap.rec = rec;
        A.pieces[slot0 + p] = ap;
        nb += A.sums[slot0 + p].cnt & 0xffffu;
    }
    A.flat_done[rec] = 2; /* in progress: k_add_final decides */
}

/* one wave per piece: what the piece looks like from outside, and the ops it becomes */
__global__ __launch_bounds__(64 * ADD_WAVES) void k_rm_edges(RmParams R) {
    const AddParams &A = R.A;
    const KParams &P = A.P;
    const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * ADD_WAVES;
    for (uint32_t slot = uni(blockIdx.x * ADD_WAVES + (threadIdx.x >> 6)); slot < A.n_piece_slots; slot += n_waves) {
        const uint32_t rec = uni(A.pieces[slot].rec);
        if (rec == FLAT_NO_CHUNK) continue;
        const uint32_t op_base = uni(A.pieces[slot].op_base);
        uint32_t cnt = uni(A.sums[slot].cnt) & 0xffffu;
        if (cnt > FLAT_P_CAP) cnt = FLAT_P_CAP; /* never: such a piece is FLAT_F_IRREG */
        const uint16_t *ops = rm_piece_ops(P, rec, op_base);
        const uint32_t cont = op_base ? (rm_match_type(uni(ops[-1]) & 7u) ? 1u : 0u) : 0u;
        uint32_t lead = 0, trail = 0, heads = 0, cin = cont;
        bool seen = false; /* an I or D so far */
        for (uint32_t i0 = 0; i0 < cnt; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const uint32_t w = i < cnt ? ops[i] : 0xffffu;
            const bool mt = i < cnt && rm_match_type(w & 7u);
            const uint64_t M = __ballot(mt), V = rm_valid(cnt, i0), ID = V & ~M;
            heads += (uint32_t)__popcll(rm_heads(V, M, cin));
            cin = (uint32_t)(M >> 63);
            const uint32_t mlen = mt ? w >> 3 : 0u;
            if (ID == 0) {
                const uint32_t tot = wave_sum_u32(mlen);
                if (!seen) lead += tot;
                trail += tot;
            } else {
                const uint32_t first = (uint32_t)__ffsll((long long)ID) - 1u, last = 63u - (uint32_t)__clzll((long long)ID);
                if (!seen) lead += wave_sum_u32(lane < first ? mlen : 0u);
                trail = wave_sum_u32(lane > last ? mlen : 0u);
                seen = true;
            }
        }
        if (lane == 0) {
            RmEdge e;
            e.lead = lead; e.trail = trail;
            R.edges[slot] = e;
            R.carry[slot] = (cont ? RM_F_CONT : 0u) | (seen ? 0u : RM_F_NOINDEL);
            A.new_cnt[slot] = heads;
        }
    }
}

/* one lane per record, from its last piece to its first: what the run open at a piece's end gains from the pieces behind it */
__global__ __launch_bounds__(256) void k_rm_carry(RmParams R) {
    const AddParams &A = R.A;
    const KParams &P = A.P;
    const uint32_t rec = blockIdx.x * 256u + threadIdx.x;
    if (rec >= P.n_rec || A.flat_done[rec] != 2) return;
    const RecMeta &m = P.meta[rec];
    const uint32_t cg_off = m.cg_off, cg_end = cg_off + m.cg_len;
    const uint32_t np = ((cg_end - 1u) >> FLAT_TILE_SHIFT) - (cg_off >> FLAT_TILE_SHIFT) + 1u;
    const uint32_t slot0 = (cg_off >> FLAT_TILE_SHIFT) + rec;
    uint32_t gain = 0; /* below 2^30: the record's aligned bases are (k_rm_prep) */
    for (uint32_t p = np; p-- > 0;) {
        const uint32_t f = R.carry[slot0 + p] & ~RM_CARRY_MASK;
        const RmEdge e = R.edges[slot0 + p];
        R.carry[slot0 + p] = f | gain;
        gain = (f & RM_F_CONT) ? e.lead + ((f & RM_F_NOINDEL) ? gain : 0u) : 0u;
    }
}

/* one wave per piece: the new ops and the bytes of their text */
__global__ __launch_bounds__(64 * ADD_WAVES) void k_rm_fill(RmParams R) {
    const AddParams &A = R.A;
    const KParams &P = A.P;
    const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * ADD_WAVES;
    for (uint32_t slot = uni(blockIdx.x * ADD_WAVES + (threadIdx.x >> 6)); slot < A.n_piece_slots; slot += n_waves) {
        const uint32_t rec = uni(A.pieces[slot].rec);
        if (rec == FLAT_NO_CHUNK) continue;
        const uint32_t op_base = uni(A.pieces[slot].op_base);
        uint32_t cnt = uni(A.sums[slot].cnt) & 0xffffu;
        if (cnt > FLAT_P_CAP) cnt = FLAT_P_CAP;
        const uint32_t fl = uni(R.carry[slot]), n_new = uni(A.new_cnt[slot]);
        const uint64_t at = ((uint64_t)uni((uint32_t)(A.new_off[slot] >> 32)) << 32) | uni((uint32_t)A.new_off[slot]);
        uint32_t text = 0;
        bool wide = false;
        if (cnt && at + n_new <= A.new_cap) {
            const uint16_t *ops = rm_piece_ops(P, rec, op_base);
            uint32_t w[RM_WINDOWS]; /* the ops of the piece's windows, and which of them are M/=/X */
            uint64_t M[RM_WINDOWS];
#pragma unroll
            for (uint32_t k = 0; k < RM_WINDOWS; k++) {
                const uint32_t i = 64u * k + lane;
                w[k] = i < cnt ? ops[i] : 0xffffu;
                M[k] = __ballot(i < cnt && rm_match_type(w[k] & 7u));
            }
            uint32_t hb = n_new; /* the heads in front of the window: k_rm_edges counted the piece's */
            uint32_t after = fl & RM_CARRY_MASK; /* what the run open at the window's end gains behind the window */
#pragma unroll
            for (int k = (int)RM_WINDOWS - 1; k >= 0; k--) {
                if (64u * (uint32_t)k >= cnt) continue; /* wave-uniform */
                const uint32_t nv = cnt - 64u * (uint32_t)k < 64u ? cnt - 64u * (uint32_t)k : 64u;
                const uint64_t Mk = M[k];
                const uint32_t cin = k == 0 ? fl >> 31 : (uint32_t)(M[k > 0 ? k - 1 : 0] >> 63);
                const uint64_t H = rm_heads(rm_valid(cnt, 64u * (uint32_t)k), Mk, cin);
                const bool mt = (Mk >> lane) & 1ull, head = (H >> lane) & 1ull;
                hb -= (uint32_t)__popcll(H);
                const uint32_t len = w[k] >> 3, mlen = mt ? len : 0u;
                const uint32_t S = wave_incl_scan_u32(mlen);
                /* the lane's run ends in front of the first lane above it without an M/=/X op (lanes past the piece's end hold none) */
                const uint64_t z = ~Mk & ((~0ull << lane) << 1);
                const uint32_t fz = z ? (uint32_t)__ffsll((long long)z) - 1u : 64u;
                const uint32_t Se = (uint32_t)__shfl((int)S, (int)(fz - 1u));
                const uint32_t total = Se - S + mlen + (fz >= nv ? after : 0u);
                wide = wide || (head && mt && total >= (1u << 29));
                const uint32_t idx = hb + (uint32_t)__popcll(H & ((1ull << lane) - 1ull));
                const uint32_t val = mt ? total : len;
                if (head && idx < n_new) A.new_ops[at + idx] = mt ? (total << 3) | (uint32_t)OP_M : (uint32_t)w[k];
                const uint32_t dl = dec_len_short(val);
                text += head ? dl + 1u : 0u;
                /* for the window in front: this window's leading M/=/X ops, and what follows them when it holds nothing else */
                const uint64_t z0 = ~Mk;
                const uint32_t f0 = uni(z0 ? (uint32_t)__ffsll((long long)z0) - 1u : 64u);
                after = f0 ? lane_val(S, f0 - 1u) + (f0 >= nv ? after : 0u) : 0u;
            }
            text = wave_sum_u32(text);
        }
        const bool any_wide = __any(wide) != 0;
        if (lane == 0) {
            A.text_cnt[slot] = text;
            if (any_wide) A.rec_bad[rec] = 1; /* a merged run of 2^29 bases or more: the record kernels' 8-byte ops */
        }
    }
}

#endif

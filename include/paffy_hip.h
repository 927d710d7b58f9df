/*
 * paffy_hip.h -- C-ABI of the MI355X (gfx950) PAF hot path.
 *
 * Boundary: the reference has no FFI; its hot path is the per-command loop
 *     while ((paf = paf_read_with_buffer(..)) != NULL) { <transform>; paf_check; paf_write_with_buffer; }
 * in impl/paf_{shatter,invert,trim,add_mismatches}.c and the whole-file body of
 * impl/paf_tile.c. Each entry point below replaces that loop for a whole batch of PAF text
 * at once; the host drivers (host/paffy_*.c, same `paffy <cmd>` CLI and flags) call nothing
 * else. Signatures are plain pointers and sizes: no HIP or torch types.
 *
 * Data stays text at the boundary (the PAF line grammar of impl/paf.c:317-389 is the wire
 * format between paffy processes), so a batch is: device pointer to '\n'-separated lines in,
 * device pointer to the output lines out, byte-exact to what the reference command(s) write.
 *
 * Two-phase protocol, mirroring paf_estimate_buffer_size -> realloc -> paf_write_to_buffer
 * (impl/paf.c:391-406): paffy_hip_plan() parses and transforms the batch and reports the exact
 * output size and the first failing record; paffy_hip_emit() writes the bytes.
 */
#ifndef PAFFY_HIP_H_
#define PAFFY_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct paffy_hip_ctx paffy_hip_ctx;

/* One stage = one reference command in a `paffy a | paffy b | ...` chain. */
enum {
    PAFFY_INVERT = 1,            /* impl/paf_invert.c:84-89: paf_invert, paf_check, write            */
    PAFFY_TRIM_IDENTITY = 2,     /* impl/paf_trim.c:117-119: paf_trim_unreliable_tails(p0=-r, p1=-t)  */
    PAFFY_TRIM_FIXED = 3,        /* impl/paf_trim.c:120-122: paf_trim_end_fraction(p1=-t)             */
    PAFFY_SHATTER = 4,           /* impl/paf_shatter.c:88-95: paf_shatter, write each block (last stage only) */
    PAFFY_ADD_MISMATCHES = 5,    /* impl/paf_add_mismatches.c:113-131: paf_encode_mismatches          */
    PAFFY_REMOVE_MISMATCHES = 6, /* impl/paf_add_mismatches.c:110-112: paf_remove_mismatches          */
    PAFFY_PASS = 7,              /* paf_read -> paf_write only (normalises tags, impl/paf.c:317-389)  */
    PAFFY_FILTER = 8,            /* impl/paf_filter.c:120-156: records failing the thresholds of paffy_hip_set_filter vanish */
    PAFFY_STATS = 10,            /* paf_stats_calc(.., zero_counts = 0) of every record into the plan's running sums (the aggregate of
                                    `paffy view -s`, impl/paf_view.c:163-168); the record passes on unchanged. See paffy_hip_plan_stats() */
    PAFFY_TRIM_ENDS = 9,         /* paf_trim_ends(paf, n), impl/paf.c:575-598: n aligned bases off each end; n = the 64 bits of (p0, p1),
                                    see paffy_stage_trim_ends(); then paf_check like the other trims */
    PAFFY_CHECK = 11,            /* paf_check alone (impl/paf.c:427-461): the record passes on unchanged or fails */
    PAFFY_DECHUNK = 12,          /* impl/paf_dechunk.c:24-37,114-118: names "name|length|chunk start" decoded (decode_fasta_header, impl/paf.c:716-731),
                                    the chunk start added to start and end, length = the decoded length; then paf_check. The first stage only,
                                    any list that fuses today may follow it; p0 != 0: fix the query side, p1 != 0: the target side
                                    (paffy_stage_dechunk()) */
    PAFFY_UPCONVERT = 13         /* impl/paf_upconvert.c:26-66,148-153: each side that falls in an interval of paffy_hip_set_intervals is
                                    renamed "name|length|start" and shifted into it; paf_check on the coordinates; the cigar text is not
                                    parsed and is written verbatim (paf_read(.., 0)). A stage list of its own */
};
/* OR-ed into a transform's kind: without the paf_check that the command loops run after it (impl/paf_invert.c:84-89) -- what the
 * library functions of inc/paf.h do (paf_invert, paf_trim_ends ... check nothing, impl/paf.c:463-598) */
#define PAFFY_NO_CHECK 0x100
#define PAFFY_MAX_STAGES 8

typedef struct {
    int32_t kind;
    float p0; /* trim: trim_by_identity_fraction, a float as in impl/paf_trim.c:16 (default 0.05) */
    float p1; /* trim: trim_end_fraction, a float as in impl/paf_trim.c:14 (default 1.0)          */
} paffy_stage;

/* PAFFY_TRIM_ENDS carries its int64 argument in the two float slots, bit for bit. */
static inline paffy_stage paffy_stage_trim_ends(int64_t end_bases) {
    paffy_stage s;
    union { int64_t i; float f[2]; } u;
    u.i = end_bases;
    s.kind = PAFFY_TRIM_ENDS;
    s.p0 = u.f[0];
    s.p1 = u.f[1];
    return s;
}

/* `paffy dechunk` (-q: fix_target = 0, -t: fix_query = 0) */
static inline paffy_stage paffy_stage_dechunk(int fix_query, int fix_target) {
    paffy_stage s;
    s.kind = PAFFY_DECHUNK;
    s.p0 = fix_query ? 1.0f : 0.0f;
    s.p1 = fix_target ? 1.0f : 0.0f;
    return s;
}

/* Record-level failures: what the reference turns into st_errAbort / assert / a crash. */
enum {
    PAFFY_OK = 0,
    PAFFY_ERR_FEW_FIELDS = 1,          /* impl/paf.c:144-172 (NULL token dereferenced)  */
    PAFFY_ERR_STRAND = 2,              /* impl/paf.c:155-157 st_errAbort                */
    PAFFY_ERR_TP_ASSERT = 3,           /* impl/paf.c:190 assert                         */
    PAFFY_ERR_CIGAR_CHAR = 4,          /* impl/paf.c:102 st_errAbort                    */
    PAFFY_ERR_CHECK_QSTART = 5,        /* impl/paf.c:428                                */
    PAFFY_ERR_CHECK_QEND = 6,          /* impl/paf.c:431                                */
    PAFFY_ERR_CHECK_TSTART = 7,        /* impl/paf.c:434                                */
    PAFFY_ERR_CHECK_TEND = 8,          /* impl/paf.c:437                                */
    PAFFY_ERR_CHECK_CIGAR_Q = 9,       /* impl/paf.c:452                                */
    PAFFY_ERR_CHECK_CIGAR_T = 10,      /* impl/paf.c:456                                */
    PAFFY_ERR_SHATTER_ZERO_LEN = 11,   /* impl/paf.c:635 assert                         */
    PAFFY_ERR_SHATTER_BAD_OP = 12,     /* impl/paf.c:650 assert                         */
    PAFFY_ERR_SHATTER_END = 13,        /* impl/paf.c:654-660 asserts                    */
    PAFFY_ERR_TRIM_IDENTITY_ASSERT = 14, /* impl/paf.c:952 assert                       */
    PAFFY_ERR_TRIM_FIXED_ASSERT = 15,  /* impl/paf.c:591 assert                         */
    PAFFY_ERR_NULL_CIGAR = 16,         /* impl/paf.c:520 (NULL cigar dereferenced)      */
    PAFFY_ERR_MISSING_QUERY_SEQ = 17,  /* impl/paf_add_mismatches.c:117-120 exit(1)     */
    PAFFY_ERR_MISSING_TARGET_SEQ = 18, /* impl/paf_add_mismatches.c:123-127 exit(1)     */
    PAFFY_ERR_TILE_ASSERT = 19,        /* impl/paf.c:685,698,708; impl/paf_tile.c:57,86,171 */
    PAFFY_ERR_SEQ_RANGE = 21,          /* paf_encode_mismatches would read outside a sequence */
    PAFFY_ERR_CHAIN_ASSERT = 22,       /* impl/chaining.c:275,278-281 asserts              */
    PAFFY_ERR_DECHUNK_HEADER = 23,     /* impl/paf.c:722,725 asserts: a name without "|length|start" (stage 0) */
    PAFFY_ERR_UPCONVERT_ASSERT = 24,   /* impl/paf_upconvert.c:33 assert: a side starts inside an interval and ends beyond it */
    PAFFY_ERR_FAFFY_ASSERT = 25,       /* faffy asserts: chunk size <= overlap (impl/fasta_chunk.c:74), extract bounds (impl/fasta_extract.c:211)
                                          or a BED line of fewer than 3 tokens, merge order / gap / header (impl/fasta_merge.c) */
    PAFFY_ERR_FAFFY_BASE = 26,         /* chunk / extract: a base whose tolower() is not a, c, g, t or n (assert) */
    PAFFY_ERR_FAFFY_MISSING_SEQ = 27   /* extract: a BED name without a sequence, "Missing sequence: %s" (st_errAbort, exit 1) */
};

/* Call-level failures (negative return values). */
enum {
    PAFFY_E_HIP = -1,         /* a HIP runtime call failed; see paffy_hip_last_error()         */
    PAFFY_E_ARG = -2,         /* bad argument (NULL, misaligned pointer, a batch of 2 GiB - 64 bytes or more) */
    PAFFY_E_UNSUPPORTED = -3, /* stage list this build cannot fuse (run the stages one by one)  */
    PAFFY_E_CAPACITY = -4,    /* output buffer smaller than the planned size                   */
    PAFFY_E_STATE = -5,       /* emit without a successful plan                                */
    PAFFY_E_HEADER = -6       /* paffy_hip_set_intervals: a FASTA header without "|length|start" (the reference asserts) */
};

typedef struct {
    int32_t code;   /* PAFFY_ERR_*, 0 = none */
    int32_t stage;  /* index into the stage list, -1 = while parsing */
    int64_t record; /* zero-based record in the batch */
    int64_t aux;    /* offending character for STRAND / TP / CIGAR_CHAR */
} paffy_error;

typedef struct {
    int64_t n_records; /* lines in the batch                                              */
    int64_t n_rows;    /* lines emit will write                                           */
    int64_t in_bytes;
    int64_t out_bytes; /* bytes emit will write: all records before the first failing one */
    paffy_error error; /* first failure in stream order (code 0 = none)                   */
} paffy_plan_info;

/* Lifetime. `device` < 0 keeps the current HIP device. */
int paffy_hip_create(paffy_hip_ctx **ctx, int device);
void paffy_hip_destroy(paffy_hip_ctx *ctx);
/* Stream all kernels of this context are launched on (a hipStream_t; NULL = default stream). */
int paffy_hip_set_stream(paffy_hip_ctx *ctx, void *hip_stream);

/*
 * plan: index the lines of d_in[0, in_len) (16-byte aligned device pointer; the allocation
 * must be readable up to the next multiple of 16; in_len < 2 GiB - 64: offsets inside a batch are 32 bits --
 * a stream command takes any input as a sequence of batches, tile / to_bed through the begin / add / run calls below),
 * parse every record, run the stage list,
 * and compute each record's exact output size. Blocks until the numbers are known.
 * A final line without '\n' is a record (impl/paf.c:213).
 */
int paffy_hip_plan(paffy_hip_ctx *ctx, const paffy_stage *stages, int32_t n_stages, const void *d_in, int64_t in_len,
                   paffy_plan_info *info);

/*
 * tile_plan: `paffy tile` (impl/paf_tile.c:156-178) over the whole batch: every record gets its
 * tile level (tl) from per-base coverage counters of its QUERY sequence, visiting records by
 * (s1 desc, AS desc, input order); the output lists all records in that order with the cigar text
 * unchanged. A failing record means no output at all. Followed by paffy_hip_emit().
 */
int paffy_hip_tile_plan(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, paffy_plan_info *info);
/*
 * The same over an input of any size (the reference reads the whole file, read_pafs, impl/paf.c:492-499): begin, add every batch
 * of text (each a whole number of lines, < 2 GiB - 64 bytes, 16-byte aligned; it must stay where it is until the output has been
 * emitted: the lines are written from it), run. Records are ordered and grouped across all batches; info->error.record counts
 * records from the first batch on. Followed by paffy_hip_emit() or paffy_hip_emit_lines().
 */
int paffy_hip_tile_begin(paffy_hip_ctx *ctx);
int paffy_hip_tile_add(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len);
int paffy_hip_tile_run(paffy_hip_ctx *ctx, paffy_plan_info *info);
/*
 * After a tile run: five int64 per output line, in output order, into device memory -- chain_score, score, input record, bytes of
 * the line, tile level. This is what the ranks of a `paffy tile` sharded by query sequence exchange (an all-gather of 40 bytes per
 * record) to find the place of their lines in the ordered output. Returns the number of lines or a negative error.
 */
int64_t paffy_hip_tile_keys(paffy_hip_ctx *ctx, int64_t cap_lines, void *d_keys);
/*
 * Sharding `paffy tile` by query sequence across GPUs (what `paffy split_file -q` does with files in the reference
 * pipeline, tests/paf_pipeline_test.sh:42, impl/paf_split_file.c:142-173). Names travel as 64-bit hashes.
 *   query_names:    the distinct query names of a batch (hashes[], host) and the bytes of their lines (weights[], host): what a
 *                   partitioner balances. Returns their number (<= cap) or a negative error. The line index built here is KEPT for
 *                   the batch (keyed by d_in and in_len, up to 64 batches) and consumed by the split of the same batch. Contract:
 *                   the bytes of the batch must not change between its query_names and its split -- the kept index is not
 *                   re-validated against the text. A batch that will not be split after all: paffy_hip_drop_index(ctx, d_in)
 *                   (d_in NULL: every kept index). Kept indexes are also dropped by any query_names / split call that fails and
 *                   by paffy_hip_tile_begin / _bed_begin / _chain_begin; paffy_hip_plan and the other index-building calls on the
 *                   same d_in drop that batch's entry.
 *   split_by_owner: the lines of the batch regrouped by part -- part = table_owner[i] for a query name with hash table_hash[i]
 *                   (ascending hashes; a name the table lacks goes to hash % n_parts) -- input order kept inside a part, every line
 *                   newline-terminated, into d_out (out_cap >= in_len + 1). part_bytes / part_records (host, n_parts each) say where
 *                   the parts end; d_rec_index (device, rec_index_cap int64, may be NULL) gets the batch index of every output line.
 *                   This is the send buffer of the all-to-all that gives every rank the records of its sequences.
 *   split_to:       the same, straight into a send buffer that gathers the parts of several batches per destination: part p's lines
 *                   go to d_out + part_dst[p], its record indices (+ rec_base: the batch's first global record) to
 *                   d_rec_index + rec_dst[p] (host arrays of n_parts byte / entry offsets; checked against out_cap / rec_index_cap
 *                   before anything is written: PAFFY_E_CAPACITY). No second copy of the text is needed to build the send buffer.
 *   scatter_lines:  line k = d_src[src_off[k], src_off[k + 1]) goes to d_dst + dst_off[k] (int64 offsets in device memory; n_lines + 1
 *                   source offsets): the ordered write once every line's place in the global output is known.
 */
int64_t paffy_hip_query_names(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int64_t cap, uint64_t *hashes, int64_t *weights);
/* the same, with the number of lines of every name (records[], host): with bytes AND records per name a caller can lay out the send
   buffer of the partition before it splits the first batch (paffy_hip_split_to) */
int64_t paffy_hip_query_names_counts(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int64_t cap, uint64_t *hashes, int64_t *weights, int64_t *records);
int paffy_hip_split_by_owner(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner,
                             int64_t n_table, void *d_out, int64_t out_cap, int64_t *part_bytes, int64_t *part_records, void *d_rec_index, int64_t rec_index_cap,
                             int64_t *n_records);
int paffy_hip_split_to(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int32_t n_parts, const uint64_t *table_hash, const uint32_t *table_owner,
                       int64_t n_table, void *d_out, int64_t out_cap, const int64_t *part_dst, const int64_t *rec_dst, int64_t rec_base, int64_t *part_bytes,
                       int64_t *part_records, void *d_rec_index, int64_t rec_index_cap, int64_t *n_records);
int paffy_hip_drop_index(paffy_hip_ctx *ctx, const void *d_in);
int paffy_hip_scatter_lines(paffy_hip_ctx *ctx, const void *d_src, const void *d_src_off, const void *d_dst_off, int64_t n_lines, void *d_dst);
/*
 * Lines [first, first + n) of a tile / dedupe plan into d_out, the first of them at d_out[0] (16-byte aligned): for hosts that
 * drain an output larger than their staging buffer. *bytes = what was written.
 */
int paffy_hip_emit_lines(paffy_hip_ctx *ctx, int64_t first, int64_t n, void *d_out, int64_t out_cap, int64_t *bytes);

/*
 * dedupe_plan: `paffy dedupe [-a]` (impl/paf_dedupe.c:117-143). A record is kept unless a record kept earlier -- in this
 * batch or in an earlier batch of the same context since the last paffy_hip_dedupe_reset -- has the same query name,
 * target name, strand and four coordinates (with check_inverse: or equals it with query and target swapped; paf_check
 * then runs on the record, as in the reference). Kept records are written in input order with the cigar text verbatim.
 * Keys are compared as 128-bit hashes of those fields (two independent 64-bit hashes). The selection runs on the device (sort by key,
 * first of every run, binary searches in the sorted keys of the earlier batches); the context's memory lives in HBM, 16 bytes per
 * record written. Followed by paffy_hip_emit().
 */
int paffy_hip_dedupe_plan(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int check_inverse, paffy_plan_info *info);
int paffy_hip_dedupe_reset(paffy_hip_ctx *ctx);
/* check_inverse value that keeps every record: `paf_read(.., 0)` -> `paf_write` (the normalised line, cigar text verbatim),
 * the read/write pair of `paffy split_file` (impl/paf_split_file.c:131-173). The context's dedupe memory is not touched. */
#define PAFFY_DEDUPE_KEEP_ALL 2

/*
 * `paffy split_file [-q] [-m min_length]` (impl/paf_split_file.c:142-170): the lines of a batch grouped by output file.
 *   split_begin: starts a run -- the contig is the query (by_query) or the target, min_length as -m -- and forgets the files of an
 *                earlier run. PAFFY_SPLIT_NARROW_SALT0 (environment, read here; anything but empty or "0") cuts the first name hash
 *                to two bits, so that a test gets the regrouping of colliding names to run.
 *   split_plan:  the normalised lines of paffy_hip_dedupe_plan(.., PAFFY_DEDUPE_KEEP_ALL, ..) -- every record in front of the first one
 *                that fails, which info->error reports as there -- regrouped: a group is a contig name with its "small" bit
 *                (min_length > 0 and the contig length on the record's own line < min_length), groups come in the order of their first
 *                record, lines inside a group keep input order. Names are grouped by a salted 64-bit hash and checked byte for byte; names
 *                that collide under eight salts: PAFFY_E_UNSUPPORTED. The file of every group is decided here, once per distinct (name,
 *                small bit) of the batch: a name's own file, or the current small_<k> file, which a new small contig joins unless there
 *                is none or its length would take the file's contig lengths past min_length. Groups of the batch that share a small_<k>
 *                file are merged, their lines in input order as the reference writes them. Followed by paffy_hip_emit (or _emit_lines,
 *                _plan_rows): every file's lines are one stretch of the output. Without a split_begin: PAFFY_E_STATE.
 *   split_groups: the stretches of the plan in output order, one per file that gets lines of the batch, in the order of the files' first
 *                records (cap smaller than their number: PAFFY_E_CAPACITY). file: dense id in opening order over the run; new_file: the
 *                batch opens it (open files in this order to open them in the reference's order); first_record: the batch's record behind
 *                the stretch's first line. Returns their number; PAFFY_E_STATE unless the last plan is a split plan.
 *   split_file_name: the file's name without the caller's prefix and ".paf" -- the contig name with '/' replaced by '_', or small_<k> --
 *                NUL-terminated into buf. Returns its length (cap <= length: PAFFY_E_CAPACITY, nothing written).
 *   split_file_count: files opened by the run so far. split_salt: the salt the last plan's grouping passed its byte check with.
 */
typedef struct {
    int64_t file, out_off, bytes, lines, first_record;
    int32_t new_file, is_small;
} paffy_split_group;
int paffy_hip_split_begin(paffy_hip_ctx *ctx, int by_query, int64_t min_length);
int paffy_hip_split_plan(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, paffy_plan_info *info);
int64_t paffy_hip_split_groups(paffy_hip_ctx *ctx, int64_t cap, paffy_split_group *groups);
int64_t paffy_hip_split_file_name(paffy_hip_ctx *ctx, int64_t file, char *buf, int64_t cap);
int64_t paffy_hip_split_file_count(paffy_hip_ctx *ctx);
int paffy_hip_split_salt(paffy_hip_ctx *ctx);

/*
 * Dedupe in parts: `paffy dedupe [-a]` sharded by KEY OWNER. "First seen wins" is a decision per class of records -- a class
 * is a key (the 128-bit hash of paffy_hip_dedupe_plan), with check_inverse a key and its swapped key, named by the smaller of the two --
 * so it needs a class's records in one place, not the input. A part is a context that holds any share of the records, each with a global
 * input number (rec_base + its index in the part's batch). Per ROUND (one batch per part) a part sends one 32-byte entry per record to
 * the part that owns the record's class, the owner answers one byte per entry, and the text never leaves the part that read it. The
 * concatenation of the parts' outputs in part order, round by round, is what one context writes for the same records in the order of
 * their global numbers, when the parts' shares are consecutive stretches of it.
 *   entry:       four 64-bit words -- class key hi, class key lo, global number (int64), flags: bit 0 the record's own key is its class
 *                key (its orientation), bit 1 its coordinates fail paf_check (impl/paf.c:427-438).
 *   owner:       a pure function of the class key and n_parts (shard.dedupe_owner mirrors it):
 *                    x = hi ^ lo;  x ^= x >> 33;  x *= 0xff51afd7ed558ccd;  x ^= x >> 33;  x *= 0xc4ceb9fe1a85ec53;  x ^= x >> 33;
 *                    owner = (x * n_parts) >> 64
 *                (64-bit arithmetic, the last product 128 bits wide).
 *   part_keys:   source side. Indexes and parses the batch as paffy_hip_dedupe_plan does and keeps that state for part_plan. Writes the
 *                entries of the records that parsed to d_entries (device, 16-byte aligned, cap_entries entries), grouped by owner:
 *                owner p's segment has part_counts[p] entries (host, n_parts values) and follows owner p - 1's; the order inside a segment
 *                is not defined (the entry carries its number). A record that does not parse has no entry: it is a failure of this
 *                part at its global number. *n_records = the batch's records. n_parts >= 1 as for paffy_hip_split_to. More entries than
 *                cap_entries: PAFFY_E_CAPACITY, found before anything is written; the round is then not begun.
 *   part_decide: owner side, once per round. n_entries entries of any parts, in any order, in device memory; d_verdicts gets one byte per
 *                entry, in the same order: bit 0 the record is written -- it has the lowest global number of its class in this round and
 *                the class is not in the owner's memory --, bit 1 the record fails: check_inverse, its own key was not found among the
 *                records written before it, and flag bit 1. The memory holds the classes this context declared written since the last
 *                paffy_hip_dedupe_reset, each with its head's orientation; "own key found" is: the class's written record (memory, or
 *                this round's head when it is another record) has the record's orientation. A record that is its own swap has own key =
 *                swapped key, as has every record of its class. The memory is separate from that of paffy_hip_dedupe_plan; reset clears
 *                both. A context may be source and owner at once: part_decide does not touch the round's source state.
 *   part_verdicts: source side. The verdict bytes of this part's entries in the order part_keys wrote them (the owners' answers, segment
 *                by segment; device memory, n_entries = the sum of part_counts). *first_bad_global = the lowest global number of this
 *                part that fails -- a record that did not parse or a verdict with bit 1 -- or -1.
 *   part_plan:   source side. first_bad_global: the minimum over all parts (-1: none). Plans the lines of this part's records with verdict
 *                bit 0 and a global number below first_bad_global, in input order, with the verbatim writer of paffy_hip_dedupe_plan;
 *                paffy_hip_emit, _emit_lines and _plan_rows (records: indices into the part's batch) work as after a dedupe plan. The
 *                part that holds the failing record reports it in info->error, error.record being the global number. With
 *                first_bad_global >= 0 the run is over in every part: until paffy_hip_dedupe_reset all four calls return PAFFY_E_STATE.
 * Order: part_keys, part_verdicts, part_plan per round; part_verdicts or part_plan out of turn: PAFFY_E_STATE. The round's state lies in
 * the context's index buffers: any other plan, and any call that indexes another batch (query_names, the split calls), ends the round.
 * With n_parts = 1 and one context the four calls write what paffy_hip_dedupe_plan writes.
 */
int paffy_hip_dedupe_part_keys(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int check_inverse, int64_t rec_base, int32_t n_parts, void *d_entries,
                               int64_t cap_entries, int64_t *part_counts, int64_t *n_records);
int paffy_hip_dedupe_part_decide(paffy_hip_ctx *ctx, const void *d_entries, int64_t n_entries, int check_inverse, void *d_verdicts);
int paffy_hip_dedupe_part_verdicts(paffy_hip_ctx *ctx, const void *d_verdicts, int64_t n_entries, int64_t *first_bad_global);
int paffy_hip_dedupe_part_plan(paffy_hip_ctx *ctx, int64_t first_bad_global, paffy_plan_info *info);

/*
 * bed_plan: `paffy to_bed` (impl/paf_to_bed.c:33-55, 166-190) over the whole batch: per-base coverage counters of every query
 * sequence (with include_inverted also of every target sequence, as the inverted record would count), written as maximal runs
 * "name start end value\n"; binary / exclude_unaligned / exclude_aligned / min_size are the reference's -b -e -f -m. Sequences come
 * in order of first appearance (the reference walks a hash table: no order defined). A failing record means no output at all.
 * Followed by paffy_hip_emit().
 */
typedef struct {
    int32_t binary, exclude_unaligned, exclude_aligned, include_inverted;
    int64_t min_size; /* default 1 */
} paffy_bed_opts;
int paffy_hip_bed_plan(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, const paffy_bed_opts *opts, paffy_plan_info *info);
/* to_bed over an input of any size, as a sequence of batches (see paffy_hip_tile_begin); the same opts for begin and run */
int paffy_hip_bed_begin(paffy_hip_ctx *ctx, const paffy_bed_opts *opts);
int paffy_hip_bed_add(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len);
int paffy_hip_bed_run(paffy_hip_ctx *ctx, const paffy_bed_opts *opts, paffy_plan_info *info);
/*
 * After a bed run: the per-base counters themselves (what get_alignment_count_array / increase_alignment_level_counts keep per
 * sequence, impl/paf.c:667-712). _sequences = how many sequences the run saw; they are numbered in order of first appearance.
 * _counts copies counters [start, end) of one of them to h_counts; with accumulate != 0 it adds them to the values already in
 * h_counts instead, on the GPU, stopping at INT16_MAX - 1 as the reference's increments do (impl/paf.c:701).
 */
int64_t paffy_hip_bed_sequences(paffy_hip_ctx *ctx);
int paffy_hip_bed_counts(paffy_hip_ctx *ctx, int64_t sequence, int64_t start, int64_t end, uint16_t *h_counts, int accumulate);

/*
 * to_bed in parts: `paffy to_bed` sharded by sequence. The counters are per sequence (2 bytes per base) and all records that
 * count on a sequence must meet in one context; with include_inverted a record counts on its query sequence AND on its target sequence
 * (impl/paf_to_bed.c:170-177), which may have different owners. So a line travels to owner(query name) and, when that is another part,
 * to owner(target name) too, every copy with a one-byte SIDE MASK: bit 0 = count the query side here, bit 1 = count the target side
 * (as the inverted record would). One copy with mask 3 where both owners coincide, copies with masks 1 and 2 otherwise, mask 1 always
 * without include_inverted. A line that does not parse far enough to have a target name goes with its query side only.
 *   side_names_counts: paffy_hip_query_names_counts over the names of the counted sides: per distinct name its hash and the bytes and
 *                lines of the records that name it as query or (include_inverted) as target -- the weights a partitioner balances. A
 *                record counts once per side (a line without a target name mentions its query name twice, the second time with no
 *                bytes). Without include_inverted this is exactly the query-name pass. The batch's index is kept as there.
 *   split_sides_count: bytes and lines every part gets of this batch under the owner table (ascending hashes, a name the table lacks
 *                goes to hash % n_parts, as paffy_hip_split_to): NOT the sums of the per-name counts, a line whose two names share an
 *                owner is sent once. Nothing is written and the batch's kept index stays, so a caller sizes its send buffer, its index
 *                array and its mask array exactly before it splits the first batch.
 *   split_sides_to: paffy_hip_split_to by sides: part p's lines go to d_out + part_dst[p] in input order, the global input index
 *                (+ rec_base) of every written line to d_rec_index + rec_dst[p] (int64, may be NULL) and its side mask to
 *                d_sides + rec_dst[p] (one byte per line). Destinations are checked against out_cap / rec_index_cap (entries of both
 *                arrays) before anything is written: PAFFY_E_CAPACITY. A failing call drops every kept index.
 *   bed_add_sides: paffy_hip_bed_add with one mask byte per line of the batch (d_sides: device memory, read before the call returns).
 *                An entry whose side is masked off bumps nothing, creates no sequence, takes no part in the length assert
 *                (impl/paf.c:675-688) and raises no failure of its own; a line that does not parse is still reported. With
 *                include_inverted = 0 only bit 0 is looked at. d_sides NULL: every side -- a run of NULL masks only is paffy_hip_bed_add.
 *   bed_failure_side: after a bed run that reported a failure: 0 = found on the record's query side, 1 = on its target side, -1 = the
 *                line did not parse (or there is no failure). Of a record's failures one context reports the first of (parse, query
 *                side, target side); parts are compared by (global record, that order).
 *   bed_sequence_keys: after a bed run without failure: three int64 per sequence into device memory, in the run's order of first
 *                appearance -- the local entry it first appeared with (2 * record + side; record counts the lines of the run's batches
 *                in the order they were added), the bytes of its block of BED lines, the number of those lines. A sequence whose lines
 *                are all excluded has 0 bytes and still has a key. The emitted output is the blocks back to back in this order, so
 *                paffy_hip_scatter_lines places blocks as it places lines. Returns the number of sequences.
 * paffy_hip_bed_sequences / paffy_hip_bed_counts after such a run address this context's sequences only.
 */
int64_t paffy_hip_side_names_counts(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int include_inverted, int64_t cap, uint64_t *hashes, int64_t *weights,
                                    int64_t *records);
int paffy_hip_split_sides_count(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int include_inverted, int32_t n_parts, const uint64_t *table_hash,
                                const uint32_t *table_owner, int64_t n_table, int64_t *part_bytes, int64_t *part_records, int64_t *n_records);
int paffy_hip_split_sides_to(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, int include_inverted, int32_t n_parts, const uint64_t *table_hash,
                             const uint32_t *table_owner, int64_t n_table, void *d_out, int64_t out_cap, const int64_t *part_dst, const int64_t *rec_dst, int64_t rec_base,
                             int64_t *part_bytes, int64_t *part_records, void *d_rec_index, void *d_sides, int64_t rec_index_cap, int64_t *n_records);
int paffy_hip_bed_add_sides(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, const void *d_sides);
int paffy_hip_bed_failure_side(paffy_hip_ctx *ctx);
int64_t paffy_hip_bed_sequence_keys(paffy_hip_ctx *ctx, int64_t cap_sequences, void *d_keys);

/*
 * `paffy chain` (impl/paf_chain.c:123-127, paf_chain impl/chaining.c:266-343): the records of all batches are chained per (query,
 * target, strand) with the affine gap cost of impl/paf_chain.c:36-45 (no gap: 0, else gap_open + gap_extend * (query gap + target
 * gap)); every record gets its chain's id (cn) and score (s1) and the lines come out by descending own score. begin / add / run
 * as for tile; the text stays where it is until the output has been emitted (paffy_hip_emit, paffy_hip_emit_lines).
 * paffy_hip_plan_rows gives the input record of every output line, paffy_hip_chain_tags its two tags.
 * Where the reference's comparators fall back on object addresses (impl/chaining.c:18,47,62) creation order is used.
 */
typedef struct {
    int64_t gap_open, gap_extend; /* defaults of the command: 5000, 1 */
    int64_t max_gap_length;       /* 1000000 */
    float trim_fraction;          /* 1.0: alignments are shortened to their centre while chaining */
} paffy_chain_opts;
int paffy_hip_chain_begin(paffy_hip_ctx *ctx);
int paffy_hip_chain_add(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len);
int paffy_hip_chain_run(paffy_hip_ctx *ctx, const paffy_chain_opts *opts, paffy_plan_info *info);
int64_t paffy_hip_chain_tags(paffy_hip_ctx *ctx, int64_t cap, int64_t *chain_id, int64_t *chain_score);
/*
 * The reference's walk from a fresh iterator (impl/chaining.c:71-86): when its search finds no active chain <= the search key it walks
 * the whole set from the top, so an alignment that abuts the record exactly on both sequences but stands later in the input is chained
 * after all. Off (the default) paffy_hip_chain_run leaves that walk out; on, it restates it exactly: a context switch in the
 * manner of paffy_hip_stats_only, read by paffy_hip_chain_run. paffy_hip_chain_run_part returns PAFFY_E_UNSUPPORTED and changes nothing
 * while it is on. fresh_stats, of the last run: out[0] the records of the strands' leading runs that the flag kernel processed (0: it was
 * not launched), out[1] how many of them it flagged fresh, out[2] the links of the result that join a record to such an alignment,
 * out[3] how many such candidates the first recurrence skipped. All zero with the switch off.
 */
int paffy_hip_chain_fresh_walk(paffy_hip_ctx *ctx, int on);
int paffy_hip_chain_fresh_stats(paffy_hip_ctx *ctx, int64_t out[4]);
/*
 * Chain in parts: `paffy chain` sharded by query sequence. The recurrence is independent per (query, target, strand), so
 * a context that holds ALL records of some query names (the partition of paffy_hip_query_names_counts / paffy_hip_split_to) finds the
 * links, chain scores and cuts one process would. Three things are global -- the chain numbers (cn), the place of every line, the
 * failing record that ends the run -- and are settled from 32 bytes per chain and per line; the text never moves after the partition.
 * paffy_hip_chain_run is these calls with the part's own numbering.
 *   add_indexed: paffy_hip_chain_add plus the global input record number of every line of the batch (d_gidx: one int64 per line, device
 *                memory -- what paffy_hip_split_to wrote to d_rec_index; read before the call returns). Batches added with plain
 *                chain_add get their running local index. Where the reference compares object addresses (impl/chaining.c:18,47,62)
 *                this number stands in for creation order, and every error.record of the calls below is one.
 *   run_part:    everything up to and including the cut of the chains, and their numbering inside the part by (strand, chain-end
 *                score desc, processing key desc, global number desc). No lines are planned (emit refuses). Parse errors and the asserts
 *                of the trim (PAFFY_ERR_CHAIN_ASSERT) are reported as by chain_run: of a part's lines that do not parse, the one with
 *                the lowest global number. After an error the part is over: tail_keys / renumber return PAFFY_E_STATE.
 *   tail_keys:   four int64 per chain of the part into device memory, in the part's chain order: strand class (0 '+', 1 '-'), the
 *                chain end's score as the recurrence left it (the key of chain_cmp_by_score; not s1, which is the score of the chain as
 *                cut), the chain end's processing key (trimmed, for '-' mirrored query start), the chain end's global record number.
 *                A pure function of the records: chains of different parts compare as inside one process, whose numbering is the rank
 *                by (class asc, score desc, key desc, number desc). Returns the number of chains (cap_chains smaller: PAFFY_E_CAPACITY).
 *   renumber:    d_global_id: one int64 per chain of the part, in the same order, in [0, 2^31): installed as the chains' cn. Then the
 *                rest of chain_run: output order inside the part (own score desc, chain id asc, link asc), tags, paf_check of the
 *                un-trimmed records, line sizes (they depend on the digits of cn). Afterwards paffy_hip_emit, _emit_lines, _plan_rows
 *                (records: indices into the part's batches, in the order they were added) and _chain_tags work as after chain_run. A
 *                failing check is reported in info->error and fail_key (may be NULL) gets the failing line's (own score, chain id,
 *                link). The check runs chain by chain, link by link (impl/chaining.c:321-334, before the sort by score): of several parts
 *                that fail, the one with the smallest (chain id, link) is what one process reports. Nothing is to be written then.
 *   line_keys:   four int64 per output line into device memory, in the part's output order: own score, chain id, link position, bytes
 *                of the line. (Own score desc, chain id, link) is a total order; the whole output is the merge of the parts by it.
 */
int paffy_hip_chain_add_indexed(paffy_hip_ctx *ctx, const void *d_in, int64_t in_len, const void *d_gidx);
int paffy_hip_chain_run_part(paffy_hip_ctx *ctx, const paffy_chain_opts *opts, paffy_plan_info *info);
int64_t paffy_hip_chain_tail_keys(paffy_hip_ctx *ctx, int64_t cap_chains, void *d_keys);
int paffy_hip_chain_renumber(paffy_hip_ctx *ctx, const void *d_global_id, paffy_plan_info *info, int64_t fail_key[3]);
int64_t paffy_hip_chain_line_keys(paffy_hip_ctx *ctx, int64_t cap_lines, void *d_keys);

/*
 * After a tile or dedupe plan: the lines emit will write, in output order -- record[k] = zero-based input record of line k,
 * out_off[k] = its first output byte, out_off[n] = the total (cap >= n + 1 entries each). Returns n, or a negative error.
 * This is what a router such as `paffy split_file` needs to send every written line to the file of its contig.
 */
int64_t paffy_hip_plan_rows(paffy_hip_ctx *ctx, int64_t cap, uint32_t *record, int64_t *out_off);

/*
 * emit: write the planned output to d_out (16-byte aligned, out_cap >= info.out_bytes). Returns
 * after enqueueing; paffy_hip_sync() or any synchronisation of the stream completes it.
 */
int paffy_hip_emit(paffy_hip_ctx *ctx, void *d_out, int64_t out_cap);
int paffy_hip_sync(paffy_hip_ctx *ctx);

/* Host-buffer convenience used by the CLI drivers: H2D, plan, emit, D2H. *h_out is malloc'ed. */
int paffy_hip_run_host(paffy_hip_ctx *ctx, const paffy_stage *stages, int32_t n_stages, const char *h_in, int64_t in_len,
                       char **h_out, int64_t *out_len, paffy_plan_info *info);

/*
 * Streaming through host buffers: what the CLI drivers use (the reference's read / transform / write loop, impl/paf_invert.c:84-89,
 * with H2D, kernels and D2H overlapped on three streams). Two slots of pinned input; the output returns in pinned pieces.
 *   open(chunk_bytes: capacity of an input buffer, < 2 GiB - 64; piece_bytes: size of an output piece)
 *   input(want, keep, &cap): the buffer the next chunk is written into (NULL while both slots hold unread output); with want above its
 *                        capacity it is enlarged, the first `keep` bytes kept (a line longer than the chunk)
 *   submit(in_len, &info): the first in_len bytes (whole lines) go through the stage list; info is complete on return
 *   read(&piece, &len):  the next piece of the oldest submitted chunk; len = 0: that chunk is done (submit the next, or stop).
 *                        A piece stays valid until the call after next (three pinned pieces rotate) or close.
 * Submit chunk k + 1 before reading chunk k and the GPU works on k + 1 while the host drains k.
 */
typedef struct paffy_hip_stream paffy_hip_stream;
int paffy_hip_stream_open(paffy_hip_ctx *ctx, const paffy_stage *stages, int32_t n_stages, int64_t chunk_bytes, int64_t piece_bytes, paffy_hip_stream **stream);
char *paffy_hip_stream_input(paffy_hip_stream *stream, int64_t want, int64_t keep, int64_t *cap);
int paffy_hip_stream_submit(paffy_hip_stream *stream, int64_t in_len, paffy_plan_info *info);
int paffy_hip_stream_read(paffy_hip_stream *stream, const char **piece, int64_t *len);
void paffy_hip_stream_close(paffy_hip_stream *stream);
/* A closed stream leaves the device buffers of its two slots (input text, output) with the context; the context's next stream takes them
   again instead of allocating (a hipMalloc of the tens of GB a slot's output needs takes 16 ms most of the time and seconds right behind
   the hipFree of the stream before). paffy_hip_stream_trim frees them; paffy_hip_destroy does too, and so do the whole-input commands when
   they begin (tile_begin / bed_begin / chain_begin: the memory is theirs to use). A context that is destroyed while a stream of its is still
   open detaches the stream: paffy_hip_stream_close stays valid afterwards (it then frees the stream's own buffers), every other stream call
   needs the context. */
int paffy_hip_stream_trim(paffy_hip_ctx *ctx);

/*
 * Sums of the PAFFY_STATS stages of the last plan, in the argument order of paf_stats_calc (impl/paf.c:236-260): matches (M and =
 * bases), mismatches (X bases), query inserts, query deletes, query insert bases, query delete bases -- over the whole batch;
 * meaningful when no record failed (a failing record ends the reference process before it prints anything).
 */
int paffy_hip_plan_stats(paffy_hip_ctx *ctx, int64_t sums[6]);
/*
 * Diagnostics of the last paffy_hip_plan: the lean pipes (invert / identity trim / shatter / pass) are sized by the flat pass
 * (paffy_amd/csrc/flat_kernel.h); *left = the records it left to the record kernels (-1: the plan did not take the flat pass),
 * reasons[k] = how many for reason k (FLAT_WHY_* there). The outputs do not depend on who sized a record; the tests use this to
 * know that the pass under test really ran.
 * Stage lists with PAFFY_ADD_MISMATCHES: the flat pass takes the list that consists of it alone, [PAFFY_ADD_MISMATCHES, PAFFY_STATS]
 * under paffy_hip_stats_only, and -- `paffy add_mismatches | paffy trim -r | paffy filter` -- [PAFFY_ADD_MISMATCHES, PAFFY_TRIM_IDENTITY],
 * [PAFFY_ADD_MISMATCHES, PAFFY_FILTER] and [PAFFY_ADD_MISMATCHES, PAFFY_TRIM_IDENTITY, PAFFY_FILTER] (paffy_amd/csrc/flat_add_pipe_kernel.h:
 * *left >= 0; reasons[11], FLAT_WHY_ENCODER, counts the records the encoder on the pieces did not keep -- a missing or short sequence, an
 * irregular cigar, no cigar at all, a failing paf_check). Any other list with PAFFY_ADD_MISMATCHES and a further stage, and any
 * PAFFY_NO_CHECK form, is sized by the record kernels (*left = -1).
 */
int paffy_hip_flat_stats(paffy_hip_ctx *ctx, int64_t *left, int64_t reasons[16]);
/* The same six sums for every record of the batch (6 * n_records values, record by record): the numbers of the per-alignment line of
 * `paffy view` (paf_pretty_print, impl/paf.c:269-281). Returns n_records or a negative error. */
int64_t paffy_hip_plan_record_stats(paffy_hip_ctx *ctx, int64_t cap_records, int64_t *sums);
/*
 * Sums only: the caller declares that all it will ask of a plan is paffy_hip_plan_stats, paffy_hip_plan_record_stats and, with
 * with_rows = 0, paffy_hip_plan_view_sizes and paffy_hip_plan_view_text (`paffy view` when it prints no base-level rows: its stats
 * lines need the header fields and the sums, which such a plan has). Sticky, like paffy_hip_keep_raw_sequences. It takes effect for the stage list that is exactly
 * [PAFFY_ADD_MISMATCHES, PAFFY_STATS], both with their paf_check, with sequences loaded and PAFFY_NO_FLAT unset: the plan then counts
 * the matching columns of every M op on the pieces of the flat pass (paffy_amd/csrc/flat_view_kernel.h) and builds neither the = / X ops
 * nor a line: info.n_records and info.error are as ever, info.out_bytes and info.n_rows are 0, the sums are those of the default plan,
 * and paffy_hip_emit, paffy_hip_emit_lines, paffy_hip_plan_rows, paffy_hip_plan_record_layout, paffy_hip_plan_alignment_sizes,
 * paffy_hip_plan_alignment_rows and the two paffy_hip_plan_view_* calls with with_rows != 0 return PAFFY_E_STATE (paffy_hip_last_error names this setting). paffy_hip_flat_stats tells how many
 * records went through the record kernels all the same. Every other stage list plans exactly as without the setting.
 */
int paffy_hip_stats_only(paffy_hip_ctx *ctx, int on);
/*
 * Diagnostics of the last paffy_hip_plan, read only: for records [first, first + count) of the planned batch, flags[i] = the record's
 * RecPlan.flags (paffy_amd/csrc/record_types.h: bit 0 reversed view, bit 1 I / D exchanged, bit 2 query / target exchanged, bit 3 has a
 * cigar, bit 17 4-byte ops in an arena block, bit 18 2-byte words in the mirror, bit 20 the arena block is the flat add pass's) and
 * klass[i] = its class (0 LDS, 1 arena: 8-byte ops). Both are meaningful for records the plan did not fail on. The outputs do not depend
 * on how a record's ops are kept; the tests use this to know which representation the code under test really read.
 * PAFFY_E_STATE without a record plan, PAFFY_E_ARG for a range outside the batch.
 */
int paffy_hip_plan_record_layout(paffy_hip_ctx *ctx, int64_t first, int64_t count, uint32_t *flags, uint32_t *klass);

/*
 * The base-level rows of paf_pretty_print(..., include_alignment = true) (impl/paf.c:283-315; `paffy view -a`, impl/paf_view.c:158-160)
 * for records [first, first + count) of the planned batch, as the plan's stages left them: per window of 150 columns the target
 * row, the query row ('-' strand: read backwards and complemented) and the row of '*' under agreeing columns. The bases are shown
 * in the case they were loaded in, so the sequences must have been set after paffy_hip_keep_raw_sequences(ctx, 1).
 * _sizes gives the bytes of each record's block (0: no cigar); _rows writes the blocks to h_out at h_off[i] - h_off[0] (h_off:
 * count + 1 running sums of the sizes, so that a batch can be fetched in pieces). A record whose sequences are missing or shorter
 * than its coordinates (the reference reads outside the strings) is reported in *err (stage -1) and h_out is then not complete:
 * err->record is the record's index in the planned batch, as in every other paffy_error -- not its index in [first, first + count) --
 * and of several failing records of the call the one with the smallest index is reported. PAFFY_E_ARG when first + count exceeds the
 * batch; PAFFY_E_STATE without a record plan (a tile, dedupe, chain or to_bed plan made since does not count) or without raw sequences.
 * The batch text must still be in place (names are looked up in it when the plan had no PAFFY_ADD_MISMATCHES stage).
 */
int paffy_hip_keep_raw_sequences(paffy_hip_ctx *ctx, int on);
int paffy_hip_plan_alignment_sizes(paffy_hip_ctx *ctx, int64_t first, int64_t count, int64_t *h_bytes);
int paffy_hip_plan_alignment_rows(paffy_hip_ctx *ctx, int64_t first, int64_t count, const int64_t *h_off, char *h_out, paffy_error *err);

/*
 * What `paffy view` writes per record, as text in device memory: for records [first, first + count) of the planned batch the stats
 * line of paf_pretty_print (impl/paf.c:269-281) and, with with_rows != 0, the record's base-level rows right behind it (the block of
 * paffy_hip_plan_alignment_rows). The line's fields are those of the record as it was read (the header parse of the plan; the stage
 * list of `view`, [PAFFY_ADD_MISMATCHES, PAFFY_STATS], changes none of them), its six sums those of the plan's PAFFY_STATS stage, its
 * two %f fields the reference's float quotients as glibc prints them ("-nan" for a record without aligned bases). Nothing is parsed
 * again and nothing but the sizes comes to the host.
 * _sizes gives the bytes of each record's block. _text writes the blocks to d_out, record first + i at d_out + h_off[i] - h_off[0]
 * (h_off: count + 1 running sums of the sizes, so that a batch can be fetched in pieces), and returns when they are written; no byte
 * outside [d_out, d_out + h_off[count] - h_off[0]) is touched. Offsets that are not the running sums of the sizes: PAFFY_E_ARG.
 * PAFFY_E_ARG also when first + count exceeds the batch or h_off[count] - h_off[0] > out_cap. PAFFY_E_STATE, with a
 * paffy_hip_last_error that names the reason, when the last plan is not a record plan, had no PAFFY_STATS stage or reported a failing
 * record, and with with_rows != 0 also without raw sequences (paffy_hip_keep_raw_sequences) and for a plan made under
 * paffy_hip_stats_only. The rows' failures (a missing or short sequence) are reported in *err exactly as paffy_hip_plan_alignment_rows
 * reports them. The batch text must still be in place: the names are copied from it.
 */
int paffy_hip_plan_view_sizes(paffy_hip_ctx *ctx, int64_t first, int64_t count, int with_rows, int64_t *h_bytes);
int paffy_hip_plan_view_text(paffy_hip_ctx *ctx, int64_t first, int64_t count, int with_rows, const int64_t *h_off, void *d_out, int64_t out_cap,
                             paffy_error *err);

/*
 * The same text with its layout kept on the device: nothing per record crosses to the host and back (the two calls above bring the
 * sizes to the host, 8 bytes per record, and take their running sums back, 8 more).
 * _layout sizes every block of the planned batch, leaves the n_records + 1 running sums on the device and cuts the records into ranges
 * of at most range_bytes (>= 1) of text each, greedily from record 0: a range takes records while the sum stays within range_bytes and
 * one record at least, so a longer block is a range of its own. *total_bytes = the batch's text, *n_ranges = the ranges (0 for an
 * empty batch). Only the range table comes to the host: _ranges copies it out -- n_ranges + 1 entries, the first record and the first
 * byte of every range and the closing {n_records, total_bytes}; returns n_ranges (cap_ranges <= n_ranges: PAFFY_E_CAPACITY).
 * _emit_range writes range `range` at d_out (out_cap at least the range's bytes, or PAFFY_E_CAPACITY) and returns when it is written;
 * *bytes = the range's bytes. The rows' failures come back in *err exactly as paffy_hip_plan_view_text reports them (err->record counts
 * from the batch's first record), and *bytes is then what the reference had printed of this range by then: every block in front of the
 * failing record and that record's stats line. The state checks are those of paffy_hip_plan_view_text; _ranges and _emit_range without
 * a _layout of the current plan: PAFFY_E_STATE. The batch text must still be in place.
 */
int paffy_hip_plan_view_layout(paffy_hip_ctx *ctx, int with_rows, int64_t range_bytes, int64_t *total_bytes, int64_t *n_ranges);
int64_t paffy_hip_plan_view_ranges(paffy_hip_ctx *ctx, int64_t cap_ranges, int64_t *first_record, int64_t *first_byte);
int paffy_hip_plan_view_emit_range(paffy_hip_ctx *ctx, int64_t range, void *d_out, int64_t out_cap, int64_t *bytes, paffy_error *err);

/*
 * A stream in view mode (`paffy view`): open / input / submit / read / close as above, the stage list is [PAFFY_ADD_MISMATCHES,
 * PAFFY_STATS] and what read hands out is the view text of the chunk. text: 0 nothing (the sums only: `view -s -t`), 1 the stats
 * lines, 2 the lines with the base-level rows (raw sequences needed). paffy_hip_stats_only and paffy_hip_keep_raw_sequences of the
 * context apply as ever.
 *   submit: copies in, plans, and on a plan without a failing record adds the six sums and the records to the stream's totals, lays the
 *           text out (ranges of range_bytes) and writes range 0; info.out_bytes = the chunk's text. A chunk with a failing record has no
 *           output and info.error tells why -- a line that does not parse before an earlier record a stage fails on, the order the
 *           reference meets them in.
 *   A chunk of more than one range is open: read writes its later ranges as the earlier ones have been handed out, from the plan of
 *           the chunk, so input returns NULL until the chunk is read out (read it, then ask again). A chunk of one range pipelines
 *           like a chunk of any other stream.
 *   view_status: the totals, and in *rows_err the rows' failure of the chunk read last (code 0: none; the record counts from that
 *           chunk's first record). The text read of that chunk ends with the failing record's stats line. Once a chunk's rows have
 *           failed, submit returns PAFFY_E_STATE.
 */
int paffy_hip_stream_open_view(paffy_hip_ctx *ctx, int text, int64_t chunk_bytes, int64_t piece_bytes, int64_t range_bytes, paffy_hip_stream **stream);
int paffy_hip_stream_view_status(paffy_hip_stream *stream, int64_t sums[6], int64_t *n_records, paffy_error *rows_err);

/*
 * Records as structs, for hosts that hold `Paf` objects (the per-record API of inc/paf.h:75-269, host/paf_api.c): the text is
 * parsed on the GPU (paf_parse + cigar_parse, impl/paf.c:70-209) and the fields come back as arrays -- one paffy_record per line,
 * names and cigar text as slices of h_in, the ops of all records back to back in the CigarRecord layout of inc/paf.h:61-64
 * (bits 0-55 length, bits 56-63 op). *recs and *ops are malloc'ed. A failing line is reported in info->error and nothing is returned.
 */
typedef struct {
    int64_t query_length, query_start, query_end, target_length, target_start, target_end;
    int64_t score, mapping_quality, num_matches, num_bases, tile_level, chain_id, chain_score;
    int64_t ops_first; /* index of this record's first op in *ops */
    int64_t n_ops;     /* -1: no cigar (Paf.cigar == NULL: no cg tag, or an empty one) */
    uint32_t query_name_off, query_name_len, target_name_off, target_name_len;
    uint32_t cigar_off, cigar_len; /* the cg:Z: value in h_in (cigar_len 0: none) */
    uint8_t same_strand, type, pad[6];
} paffy_record;
int paffy_hip_parse_host(paffy_hip_ctx *ctx, const char *h_in, int64_t in_len, paffy_record **recs, uint64_t **ops, int64_t *n_ops_total,
                         paffy_plan_info *info);

/*
 * Sequences for PAFFY_ADD_MISMATCHES: what the reference loads with fastaReadToFunction into a
 * name -> sequence hash (impl/paf_add_mismatches.c:89-97). names[i] is the NUL-terminated FASTA
 * header used as key, seqs[i] / lens[i] the bases (host memory; copied to HBM here).
 */
int paffy_hip_set_sequences(paffy_hip_ctx *ctx, int64_t n, const char *const *names, const char *const *seqs, const int64_t *lens);

/*
 * Intervals for PAFFY_UPCONVERT: what impl/paf_upconvert.c:26-32 makes of every FASTA record of the command's files -- headers[i] decoded
 * as "name|length|start" (decode_fasta_header, impl/paf.c:716-731), end = start + seq_lens[i] (strlen of the sequence) -- sorted by
 * (name, start) with the C library's qsort as stList_sort does (equal keys keep whatever order qsort gives them). A header that does not
 * decode: PAFFY_E_HEADER and no intervals (the reference aborts before it writes anything). n = 0: no side is ever renamed.
 */
int paffy_hip_set_intervals(paffy_hip_ctx *ctx, const char *const *headers, const int64_t *seq_lens, int64_t n);

/*
 * `faffy chunk | extract | merge` (impl/fasta_{chunk,extract,merge}.c). The text of one or more FASTA files lies back to back in device
 * memory (16-byte aligned, readable up to the next multiple of 16 past text_len; it must stay there until the last emit), file_starts[k]
 * is the first byte of file k (file_starts[0] = 0, non-decreasing). paffy_hip_fasta_index reads it as host/paffy_cmds.c:fasta_read
 * does, per file, into a compact buffer of all bases and a record table (64-bit offsets: a genome passes 4 GiB).
 */
typedef struct {
    int64_t hdr_off, hdr_len; /* the header in the text (after '>', without the line end) */
    int64_t seq_off, seq_len; /* the bases in the compact buffer */
} paffy_fasta_record;
int paffy_hip_fasta_index(paffy_hip_ctx *ctx, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, int64_t *n_records,
                          int64_t *n_bases);
/* records [first, first + cap) to recs (host); returns the number of records */
int64_t paffy_hip_fasta_records(paffy_hip_ctx *ctx, int64_t first, int64_t cap, paffy_fasta_record *recs);
/* bases [first, first + n) of the compact buffer to device memory */
int paffy_hip_fasta_copy_bases(paffy_hip_ctx *ctx, int64_t first, int64_t n, void *d_dst);
/*
 * FASTA files as the paffy commands load them, from text in device memory with the contract of paffy_hip_fasta_index. The
 * text is indexed into a state of the call's own (an index of paffy_hip_fasta_index stays as it is) and may be freed when the call
 * returns; n_records (may be NULL) gets the number of FASTA records.
 * set_sequences_fasta: the store paffy_hip_set_sequences builds from the same records (names = the headers up to a NUL byte, in input
 *   order), with the raw copy under paffy_hip_keep_raw_sequences; the bases never leave the device.
 * set_intervals_fasta: the table paffy_hip_set_intervals makes of the records' headers (up to a NUL byte) and sequence lengths, built on
 *   the device: the headers are decoded, sorted by (name, start, input index) and printed there, and never come to the host
 *   (PAFFY_E_HEADER, with no intervals, as there; n_records is set all the same).
 */
int paffy_hip_set_sequences_fasta(paffy_hip_ctx *ctx, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, int64_t *n_records);
int paffy_hip_set_intervals_fasta(paffy_hip_ctx *ctx, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files, int64_t *n_records);
/* paffy_hip_fasta_index without the compact base buffer (record table and headers only; the faffy plans and copy_bases then refuse) */
int paffy_hip_fasta_index_headers(paffy_hip_ctx *ctx, const void *d_text, int64_t text_len, const int64_t *file_starts, int32_t n_files,
                                  int64_t *n_records);
/* the interval table of the context as upconvert searches it. out[0] intervals, out[1] bytes of the names blob,
   out[2] 1 when the last table was built on the device (set_intervals_fasta), 0 from host strings (set_intervals),
   out[3] name-sort rounds of that build (0 for host strings); zeros before the first table */
int paffy_hip_intervals_info(paffy_hip_ctx *ctx, int64_t out[4]);
/* copies the table to host memory: nums[3k..3k+2] = start, end, length; slices[4k..4k+3] = name_off, name_len, out_off, out_len;
   blob = the names. PAFFY_E_CAPACITY when cap < intervals or blob_cap < blob bytes; any pointer may be NULL */
int paffy_hip_intervals_read(paffy_hip_ctx *ctx, int64_t cap, int64_t blob_cap, int64_t *nums, uint32_t *slices, void *blob);
/* to_bed -q: seen[r] (host, one byte per record of the context's index) = 1 when a line of the PAF text d_paf (16-byte aligned, readable
   to the next multiple of 16) names record r's header (up to a NUL byte) as its query -- the bytes before its first tab -- or, with
   with_target, as its target -- between its fifth and sixth tab --, else 0. One device lookup per line in the sorted distinct names. */
int paffy_hip_fasta_seen(paffy_hip_ctx *ctx, const void *d_paf, int64_t paf_len, int with_target, uint8_t *seen);
/*
 * The names of the context's index (paffy_hip_fasta_index or paffy_hip_fasta_index_headers) in the order of the name tables: a record's
 * name is its header up to a NUL byte; names order by unsigned bytes, then the shorter first, then the record's input index. The sort
 * runs on the device and builds the index's table of distinct names if it is not built. Into device memory, one int32 per record (cap:
 * the records each array has room for): d_order[k] = the record at place k, d_name_of[r] = the index of record r's name among the
 * distinct names; either may be NULL. n_names (may be NULL) gets the number of distinct names. PAFFY_E_STATE without an index,
 * PAFFY_E_CAPACITY when cap < the index's records.
 */
int paffy_hip_fasta_name_order(paffy_hip_ctx *ctx, int64_t cap, void *d_order, void *d_name_of, int64_t *n_names);
/* the last name sort of the context, whichever call ran it (name_order, fasta_seen, the extract plan, set_sequences_fasta,
   set_intervals_fasta, whose keys are the decoded names): out[0] records, out[1] rounds, out[2] records still tied after the first round,
   out[3] distinct names; zeros before the first */
int paffy_hip_name_sort_stats(paffy_hip_ctx *ctx, int64_t out[4]);
/*
 * Plans over the index: info->out_bytes, info->n_rows (items), info->error (PAFFY_ERR_FAFFY_*: nothing is to be written; record = the
 * record (chunk, merge), the BED line (extract: missing name, short line) or the sorted interval (extract bounds)).
 * chunk: PAFFY_E_ARG where chunk_size > overlap but chunk_size <= 0 or chunk_size + overlap < 0 (the reference loops forever / takes
 * negative lengths); the output files are byte ranges of the output, paffy_hip_faffy_chunk_files gives their ends.
 * extract: duplicate FASTA names: the last record wins. The plan runs on the device: lines, tokens, atol, the name lookup, the sort by
 * (name, start, end) and the merge of overlapping intervals. paffy_hip_faffy_extract_plan_device takes the BED text in device memory
 * (16-byte aligned, readable to the next multiple of 16; a misaligned or NULL pointer with bed_len > 0: PAFFY_E_ARG) and keeps nothing
 * of it: d_bed may be freed on return. paffy_hip_faffy_extract_plan takes host text and is one copy to the device plus that call.
 * bed_len == 0: an empty plan. More than 2^31 - 1 lines: PAFFY_E_UNSUPPORTED.
 */
int paffy_hip_faffy_chunk_plan(paffy_hip_ctx *ctx, int64_t chunk_size, int64_t overlap, paffy_plan_info *info);
int64_t paffy_hip_faffy_chunk_files(paffy_hip_ctx *ctx, int64_t cap, int64_t *file_end);
int paffy_hip_faffy_extract_plan(paffy_hip_ctx *ctx, const char *bed, int64_t bed_len, int64_t flank, int64_t min_size, int skip_missing,
                                 paffy_plan_info *info);
int paffy_hip_faffy_extract_plan_device(paffy_hip_ctx *ctx, const void *d_bed, int64_t bed_len, int64_t flank, int64_t min_size, int skip_missing,
                                        paffy_plan_info *info);
int paffy_hip_faffy_merge_plan(paffy_hip_ctx *ctx, paffy_plan_info *info);
/* the planned bytes to d_out (16-byte aligned, out_cap >= out_bytes rounded up to 16); err->code = PAFFY_ERR_FAFFY_BASE, err->record =
   the first item with a bad base (chunk, extract): the output is then not to be written */
int paffy_hip_faffy_emit(paffy_hip_ctx *ctx, void *d_out, int64_t out_cap, paffy_error *err);

/*
 * Thresholds of `paffy filter` as its main() holds them (impl/paf_filter.c:27-32; -s -t -w pass through atoi, -u -v
 * through atof). A record is kept when score >= min_alignment_score && chain_score >= min_chain_score &&
 * (max_tile_level == -1 || tile_level <= max_tile_level) && identity >= min_identity && identity_with_gaps >=
 * min_identity_with_gaps, the identities being float32 quotients of paf_stats_calc sums (impl/paf_filter.c:129-133);
 * `invert` keeps the others instead. Used by every PAFFY_FILTER stage of later plans; defaults -1, -1, -1.0, -1.0, -1, 0.
 */
typedef struct {
    int64_t min_chain_score;
    int64_t min_alignment_score;
    double min_identity;
    double min_identity_with_gaps;
    int64_t max_tile_level;
    int32_t invert;
} paffy_filter;
int paffy_hip_set_filter(paffy_hip_ctx *ctx, const paffy_filter *f);

/* Exit status the reference process ends with for a record error (1, 134 or 139). */
int paffy_hip_error_exit_status(int32_t code);
const char *paffy_hip_error_string(int32_t code);
const char *paffy_hip_last_error(paffy_hip_ctx *ctx);

/* Per-kernel timing with HIP events on the context's stream (for bench.py's roofline line). */
int paffy_hip_profile_enable(paffy_hip_ctx *ctx, int on);
/* Bracket only the launches of one kernel (its name as paffy_hip_profile_read reports it); NULL or "": every kernel again. Two events per
   launch cost the stream about 8 us each: a step of a dozen kernels measured with all of them bracketed runs 3 % slower than without. */
int paffy_hip_profile_only(paffy_hip_ctx *ctx, const char *kernel);
/* Fills up to cap entries; returns the number of distinct kernels seen since the last reset. */
int paffy_hip_profile_read(paffy_hip_ctx *ctx, const char **names, double *total_ms, int64_t *launches, int cap);
int paffy_hip_profile_reset(paffy_hip_ctx *ctx);

/* Plain device-memory helpers so that C hosts need no HIP headers. */
int paffy_hip_malloc(void **d_ptr, int64_t bytes);
int paffy_hip_free(void *d_ptr);
int paffy_hip_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes);
int paffy_hip_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes);
int paffy_hip_device_count(void);
/* device buffers the library owns in this process right now (contexts, their command states, streams); not paffy_hip_malloc's */
int paffy_hip_device_buffers(int64_t *buffers, int64_t *bytes);

/*
 * Synthetic workload of SURVEY.md section 8d, generated on the device (same bytes as
 * tools/paf_synth.c): records [r0, r0+n) of (seed, mean_ops). With d_out == NULL only the
 * byte count is returned in *bytes.
 */
int paffy_hip_synth(paffy_hip_ctx *ctx, uint64_t seed, uint32_t mean_ops, uint64_t r0, uint64_t n, void *d_out,
                    int64_t out_cap, int64_t *bytes);
/* the same with n_contigs contigs per genome instead of 24 (fewer contigs = deeper coverage for a given record count) */
int paffy_hip_synth_contigs(paffy_hip_ctx *ctx, uint64_t seed, uint32_t mean_ops, uint32_t n_contigs, uint64_t r0, uint64_t n, void *d_out,
                            int64_t out_cap, int64_t *bytes);

/*
 * cfg4 workload (records + two genomes for PAFFY_ADD_MISMATCHES), generated on the device: every
 * contig pair (hs.chr<k>, pt.chr<k>) has one master alignment and a record is a window of it, so the aligned columns pair
 * homologous bases (2 % substitutions; a quarter of the contigs hold the query reverse-complemented and give '-' records).
 * setup builds the master tables for target contigs of tlen_min + hash % (tlen_span + 1) bases and, with with_genomes,
 * writes both genomes into the context's sequence store (replacing paffy_hip_set_sequences' content). synth4 then writes
 * records [r0, r0+n) like paffy_hip_synth. Same bytes as the host build in tools/paf_synth.c.
 */
int paffy_hip_synth4_setup(paffy_hip_ctx *ctx, uint64_t seed, uint32_t mean_ops, uint32_t n_contigs, int64_t tlen_min, int64_t tlen_span,
                           int with_genomes);
int paffy_hip_synth4(paffy_hip_ctx *ctx, uint64_t r0, uint64_t n, void *d_out, int64_t out_cap, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif

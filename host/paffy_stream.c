/*
 * paffy_stream.c -- chunked streaming of PAF text through the C-ABI (host side of the
 * shatter / invert / trim drivers; replaces the read-transform-write loop of
 * impl/paf_invert.c:84-89 and friends).
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <errno.h>
#include <signal.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <fcntl.h>
#include <unistd.h>

#include "paffy_host.h"

/* ---- what the N-GPU launcher (host/paffy_launch.c) tells a worker through its environment ---- */
int host_device(void) {
    const char *e = getenv("PAFFY_DEVICE");
    return e && *e ? atoi(e) : -1;
}
typedef struct {
    int fd;
    int64_t pos, end;
} range_cookie;
static ssize_t range_read(void *c, char *buf, size_t n) {
    range_cookie *r = (range_cookie *)c;
    const int64_t left = r->end - r->pos;
    if (left <= 0) return 0;
    if ((int64_t)n > left) n = (size_t)left;
    const ssize_t got = pread(r->fd, buf, n, (off_t)r->pos);
    if (got > 0) r->pos += got;
    return got;
}
static int range_close(void *c) {
    range_cookie *r = (range_cookie *)c;
    close(r->fd);
    free(r);
    return 0;
}
FILE *host_open_input(const char *path) {
    if (!path) return stdin;
    const char *rg = getenv("PAFFY_RANGE");
    long long a = 0, b = 0;
    if (!rg || sscanf(rg, "%lld:%lld", &a, &b) != 2) return fopen(path, "r");
    range_cookie *r = (range_cookie *)malloc(sizeof(range_cookie));
    if (!r) return NULL;
    r->fd = open(path, O_RDONLY);
    r->pos = a;
    r->end = b;
    if (r->fd < 0) {
        free(r);
        return NULL;
    }
    cookie_io_functions_t io = {range_read, NULL, NULL, range_close};
    FILE *fh = fopencookie(r, "r", io);
    if (fh) setvbuf(fh, NULL, _IOFBF, 1 << 22);
    return fh;
}

static int g_log_level = 0;
static const fasta_text *g_seq_text = NULL;
static int g_seq_log = 0;

void host_set_sequences(const fasta_text *t, int log_count) {
    g_seq_text = t;
    g_seq_log = log_count;
}

static int g_keep_raw = 0;
void host_keep_raw_sequences(int on) { g_keep_raw = on; }
static int g_stats_only = 0; /* paffy view without rows: the plans are asked for their sums only (paffy_hip_stats_only) */
void host_set_stats_only(int on) { g_stats_only = on; }

void host_set_log_level(const char *s) {
    g_log_level = 0;
    if (!s) return;
    if (!strcasecmp(s, "INFO")) g_log_level = 1;
    else if (!strcasecmp(s, "DEBUG")) g_log_level = 2;
}

void host_log_info(const char *fmt, ...) {
    if (g_log_level < 1) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}

/* PAFFY_CHUNK_MB, or the command's default */
static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static size_t chunk_bytes(long default_mb) {
    const char *e = getenv("PAFFY_CHUNK_MB");
    long mb = e ? atol(e) : default_mb;
    if (mb < 1) mb = 1;
    if (mb > 1900) mb = 1900; /* one batch stays below 2 GiB */
    return (size_t)mb << 20;
}

/* Ends the process the way the reference would for this record error. */
static void die_like_reference(const paffy_error *e, int64_t record_base) {
    int status = paffy_hip_error_exit_status(e->code);
    fflush(stdout);
    if (e->code == PAFFY_ERR_STRAND)
        fprintf(stderr, "Got an unexpected strand character (%c) in a paf string\n", (int)e->aux);
    else if (e->code == PAFFY_ERR_CIGAR_CHAR)
        fprintf(stderr, "Got an unexpected character paf cigar string: %c\n", (int)e->aux);
    else if (e->code == PAFFY_ERR_MISSING_QUERY_SEQ)
        fprintf(stderr, "No query sequence found for record %lld\n", (long long)(record_base + e->record));
    else if (e->code == PAFFY_ERR_MISSING_TARGET_SEQ)
        fprintf(stderr, "No target sequence found for record %lld\n", (long long)(record_base + e->record));
    else
        fprintf(stderr, "%s (record %lld)\n", paffy_hip_error_string(e->code), (long long)(record_base + e->record));
    if (status == 134) raise(SIGABRT);
    if (status == 139) raise(SIGSEGV);
    exit(status ? status : 1);
}

static paffy_filter g_filter = {-1, -1, -1.0, -1.0, -1, 0};
void host_set_filter(const paffy_filter *f) { g_filter = *f; }

/* paffy dedupe: the chunks of the stream go through paffy_hip_dedupe_plan of one context, which remembers what it wrote */
static int g_dedupe_mode = 0; /* 0: stage list, 1: dedupe, 2: dedupe -a */
void host_set_dedupe(int check_inverse) { g_dedupe_mode = check_inverse ? 2 : 1; }
static int dedupe_chunk(paffy_hip_ctx *ctx, const char *h_in, int64_t in_len, char **h_out, int64_t *out_len, paffy_plan_info *info) {
    void *d_in = NULL, *d_out = NULL;
    int rc = -1;
    *h_out = NULL;
    *out_len = 0;
    if (paffy_hip_malloc(&d_in, in_len + 64) == 0 && paffy_hip_memcpy_h2d(d_in, h_in, in_len) == 0 &&
        paffy_hip_dedupe_plan(ctx, d_in, in_len, g_dedupe_mode == 2, info) == 0) {
        rc = 0;
        if (info->out_bytes > 0) {
            *h_out = (char *)malloc((size_t)info->out_bytes);
            if (paffy_hip_malloc(&d_out, info->out_bytes + 64) == 0 && paffy_hip_emit(ctx, d_out, info->out_bytes + 64) == 0 &&
                paffy_hip_sync(ctx) == 0 && paffy_hip_memcpy_d2h(*h_out, d_out, info->out_bytes) == 0)
                *out_len = info->out_bytes;
            else
                rc = -1;
        }
    }
    if (d_in) paffy_hip_free(d_in);
    if (d_out) paffy_hip_free(d_out);
    return rc;
}

/* paffy view: the chunks go through a stream in view mode (paffy_hip_stream_open_view), which adds up the PAFFY_STATS sums of every
   chunk; under -s -t nothing is written per record */
static int g_stats_mode = 0;
static int64_t g_stats[6], g_stats_records;
void host_set_stats(int on) {
    g_stats_mode = on;
    memset(g_stats, 0, sizeof(g_stats));
    g_stats_records = 0;
}
void host_get_stats(int64_t sums[6], int64_t *n_records) {
    memcpy(sums, g_stats, sizeof(g_stats));
    *n_records = g_stats_records;
}
static FILE *g_stats_lines = NULL; /* paffy view without -t: one paf_pretty_print stats line per record goes here */
void host_set_stats_lines(FILE *fh) { g_stats_lines = fh; }

static int g_alignment_rows = 0; /* paffy view -a: the base-level rows under every stats line */
void host_set_alignment_rows(int on) { g_alignment_rows = on; }

/* paf_pretty_print per record (impl/paf.c:269-315): the text is fetched in ranges of records of at most this much (at least one record) */
#define VIEW_RANGE_BYTES ((int64_t)128 << 20)

/* every piece of the oldest submitted chunk to `out` */
static int drain_chunk(paffy_hip_stream *st, FILE *out) {
    for (;;) {
        const char *piece = NULL;
        int64_t len = 0;
        if (paffy_hip_stream_read(st, &piece, &len) != 0) return 1;
        if (len == 0) return 0;
        if (fwrite(piece, 1, (size_t)len, out) != (size_t)len) return 1;
    }
}

/* paffy view, after a chunk has been drained: rows that reach outside a sequence (only = / X / I / D ops: the mismatch encoder looked at no
   base of the record) end the process where the reference's read ends it, with the text up to the record's stats line written */
static void view_rows_check(paffy_hip_stream *st, FILE *out, int64_t record_base) {
    int64_t sums[6], n = 0;
    paffy_error e;
    if (paffy_hip_stream_view_status(st, sums, &n, &e) != 0 || !e.code) return;
    fflush(out);
    die_like_reference(&e, record_base);
}

/*
 * The stream commands (impl/paf_invert.c:84-89 and friends): chunks of whole lines go through pinned buffers; while the GPU works on
 * chunk k + 1 (copy in, sizing, line writer) the host drains the output of chunk k piece by piece into `out`. `paffy view` is one of
 * them (g_stats_mode): its stream is in view mode, the text of a chunk comes in ranges, and a chunk of more than one range has to be
 * drained before the next buffer is to be had.
 */
static int pipelined_stream(paffy_hip_ctx *ctx, const paffy_stage *stages, int n_stages, FILE *in, FILE *out) {
    const int view = g_stats_mode;
    /* the stream's two input buffers are pinned, and pinning costs by the byte: `paffy view`, whose output is a fraction of its input,
       takes chunks of 64 MiB unless PAFFY_CHUNK_MB says otherwise */
    const int64_t cap0 = (int64_t)chunk_bytes(view ? 64 : 256);
    /* PAFFY_STREAM_TIMES=1: where the loop's time went, on stderr when it ends well (tools/view_stream_bench.py reads it) */
    const int timed = getenv("PAFFY_STREAM_TIMES") != NULL;
    double t_open = 0, t_read = 0, t_submit = 0, t_drain = 0, t_close = 0, t0 = now_s();
    int64_t n_chunks = 0;
    /* the pinned output pieces as well: 8 MiB each for text (three of 64 MiB cost more to pin and unpin than their longer copies save: 0.14 s of
       `view -a -s` on 100 MB of input went into opening and closing the stream), next to nothing where nothing is written */
    const int view_text = g_stats_lines ? (g_alignment_rows ? 2 : 1) : 0;
    const int64_t view_piece = view_text ? (int64_t)8 << 20 : 4096;
    paffy_hip_stream *st = NULL;
    if ((view ? paffy_hip_stream_open_view(ctx, view_text, cap0, view_piece, VIEW_RANGE_BYTES, &st)
              : paffy_hip_stream_open(ctx, stages, n_stages, cap0, (int64_t)64 << 20, &st)) != 0) {
        fprintf(stderr, "paffy: could not set up the streaming buffers: %s\n", paffy_hip_last_error(ctx));
        return 1;
    }
    t_open = now_s() - t0;
    const char *carry = NULL; /* the partial last line of the chunk before, still in that chunk's buffer */
    int64_t carry_len = 0, records_done = 0, pending_base = 0; /* pending_base: the first record of the chunk not yet drained */
    int eof = 0, rc = 0, pending = 0;
    paffy_plan_info info;
    memset(&info, 0, sizeof(info));
    while (!rc && (!eof || carry_len > 0)) {
        int64_t cap = 0;
        char *buf = paffy_hip_stream_input(st, cap0, 0, &cap);
        if (!buf && view && pending) { /* the chunk before has ranges still to be written: it is read out first */
            if (drain_chunk(st, out)) {
                rc = 1;
                break;
            }
            pending = 0;
            view_rows_check(st, out, pending_base);
            buf = paffy_hip_stream_input(st, cap0, 0, &cap);
        }
        if (!buf) {
            rc = 1;
            break;
        }
        int64_t have = carry_len;
        if (carry_len > cap) buf = paffy_hip_stream_input(st, carry_len * 2, 0, &cap);
        if (!buf) {
            rc = 1;
            break;
        }
        if (carry_len) memcpy(buf, carry, (size_t)carry_len);
        int64_t use = 0;
        t0 = now_s();
        for (;;) {
            if (!eof && have < cap) {
                size_t got = fread(buf + have, 1, (size_t)(cap - have), in);
                have += (int64_t)got;
                if ((int64_t)got < cap - have + (int64_t)got) eof = feof(in) || ferror(in);
            }
            use = have;
            if (!eof) /* keep the partial last line for the next chunk */
                while (use > 0 && buf[use - 1] != '\n') use--;
            if (use > 0 || eof) break;
            buf = paffy_hip_stream_input(st, cap * 2, have, &cap); /* a single line longer than the buffer: grow */
            if (!buf) {
                fprintf(stderr, "paffy: a line too long for one batch (2 GiB)\n");
                rc = 1;
                break;
            }
        }
        t_read += now_s() - t0;
        if (rc || use == 0) break;
        t0 = now_s();
        n_chunks++;
        if (paffy_hip_stream_submit(st, use, &info) != 0) {
            fprintf(stderr, "paffy: GPU call failed: %s\n", paffy_hip_last_error(ctx));
            rc = 1;
            break;
        }
        t_submit += now_s() - t0;
        carry = buf + use; /* stays where it is until this slot is filled again, two chunks from now */
        carry_len = have - use;
        t0 = now_s();
        if (pending && drain_chunk(st, out)) rc = 1; /* the chunk before, while the GPU works on this one */
        t_drain += now_s() - t0;
        if (view && pending && !rc) view_rows_check(st, out, pending_base); /* the earlier failure speaks */
        pending = 1;
        pending_base = records_done;
        if (info.error.code) { /* everything before the failing record is written, then the process ends like the reference */
            if (!rc) rc = drain_chunk(st, out);
            fflush(out);
            die_like_reference(&info.error, records_done);
        }
        records_done += info.n_records;
    }
    t0 = now_s();
    if (!rc && pending && drain_chunk(st, out)) rc = 1;
    t_drain += now_s() - t0;
    if (view && !rc) {
        if (pending) view_rows_check(st, out, pending_base);
        paffy_error e;
        if (paffy_hip_stream_view_status(st, g_stats, &g_stats_records, &e) != 0) rc = 1;
    }
    if (rc && ctx) fprintf(stderr, "paffy: streaming failed: %s\n", paffy_hip_last_error(ctx));
    t0 = now_s();
    paffy_hip_stream_close(st);
    t_close = now_s() - t0;
    if (timed && !rc)
        fprintf(stderr, "paffy stream times: chunks %lld open %.4f read %.4f submit %.4f drain %.4f close %.4f\n", (long long)n_chunks, t_open, t_read, t_submit,
                t_drain, t_close);
    return rc;
}

/* paffy upconvert: the FASTA files of its intervals */
static const fasta_text *g_iv_text = NULL;
void host_set_intervals(const fasta_text *t) { g_iv_text = t; }

/* the FASTA text to the device, one of the paffy_hip_set_*_fasta loaders, the text freed; the loader's code (or the copy's) */
static int load_fasta(paffy_hip_ctx *ctx, const fasta_text *t, int intervals, int64_t *n_records) {
    void *d_text = NULL;
    int rc = fasta_text_to_device(t, &d_text);
    if (rc) return rc;
    rc = intervals ? paffy_hip_set_intervals_fasta(ctx, d_text, t->len, t->starts, t->n_files, n_records)
                   : paffy_hip_set_sequences_fasta(ctx, d_text, t->len, t->starts, t->n_files, n_records);
    paffy_hip_free(d_text);
    return rc;
}

int host_fasta_seen(const fasta_text *t, const char *paf, int64_t paf_len, int with_target, paffy_fasta_record **recs, uint8_t **seen, int64_t *n) {
    paffy_hip_ctx *ctx = NULL;
    *recs = NULL;
    *seen = NULL;
    *n = 0;
    if (paffy_hip_create(&ctx, host_device()) != 0) {
        fprintf(stderr, "paffy: no usable GPU (this build has no CPU path)\n");
        return 1;
    }
    void *d_text = NULL, *d_paf = NULL;
    int rc = fasta_text_to_device(t, &d_text);
    if (!rc) rc = paffy_hip_fasta_index_headers(ctx, d_text, t->len, t->starts, t->n_files, n);
    if (d_text) paffy_hip_free(d_text); /* the index keeps the table and the headers on the host */
    if (!rc && *n > 0) {
        *recs = (paffy_fasta_record *)malloc(sizeof(paffy_fasta_record) * (size_t)*n);
        *seen = (uint8_t *)malloc((size_t)*n);
        if (!*recs || !*seen) {
            fprintf(stderr, "paffy: out of memory\n");
            exit(1);
        }
        paffy_hip_fasta_records(ctx, 0, *n, *recs);
        rc = paffy_hip_malloc(&d_paf, (paf_len + 15) / 16 * 16 + 16);
        if (!rc && paf_len) rc = paffy_hip_memcpy_h2d(d_paf, paf, paf_len);
        if (!rc) rc = paffy_hip_fasta_seen(ctx, d_paf, paf_len, with_target, *seen);
        if (d_paf) paffy_hip_free(d_paf);
    }
    if (rc) fprintf(stderr, "paffy: GPU call failed (%d): %s\n", rc, paffy_hip_last_error(ctx));
    paffy_hip_destroy(ctx);
    return rc ? 1 : 0;
}

/* the context host_load_fasta prepared for the next host_stream (NULL: host_stream creates its own) */
static paffy_hip_ctx *g_ctx = NULL;
static int g_bad_header = 0;

static paffy_hip_ctx *open_ctx(void) {
    paffy_hip_ctx *ctx = NULL;
    if (paffy_hip_create(&ctx, host_device()) != 0) {
        fprintf(stderr, "paffy: no usable GPU (this build has no CPU path)\n");
        return NULL;
    }
    return ctx;
}

int host_load_fasta(void) {
    if (!(g_ctx = open_ctx())) return 1;
    if (g_keep_raw) paffy_hip_keep_raw_sequences(g_ctx, 1);
    if (g_stats_only) paffy_hip_stats_only(g_ctx, 1);
    int64_t n_fasta = 0;
    if (g_seq_text) {
        if (load_fasta(g_ctx, g_seq_text, 0, &n_fasta) != 0) {
            fprintf(stderr, "paffy: could not load the sequences onto the GPU: %s\n", paffy_hip_last_error(g_ctx));
            return 1;
        }
        if (g_seq_log) host_log_info("Read %i sequences from sequence files\n", (int)n_fasta);
    }
    if (g_iv_text) {
        const int rc = load_fasta(g_ctx, g_iv_text, 1, &n_fasta);
        if (rc == 0 || rc == PAFFY_E_HEADER) host_log_info("Read %i sequences from sequence files\n", (int)n_fasta); /* read before the header check */
        g_bad_header = rc == PAFFY_E_HEADER; /* host_stream ends the process where the reference's assert does */
        if (rc != 0 && rc != PAFFY_E_HEADER) {
            fprintf(stderr, "paffy: could not load the intervals onto the GPU: %s\n", paffy_hip_last_error(g_ctx));
            return 1;
        }
    }
    return 0;
}

int host_stream(const paffy_stage *stages, int n_stages, FILE *in, FILE *out) {
    paffy_hip_ctx *ctx = g_ctx;
    g_ctx = NULL;
    if (!ctx && !(ctx = open_ctx())) return 1;
    if (g_bad_header) { /* the reference's assert in decode_fasta_header, before it reads a record */
        fprintf(stderr, "%s\n", paffy_hip_last_error(ctx));
        fflush(out);
        abort();
    }
    paffy_hip_set_filter(ctx, &g_filter);
    if (!g_dedupe_mode) {
        int rc = pipelined_stream(ctx, stages, n_stages, in, out);
        paffy_hip_destroy(ctx);
        fflush(out);
        return rc;
    }
    const size_t cap = chunk_bytes(256);
    size_t buf_cap = cap + (1 << 20), have = 0;
    char *buf = (char *)malloc(buf_cap);
    int64_t records_done = 0;
    int eof = 0, rc = 0;
    while (!eof || have > 0) {
        if (!eof) {
            if (have == buf_cap) { /* a single line longer than the chunk: grow */
                buf_cap *= 2;
                buf = (char *)realloc(buf, buf_cap);
            }
            size_t want = (have < cap ? cap : buf_cap) - have;
            size_t got = fread(buf + have, 1, want, in);
            have += got;
            if (got < want) eof = 1;
        }
        size_t use = have;
        if (!eof) { /* keep the partial last line for the next chunk */
            while (use > 0 && buf[use - 1] != '\n') use--;
            if (use == 0) continue; /* no complete line yet: read more */
        }
        if (use == 0) break;
        char *h_out = NULL;
        int64_t out_len = 0;
        paffy_plan_info info;
        int r = dedupe_chunk(ctx, buf, (int64_t)use, &h_out, &out_len, &info);
        if (r != 0) {
            fprintf(stderr, "paffy: GPU call failed (%d): %s\n", r, paffy_hip_last_error(ctx));
            rc = 1;
            free(h_out);
            break;
        }
        if (out_len > 0) fwrite(h_out, 1, (size_t)out_len, out);
        free(h_out);
        if (info.error.code) die_like_reference(&info.error, records_done);
        records_done += info.n_records;
        memmove(buf, buf + use, have - use);
        have -= use;
    }
    free(buf);
    paffy_hip_destroy(ctx);
    fflush(out);
    return rc;
}

/* ---- paffy split_file (impl/paf_split_file.c:131-173): the GPU normalises the lines, groups them by output file and decides the
   files (paffy_hip_split_plan); the host opens the files and writes a chunk's lines of every file with one fwrite ---- */
static FILE *open_or_die(const char *path) {
    FILE *fh = fopen(path, "w");
    if (!fh) {
        fprintf(stderr, "Could not open output file: %s\n", path);
        exit(1);
    }
    host_log_info("Opened output file: %s\n", path);
    return fh;
}
/* file `id` of the run: "<prefix><name>.paf" */
static FILE *split_open(paffy_hip_ctx *ctx, int64_t id, const char *prefix) {
    int64_t cap = 256, len;
    char *name = (char *)malloc((size_t)cap);
    while ((len = paffy_hip_split_file_name(ctx, id, name, cap)) == PAFFY_E_CAPACITY) {
        cap *= 4;
        name = (char *)realloc(name, (size_t)cap);
    }
    if (len < 0) {
        free(name);
        return NULL;
    }
    char path[4096];
    int w = snprintf(path, sizeof(path), "%s", prefix);
    if (w > (int)sizeof(path) - 8) w = (int)sizeof(path) - 8;
    for (int64_t i = 0; i < len && w < (int)sizeof(path) - 8; i++) path[w++] = name[i];
    snprintf(path + w, sizeof(path) - (size_t)w, ".paf");
    free(name);
    return open_or_die(path);
}
/* a device buffer that stays for the run and grows when a chunk needs more */
static int split_room(void **d, int64_t *cap, int64_t want) {
    if (want <= *cap) return 0;
    if (*d) paffy_hip_free(*d);
    *d = NULL;
    *cap = 0;
    want += want / 4;
    if (paffy_hip_malloc(d, want) != 0) return -1;
    *cap = want;
    return 0;
}

int host_split_file(FILE *in, const char *prefix, int by_query, int64_t min_length) {
    paffy_hip_ctx *ctx = NULL;
    if (paffy_hip_create(&ctx, host_device()) != 0) {
        fprintf(stderr, "paffy: no usable GPU (this build has no CPU path)\n");
        return 1;
    }
    FILE **files = NULL; /* by the library's file id */
    int64_t n_files = 0, records_done = 0;
    void *d_in = NULL, *d_out = NULL;
    int64_t d_in_cap = 0, d_out_cap = 0, h_out_cap = 0, groups_cap = 0;
    char *h_out = NULL;
    paffy_split_group *groups = NULL;
    const size_t cap = chunk_bytes(256);
    size_t buf_cap = cap + (1 << 20), have = 0;
    char *buf = (char *)malloc(buf_cap);
    int eof = 0, rc = 0;
    if (paffy_hip_split_begin(ctx, by_query, min_length) != 0) {
        fprintf(stderr, "paffy split_file: GPU call failed: %s\n", paffy_hip_last_error(ctx));
        rc = 1;
        eof = 1;
    }
    while (!rc && (!eof || have > 0)) {
        if (!eof) {
            if (have == buf_cap) {
                buf_cap *= 2;
                buf = (char *)realloc(buf, buf_cap);
            }
            size_t want = (have < cap ? cap : buf_cap) - have;
            size_t got = fread(buf + have, 1, want, in);
            have += got;
            if (got < want) eof = 1;
        }
        size_t use = have;
        if (!eof) {
            while (use > 0 && buf[use - 1] != '\n') use--;
            if (use == 0) continue;
        }
        if (use == 0) break;
        paffy_plan_info info;
        int64_t n_groups = 0;
        int ok = split_room(&d_in, &d_in_cap, (int64_t)use + 64) == 0 && paffy_hip_memcpy_h2d(d_in, buf, (int64_t)use) == 0 &&
                 paffy_hip_split_plan(ctx, d_in, (int64_t)use, &info) == 0;
        if (ok && info.out_bytes > 0) {
            if (info.out_bytes > h_out_cap) {
                h_out_cap = info.out_bytes + info.out_bytes / 4;
                free(h_out);
                h_out = (char *)malloc((size_t)h_out_cap);
            }
            ok = split_room(&d_out, &d_out_cap, info.out_bytes + 64) == 0 && paffy_hip_emit(ctx, d_out, d_out_cap) == 0 && paffy_hip_sync(ctx) == 0 &&
                 paffy_hip_memcpy_d2h(h_out, d_out, info.out_bytes) == 0;
        }
        while (ok && (n_groups = paffy_hip_split_groups(ctx, groups_cap, groups)) == PAFFY_E_CAPACITY) {
            groups_cap = groups_cap ? groups_cap * 4 : 1024;
            groups = (paffy_split_group *)realloc(groups, sizeof(paffy_split_group) * (size_t)groups_cap);
        }
        if (ok && n_groups < 0) ok = 0;
        /* one write per file of the chunk; files open in this order, which is the order their first lines come in */
        for (int64_t g = 0; ok && g < n_groups; g++) {
            const paffy_split_group *sg = &groups[g];
            if (sg->new_file) {
                if (sg->file >= n_files) {
                    files = (FILE **)realloc(files, sizeof(FILE *) * (size_t)(sg->file + 1));
                    while (n_files <= sg->file) files[n_files++] = NULL;
                }
                files[sg->file] = split_open(ctx, sg->file, prefix);
                if (!files[sg->file]) ok = 0;
            }
            if (ok) fwrite(h_out + sg->out_off, 1, (size_t)sg->bytes, files[sg->file]);
        }
        if (!ok) {
            fprintf(stderr, "paffy split_file: GPU call failed: %s\n", paffy_hip_last_error(ctx));
            rc = 1;
            break;
        }
        if (info.error.code) {
            for (int64_t i = 0; i < n_files; i++)
                if (files[i]) fclose(files[i]);
            die_like_reference(&info.error, records_done);
        }
        records_done += info.n_records;
        memmove(buf, buf + use, have - use);
        have -= use;
    }
    for (int64_t i = 0; i < n_files; i++)
        if (files[i]) fclose(files[i]);
    free(files);
    free(groups);
    free(h_out);
    if (d_in) paffy_hip_free(d_in);
    if (d_out) paffy_hip_free(d_out);
    free(buf);
    paffy_hip_destroy(ctx);
    host_log_info("Split %lld records\n", (long long)records_done);
    return rc;
}

/*
 * ---- `paffy chain` as one of N workers of the launcher (host/paffy_launch.c): the part mode ----
 * PAFFY_CHAIN_PART=<prefix> names the part's files -- <prefix>.idx (read: the global record number of every input line, one int64 each),
 * <prefix>.tails (written: four int64 per chain), <prefix>.ids (read: one int64 per chain, its number in the whole input), <prefix>.lkeys
 * (written: four int64 per output line) -- and PAFFY_CHAIN_FDS=<from_launcher>,<to_launcher> two inherited pipe descriptors. After each of
 * the two phases the worker writes eight int64 {phase, failed, sort key x 3, count, 0, 0} and reads one int64: 0 go on, 1 this worker's
 * failure is the one the user sees (it ends as die_like_reference ends), anything else, or end-of-file: end silently. Every
 * error.record is a global record number (paffy_hip_chain_add_indexed), so the message is the one-worker run's.
 */
typedef struct {
    const char *prefix;
    int from_fd, to_fd;
    FILE *idx;
} chain_part;

static int chain_part_open(chain_part *p) { /* 1: part mode; 0: not under the launcher; -1 after a message */
    const char *prefix = getenv("PAFFY_CHAIN_PART"), *fds = getenv("PAFFY_CHAIN_FDS");
    if (!prefix || !*prefix || !fds) return 0;
    char path[4096];
    p->prefix = prefix;
    snprintf(path, sizeof(path), "%s.idx", prefix);
    if (sscanf(fds, "%d,%d", &p->from_fd, &p->to_fd) != 2 || !(p->idx = fopen(path, "r"))) {
        fprintf(stderr, "paffy chain: cannot use the part %s (PAFFY_CHAIN_FDS=%s)\n", prefix, fds);
        return -1;
    }
    return 1;
}

/* a batch of the part: its lines' global record numbers go to the device with it */
static int chain_part_add(paffy_hip_ctx *ctx, chain_part *p, const void *d, const char *buf, size_t use) {
    size_t lines = use > 0 && buf[use - 1] != '\n';
    for (const char *q = buf, *e = buf + use; q < e && (q = (const char *)memchr(q, '\n', (size_t)(e - q))) != NULL; q++) lines++;
    int64_t *g = (int64_t *)malloc(sizeof(int64_t) * (lines + 1));
    void *d_g = NULL;
    int rc = -1;
    if (g && fread(g, sizeof(int64_t), lines, p->idx) == lines && paffy_hip_malloc(&d_g, (int64_t)(sizeof(int64_t) * lines) + 64) == 0 &&
        paffy_hip_memcpy_h2d(d_g, g, (int64_t)(sizeof(int64_t) * lines)) == 0)
        rc = paffy_hip_chain_add_indexed(ctx, d, (int64_t)use, d_g);
    if (d_g) paffy_hip_free(d_g); /* read before the call returned */
    free(g);
    return rc;
}

/* `count` rows of four int64 from device memory to <prefix>.<ext>, complete before the report that mentions them */
static int chain_part_keys(paffy_hip_ctx *ctx, const chain_part *p, const char *ext, const void *d_keys, int64_t count) {
    char path[4096];
    snprintf(path, sizeof(path), "%s.%s", p->prefix, ext);
    const size_t bytes = (size_t)count * 32;
    char *h = (char *)malloc(bytes + 1);
    int rc = !h || paffy_hip_sync(ctx) != 0 || (bytes && paffy_hip_memcpy_d2h(h, d_keys, (int64_t)bytes) != 0);
    FILE *f = rc ? NULL : fopen(path, "w");
    if (!f || fwrite(h, 1, bytes, f) != bytes) rc = 1;
    if (f && fclose(f) != 0) rc = 1;
    free(h);
    return rc;
}

/* a verdict from the launcher; end-of-file in its place ends the process */
static int64_t part_verdict(int from_fd) {
    int64_t verdict = -1;
    for (size_t at = 0; at < sizeof(verdict);) {
        const ssize_t k = read(from_fd, (char *)&verdict + at, sizeof(verdict) - at);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) exit(1); /* end-of-file in place of a verdict */
        at += (size_t)k;
    }
    return verdict;
}

/* a report of eight int64 up the pipe, then the launcher's verdict: returns on "go on", ends the process otherwise (chain and to_bed) */
static void part_settle(int to_fd, int from_fd, const int64_t rep[8], const paffy_error *e) {
    size_t at = 0;
    while (at < 8 * sizeof(int64_t)) {
        const ssize_t k = write(to_fd, (const char *)rep + at, 8 * sizeof(int64_t) - at);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) exit(1); /* the launcher is gone */
        at += (size_t)k;
    }
    const int64_t verdict = part_verdict(from_fd);
    if (verdict == 0 && !e->code) return;
    if (verdict == 1 && e->code) die_like_reference(e, 0);
    exit(verdict == 2 ? 0 : 1);
}

/* the report of a phase, then the launcher's verdict: returns on "go on", ends the process otherwise */
static void chain_part_report(const chain_part *p, int64_t phase, const paffy_error *e, const int64_t key[3], int64_t count) {
    const int64_t rep[8] = {phase, e->code != 0, key[0], key[1], key[2], count, 0, 0};
    part_settle(p->to_fd, p->from_fd, rep, e);
}

/* paffy_hip_chain_run in two phases with the launcher between them; 0 with the lines planned, or the failing call's code */
static int chain_part_run(paffy_hip_ctx *ctx, const paffy_chain_opts *opts, chain_part *p, paffy_plan_info *info) {
    int rc = paffy_hip_chain_run_part(ctx, opts, info);
    if (rc) return rc;
    void *d_keys = NULL;
    int64_t key[3] = {info->error.stage, info->error.record, 0}, n_chains = 0; /* shard.part_failure */
    if (!info->error.code) {
        const int64_t cap = info->n_records > 0 ? info->n_records : 1; /* every chain has a record of its own */
        if (paffy_hip_malloc(&d_keys, cap * 32 + 64) != 0) return PAFFY_E_HIP;
        n_chains = paffy_hip_chain_tail_keys(ctx, cap, d_keys);
        if (n_chains >= 0 && chain_part_keys(ctx, p, "tails", d_keys, n_chains) != 0) n_chains = PAFFY_E_HIP;
        paffy_hip_free(d_keys);
        if (n_chains < 0) return (int)n_chains;
    }
    chain_part_report(p, 1, &info->error, key, n_chains);
    /* the chains' numbers in the whole input */
    char path[4096];
    snprintf(path, sizeof(path), "%s.ids", p->prefix);
    int64_t *ids = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n_chains + 1));
    FILE *f = fopen(path, "r");
    void *d_ids = NULL;
    int64_t fail_key[3] = {0, 0, 0};
    rc = PAFFY_E_HIP;
    if (ids && f && fread(ids, sizeof(int64_t), (size_t)n_chains, f) == (size_t)n_chains && paffy_hip_malloc(&d_ids, n_chains * 8 + 64) == 0 &&
        paffy_hip_memcpy_h2d(d_ids, ids, n_chains * 8) == 0)
        rc = paffy_hip_chain_renumber(ctx, n_chains ? d_ids : NULL, info, fail_key);
    else
        fprintf(stderr, "paffy chain: cannot read %s\n", path);
    if (f) fclose(f);
    if (d_ids) paffy_hip_free(d_ids);
    free(ids);
    if (rc) return rc;
    key[0] = fail_key[1]; /* a failed paf_check: (chain id, link), the order the reference checks in */
    key[1] = fail_key[2];
    if (!info->error.code) {
        const int64_t cap = info->n_rows > 0 ? info->n_rows : 1;
        if (paffy_hip_malloc(&d_keys, cap * 32 + 64) != 0) return PAFFY_E_HIP;
        int64_t n_lines = paffy_hip_chain_line_keys(ctx, cap, d_keys);
        if (n_lines >= 0 && n_lines != info->n_rows) n_lines = PAFFY_E_STATE;
        if (n_lines >= 0 && chain_part_keys(ctx, p, "lkeys", d_keys, n_lines) != 0) n_lines = PAFFY_E_HIP;
        paffy_hip_free(d_keys);
        if (n_lines < 0) return (int)n_lines;
    }
    chain_part_report(p, 2, &info->error, key, info->n_rows);
    return 0;
}

/*
 * ---- `paffy to_bed` as one of N workers of the launcher (host/paffy_launch.c): the part mode ----
 * PAFFY_BED_PART=<prefix> names the part's files -- <prefix>.idx (read: the global record number of every input line, one int64 each),
 * <prefix>.sides (read: one side mask byte per input line, paffy_hip_bed_add_sides), <prefix>.bkeys (written: three int64 per sequence in
 * output order: 2 * global record of first appearance + side, the bytes of its block of BED lines, its lines), and under -f -q <prefix>.seen
 * (written: one byte per record of the FASTA file, whether a line of the part names it), <prefix>.seen_all (read by the one worker that
 * is asked for the tail: the union over all parts) and <prefix>.tail (written by that worker: the "name 0 length\t0" lines) -- and
 * PAFFY_BED_FDS=<from_launcher>,<to_launcher> two inherited pipe descriptors with chain's protocol: after the run eight int64
 * {1, failed, global record, kind, 0, sequences, 0, 0} (kind: 0 the line does not parse, 1 its query side fails, 2 its target side,
 * shard.part_failure) and one int64 back: 0 go on (write the blocks), 1 this worker's failure is the one the user sees, anything else or
 * end-of-file: end silently. Under -f -q a second verdict follows once the blocks are written: 2 end well, 0 write the tail, report
 * {2, 0, ...} and read a last verdict.
 */
typedef struct {
    const char *prefix;
    int from_fd, to_fd;
    int64_t *idx;           /* the global record number of every line of the part */
    int64_t n_lines, added; /* lines of the part; lines of the batches added so far */
    FILE *sides;
    int with_target;
    /* -f -q: the FASTA records (indexed in a context of their own) and whether a line of the part names them */
    int tail;
    const fasta_text *fasta;
    paffy_hip_ctx *fctx;
    int64_t n_fasta;
    uint8_t *seen, *seen_batch;
} bed_part;

static int g_bed_tail = 0;
static const fasta_text *g_bed_fasta = NULL;
void host_set_bed_tail(const fasta_text *t) {
    g_bed_tail = 1;
    g_bed_fasta = t;
}

static int bed_part_open(bed_part *p, const paffy_bed_opts *opts) { /* 1: part mode; 0: not under the launcher; -1 after a message */
    const char *prefix = getenv("PAFFY_BED_PART"), *fds = getenv("PAFFY_BED_FDS");
    if (!prefix || !*prefix || !fds) return 0;
    char path[4096];
    p->prefix = prefix;
    p->with_target = opts->include_inverted != 0;
    snprintf(path, sizeof(path), "%s.idx", prefix);
    FILE *fi = fopen(path, "r");
    snprintf(path, sizeof(path), "%s.sides", prefix);
    p->sides = fopen(path, "r");
    int ok = sscanf(fds, "%d,%d", &p->from_fd, &p->to_fd) == 2 && fi && p->sides && fseek(fi, 0, SEEK_END) == 0;
    if (ok) {
        p->n_lines = (int64_t)(ftell(fi) / (long)sizeof(int64_t));
        rewind(fi);
        p->idx = (int64_t *)malloc(sizeof(int64_t) * (size_t)(p->n_lines + 1));
        ok = p->idx && fread(p->idx, sizeof(int64_t), (size_t)p->n_lines, fi) == (size_t)p->n_lines;
    }
    if (fi) fclose(fi);
    if (!ok) {
        fprintf(stderr, "paffy to_bed: cannot use the part %s (PAFFY_BED_FDS=%s)\n", prefix, fds);
        return -1;
    }
    p->tail = g_bed_tail;
    p->fasta = g_bed_fasta;
    if (p->tail && p->fasta) { /* a file that cannot be opened adds nothing: no record, no flag */
        void *d_text = NULL;
        int rc = paffy_hip_create(&p->fctx, host_device()) != 0;
        if (!rc) rc = fasta_text_to_device(p->fasta, &d_text);
        if (!rc) rc = paffy_hip_fasta_index_headers(p->fctx, d_text, p->fasta->len, p->fasta->starts, p->fasta->n_files, &p->n_fasta);
        if (d_text) paffy_hip_free(d_text); /* the index keeps the table and the headers on the host */
        if (!rc) {
            p->seen = (uint8_t *)calloc((size_t)p->n_fasta + 1, 1);
            p->seen_batch = (uint8_t *)calloc((size_t)p->n_fasta + 1, 1);
        }
        if (rc || !p->seen || !p->seen_batch) {
            fprintf(stderr, "paffy to_bed: could not index the FASTA file on the GPU: %s\n", p->fctx ? paffy_hip_last_error(p->fctx) : "no context");
            return -1;
        }
    }
    return 1;
}

/* a batch of the part: its lines' side masks go to the device with it; under -f -q the names it uses are flagged while it is there */
static int bed_part_add(paffy_hip_ctx *ctx, bed_part *p, const void *d, const char *buf, size_t use) {
    size_t lines = use > 0 && buf[use - 1] != '\n';
    for (const char *q = buf, *e = buf + use; q < e && (q = (const char *)memchr(q, '\n', (size_t)(e - q))) != NULL; q++) lines++;
    uint8_t *m = (uint8_t *)malloc(lines + 1);
    void *d_m = NULL;
    int rc = -1;
    if (m && p->added + (int64_t)lines <= p->n_lines && fread(m, 1, lines, p->sides) == lines && paffy_hip_malloc(&d_m, (int64_t)lines + 64) == 0 &&
        paffy_hip_memcpy_h2d(d_m, m, (int64_t)lines) == 0)
        rc = paffy_hip_bed_add_sides(ctx, d, (int64_t)use, d_m);
    if (d_m) paffy_hip_free(d_m); /* read before the call returned */
    free(m);
    p->added += (int64_t)lines;
    if (!rc && p->fctx && p->n_fasta > 0) {
        rc = paffy_hip_fasta_seen(p->fctx, d, (int64_t)use, p->with_target, p->seen_batch);
        for (int64_t k = 0; !rc && k < p->n_fasta; k++) p->seen[k] |= p->seen_batch[k];
    }
    return rc;
}

static int bed_part_file(const bed_part *p, const char *ext, const void *data, size_t bytes) {
    char path[4096];
    snprintf(path, sizeof(path), "%s.%s", p->prefix, ext);
    FILE *f = fopen(path, "w");
    int rc = !f || fwrite(data, 1, bytes, f) != bytes;
    if (f && fclose(f) != 0) rc = 1;
    if (rc) fprintf(stderr, "paffy to_bed: cannot write %s\n", path);
    return rc;
}

/* paffy_hip_bed_run, then the launcher: 0 with the blocks planned and "go on" received, or the failing call's code */
static int bed_part_run(paffy_hip_ctx *ctx, const paffy_bed_opts *opts, bed_part *p, paffy_plan_info *info) {
    int rc = paffy_hip_bed_run(ctx, opts, info);
    if (rc) return rc;
    if (p->added != p->n_lines) {
        fprintf(stderr, "paffy to_bed: %lld record numbers for %lld lines\n", (long long)p->n_lines, (long long)p->added);
        return PAFFY_E_STATE;
    }
    int64_t rep[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    if (info->error.code) { /* the failing line's global number, and which of its sides failed: what the launcher compares */
        if (info->error.record < 0 || info->error.record >= p->n_lines) return PAFFY_E_STATE;
        info->error.record = p->idx[info->error.record];
        rep[1] = 1;
        rep[2] = info->error.record;
        rep[3] = paffy_hip_bed_failure_side(ctx) + 1;
    } else {
        const int64_t cap = paffy_hip_bed_sequences(ctx) > 0 ? paffy_hip_bed_sequences(ctx) : 1;
        void *d_keys = NULL;
        int64_t *keys = (int64_t *)malloc((size_t)cap * 24);
        int64_t n_seq = PAFFY_E_HIP;
        if (keys && paffy_hip_malloc(&d_keys, cap * 24 + 64) == 0) n_seq = paffy_hip_bed_sequence_keys(ctx, cap, d_keys);
        if (n_seq > 0 && (paffy_hip_sync(ctx) != 0 || paffy_hip_memcpy_d2h(keys, d_keys, n_seq * 24) != 0)) n_seq = PAFFY_E_HIP;
        for (int64_t s = 0; s < n_seq; s++) { /* the local entry of first appearance (2 * line + side) -> the global one */
            const int64_t line = keys[3 * s] >> 1;
            if (line < 0 || line >= p->n_lines) n_seq = PAFFY_E_STATE;
            else keys[3 * s] = 2 * p->idx[line] + (keys[3 * s] & 1);
        }
        if (n_seq >= 0 && bed_part_file(p, "bkeys", keys, (size_t)n_seq * 24) != 0) n_seq = PAFFY_E_HIP;
        if (n_seq >= 0 && p->tail && bed_part_file(p, "seen", p->seen ? p->seen : (const uint8_t *)"", (size_t)p->n_fasta) != 0) n_seq = PAFFY_E_HIP;
        if (d_keys) paffy_hip_free(d_keys);
        free(keys);
        if (n_seq < 0) return (int)n_seq;
        rep[5] = n_seq;
    }
    part_settle(p->to_fd, p->from_fd, rep, &info->error);
    return 0;
}

/* under -f -q, once the blocks are written: the launcher either ends this worker or asks it for the tail -- the records of the FASTA
   file that no line of ANY part names (<prefix>.seen_all), in file order: the loop of paffy_to_bed_main */
static int bed_part_tail(bed_part *p) {
    if (!p->tail) return 0;
    if (part_verdict(p->from_fd) != 0) exit(0);
    char path[4096];
    snprintf(path, sizeof(path), "%s.tail", p->prefix);
    FILE *tf = fopen(path, "w");
    int rc = !tf;
    if (!rc && p->n_fasta > 0) {
        paffy_fasta_record *recs = (paffy_fasta_record *)malloc(sizeof(paffy_fasta_record) * (size_t)p->n_fasta);
        uint8_t *all = (uint8_t *)malloc((size_t)p->n_fasta);
        snprintf(path, sizeof(path), "%s.seen_all", p->prefix);
        FILE *sf = fopen(path, "r");
        rc = !recs || !all || !sf || fread(all, 1, (size_t)p->n_fasta, sf) != (size_t)p->n_fasta || paffy_hip_fasta_records(p->fctx, 0, p->n_fasta, recs) != p->n_fasta;
        for (int64_t k = 0; k < p->n_fasta && !rc; k++)
            if (!all[k]) { /* the name is the header up to a NUL byte */
                const char *h = p->fasta->data + recs[k].hdr_off;
                fprintf(tf, "%.*s 0 %" PRIi64 "\t0\n", (int)strnlen(h, (size_t)recs[k].hdr_len), h, recs[k].seq_len);
            }
        if (sf) fclose(sf);
        free(recs);
        free(all);
    }
    if (tf && fclose(tf) != 0) rc = 1;
    if (rc) {
        fprintf(stderr, "paffy to_bed: cannot write the sequences without alignments of the part %s\n", p->prefix);
        return 1;
    }
    const int64_t rep[8] = {2, 0, 0, 0, 0, 0, 0, 0};
    const paffy_error none = {0};
    part_settle(p->to_fd, p->from_fd, rep, &none);
    return 0;
}

static void bed_part_close(bed_part *p) {
    if (p->sides) fclose(p->sides);
    if (p->fctx) paffy_hip_destroy(p->fctx);
    free(p->idx);
    free(p->seen);
    free(p->seen_batch);
}

static int whole_file(FILE *in, FILE *out, const paffy_bed_opts *bed, const paffy_chain_opts *chain);
int host_tile(FILE *in, FILE *out) { return whole_file(in, out, NULL, NULL); }
/* paffy to_bed: every record counts before anything is written, like tile */
int host_to_bed(FILE *in, FILE *out, const paffy_bed_opts *opts) { return whole_file(in, out, opts, NULL); }
/* paffy chain: read_pafs, paf_chain, write_pafs (impl/paf_chain.c:123-127) */
int host_chain(FILE *in, FILE *out, const paffy_chain_opts *opts) { return whole_file(in, out, NULL, opts); }

/*
 * tile / to_bed / chain read the whole input before they write (read_pafs, impl/paf.c:492-499; the loop of impl/paf_to_bed.c:166-190).
 * The text goes to the GPU in batches of whole lines (at most PAFFY_CHUNK_MB each, below the 2 GiB a batch may hold) and stays
 * there; the output comes back through a bounded staging buffer. Inputs are limited by the GPU's memory, not by a batch.
 */
static int whole_file(FILE *in, FILE *out, const paffy_bed_opts *bed, const paffy_chain_opts *chain) {
    paffy_hip_ctx *ctx = NULL;
    if (paffy_hip_create(&ctx, host_device()) != 0) {
        fprintf(stderr, "paffy: no usable GPU (this build has no CPU path)\n");
        return 1;
    }
    const char *what = bed ? "to_bed" : (chain ? "chain" : "tile");
    chain_part part; /* chain under the N-GPU launcher */
    memset(&part, 0, sizeof(part));
    const int in_part = chain ? chain_part_open(&part) : 0;
    if (in_part < 0) return 1;
    bed_part bpart; /* to_bed under the N-GPU launcher */
    memset(&bpart, 0, sizeof(bpart));
    const int in_bed_part = bed ? bed_part_open(&bpart, bed) : 0;
    if (in_bed_part < 0) return 1;
    const size_t cap = chunk_bytes(256);
    size_t buf_cap = cap + (1 << 20), have = 0;
    char *buf = (char *)malloc(buf_cap);
    void **d_batches = NULL;
    size_t n_batches = 0;
    int eof = 0, rc = 0;
    if (!buf) {
        fprintf(stderr, "paffy %s: out of memory\n", what);
        return 1;
    }
    if (chain && host_chain_fresh_walk() && paffy_hip_chain_fresh_walk(ctx, 1) != 0) rc = 1; /* a part under it is refused by the run */
    if ((bed ? paffy_hip_bed_begin(ctx, bed) : (chain ? paffy_hip_chain_begin(ctx) : paffy_hip_tile_begin(ctx))) != 0) rc = 1;
    while (!rc && (!eof || have > 0)) {
        if (!eof) {
            if (have == buf_cap) { /* a single line longer than the chunk: grow */
                char *nb = (char *)realloc(buf, buf_cap * 2);
                if (!nb) {
                    fprintf(stderr, "paffy %s: out of memory\n", what);
                    rc = 1;
                    break;
                }
                buf = nb;
                buf_cap *= 2;
            }
            size_t want = (have < cap ? cap : buf_cap) - have;
            size_t got = fread(buf + have, 1, want, in);
            have += got;
            if (got < want) eof = 1;
        }
        size_t use = have;
        if (!eof) {
            while (use > 0 && buf[use - 1] != '\n') use--;
            if (use == 0) continue;
        }
        if (use == 0) break;
        if (use >= ((size_t)1 << 31) - 64) {
            fprintf(stderr, "paffy %s: a single line of 2 GiB or more\n", what);
            rc = 1;
            break;
        }
        void *d = NULL;
        if (paffy_hip_malloc(&d, (int64_t)use + 64) != 0 || paffy_hip_memcpy_h2d(d, buf, (int64_t)use) != 0 ||
            (bed ? (in_bed_part ? bed_part_add(ctx, &bpart, d, buf, use) : paffy_hip_bed_add(ctx, d, (int64_t)use)) : (chain ? (in_part ? chain_part_add(ctx, &part, d, buf, use) : paffy_hip_chain_add(ctx, d, (int64_t)use)) : paffy_hip_tile_add(ctx, d, (int64_t)use))) != 0) {
            fprintf(stderr, "paffy %s: GPU call failed: %s (the input must fit the GPU's memory)\n", what, paffy_hip_last_error(ctx));
            if (d) paffy_hip_free(d);
            rc = 1;
            break;
        }
        d_batches = (void **)realloc(d_batches, sizeof(void *) * (n_batches + 1));
        d_batches[n_batches++] = d;
        memmove(buf, buf + use, have - use);
        have -= use;
    }
    free(buf);
    paffy_plan_info info;
    memset(&info, 0, sizeof(info));
    if (!rc && (bed ? (in_bed_part ? bed_part_run(ctx, bed, &bpart, &info) : paffy_hip_bed_run(ctx, bed, &info)) : (chain ? (in_part ? chain_part_run(ctx, chain, &part, &info) : paffy_hip_chain_run(ctx, chain, &info)) : paffy_hip_tile_run(ctx, &info))) != 0) {
        fprintf(stderr, "paffy %s: GPU call failed: %s\n", what, paffy_hip_last_error(ctx));
        rc = 1;
    }
    if (!rc && info.error.code) die_like_reference(&info.error, 0);
    if (!rc && info.out_bytes <= 0 && !bed && !chain && getenv("PAFFY_ROWS_FILE")) { /* under the N-GPU launcher: no output line, an empty list */
        FILE *rf = fopen(getenv("PAFFY_ROWS_FILE"), "w");
        if (!rf || fclose(rf) != 0) {
            fprintf(stderr, "paffy %s: cannot write %s\n", what, getenv("PAFFY_ROWS_FILE"));
            rc = 1;
        }
    }
    if (!rc && info.out_bytes > 0) {
        if (bed) { /* the runs: one buffer */
            void *d_out = NULL;
            char *h = (char *)malloc((size_t)info.out_bytes);
            if (h && paffy_hip_malloc(&d_out, info.out_bytes + 64) == 0 && paffy_hip_emit(ctx, d_out, info.out_bytes + 64) == 0 && paffy_hip_sync(ctx) == 0 &&
                paffy_hip_memcpy_d2h(h, d_out, info.out_bytes) == 0)
                fwrite(h, 1, (size_t)info.out_bytes, out);
            else
                rc = 1;
            free(h);
            if (d_out) paffy_hip_free(d_out);
        } else { /* the lines, as many at a time as fit the staging buffer */
            const int64_t n = info.n_rows;
            uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(n + 1));
            int64_t *offs = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1));
            int64_t stage = (int64_t)256 << 20;
            if (!rows || !offs || paffy_hip_plan_rows(ctx, n + 1, rows, offs) != n) rc = 1;
            if (!rc && getenv("PAFFY_ROWS_FILE")) { /* under the N-GPU launcher: the input record of every output line, for its merge */
                FILE *rf = fopen(getenv("PAFFY_ROWS_FILE"), "w");
                if (!rf || fwrite(rows, sizeof(uint32_t), (size_t)n, rf) != (size_t)n || fclose(rf) != 0) {
                    fprintf(stderr, "paffy %s: cannot write %s\n", what, getenv("PAFFY_ROWS_FILE"));
                    rc = 1;
                }
            }
            for (int64_t k = 0; !rc && k < n; k++)
                if (offs[k + 1] - offs[k] > stage) stage = offs[k + 1] - offs[k];
            void *d_stage = NULL;
            char *h = rc ? NULL : (char *)malloc((size_t)stage);
            if (!rc && (!h || paffy_hip_malloc(&d_stage, stage + 64) != 0)) rc = 1;
            int64_t first = 0;
            while (!rc && first < n) {
                int64_t last = first + 1;
                while (last < n && offs[last + 1] - offs[first] <= stage) last++;
                int64_t bytes = 0;
                if (paffy_hip_emit_lines(ctx, first, last - first, d_stage, stage + 64, &bytes) != 0 || paffy_hip_sync(ctx) != 0 ||
                    paffy_hip_memcpy_d2h(h, d_stage, bytes) != 0)
                    rc = 1;
                else
                    fwrite(h, 1, (size_t)bytes, out);
                first = last;
            }
            free(rows);
            free(offs);
            free(h);
            if (d_stage) paffy_hip_free(d_stage);
        }
        if (rc) fprintf(stderr, "paffy %s: GPU call failed: %s\n", what, paffy_hip_last_error(ctx));
    }
    for (size_t i = 0; i < n_batches; i++) paffy_hip_free(d_batches[i]);
    free(d_batches);
    if (part.idx) fclose(part.idx);
    if (in_bed_part) {
        fflush(out);
        if (!rc) rc = bed_part_tail(&bpart);
        bed_part_close(&bpart);
    }
    paffy_hip_destroy(ctx);
    fflush(out);
    return rc;
}

/*
 * ---- `paffy dedupe` as one of N workers of the launcher (host/paffy_launch.c): the part mode ----
 * PAFFY_DEDUPE_PART=<spooldir>/<rank>, PAFFY_DEDUPE_FDS=<from_launcher>,<to_launcher> (two inherited pipe descriptors), PAFFY_RANK,
 * PAFFY_WORLD = N and PAFFY_DEDUPE_SHARE_BYTES = C. Every worker reads the one input itself. cut(j) is the first line end at or after
 * j * C (cut(0) = 0, the last cut the file's size), share j is [cut(j), cut(j + 1)), round k is shares kN .. kN + N - 1 and this worker
 * takes share kN + rank: within a round the workers' shares are consecutive stretches of the input, which is what the part calls of
 * include/paffy_hip.h ask for, and every worker knows the number of rounds from the file's size. A record's number is cut(j) + its index
 * in the share -- a share has no more lines than bytes, so the numbers are unique and rise with the input order; nobody has to count the
 * lines in front of a share before the keys are made. A worker whose share is empty skips the source-side calls and still decides.
 * A round has four phases; after each the worker writes eight int64 {phase, 0, a, 0, 0, count, 0, 0} and reads one int64, code in the two
 * low bits (0 go on, 1 speak, 2 end), a number above them. The files, reused from round to round, lie next to each other:
 *   1 keys      <rank>.ent: the entries of part_keys, grouped by owner; <rank>.cnt: N int64, the entries per owner. count = the records
 *   2 decide    owner p reads its stretch of every <s>.ent (the counts say where) into one buffer; <p>.ver: part_decide's verdict bytes
 *   3 verdicts  the worker reads its stretch of every <p>.ver; a = its lowest failing number or -1; the answer's number is the run's + 1
 *   4 write     part_plan(the run's), the lines appended to the output spool; count = their bytes, a = 1: the failing record is here.
 *               That worker is told to speak, the number being the records in front of its share: the message is the one-worker run's.
 * End-of-file in place of an answer ends the worker.
 */
typedef struct {
    char dir[4096];
    int from_fd, to_fd, fd;
    int rank, world;
    int64_t size, share;
    double t_files, t_wait; /* seconds in the exchange files and between a report and its answer (-l INFO) */
} dedupe_part;

static double dedupe_now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static int64_t dedupe_cut(const dedupe_part *p, int64_t j) {
    if (j <= 0) return 0;
    if (j >= p->size / p->share + (p->size % p->share != 0)) return p->size;
    char blk[65536];
    for (int64_t at = j * p->share; at < p->size;) {
        const ssize_t got = pread(p->fd, blk, sizeof(blk), (off_t)at);
        if (got < 0 && errno == EINTR) continue;
        if (got <= 0) break;
        const char *nl = (const char *)memchr(blk, '\n', (size_t)got);
        if (nl) return at + (nl - blk) + 1;
        at += got;
    }
    return p->size;
}

static int dedupe_file_put(dedupe_part *p, int rank, const char *ext, const void *data, size_t bytes) {
    char path[4200];
    const double t0 = dedupe_now();
    snprintf(path, sizeof(path), "%s/%d.%s", p->dir, rank, ext);
    FILE *f = fopen(path, "w");
    int rc = !f || (bytes && fwrite(data, 1, bytes, f) != bytes);
    if (f && fclose(f) != 0) rc = 1;
    p->t_files += dedupe_now() - t0;
    if (rc) fprintf(stderr, "paffy dedupe: cannot write %s\n", path);
    return rc;
}

static int fd_get(int fd, int64_t at, void *buf, size_t bytes) {
    for (size_t have = 0; have < bytes;) {
        const ssize_t got = pread(fd, (char *)buf + have, bytes - have, (off_t)(at + (int64_t)have));
        if (got < 0 && errno == EINTR) continue;
        if (got <= 0) return 1;
        have += (size_t)got;
    }
    return 0;
}

static int dedupe_file_get(dedupe_part *p, int rank, const char *ext, int64_t at, void *buf, size_t bytes) {
    if (!bytes) return 0;
    char path[4200];
    const double t0 = dedupe_now();
    snprintf(path, sizeof(path), "%s/%d.%s", p->dir, rank, ext);
    const int fd = open(path, O_RDONLY);
    const int rc = fd < 0 || fd_get(fd, at, buf, bytes);
    if (fd >= 0) close(fd);
    p->t_files += dedupe_now() - t0;
    if (rc) fprintf(stderr, "paffy dedupe: cannot read %s\n", path);
    return rc;
}

/* a report up the pipe, the launcher's answer back; "end" ends the process here */
static int64_t dedupe_settle(dedupe_part *p, int64_t phase, int64_t a, int64_t count) {
    const int64_t rep[8] = {phase, 0, a, 0, 0, count, 0, 0};
    const double t0 = dedupe_now();
    for (size_t at = 0; at < sizeof(rep);) {
        const ssize_t k = write(p->to_fd, (const char *)rep + at, sizeof(rep) - at);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) exit(1); /* the launcher is gone */
        at += (size_t)k;
    }
    const int64_t verdict = part_verdict(p->from_fd);
    p->t_wait += dedupe_now() - t0;
    if ((verdict & 3) == 2) exit(0);
    if ((verdict & 3) == 3 || ((verdict & 3) == 1 && phase != 4)) exit(1);
    return verdict;
}

int host_dedupe_in_part(void) { return getenv("PAFFY_DEDUPE_PART") && *getenv("PAFFY_DEDUPE_PART") && getenv("PAFFY_DEDUPE_FDS"); }

int host_dedupe_part(const char *in_path, const char *out_path, int check_inverse) {
    dedupe_part P;
    memset(&P, 0, sizeof(P));
    const char *prefix = getenv("PAFFY_DEDUPE_PART"), *fds = getenv("PAFFY_DEDUPE_FDS"), *share = getenv("PAFFY_DEDUPE_SHARE_BYTES");
    const char *rank = getenv("PAFFY_RANK"), *world = getenv("PAFFY_WORLD");
    const char *slash = prefix ? strrchr(prefix, '/') : NULL;
    if (!slash || !fds || sscanf(fds, "%d,%d", &P.from_fd, &P.to_fd) != 2 || !rank || !world || !in_path || !out_path || (size_t)(slash - prefix) >= sizeof(P.dir)) {
        fprintf(stderr, "paffy dedupe: cannot use the part %s (PAFFY_DEDUPE_FDS=%s)\n", prefix ? prefix : "", fds ? fds : "");
        return 1;
    }
    memcpy(P.dir, prefix, (size_t)(slash - prefix));
    P.rank = atoi(rank);
    P.world = atoi(world);
    P.share = share && atoll(share) >= 1 ? (int64_t)atoll(share) : (int64_t)chunk_bytes(256);
    P.fd = open(in_path, O_RDONLY);
    const off_t size = P.fd < 0 ? -1 : lseek(P.fd, 0, SEEK_END);
    if (size < 0 || P.world < 1 || P.rank < 0 || P.rank >= P.world) {
        fprintf(stderr, "paffy dedupe: cannot open %s\n", in_path);
        return 1;
    }
    P.size = (int64_t)size;
    FILE *out = fopen(out_path, "w");
    if (!out) {
        fprintf(stderr, "paffy dedupe: cannot open %s\n", out_path);
        return 1;
    }
    const double t_start = dedupe_now();
    paffy_hip_ctx *ctx = open_ctx();
    if (!ctx) return 1;
    const int N = P.world, me = P.rank;
    int64_t *cnt = (int64_t *)calloc((size_t)N * (size_t)N, sizeof(int64_t)); /* cnt[s * N + p]: entries of source s for owner p */
    const int64_t shares = P.size / P.share + (P.size % P.share != 0), rounds = (shares + N - 1) / N;
    int rc = !cnt;
    for (int64_t k = 0; k < rounds && !rc; k++) {
        const int64_t a = dedupe_cut(&P, k * N + me), len = dedupe_cut(&P, k * N + me + 1) - a;
        if (len >= ((int64_t)1 << 31) - 64) {
            fprintf(stderr, "paffy dedupe: a share of 2 GiB or more\n");
            return 1;
        }
        void *d_in = NULL, *d_ent = NULL, *d_own = NULL, *d_ver = NULL, *d_out = NULL;
        char *h_in = NULL, *h_ent = NULL, *h_own = NULL, *h_ver = NULL, *h_out = NULL;
        int64_t *mine = cnt + (size_t)me * (size_t)N, n_rec = 0, n_ent = 0;
        memset(mine, 0, sizeof(int64_t) * (size_t)N);
        /* 1: the keys of this share */
        if (len > 0) {
            h_in = (char *)malloc((size_t)len);
            rc = !h_in || fd_get(P.fd, a, h_in, (size_t)len);
            int64_t lines = !rc && h_in[len - 1] != '\n';
            for (const char *q = h_in, *e = h_in + len; !rc && q < e && (q = (const char *)memchr(q, '\n', (size_t)(e - q))) != NULL; q++) lines++;
            if (!rc) rc = paffy_hip_malloc(&d_in, len + 64) || paffy_hip_memcpy_h2d(d_in, h_in, len) || paffy_hip_malloc(&d_ent, lines * 32 + 64);
            if (!rc) rc = paffy_hip_dedupe_part_keys(ctx, d_in, len, check_inverse, a, N, d_ent, lines, mine, &n_rec);
            for (int p = 0; p < N; p++) n_ent += mine[p];
            if (!rc && n_ent > 0) {
                h_ent = (char *)malloc((size_t)n_ent * 32);
                rc = !h_ent || paffy_hip_sync(ctx) || paffy_hip_memcpy_d2h(h_ent, d_ent, n_ent * 32);
            }
            free(h_in);
        }
        if (rc) break;
        if (dedupe_file_put(&P, me, "ent", h_ent, (size_t)n_ent * 32) || dedupe_file_put(&P, me, "cnt", mine, sizeof(int64_t) * (size_t)N)) return 1;
        free(h_ent);
        dedupe_settle(&P, 1, 0, n_rec);
        /* 2: the entries every worker addressed to this one, decided in one call */
        int64_t total = 0;
        for (int s = 0; s < N; s++) {
            if (dedupe_file_get(&P, s, "cnt", 0, cnt + (size_t)s * (size_t)N, sizeof(int64_t) * (size_t)N)) return 1;
            total += cnt[(size_t)s * (size_t)N + (size_t)me];
        }
        if (total > 0) {
            h_own = (char *)malloc((size_t)total * 32);
            h_ver = (char *)malloc((size_t)total);
            if (!h_own || !h_ver) return 1;
            int64_t at = 0;
            for (int s = 0; s < N; s++) {
                int64_t skip = 0;
                for (int p = 0; p < me; p++) skip += cnt[(size_t)s * (size_t)N + (size_t)p];
                const int64_t c = cnt[(size_t)s * (size_t)N + (size_t)me];
                if (dedupe_file_get(&P, s, "ent", skip * 32, h_own + at * 32, (size_t)c * 32)) return 1;
                at += c;
            }
            rc = paffy_hip_malloc(&d_own, total * 32 + 64) || paffy_hip_memcpy_h2d(d_own, h_own, total * 32) || paffy_hip_malloc(&d_ver, total + 64);
            if (!rc) rc = paffy_hip_dedupe_part_decide(ctx, d_own, total, check_inverse, d_ver);
            if (!rc) rc = paffy_hip_sync(ctx) || paffy_hip_memcpy_d2h(h_ver, d_ver, total);
            if (d_own) paffy_hip_free(d_own);
            if (d_ver) paffy_hip_free(d_ver);
            free(h_own);
            if (rc) break;
        }
        if (dedupe_file_put(&P, me, "ver", h_ver, (size_t)total)) return 1;
        free(h_ver);
        dedupe_settle(&P, 2, 0, total);
        /* 3: the owners' answers about this share */
        int64_t first_bad = -1;
        if (len > 0) {
            h_ver = (char *)malloc((size_t)n_ent + 1);
            if (!h_ver) return 1;
            int64_t at = 0;
            for (int p = 0; p < N; p++) {
                int64_t skip = 0;
                for (int s = 0; s < me; s++) skip += cnt[(size_t)s * (size_t)N + (size_t)p];
                if (dedupe_file_get(&P, p, "ver", skip, h_ver + at, (size_t)mine[p])) return 1;
                at += mine[p];
            }
            rc = paffy_hip_malloc(&d_ver, n_ent + 64) || (n_ent && paffy_hip_memcpy_h2d(d_ver, h_ver, n_ent));
            if (!rc) rc = paffy_hip_dedupe_part_verdicts(ctx, d_ver, n_ent, &first_bad);
            if (!rc) rc = paffy_hip_sync(ctx);
            if (d_ver) paffy_hip_free(d_ver);
            free(h_ver);
            if (rc) break;
        }
        const int64_t run_bad = (dedupe_settle(&P, 3, first_bad, 0) >> 2) - 1;
        /* 4: the lines of this share in front of the run's failing record */
        paffy_plan_info info;
        memset(&info, 0, sizeof(info));
        if (len > 0) {
            rc = paffy_hip_dedupe_part_plan(ctx, run_bad, &info);
            if (!rc && info.out_bytes > 0) {
                h_out = (char *)malloc((size_t)info.out_bytes);
                rc = !h_out || paffy_hip_malloc(&d_out, info.out_bytes + 64) || paffy_hip_emit(ctx, d_out, info.out_bytes + 64) || paffy_hip_sync(ctx) ||
                     paffy_hip_memcpy_d2h(h_out, d_out, info.out_bytes);
                if (!rc) rc = fwrite(h_out, 1, (size_t)info.out_bytes, out) != (size_t)info.out_bytes;
                if (d_out) paffy_hip_free(d_out);
                free(h_out);
            }
            if (!rc) rc = fflush(out) != 0; /* complete before the report that mentions the bytes */
            paffy_hip_free(d_in);
            paffy_hip_free(d_ent);
            if (rc) break;
        }
        const int64_t verdict = dedupe_settle(&P, 4, info.error.code != 0, info.out_bytes > 0 ? info.out_bytes : 0);
        if ((verdict & 3) == 1) { /* the failing record is this share's: its index here, the records in front of the share from the launcher */
            if (!info.error.code) exit(1);
            info.error.record -= a;
            die_like_reference(&info.error, verdict >> 2);
        }
    }
    if (rc) fprintf(stderr, "paffy: GPU call failed (%d): %s\n", rc, paffy_hip_last_error(ctx));
    host_log_info("paffy dedupe: part %d of %d, %lld rounds: exchange files %.3f s, waiting for the others %.3f s of %.3f s\n", me, N, (long long)rounds, P.t_files, P.t_wait,
                  dedupe_now() - t_start);
    free(cnt);
    close(P.fd);
    paffy_hip_destroy(ctx);
    return (fclose(out) != 0 || rc) ? 1 : 0;
}

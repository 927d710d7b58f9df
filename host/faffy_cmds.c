/*
 * faffy_cmds.c -- `faffy chunk | extract | merge` over the C-ABI. Each command reads its whole input into host memory, copies the
 * FASTA text to the device, indexes it (paffy_hip_fasta_index), plans its items (chunk, merge: on the host; extract: on the device, from the BED text), emits them on the device and writes the
 * bytes. Nothing is written when the plan or the base check fails: the process ends as the reference's would (status 1 for a missing
 * sequence, SIGABRT -- status 134 -- for its asserts). Files that cannot be opened give "faffy <cmd>: cannot open <path>", status 1
 * (the reference crashes instead).
 */
#define _GNU_SOURCE
#include <dirent.h>
#include <errno.h>
#include <getopt.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>

#include "../include/paffy_hip.h"
#include "faffy_host.h"
#include "fasta_files.h"

typedef struct {
    char *data;
    int64_t len, cap;
} buf_t;

static void buf_reserve(buf_t *b, int64_t more) {
    if (b->len + more + 32 <= b->cap) return;
    b->cap = (b->len + more + 32) * 2;
    b->data = (char *)realloc(b->data, (size_t)b->cap);
    if (!b->data) {
        fprintf(stderr, "faffy: out of memory\n");
        exit(1);
    }
}

/* appends the whole stream */
static void buf_read(buf_t *b, FILE *fh) {
    for (;;) {
        buf_reserve(b, 1 << 20);
        size_t got = fread(b->data + b->len, 1, (size_t)(b->cap - b->len - 32), fh);
        b->len += (int64_t)got;
        if (got == 0) break;
    }
}

static void fail_hip(const char *cmd, paffy_hip_ctx *ctx, int rc) {
    fprintf(stderr, "faffy %s: device call failed (%d): %s\n", cmd, rc, ctx ? paffy_hip_last_error(ctx) : "");
    exit(1);
}

/* the reference's ending for an error code: its message, then exit(1) or abort() */
static void fail_code(const char *cmd, int32_t code, const char *what) {
    if (paffy_hip_error_exit_status(code) == 1) {
        fprintf(stderr, "%s", what);
        exit(1);
    }
    fprintf(stderr, "faffy %s: %s\n", cmd, paffy_hip_error_string(code));
    fflush(stdout);
    abort();
}

typedef struct {
    paffy_hip_ctx *ctx;
    void *d_text, *d_out;
    char *h_out;
    int64_t out_bytes;
} faffy_run;

/* FASTA files -> device text -> index */
static void run_index(const char *cmd, faffy_run *r, const fasta_text *text) {
    int rc = paffy_hip_create(&r->ctx, -1);
    if (rc) fail_hip(cmd, NULL, rc);
    if ((rc = fasta_text_to_device(text, &r->d_text)) != 0) fail_hip(cmd, r->ctx, rc);
    int64_t n_rec = 0, n_bases = 0;
    if ((rc = paffy_hip_fasta_index(r->ctx, r->d_text, text->len, text->starts, text->n_files, &n_rec, &n_bases)) != 0) fail_hip(cmd, r->ctx, rc);
}

/* emit the planned items and bring them back; a bad base ends the process before anything is written */
static void run_emit(const char *cmd, faffy_run *r, const paffy_plan_info *info) {
    r->out_bytes = info->out_bytes;
    r->h_out = NULL;
    if (!r->out_bytes) return;
    const int64_t cap = (r->out_bytes + 15) / 16 * 16 + 16;
    int rc = paffy_hip_malloc(&r->d_out, cap);
    if (rc) fail_hip(cmd, r->ctx, rc);
    paffy_error err;
    if ((rc = paffy_hip_faffy_emit(r->ctx, r->d_out, cap, &err)) != 0) fail_hip(cmd, r->ctx, rc);
    if (err.code) fail_code(cmd, err.code, "");
    r->h_out = (char *)malloc((size_t)r->out_bytes);
    if (!r->h_out) {
        fprintf(stderr, "faffy: out of memory\n");
        exit(1);
    }
    if ((rc = paffy_hip_memcpy_d2h(r->h_out, r->d_out, r->out_bytes)) != 0) fail_hip(cmd, r->ctx, rc);
}

static void run_close(faffy_run *r) {
    free(r->h_out);
    if (r->d_out) paffy_hip_free(r->d_out);
    if (r->d_text) paffy_hip_free(r->d_text);
    if (r->ctx) paffy_hip_destroy(r->ctx);
}

/* positional FASTA files, back to back */
static int read_fastas(const char *cmd, char **paths, int n, fasta_text *text) {
    for (int i = 0; i < n; i++) {
        if (fasta_text_add(text, paths[i]) != 0) {
            fprintf(stderr, "faffy %s: cannot open %s\n", cmd, paths[i]);
            return -1;
        }
    }
    return 0;
}

static int write_all(FILE *fh, const char *p, int64_t n) { return n == 0 || fwrite(p, 1, (size_t)n, fh) == (size_t)n ? 0 : -1; }

/* ---------------------------------------------------------------- chunk */

static void chunk_usage(void) {
    fprintf(stderr, "faffy chunk [fasta_file]xN [options], MI355X build\n"
                    "Cut the sequences into chunks of chunkSize bases plus overlap; each chunk's header gets \"|length|start\" appended.\n"
                    "Chunks go into files of about chunkSize bases in the directory, whose paths are printed to stdout.\n");
    fprintf(stderr, "-c --chunkSize : chunk size (default 10000000)\n-o --overlap : overlap added to each chunk (default 100000)\n");
    fprintf(stderr, "-d --dir : an empty or missing directory for the chunk files (default ./temp_fastas)\n");
    fprintf(stderr, "-l --logLevel : log level\n-h --help : print this message\n");
}

int faffy_chunk_main(int argc, char *argv[]) {
    static struct option opts[] = {{"logLevel", required_argument, 0, 'l'}, {"chunkSize", required_argument, 0, 'c'},
                                   {"overlap", required_argument, 0, 'o'},  {"dir", required_argument, 0, 'd'},
                                   {"help", no_argument, 0, 'h'},           {0, 0, 0, 0}};
    int64_t chunk = 10000000, overlap = 100000;
    const char *dir = "./temp_fastas";
    optind = 1;
    for (;;) {
        int idx = 0, key = getopt_long(argc, argv, "l:c:o:d:h", opts, &idx);
        if (key == -1) break;
        switch (key) {
            case 'l': break;
            case 'c': chunk = atol(optarg); break;
            case 'o': overlap = atol(optarg); break;
            case 'd': dir = optarg; break;
            case 'h': chunk_usage(); return 0;
            default: chunk_usage(); return 1;
        }
    }
    int64_t sum;
    if (chunk > overlap && (chunk <= 0 || __builtin_add_overflow(chunk, overlap, &sum) || sum < 0)) {
        /* the reference loops for ever (chunkSize <= 0) or cuts negative lengths (chunkSize + overlap < 0) */
        fprintf(stderr, "faffy chunk: chunk size %" PRId64 " and overlap %" PRId64 " give no chunks (need chunkSize > 0 and chunkSize + overlap >= 0)\n",
                chunk, overlap);
        return 1;
    }
    struct stat st;
    if (stat(dir, &st) == 0) {
        if (!S_ISDIR(st.st_mode)) {
            fprintf(stderr, "Output directory is not a directory: %s", dir);
            return 1;
        }
        DIR *d = opendir(dir);
        int entries = 0;
        if (d) {
            struct dirent *e;
            while ((e = readdir(d)) != NULL)
                if (strcmp(e->d_name, ".") != 0 && strcmp(e->d_name, "..") != 0) entries++;
            closedir(d);
        }
        if (entries) {
            fprintf(stderr, "Output directory is not empty, please specify an empty directory ");
            return 1;
        }
    } else if (mkdir(dir, 0777) != 0) {
        fprintf(stderr, "faffy chunk: cannot create %s: %s\n", dir, strerror(errno));
        return 1;
    }
    fasta_text text = {0};
    if (read_fastas("chunk", argv + optind, argc - optind, &text) != 0) return 1;
    faffy_run r = {0};
    run_index("chunk", &r, &text);
    paffy_plan_info info;
    int rc = paffy_hip_faffy_chunk_plan(r.ctx, chunk, overlap, &info);
    if (rc) fail_hip("chunk", r.ctx, rc);
    if (info.error.code) fail_code("chunk", info.error.code, "");
    run_emit("chunk", &r, &info);
    const int64_t n_files = paffy_hip_faffy_chunk_files(r.ctx, 0, NULL);
    int64_t *ends = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n_files > 0 ? n_files : 1));
    paffy_hip_faffy_chunk_files(r.ctx, n_files, ends);
    int64_t at = 0;
    for (int64_t k = 0; k < n_files; k++) {
        char *path = NULL;
        if (asprintf(&path, "%s/%" PRId64 ".fa", dir, k) < 0) return 1;
        FILE *fh = fopen(path, "w");
        if (!fh || write_all(fh, r.h_out + at, ends[k] - at) != 0 || fclose(fh) != 0) {
            fprintf(stderr, "faffy chunk: cannot write %s\n", path);
            return 1;
        }
        printf("%s\n", path);
        free(path);
        at = ends[k];
    }
    free(ends);
    fasta_text_free(&text);
    run_close(&r);
    return 0;
}

/* ---------------------------------------------------------------- extract */

static void extract_usage(void) {
    fprintf(stderr, "faffy extract [fasta_file]xN [options], MI355X build\n"
                    "Write the subsequences of the intervals of a BED file (with flanks, overlapping ones merged); each header gets "
                    "\"|length|start\" appended.\n");
    fprintf(stderr, "-i --bedFile : BED intervals (default: stdin)\n-o --outputFile : FASTA output (default: stdout)\n");
    fprintf(stderr, "-f --flank : bases added at each end (default 10)\n-m --minSize : intervals shorter than this (before the flanks) are "
                    "skipped (default 100)\n");
    fprintf(stderr, "-n --skipMissing : skip intervals on sequences that are missing instead of failing\n");
    fprintf(stderr, "-l --logLevel : log level\n-h --help : print this message\n");
}

int faffy_extract_main(int argc, char *argv[]) {
    static struct option opts[] = {{"logLevel", required_argument, 0, 'l'}, {"bedFile", required_argument, 0, 'i'},
                                   {"outputFile", required_argument, 0, 'o'}, {"flank", required_argument, 0, 'f'},
                                   {"minSize", required_argument, 0, 'm'}, {"skipMissing", no_argument, 0, 'n'},
                                   {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    const char *bed_path = NULL, *out_path = NULL;
    int64_t flank = 10, min_size = 100;
    int skip = 0;
    optind = 1;
    for (;;) {
        int idx = 0, key = getopt_long(argc, argv, "l:o:f:hnm:i:", opts, &idx);
        if (key == -1) break;
        switch (key) {
            case 'l': break;
            case 'i': bed_path = optarg; break;
            case 'o': out_path = optarg; break;
            case 'f': flank = atol(optarg); break;
            case 'm': min_size = atol(optarg); break;
            case 'n': skip = 1; break;
            case 'h': extract_usage(); return 0;
            default: extract_usage(); return 1;
        }
    }
    fasta_text text = {0};
    if (read_fastas("extract", argv + optind, argc - optind, &text) != 0) return 1;
    /* the output is opened before the BED file is read (an error leaves it empty) */
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) {
        fprintf(stderr, "faffy extract: cannot open %s\n", out_path);
        return 1;
    }
    FILE *in = bed_path ? fopen(bed_path, "r") : stdin;
    if (!in) {
        fprintf(stderr, "faffy extract: cannot open %s\n", bed_path);
        return 1;
    }
    buf_t bed = {0};
    buf_read(&bed, in);
    if (bed_path) fclose(in);
    faffy_run r = {0};
    run_index("extract", &r, &text);
    paffy_plan_info info;
    int rc = paffy_hip_faffy_extract_plan(r.ctx, bed.data, bed.len, flank, min_size, skip, &info);
    if (rc) fail_hip("extract", r.ctx, rc);
    if (info.error.code == PAFFY_ERR_FAFFY_MISSING_SEQ) { /* the first token of that BED line */
        int64_t p = 0;
        for (int64_t line = 0; line < info.error.record && p < bed.len; p++)
            if (bed.data[p] == '\n') line++;
        int64_t e = p;
        while (e < bed.len && bed.data[e] != '\n') e++;
        while (p < e && (bed.data[p] == ' ' || (bed.data[p] >= '\t' && bed.data[p] <= '\r'))) p++;
        int64_t t = p;
        while (t < e && !(bed.data[t] == ' ' || (bed.data[t] >= '\t' && bed.data[t] <= '\r'))) t++;
        fprintf(stderr, "Missing sequence: %.*s\n", (int)(t - p), bed.data + p);
        exit(1);
    }
    if (info.error.code) fail_code("extract", info.error.code, "");
    run_emit("extract", &r, &info);
    if (write_all(out, r.h_out, r.out_bytes) != 0 || (out_path && fclose(out) != 0)) {
        fprintf(stderr, "faffy extract: cannot write the output\n");
        return 1;
    }
    if (!out_path) fflush(stdout);
    free(bed.data);
    fasta_text_free(&text);
    run_close(&r);
    return 0;
}

/* ---------------------------------------------------------------- merge */

static void merge_usage(void) {
    fprintf(stderr, "faffy merge [options], MI355X build\n"
                    "Join the chunks written by faffy chunk into whole sequences, splitting every overlap at its midpoint.\n");
    fprintf(stderr, "-i --inputFile : lists of chunk files, white-space separated (default: stdin)\n-o --outputFile : FASTA output (default: stdout)\n");
    fprintf(stderr, "-l --logLevel : log level\n-h --help : print this message\n");
}

int faffy_merge_main(int argc, char *argv[]) {
    static struct option opts[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'},
                                   {"outputFile", required_argument, 0, 'o'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
    const char *in_path = NULL, *out_path = NULL;
    optind = 1;
    for (;;) {
        int idx = 0, key = getopt_long(argc, argv, "l:i:o:h", opts, &idx);
        if (key == -1) break;
        switch (key) {
            case 'l': break;
            case 'i': in_path = optarg; break;
            case 'o': out_path = optarg; break;
            case 'h': merge_usage(); return 0;
            default: merge_usage(); return 1;
        }
    }
    FILE *in = in_path ? fopen(in_path, "r") : stdin;
    if (!in) {
        fprintf(stderr, "faffy merge: cannot open %s\n", in_path);
        return 1;
    }
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) {
        fprintf(stderr, "faffy merge: cannot open %s\n", out_path);
        return 1;
    }
    buf_t list = {0};
    buf_read(&list, in);
    if (in_path) fclose(in);
    buf_reserve(&list, 1);
    list.data[list.len] = '\0';
    /* every white-space separated token of the list is a chunk file, in order */
    fasta_text text = {0};
    for (char *save = NULL, *tok = strtok_r(list.data, " \t\n\r\v\f", &save); tok; tok = strtok_r(NULL, " \t\n\r\v\f", &save)) {
        if (fasta_text_add(&text, tok) != 0) {
            fprintf(stderr, "faffy merge: cannot open %s\n", tok);
            return 1;
        }
    }
    faffy_run r = {0};
    run_index("merge", &r, &text);
    paffy_plan_info info;
    int rc = paffy_hip_faffy_merge_plan(r.ctx, &info);
    if (rc) fail_hip("merge", r.ctx, rc);
    if (info.error.code) fail_code("merge", info.error.code, "");
    run_emit("merge", &r, &info);
    if (write_all(out, r.h_out, r.out_bytes) != 0 || (out_path && fclose(out) != 0)) {
        fprintf(stderr, "faffy merge: cannot write the output\n");
        return 1;
    }
    if (!out_path) fflush(stdout);
    free(list.data);
    fasta_text_free(&text);
    run_close(&r);
    return 0;
}

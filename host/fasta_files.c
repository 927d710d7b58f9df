/*
 * fasta_files.c -- see fasta_files.h.
 */
#include "fasta_files.h"

#include <stdlib.h>
#include <string.h>

#include "../include/paffy_hip.h"

static void text_reserve(fasta_text *t, int64_t more) {
    if (t->len + more + 32 <= t->cap) return;
    t->cap = (t->len + more + 32) * 2;
    t->data = (char *)realloc(t->data, (size_t)t->cap);
    if (!t->data) {
        fprintf(stderr, "out of memory reading FASTA files\n");
        exit(1);
    }
}

static void start_file(fasta_text *t) {
    if (t->n_files == t->starts_cap) {
        t->starts_cap = t->starts_cap ? t->starts_cap * 2 : 8;
        t->starts = (int64_t *)realloc(t->starts, sizeof(int64_t) * (size_t)t->starts_cap);
        if (!t->starts) {
            fprintf(stderr, "out of memory reading FASTA files\n");
            exit(1);
        }
    }
    t->starts[t->n_files++] = t->len;
}

void fasta_text_add_stream(fasta_text *t, FILE *fh) {
    start_file(t);
    for (;;) {
        text_reserve(t, 1 << 20);
        size_t got = fread(t->data + t->len, 1, (size_t)(t->cap - t->len - 32), fh);
        t->len += (int64_t)got;
        if (got == 0) break;
    }
}

int fasta_text_add(fasta_text *t, const char *path) {
    FILE *fh = fopen(path, "rb");
    if (!fh) return -1;
    fasta_text_add_stream(t, fh);
    fclose(fh);
    return 0;
}

int fasta_text_to_device(const fasta_text *t, void **d_text) {
    *d_text = NULL;
    int rc = paffy_hip_malloc(d_text, (t->len + 15) / 16 * 16 + 16);
    if (rc == 0 && t->len) rc = paffy_hip_memcpy_h2d(*d_text, t->data, t->len);
    if (rc && *d_text) {
        paffy_hip_free(*d_text);
        *d_text = NULL;
    }
    return rc;
}

void fasta_text_free(fasta_text *t) {
    free(t->data);
    free(t->starts);
    memset(t, 0, sizeof(*t));
}

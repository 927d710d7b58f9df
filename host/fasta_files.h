/*
 * fasta_files.h -- FASTA files read as raw bytes, back to back, for the device FASTA index (include/paffy_hip.h paffy_hip_fasta_index and
 * the loaders built on it). Nothing is parsed on the host: the text goes to the device as it is, with the first byte of each file.
 * Shared by bin/paffy (add_mismatches, view, upconvert, to_bed -q) and bin/faffy.
 */
#ifndef FASTA_FILES_H_
#define FASTA_FILES_H_

#include <stdint.h>
#include <stdio.h>

typedef struct {
    char *data;      /* every file's bytes, back to back */
    int64_t len, cap;
    int64_t *starts; /* starts[k]: first byte of file k */
    int32_t n_files, starts_cap;
} fasta_text;

/* appends the whole stream as one more file */
void fasta_text_add_stream(fasta_text *t, FILE *fh);
/* appends the file at path; -1 (nothing appended) when it cannot be opened */
int fasta_text_add(fasta_text *t, const char *path);
/* the text in device memory (16-byte aligned, readable to the next multiple of 16); 0 or the failing call's code */
int fasta_text_to_device(const fasta_text *t, void **d_text);
void fasta_text_free(fasta_text *t);

#endif

/*
 * paffy_host.h -- host drivers of the `paffy <command>` CLI over the gfx950 C-ABI.
 *
 * Same subcommand names, option letters / long names and exit codes as the reference CLI
 * (paffy_main.c:46-84, impl/paf_<cmd>.c getopt tables); each paffy_<cmd>_main replaces the
 * reference's per-record loop with whole-batch calls into include/paffy_hip.h.
 */
#ifndef PAFFY_HOST_H_
#define PAFFY_HOST_H_

#include <stdint.h>
#include <stdio.h>

#include "../include/paffy_hip.h"
#include "fasta_files.h"

int paffy_shatter_main(int argc, char *argv[]);
int paffy_invert_main(int argc, char *argv[]);
int paffy_filter_main(int argc, char *argv[]);
int paffy_dedupe_main(int argc, char *argv[]);
int paffy_split_file_main(int argc, char *argv[]);
int paffy_trim_main(int argc, char *argv[]);
int paffy_add_mismatches_main(int argc, char *argv[]);
int paffy_tile_main(int argc, char *argv[]);
int paffy_chain_main(int argc, char *argv[]);
int paffy_view_main(int argc, char *argv[]);
int paffy_to_bed_main(int argc, char *argv[]);
int paffy_dechunk_main(int argc, char *argv[]);
int paffy_upconvert_main(int argc, char *argv[]);

/* The input of a command: `path` (NULL: stdin). Under the N-GPU launcher (host/paffy_launch.c) a worker reads only its byte range
 * of the file: PAFFY_RANGE="first:end". */
FILE *host_open_input(const char *path);
/* The GPU this worker uses: PAFFY_DEVICE (set by the launcher), else the current device (-1). */
int host_device(void);

/* Log level shared by the drivers: 0 off, 1 info, 2 debug (set from -l/--logLevel). */
void host_set_log_level(const char *s);
void host_log_info(const char *fmt, ...);

/*
 * Stream `in` through a stage list: the input is cut into chunks that end on a line boundary,
 * every chunk is one plan/emit round trip, outputs are written in order. On a failing record
 * everything before it is written, the reference's message is printed and the process ends
 * the way the reference does (exit 1, SIGABRT or SIGSEGV). Returns 0 on success.
 */
int host_stream(const paffy_stage *stages, int n_stages, FILE *in, FILE *out);
/* Thresholds handed to the context that host_stream creates (paffy filter). */
void host_set_filter(const paffy_filter *f);
/* paffy dedupe: host_stream runs paffy_hip_dedupe_plan per chunk on one context (which remembers the records written). */
void host_set_dedupe(int check_inverse);
/* paffy dedupe under the N-GPU launcher (PAFFY_DEDUPE_PART=<spooldir>/<rank>, PAFFY_DEDUPE_FDS=<from_launcher>,<to_launcher>, PAFFY_RANK,
 * PAFFY_WORLD, PAFFY_DEDUPE_SHARE_BYTES): the worker reads share k * world + rank of the input in round k -- shares are cut at the first
 * line end at or after a multiple of the share size --, exchanges entries and verdict bytes with the other workers through files next
 * to <spooldir>/<rank> (paffy_hip_dedupe_part_keys / _decide / _verdicts / _plan), appends its lines to out_path and reports up the pipe
 * after each of a round's four phases (host/paffy_stream.c, host/paffy_launch.c). A failure is printed only by the worker the launcher
 * tells to, with the record number of the one-worker run. */
int host_dedupe_in_part(void);
int host_dedupe_part(const char *in_path, const char *out_path, int check_inverse);

/* paffy view -s -t: host_stream adds up the PAFFY_STATS sums of the chunks instead of writing lines */
void host_set_stats(int on);
void host_get_stats(int64_t sums[6], int64_t *n_records);
/* paffy view without -t: every record's paf_pretty_print stats line is written to fh as the chunks go by (NULL: off) */
void host_set_stats_lines(FILE *fh);

/* `paffy tile`: reads all of `in`, one tile_plan + emit, writes `out`. */
int host_tile(FILE *in, FILE *out);
/* `paffy to_bed`: reads all of `in`, one bed_plan + emit, writes `out`. Under the N-GPU launcher (PAFFY_BED_PART=<file prefix of the
 * part>, PAFFY_BED_FDS=<from_launcher>,<to_launcher>) `in` is one part of an input partitioned by sequence: every line has its global
 * number in <part>.idx and its side mask in <part>.sides, the block keys go to <part>.bkeys, and a failure is reported up the pipe and
 * printed only when the launcher says that it is the one the whole run ends with (host/paffy_stream.c, host/paffy_launch.c). */
int host_to_bed(FILE *in, FILE *out, const paffy_bed_opts *opts);
/* to_bed -f -q in part mode, before host_to_bed: the names of every batch are looked up in the records of t while the batch is on the
   device (<part>.seen), and the worker the launcher asks writes <part>.tail. t NULL: the file could not be opened, no records. t must
   stay valid until host_to_bed returns. */
void host_set_bed_tail(const fasta_text *t);
/* `paffy chain`: reads all of `in`, chains on the GPU, writes the records with their cn / s1 tags by descending score. Under the N-GPU
 * launcher (PAFFY_CHAIN_PART=<file prefix of the part>, PAFFY_CHAIN_FDS=<from_launcher>,<to_launcher>: two inherited pipe descriptors)
 * `in` is one part of an input partitioned by query name: the records carry the global numbers of <part>.idx, the chain keys go to
 * <part>.tails, the chain numbers come from <part>.ids, the line keys go to <part>.lkeys, and a failure is reported up the pipe and
 * printed only when the launcher says that it is the one the whole run ends with (host/paffy_stream.c, host/paffy_launch.c). */
int host_chain(FILE *in, FILE *out, const paffy_chain_opts *opts);
int host_chain_fresh_walk(void); /* PAFFY_CHAIN_FRESH_WALK=1: chain restates the reference's walk from a fresh iterator */
/* paffy split_file: normalised lines (cigar text verbatim) routed to "<prefix><contig>.paf" / "<prefix>small_<k>.paf" */
int host_split_file(FILE *in, const char *prefix, int by_query, int64_t min_length);

/* FASTA files whose sequences host_load_fasta loads (add_mismatches, view: paffy_hip_set_sequences_fasta); t must stay valid until then.
   log_count: log "Read %i sequences from sequence files" once they are loaded. */
void host_set_sequences(const fasta_text *t, int log_count);
/* FASTA files whose intervals host_load_fasta loads (upconvert: paffy_hip_set_intervals_fasta; logs the count); t must stay valid until
   then. A header that does not decode ends the process with abort() in the next host_stream, as the reference's assert does. */
void host_set_intervals(const fasta_text *t);
/* creates the context of the next host_stream and loads the FASTA files set above into it (after host_keep_raw_sequences); 0, or 1 after
   a message */
int host_load_fasta(void);
/* to_bed -q: the records of the FASTA files (header offsets into t->data, sequence lengths) and, per record, whether a line of the PAF
   text names it (paffy_hip_fasta_seen); *recs and *seen are malloc'ed. 0, or 1 after a message. */
int host_fasta_seen(const fasta_text *t, const char *paf, int64_t paf_len, int with_target, paffy_fasta_record **recs, uint8_t **seen, int64_t *n);
/* paffy view -a: keep the bases as loaded beside the upper-cased store (before host_stream), and print the rows under each stats line */
void host_keep_raw_sequences(int on);
void host_set_alignment_rows(int on);
/* paffy view without rows (every form but `-a` without `-t`): the context host_load_fasta creates next plans for the sums only
   (paffy_hip_stats_only) */
void host_set_stats_only(int on);

#endif

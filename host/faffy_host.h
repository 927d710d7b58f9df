/*
 * faffy_host.h -- host drivers of the `faffy <command>` CLI over the gfx950 C-ABI (include/paffy_hip.h, paffy_hip_fasta_* /
 * paffy_hip_faffy_*). Option letters and long names follow the reference's impl/fasta_{chunk,extract,merge}.c; numbers go through atol.
 * Options and the output directory are checked before the GPU context is created.
 */
#ifndef FAFFY_HOST_H_
#define FAFFY_HOST_H_

int faffy_chunk_main(int argc, char *argv[]);
int faffy_extract_main(int argc, char *argv[]);
int faffy_merge_main(int argc, char *argv[]);

#endif

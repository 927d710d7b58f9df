/*
 * faffy_main.c -- `faffy <command> [options]` dispatcher of the MI355X build (the reference's faffy_main.c contract): no arguments ->
 * usage, status 0; an unknown command -> "<cmd> is not a valid faffy command", usage, status 1; otherwise the command's own status.
 */
#include <stdio.h>
#include <string.h>

#include "faffy_host.h"

static void usage(void) {
    fprintf(stderr, "faffy: toolkit for working with FASTA files (MI355X build)\n\n");
    fprintf(stderr, "usage: faffy <command> [options]\n\navailable commands:\n");
    fprintf(stderr, "    chunk                    Cut FASTA sequences into overlapping chunks, one file per chunk group\n");
    fprintf(stderr, "    merge                    Join the chunks made by chunk back into whole sequences\n");
    fprintf(stderr, "    extract                  Write the subsequences of the intervals of a BED file\n\n");
}

int main(int argc, char *argv[]) {
    if (argc < 2) {
        usage();
        return 0;
    }
    if (strcmp(argv[1], "chunk") == 0) return faffy_chunk_main(argc - 1, argv + 1);
    if (strcmp(argv[1], "merge") == 0) return faffy_merge_main(argc - 1, argv + 1);
    if (strcmp(argv[1], "extract") == 0) return faffy_extract_main(argc - 1, argv + 1);
    fprintf(stderr, "%s is not a valid faffy command\n", argv[1]);
    usage();
    return 1;
}

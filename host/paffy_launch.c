/*
 * paffy_launch.c -- `bin/paffy`: the front door of the MI355X build. It never touches the GPU (it is not even linked against
 * HIP): with one GPU it replaces itself by the GPU worker `bin/paffy_gpu` (the reference's subcommands over the C-ABI,
 * host/paffy_main.c); with PAFFY_GPUS=N it is the N-GPU path behind the kept CLI -- it starts one worker process per GPU, before
 * anything has initialised a GPU, and puts their outputs together in the order one process would have written them.
 *
 * The reference's own parallelism is at this level: the user splits the input per contig and runs one `paffy` per split
 * (tests/paf_pipeline_test.sh:42-67, impl/paf_split_file.c:142-173). Here:
 *   stream commands (invert, trim, shatter, add_mismatches, filter, dechunk, upconvert): records are independent (impl/paf_invert.c:84-89), so worker r
 *     reads the r-th of N contiguous byte ranges of the input, cut at line ends (PAFFY_RANGE; no copy of the input), and writes a
 *     spool file; the spools are concatenated in rank order. A failing record ends the run as one process would: everything before it
 *     is written, the worker's exit status (or signal) becomes ours.
 *   view: a stream command whose last line is about all records. The cut, PAFFY_RANGE and the spools are the stream commands'; every worker
 *     loads the FASTA files. A worker that is given PAFFY_VIEW_SUMS=<spooldir>/<rank>.sums writes seven int64 there when it ends well (the
 *     six sums of paf_stats_calc and its record count), prints no Total-alignments line and runs neither closing assert. The spools are
 *     concatenated in rank order, the sums added up, and what paffy_view_main does behind its last record is done here: the aggregate line
 *     under -s, same float expressions and format, then the two asserts (-u, -v; an empty input fails the first: abort()). A failing worker
 *     ends the run as for the stream commands; one that ends well without sums ends it with status 1.
 *   tile: its state is per QUERY sequence (impl/paf_tile.c:160-175, impl/paf.c:675-688). The launcher makes two passes over the input
 *     (bytes of every query name; heaviest name to the lightest worker), routes every line to its worker's spool together with its
 *     global line number, each worker tiles its sequences, and the outputs -- each already in (s1 desc, AS desc, input order) order
 *     (paf_cmp_by_descending_score, impl/paf_tile.c:28-34) -- are merged by that same key. A failing record means no output at all,
 *     as in the reference (it writes after the last record).
 *   chain: records link inside one (query, target, strand) only (impl/chaining.c:37-54), so the partition is tile's (by query name,
 *     every line with its global line number). Three things are global and are settled here, on the host, from 32 bytes per chain and
 *     per line that every worker leaves in key files next to its spools:
 *       the failure that ends the run -- every worker holds its message back and reports (stage, record) after the chaining,
 *         (chain id, link) after paf_check; the launcher picks the least and only that worker speaks and sets the status;
 *       the chain numbers (cn) -- <rank>.tails: (strand class, chain-end score, processing key, global record) per chain; all chains
 *         are ranked by (class asc, score desc, key desc, number desc) and every worker gets <rank>.ids, one int64 per chain;
 *       the order of the lines -- <rank>.lkeys: (own score, chain id, link, bytes) per output line; the output is the K-way merge of
 *         the <rank>.out files by (own score desc, chain id asc, link asc), every line's length taken from its key.
 *     A chain worker is told its part by PAFFY_CHAIN_PART=<spooldir>/<rank> (it reads <part>.idx and <part>.ids, writes <part>.tails
 *     and <part>.lkeys) and talks over two inherited pipe descriptors, PAFFY_CHAIN_FDS=<from_launcher>,<to_launcher>: after each of the
 *     two phases it writes one record of eight int64 {phase, failed, sort key x 3, count, 0, 0} and reads one int64 verdict (0: go on,
 *     1: you are the failure -- say so and end as the reference would, 2: end silently). A worker that dies before it reports shows as
 *     end-of-file on its pipe: the run ends with that worker's status and nothing is written; a worker that reads end-of-file instead
 *     of a verdict exits. Nothing is written before both phases have passed everywhere (impl/paf_chain.c:128-132 writes last).
 *   to_bed: the counters are per SEQUENCE (impl/paf.c:675-712) and with -n a record counts on its query sequence and on its target
 *     sequence (impl/paf_to_bed.c:170-177), so the partition is by the names of both sides (shard.GpuBedWorker.split_sides, restated
 *     here): a name's weight is the bytes of the lines that count on it, names go heaviest first to the lightest worker, a line goes to
 *     owner(query name) with side mask 1 (3 when owner(target name) is the same worker) and, with -n and another target owner, a second
 *     time to that owner with mask 2; a line with fewer than six columns has a query side only. Worker r gets <r>.in, <r>.idx (one int64
 *     global line number per line) and <r>.sides (one mask byte per line). Three things are global and are settled here from a few int64
 *     per sequence or per part:
 *       the failure that ends the run -- a failing worker reports (global record, kind: 0 the line does not parse, 1 its query side,
 *         2 its target side: to_bed reads, counts and checks record by record, the query side first); the least speaks, of two workers
 *         that hold the same unparsable line the lower rank;
 *       the order of the sequence blocks -- <rank>.bkeys: (2 * global record of first appearance + side, block bytes, lines) per
 *         sequence, in the order of the worker's <rank>.out; all blocks are sorted by that key and copied from the mapped outputs;
 *       the -q tail (only under -f) -- <rank>.seen: one byte per FASTA record, whether a line of the part names it; the union goes
 *         to <lowest started rank>.seen_all and that one worker writes <rank>.tail, which is appended behind the last block.
 *     A bed worker is told its part by PAFFY_BED_PART=<spooldir>/<rank> and talks over PAFFY_BED_FDS=<from_launcher>,<to_launcher>,
 *     chain's protocol under names of its own: after the run it writes <part>.bkeys (and <part>.seen), reports {1, failed, record, kind,
 *     0, sequences, 0, 0} and reads a verdict; on "go on" it writes its output. Under -f -q it then reads a second verdict: 2 ends it
 *     well, 0 makes it write <part>.tail from <part>.seen_all, report {2, 0, ...} and read a last verdict. An empty input, which under
 *     -f -q still lists every FASTA record, is left to one plain worker.
 *   dedupe: "first seen wins" is a decision per class of records (a key, with -a a key and its swapped key), so it is cut by the OWNER of
 *     the class key (include/paffy_hip.h, "Dedupe in parts"), in rounds. The cut is not the stream commands': with worker r on the r-th
 *     N-th of the file, a record of worker 0's second round stands earlier in the input than its twin in worker 1's first round, and the
 *     twin would be written. With C the share size (PAFFY_CHUNK_MB), cut(j) = the first line end at or after j * C (cut(0) = 0, the last
 *     cut the file's size), share j = [cut(j), cut(j + 1)), round k = shares kN .. kN + N - 1, and worker r takes share kN + r: a round's
 *     shares are consecutive stretches of the input. Every worker reads the one input (-i, or the spooled stdin) itself and computes its
 *     cuts; we pass the path, N and C and count the rounds from the file's size, as they do. A record's number is cut(j) + its index in
 *     the share (unique, rising with the input order); the true number is needed for the message only and is summed here from the
 *     workers' record counts. Every worker is started, whatever its shares hold: it owns keys. A dedupe worker is told
 *     PAFFY_DEDUPE_PART=<spooldir>/<rank>, PAFFY_DEDUPE_FDS=<from_launcher>,<to_launcher> and PAFFY_DEDUPE_SHARE_BYTES=C and reports four
 *     times per round, eight int64 {phase, 0, a, 0, 0, count, 0, 0}; the answer is one int64, the verdict in its two low bits, a number
 *     above them:
 *       1 keys      <rank>.ent (its entries grouped by owner) and <rank>.cnt (N int64) are written; count = the share's records
 *       2 decide    it has decided the entries addressed to it (its stretch of every <s>.ent) and written <rank>.ver, a byte per entry
 *       3 verdicts  a = its lowest failing number or -1; the answer's number is the minimum over the workers + 1 (0: none)
 *       4 write     count = the bytes it appended to <rank>.out, a = 1 when it holds the failing record. The round's segments are copied
 *                   to the output in rank order. After a failure the holder is told to speak, the number being the records in front of
 *                   its share, every other worker to end, and the holder's status is ours: everything before the record is written.
 *     A worker that dies shows as end-of-file on its pipe: the run ends with its status, and what earlier rounds wrote stays. An empty
 *     input is left to one plain worker. PAFFY_DEDUPE_SHARE_BYTES in our own environment (at least 1) replaces C: a knob for rehearsals.
 * Everything between the workers goes through files under PAFFY_TMPDIR (default /dev/shm, else TMPDIR, else /tmp): host-mediated, no
 * GPU-to-GPU traffic -- a CLI's input comes from the host and its output goes back there. Other commands run on one GPU.
 *
 * Environment: PAFFY_GPUS=N; PAFFY_ONE_DEVICE=1 (rehearsal: every worker uses device 0); PAFFY_WORKER=path (another worker binary:
 * the CPU tests put a stand-in there); PAFFY_TMPDIR. Set for the workers: PAFFY_RANK, PAFFY_WORLD, PAFFY_DEVICE, PAFFY_RANGE (stream),
 * PAFFY_ROWS_FILE (tile), PAFFY_CHAIN_PART and PAFFY_CHAIN_FDS (chain), PAFFY_BED_PART and PAFFY_BED_FDS (to_bed), PAFFY_DEDUPE_PART,
 * PAFFY_DEDUPE_FDS and PAFFY_DEDUPE_SHARE_BYTES (dedupe), PAFFY_VIEW_SUMS (view).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <getopt.h>
#include <inttypes.h>
#include <limits.h>
#include <strings.h>
#include <time.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <sys/wait.h>
#include <unistd.h>

#define MAX_RANKS 64

static char g_worker[PATH_MAX];
static char g_tmpdir[PATH_MAX];  /* where the private spool directory is made */
static char g_spooldir[PATH_MAX]; /* mkdtemp(<tmpdir>/paffy.XXXXXX), mode 0700: nobody else can plant a link under a name we open */
enum { SP_IN, SP_OUT, SP_ROWS, SP_IDX, SP_TAILS, SP_IDS, SP_LKEYS, SP_SIDES, SP_BKEYS, SP_SEEN, SP_SEEN_ALL, SP_TAIL, SP_ENT, SP_CNT, SP_VER, SP_SUMS, SPOOL_KINDS };
static const char *const k_spool_ext[SPOOL_KINDS] = {"in", "out", "rows", "idx", "tails", "ids", "lkeys", "sides", "bkeys", "seen", "seen_all", "tail", "ent", "cnt", "ver", "sums"};
/* per rank: input, output, rows (tile), index, chain's tail keys, chain ids, line keys, to_bed's side masks, block keys, seen flags, their union, the -q tail,
   dedupe's entries, entry counts and verdict bytes, and view's sums */
static char g_spool[MAX_RANKS][SPOOL_KINDS][PATH_MAX];
static char g_stdin_spool[PATH_MAX];
static int g_n = 0;
static volatile pid_t g_pids[MAX_RANKS]; /* workers that are running (0: none) */

static void cleanup(void) {
    for (int r = 0; r < g_n; r++)
        for (int k = 0; k < SPOOL_KINDS; k++)
            if (g_spool[r][k][0]) unlink(g_spool[r][k]);
    if (g_stdin_spool[0]) unlink(g_stdin_spool);
    if (g_spooldir[0]) rmdir(g_spooldir);
}

/* SIGINT / SIGTERM / SIGHUP: the workers go with us and the spools (RAM-backed under /dev/shm) are removed */
static void on_signal(int sig) {
    for (int r = 0; r < MAX_RANKS; r++)
        if (g_pids[r] > 0) kill(g_pids[r], SIGTERM);
    cleanup(); /* unlink / rmdir only: async-signal-safe */
    signal(sig, SIG_DFL);
    raise(sig);
}

static int make_spooldir(void) {
    snprintf(g_spooldir, sizeof(g_spooldir), "%s/paffy.XXXXXX", g_tmpdir);
    if (!mkdtemp(g_spooldir)) {
        g_spooldir[0] = 0;
        return -1;
    }
    return 0;
}

static void find_worker(void) {
    const char *e = getenv("PAFFY_WORKER");
    if (e && *e) {
        snprintf(g_worker, sizeof(g_worker), "%s", e);
        return;
    }
    char self[PATH_MAX];
    ssize_t n = readlink("/proc/self/exe", self, sizeof(self) - 1);
    if (n <= 0) {
        snprintf(g_worker, sizeof(g_worker), "paffy_gpu");
        return;
    }
    self[n] = 0;
    char *slash = strrchr(self, '/');
    if (slash) *slash = 0;
    snprintf(g_worker, sizeof(g_worker), "%s/paffy_gpu", slash ? self : ".");
}

static void find_tmpdir(void) {
    const char *cands[] = {getenv("PAFFY_TMPDIR"), "/dev/shm", getenv("TMPDIR"), "/tmp"};
    for (size_t i = 0; i < sizeof(cands) / sizeof(cands[0]); i++)
        if (cands[i] && *cands[i] && access(cands[i], W_OK | X_OK) == 0) {
            snprintf(g_tmpdir, sizeof(g_tmpdir), "%s", cands[i]);
            return;
        }
    snprintf(g_tmpdir, sizeof(g_tmpdir), ".");
}

static int is_stream_cmd(const char *c) {
    return !strcmp(c, "invert") || !strcmp(c, "trim") || !strcmp(c, "shatter") || !strcmp(c, "add_mismatches") || !strcmp(c, "filter") ||
           !strcmp(c, "dechunk") || !strcmp(c, "upconvert");
}

/*
 * The command line of a sharded command, parsed the way the worker will parse it: getopt_long with the subcommand's own option string
 * and long options (impl/paf_invert.c:41-76, paf_trim.c:45-100, paf_add_mismatches.c:40-85, paf_filter.c:50-115,
 * paf_tile.c:100-150, paf_dechunk.c:55-66, paf_upconvert.c:84-91, paf_chain.c:62-73, paf_to_bed.c:84-135, paf_dedupe.c:63-97; --checkInverse
 * takes no value, as in host/paffy_cmds.c) -- clustered short flags (`trim -fi in.paf`), abbreviated long
 * options (`--input x`), an option's value that looks like an option (`-l -i`) all mean here what they mean there. The worker's command line is rebuilt from the parse: every
 * option but -i / -o as the worker would have seen it, then the positional arguments, then our own -i / -o. Anything getopt_long
 * rejects, and -h, leaves the command to a single worker (which prints what the reference prints).
 */
typedef struct {
    const char *in_path, *out_path;
    char *opts[256]; /* "-x" or "-x", "value" */
    int n_opts;
    char **pos; /* positional arguments (in argv order) */
    int n_pos;
    int ok;
    char **copy; /* the permuted copy of argv that pos points into (freed by main) */
} CmdLine;

static const struct option k_common[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                         {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
static const struct option k_trim[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                       {"help", no_argument, 0, 'h'}, {"trimFraction", required_argument, 0, 't'}, {"trimIdentity", required_argument, 0, 'r'},
                                       {"fixedTrim", no_argument, 0, 'f'}, {0, 0, 0, 0}};
static const struct option k_add[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                      {"removeMismatches", no_argument, 0, 'a'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
static const struct option k_filter[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                         {"minChainScore", required_argument, 0, 's'}, {"minAlignmentScore", required_argument, 0, 't'},
                                         {"minIdentity", required_argument, 0, 'u'}, {"minIdentityWithGaps", required_argument, 0, 'v'},
                                         {"maxTileLevel", required_argument, 0, 'w'}, {"invert", no_argument, 0, 'x'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

static const struct option k_dechunk[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                          {"query", no_argument, 0, 'q'}, {"target", no_argument, 0, 't'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
/* upconvert: --inFile (impl/paf_upconvert.c:84-88); its FASTA files are positional and every worker loads them */
static const struct option k_upconvert[] = {{"logLevel", required_argument, 0, 'l'}, {"inFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                            {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

static const struct option k_to_bed[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                         {"binary", no_argument, 0, 'b'}, {"excludeUnaligned", no_argument, 0, 'e'}, {"excludeAligned", no_argument, 0, 'f'},
                                         {"minSize", required_argument, 0, 'm'}, {"includeInverted", no_argument, 0, 'n'},
                                         {"queryFastaFile", required_argument, 0, 'q'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

static const struct option k_dedupe[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                         {"checkInverse", no_argument, 0, 'a'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

/* view: its FASTA files are positional and every worker loads them (impl/paf_view.c:75-105) */
static const struct option k_view[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                       {"includeAlignment", no_argument, 0, 'a'}, {"printAggregateStats", no_argument, 0, 's'}, {"noPerAlignmentStats", no_argument, 0, 't'},
                                       {"errorIfIdentityLowerThanX", required_argument, 0, 'u'}, {"errorIfAlignedBasesLowerThanX", required_argument, 0, 'v'},
                                       {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

static const struct option k_chain[] = {{"logLevel", required_argument, 0, 'l'}, {"inputFile", required_argument, 0, 'i'}, {"outputFile", required_argument, 0, 'o'},
                                        {"maxGapLength", required_argument, 0, 'g'}, {"trimFraction", required_argument, 0, 't'}, {"chainGapOpen", required_argument, 0, 'd'},
                                        {"chainGapExtend", required_argument, 0, 'e'}, {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};

static void parse_cmdline(int argc, char **argv, CmdLine *cl) {
    memset(cl, 0, sizeof(*cl));
    const char *cmd = argv[1];
    const char *optstring = "l:i:o:h";
    const struct option *lopts = k_common;
    if (!strcmp(cmd, "trim")) { optstring = "l:i:o:ht:r:f"; lopts = k_trim; }
    else if (!strcmp(cmd, "add_mismatches")) { optstring = "l:i:o:ha"; lopts = k_add; }
    else if (!strcmp(cmd, "filter")) { optstring = "l:i:o:s:t:u:v:w:xh"; lopts = k_filter; }
    else if (!strcmp(cmd, "dechunk")) { optstring = "l:i:o:hqt"; lopts = k_dechunk; }
    else if (!strcmp(cmd, "upconvert")) { optstring = "l:o:hi:"; lopts = k_upconvert; }
    else if (!strcmp(cmd, "chain")) { optstring = "l:i:o:hg:t:d:e:"; lopts = k_chain; }
    else if (!strcmp(cmd, "to_bed")) { optstring = "l:i:o:hbefm:nq:"; lopts = k_to_bed; }
    else if (!strcmp(cmd, "dedupe")) { optstring = "l:i:o:ha"; lopts = k_dedupe; }
    else if (!strcmp(cmd, "view")) { optstring = "l:i:o:hastu:v:"; lopts = k_view; }
    /* getopt_long permutes the array it is given: a copy of argv[1..] (argv[1], the subcommand, stands where the program name would) */
    char **v = (char **)calloc((size_t)argc + 1, sizeof(char *));
    for (int i = 1; i < argc; i++) v[i - 1] = argv[i];
    const int vc = argc - 1;
    static char flag[64][3];
    int n_flag = 0;
    opterr = 0;
    optind = 1;
    cl->ok = 1;
    for (;;) {
        int idx = 0;
        const int key = getopt_long(vc, v, optstring, lopts, &idx);
        if (key == -1) break;
        if (key == '?' || key == ':' || key == 'h' || cl->n_opts + 2 >= (int)(sizeof(cl->opts) / sizeof(cl->opts[0])) || n_flag >= 64) {
            cl->ok = 0;
            break;
        }
        if (key == 'i') { cl->in_path = optarg; continue; }
        if (key == 'o') { cl->out_path = optarg; continue; }
        flag[n_flag][0] = '-'; flag[n_flag][1] = (char)key; flag[n_flag][2] = 0;
        cl->opts[cl->n_opts++] = flag[n_flag++];
        if (optarg) cl->opts[cl->n_opts++] = optarg;
    }
    cl->copy = v;
    cl->pos = v + optind; /* what getopt_long moved behind the options */
    cl->n_pos = cl->ok ? vc - optind : 0;
}

static int copy_fd(int from, int to) {
    static char buf[1 << 22];
    for (;;) {
        ssize_t n = read(from, buf, sizeof(buf));
        if (n < 0) {
            if (errno == EINTR) continue;
            return -1;
        }
        if (n == 0) return 0;
        for (ssize_t o = 0; o < n;) {
            ssize_t w = write(to, buf + o, (size_t)(n - o));
            if (w < 0) {
                if (errno == EINTR) continue;
                return -1;
            }
            o += w;
        }
    }
}

/* argv of a worker: the subcommand, the options as parsed (without -i / -o), the positional arguments behind "--", then our -i / -o */
static char **worker_argv(const char *cmd, const CmdLine *cl, const char *in_path, const char *out_path) {
    char **v = (char **)calloc((size_t)cl->n_opts + (size_t)cl->n_pos + 9, sizeof(char *));
    int k = 0;
    v[k++] = g_worker;
    v[k++] = (char *)cmd;
    for (int i = 0; i < cl->n_opts; i++) v[k++] = cl->opts[i];
    v[k++] = (char *)"-i";
    v[k++] = (char *)in_path;
    v[k++] = (char *)"-o";
    v[k++] = (char *)out_path;
    if (cl->n_pos) v[k++] = (char *)"--";
    for (int i = 0; i < cl->n_pos; i++) v[k++] = cl->pos[i];
    v[k] = NULL;
    return v;
}

/* chain, to_bed, dedupe: the part's file prefix and the two pipe ends of this worker (every pipe end is close-on-exec: a worker holds its
   own two only, so the death of a worker is end-of-file on its pipe whatever the others do). kind: every command has variables of its own,
   so that a worker of one command can never take the part of another */
enum { LINK_CHAIN, LINK_BED, LINK_DEDUPE };
static const char *const k_link_part[] = {"PAFFY_CHAIN_PART", "PAFFY_BED_PART", "PAFFY_DEDUPE_PART"};
static const char *const k_link_fds[] = {"PAFFY_CHAIN_FDS", "PAFFY_BED_FDS", "PAFFY_DEDUPE_FDS"};
typedef struct {
    const char *part;
    int from_launcher, to_launcher;
    int kind;
} ChainLink;

static pid_t spawn(char **wargv, int rank, int world, int one_device, const char *range, const char *rows_path, const ChainLink *link) {
    pid_t pid = fork();
    if (pid != 0) return pid;
    char b[64];
    snprintf(b, sizeof(b), "%d", rank);
    setenv("PAFFY_RANK", b, 1);
    snprintf(b, sizeof(b), "%d", world);
    setenv("PAFFY_WORLD", b, 1);
    snprintf(b, sizeof(b), "%d", one_device ? 0 : rank);
    setenv("PAFFY_DEVICE", b, 1);
    unsetenv("PAFFY_GPUS");
    if (range) setenv("PAFFY_RANGE", range, 1);
    else unsetenv("PAFFY_RANGE");
    if (rows_path) setenv("PAFFY_ROWS_FILE", rows_path, 1);
    else unsetenv("PAFFY_ROWS_FILE");
    if (g_spool[rank][SP_SUMS][0]) setenv("PAFFY_VIEW_SUMS", g_spool[rank][SP_SUMS], 1); /* view: where this worker leaves its sums */
    else unsetenv("PAFFY_VIEW_SUMS");
    for (int k = LINK_CHAIN; k <= LINK_DEDUPE; k++) {
        unsetenv(k_link_part[k]);
        unsetenv(k_link_fds[k]);
    }
    if (link) {
        snprintf(b, sizeof(b), "%d,%d", link->from_launcher, link->to_launcher);
        setenv(k_link_part[link->kind], link->part, 1);
        setenv(k_link_fds[link->kind], b, 1);
        fcntl(link->from_launcher, F_SETFD, 0);
        fcntl(link->to_launcher, F_SETFD, 0);
    }
    execv(wargv[0], wargv);
    fprintf(stderr, "paffy: cannot start the worker %s: %s\n", wargv[0], strerror(errno));
    _exit(127);
}

/* ends this process the way worker `st` ended (after our own cleanup) */
static int status_of(int st) {
    if (WIFSIGNALED(st)) {
        cleanup();
        signal(WTERMSIG(st), SIG_DFL);
        raise(WTERMSIG(st));
        return 128 + WTERMSIG(st);
    }
    return WEXITSTATUS(st);
}

/* ---------------- stream commands, and view ---------------- */

static int read_all(int fd, void *buf, size_t n);
static int has_flag(const CmdLine *cl, char key, const char *takes_value);

/* view: the six sums and the record count of every worker that ended well, added up (paf_stats_calc's order, impl/paf.c:236-260) */
typedef struct {
    int64_t t[6], n_alignments;
} ViewTotals;

static int add_view_sums(const char *path, ViewTotals *vt) {
    int64_t rec[7];
    const int fd = open(path, O_RDONLY | O_NOFOLLOW);
    const int ok = fd >= 0 && read_all(fd, rec, sizeof(rec)) == 0;
    if (fd >= 0) close(fd);
    if (!ok) return -1;
    for (int k = 0; k < 6; k++) vt->t[k] += rec[k];
    vt->n_alignments += rec[6];
    return 0;
}

/* what paffy_view_main does behind its last record (host/paffy_cmds.c; impl/paf_view.c:163-188), on the sums of all parts: the aggregate
   line under -s, in the same float arithmetic and format, then the two asserts (NaN >= x is false: an empty input fails the first) */
static int view_close(const CmdLine *cl, const ViewTotals *vt, int out_fd) {
    float min_identity = 0.0f;
    int64_t min_aligned = 0, t[6];
    for (int i = 0; i < cl->n_opts; i++) { /* the last -u / -v holds, as in the worker's getopt loop */
        const char k = cl->opts[i][1];
        if (!strchr("luv", k)) continue;
        if (k == 'u') min_identity = (float)atof(cl->opts[i + 1]);
        if (k == 'v') min_aligned = atoi(cl->opts[i + 1]);
        i++;
    }
    memcpy(t, vt->t, sizeof(t));
    if (!has_flag(cl, 's', "luv")) memset(t, 0, sizeof(t)); /* the reference only adds the records up under -s (impl/paf_view.c:163-168) */
    else {
        char line[512];
        const int len = snprintf(line, sizeof(line), "Total-alignments:%" PRIi64 "\tAvg-Identity:%f\tAvg-Identity-with-gaps:%f\tAligned-bases:%" PRIi64
                                 "\tAligned-bases-with-gaps:%" PRIi64 "\tQuery-inserts:%" PRIi64 "\tQuery-deletes:%" PRIi64 "\n",
                                 vt->n_alignments, (float)t[0] / (t[0] + t[1]), (float)t[0] / (t[0] + t[1] + t[4] + t[5]), t[0] + t[1], t[0] + t[1] + t[4] + t[5], t[2], t[3]);
        for (int o = 0; o < len;) {
            const ssize_t w = write(out_fd, line + o, (size_t)(len - o));
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) return 1;
            o += (int)w;
        }
    }
    if (!((float)t[0] / (t[0] + t[1]) >= min_identity) || !(t[0] + t[1] >= min_aligned)) {
        fprintf(stderr, "paffy view: Assertion failed (average identity or aligned bases below the requested minimum)\n");
        cleanup();
        abort();
    }
    return 0;
}

static int run_stream(const char *cmd, const CmdLine *cl, int n, int one_device, const char *in_path, const char *out_path, ViewTotals *vt) {
    int fd = open(in_path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) {
        fprintf(stderr, "paffy %s: cannot open %s\n", cmd, in_path);
        return 1;
    }
    const int64_t size = (int64_t)sb.st_size;
    int64_t cut[MAX_RANKS + 1];
    cut[0] = 0;
    for (int r = 1; r < n; r++) { /* the first line end at or after size * r / n */
        int64_t pos = size / n * r;
        if (pos < cut[r - 1]) pos = cut[r - 1];
        char blk[65536];
        int64_t found = size;
        for (int64_t at = pos; at < size;) {
            ssize_t got = pread(fd, blk, sizeof(blk), (off_t)at);
            if (got <= 0) break;
            char *nl = (char *)memchr(blk, '\n', (size_t)got);
            if (nl) {
                found = at + (nl - blk) + 1;
                break;
            }
            at += got;
        }
        cut[r] = found;
    }
    cut[n] = size;
    close(fd);
    pid_t pids[MAX_RANKS];
    for (int r = 0; r < n; r++) {
        snprintf(g_spool[r][SP_OUT], PATH_MAX, "%s/%d.out", g_spooldir, r);
        if (vt) snprintf(g_spool[r][SP_SUMS], PATH_MAX, "%s/%d.sums", g_spooldir, r);
        char range[64];
        snprintf(range, sizeof(range), "%lld:%lld", (long long)cut[r], (long long)cut[r + 1]);
        char **wv = worker_argv(cmd, cl, in_path, g_spool[r][SP_OUT]);
        pids[r] = spawn(wv, r, n, one_device, range, NULL, NULL);
        free(wv);
        if (pids[r] < 0) {
            fprintf(stderr, "paffy: fork failed\n");
            for (int q = 0; q < r; q++) kill(pids[q], SIGTERM);
            for (int q = 0; q < r; q++) waitpid(pids[q], NULL, 0);
            return 1;
        }
        g_pids[r] = pids[r];
    }
    int out_fd = out_path ? open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666) : 1;
    if (out_fd < 0) {
        fprintf(stderr, "paffy %s: cannot open %s\n", cmd, out_path);
        for (int q = 0; q < n; q++) kill(pids[q], SIGTERM);
        for (int q = 0; q < n; q++) waitpid(pids[q], NULL, 0);
        return 1;
    }
    int rc = 0;
    for (int r = 0; r < n; r++) { /* in rank order: the output of worker r follows that of worker r - 1 */
        int st = 0;
        while (waitpid(pids[r], &st, 0) < 0 && errno == EINTR) {}
        g_pids[r] = 0;
        int sfd = open(g_spool[r][SP_OUT], O_RDONLY | O_NOFOLLOW);
        if (sfd >= 0) {
            if (copy_fd(sfd, out_fd) != 0) rc = 1;
            close(sfd);
        }
        const int failed = WIFSIGNALED(st) || WEXITSTATUS(st) != 0;
        if (failed) { /* the records before the failing one are out; nothing after them is written */
            for (int q = r + 1; q < n; q++) kill(pids[q], SIGTERM);
            for (int q = r + 1; q < n; q++) {
                waitpid(pids[q], NULL, 0);
                g_pids[q] = 0;
            }
            if (out_fd != 1) close(out_fd);
            return status_of(st);
        }
        if (vt && add_view_sums(g_spool[r][SP_SUMS], vt) != 0) { /* it ended well and left no sums: no aggregate line can be right */
            fprintf(stderr, "paffy view: worker %d left no sums in %s\n", r, g_spool[r][SP_SUMS]);
            for (int q = r + 1; q < n; q++) kill(pids[q], SIGTERM);
            for (int q = r + 1; q < n; q++) {
                waitpid(pids[q], NULL, 0);
                g_pids[q] = 0;
            }
            if (out_fd != 1) close(out_fd);
            return 1;
        }
    }
    if (vt && !rc) rc = view_close(cl, vt, out_fd);
    if (out_fd != 1) close(out_fd);
    return rc;
}

/* ---------------- tile ---------------- */

typedef struct {
    uint64_t hash;
    int64_t weight;
    int32_t owner, used;
} NameSlot;

static uint64_t name_hash(const char *s, size_t len) { /* cov_name_hash (coverage_kernel.h), shard.name_hash */
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < len; i++) h = (h ^ (unsigned char)s[i]) * 0x100000001b3ull;
    h = (h ^ (0x100u + (uint64_t)len)) * 0x100000001b3ull;
    return h ^ (h >> 29);
}

typedef struct {
    NameSlot *slot;
    size_t cap, used;
} NameTab;

static NameSlot *tab_find(NameTab *t, uint64_t h, int insert) {
    if (insert && (t->used + 1) * 2 > t->cap) { /* grow */
        NameTab nt = {NULL, t->cap ? t->cap * 2 : 1024, 0};
        nt.slot = (NameSlot *)calloc(nt.cap, sizeof(NameSlot));
        for (size_t i = 0; i < t->cap; i++)
            if (t->slot[i].used) {
                NameSlot *d = tab_find(&nt, t->slot[i].hash, 1);
                *d = t->slot[i];
            }
        free(t->slot);
        *t = nt;
    }
    if (!t->cap) return NULL;
    for (size_t i = (size_t)(h % t->cap);; i = (i + 1) % t->cap) {
        if (!t->slot[i].used) {
            if (!insert) return NULL;
            t->slot[i].used = 1;
            t->slot[i].hash = h;
            t->slot[i].weight = 0;
            t->slot[i].owner = 0;
            t->used++;
            return &t->slot[i];
        }
        if (t->slot[i].hash == h) return &t->slot[i];
    }
}

static int by_weight_desc(const void *a, const void *b) {
    const NameSlot *x = *(NameSlot *const *)a, *y = *(NameSlot *const *)b;
    if (x->weight != y->weight) return x->weight > y->weight ? -1 : 1;
    return x->hash < y->hash ? -1 : (x->hash > y->hash ? 1 : 0);
}

/* s1 and AS of an output line (impl/paf.c:343-365: tags in the order tp AS tl cn s1 cg); what paf_cmp_by_descending_score compares */
static void line_keys(const char *p, const char *e, int64_t *s1, int64_t *as) {
    *s1 = -1;
    *as = 0;
    int tabs = 0;
    while (p < e && tabs < 12) {
        const char *t = (const char *)memchr(p, '\t', (size_t)(e - p));
        if (!t) return;
        p = t + 1;
        tabs++;
    }
    while (p < e) {
        if (e - p >= 5 && p[2] == ':' && p[4] == ':') {
            if (p[0] == 'c' && p[1] == 'g') return; /* the cigar is the last tag */
            if (p[0] == 'A' && p[1] == 'S') *as = strtoll(p + 5, NULL, 10);
            if (p[0] == 's' && p[1] == '1') *s1 = strtoll(p + 5, NULL, 10);
        }
        const char *t = (const char *)memchr(p, '\t', (size_t)(e - p));
        if (!t) return;
        p = t + 1;
    }
}

typedef struct {
    const char *out, *end, *p; /* the worker's output lines */
    const uint32_t *rows;      /* local record of output line k */
    const uint64_t *idx;       /* global line number of local record j */
    int64_t k, n_rows;
    int64_t s1, as;
    uint64_t gidx;
    const char *line_end;
    size_t out_len, rows_len, idx_len;
} Cursor;

static void cursor_load(Cursor *c) {
    if (c->p >= c->end) {
        c->line_end = NULL;
        return;
    }
    const char *nl = (const char *)memchr(c->p, '\n', (size_t)(c->end - c->p));
    c->line_end = nl ? nl + 1 : c->end;
    line_keys(c->p, c->line_end, &c->s1, &c->as);
    c->gidx = c->k < c->n_rows ? c->idx[c->rows[c->k]] : ~0ull;
}

static const void *map_file(const char *path, size_t *len) {
    *len = 0;
    int fd = open(path, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) {
        if (fd >= 0) close(fd);
        return NULL;
    }
    *len = (size_t)sb.st_size;
    const void *p = *len ? mmap(NULL, *len, PROT_READ, MAP_PRIVATE, fd, 0) : (const void *)"";
    close(fd);
    return p == MAP_FAILED ? NULL : p;
}

/* the first column of the line [p, le) (le: behind its newline, nl: the newline or NULL) */
static size_t query_name_len(const char *p, const char *le, const char *nl) {
    const char *t = (const char *)memchr(p, '\t', (size_t)(le - p));
    return t ? (size_t)(t - p) : (size_t)((nl ? nl : le) - p);
}

/* the sixth column (the target name) of the line [p, e), e its newline or its end: 0 when the line has fewer than six columns */
static int target_name(const char *p, const char *e, const char **name, size_t *len) {
    for (int tabs = 0; tabs < 5; tabs++) {
        const char *t = (const char *)memchr(p, '\t', (size_t)(e - p));
        if (!t) return 0;
        p = t + 1;
    }
    const char *t = (const char *)memchr(p, '\t', (size_t)(e - p));
    *name = p;
    *len = (size_t)((t ? t : e) - p);
    return 1;
}

/*
 * The partition by name that tile, chain and to_bed share: two passes over the input (bytes of every name's lines; heaviest name to the
 * lightest worker, contig_partition of paffy_amd/shard.py), every line to <rank>.in and its global line number to <rank>.idx.
 * sides = PART_BY_QUERY (tile, chain): the names are the query names. PART_QUERY_SIDE / PART_BOTH_SIDES (to_bed without / with -n,
 * shard.GpuBedWorker.split_sides): with both sides a target name (column 6) gets the line's bytes too, the line goes to the owner of its
 * query name and, when the owner of its target name is another worker, to that one as well; <rank>.sides gets one mask byte per
 * spooled line (bit 0: count the query side here, bit 1: the target side). spooled[r]: the lines worker r got. 0, or 1 after a message.
 */
enum { PART_BY_QUERY, PART_QUERY_SIDE, PART_BOTH_SIDES };

static int partition_lines(const char *cmd, int n, const char *in_path, int64_t *spooled, int sides) {
    size_t in_len = 0;
    const char *in = (const char *)map_file(in_path, &in_len);
    if (!in) {
        fprintf(stderr, "paffy %s: cannot open %s\n", cmd, in_path);
        return 1;
    }
    /* pass 1: the bytes of every name's lines */
    NameTab tab = {NULL, 0, 0};
    for (const char *p = in, *end = in + in_len; p < end;) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl + 1 : end;
        tab_find(&tab, name_hash(p, query_name_len(p, le, nl)), 1)->weight += (int64_t)(le - p);
        const char *tn = NULL;
        size_t tlen = 0;
        if (sides == PART_BOTH_SIDES && target_name(p, nl ? nl : le, &tn, &tlen)) tab_find(&tab, name_hash(tn, tlen), 1)->weight += (int64_t)(le - p);
        p = le;
    }
    /* heaviest name to the lightest worker */
    {
        NameSlot **order = (NameSlot **)malloc(sizeof(NameSlot *) * (tab.used + 1));
        size_t m = 0;
        for (size_t i = 0; i < tab.cap; i++)
            if (tab.slot[i].used) order[m++] = &tab.slot[i];
        qsort(order, m, sizeof(NameSlot *), by_weight_desc);
        int64_t load[MAX_RANKS] = {0};
        for (size_t i = 0; i < m; i++) {
            int best = 0;
            for (int r = 1; r < n; r++)
                if (load[r] < load[best]) best = r;
            order[i]->owner = best;
            load[best] += order[i]->weight;
        }
        free(order);
    }
    /* pass 2: every line to its worker's spool, with its global line number (and its side mask) */
    FILE *fin[MAX_RANKS], *fidx[MAX_RANKS], *fsides[MAX_RANKS];
    for (int r = 0; r < n; r++) {
        for (int k = 0; k < SPOOL_KINDS; k++) snprintf(g_spool[r][k], PATH_MAX, "%s/%d.%s", g_spooldir, r, k_spool_ext[k]);
        fin[r] = fopen(g_spool[r][SP_IN], "wx"); /* O_EXCL: inside our own 0700 directory nothing can be there */
        fidx[r] = fopen(g_spool[r][SP_IDX], "wx");
        fsides[r] = sides == PART_BY_QUERY ? NULL : fopen(g_spool[r][SP_SIDES], "wx");
        if (!fin[r] || !fidx[r] || (sides != PART_BY_QUERY && !fsides[r])) {
            fprintf(stderr, "paffy %s: cannot write under %s\n", cmd, g_tmpdir);
            return 1;
        }
        setvbuf(fin[r], NULL, _IOFBF, 1 << 22);
        spooled[r] = 0;
    }
    uint64_t line_no = 0;
    for (const char *p = in, *end = in + in_len; p < end; line_no++) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *le = nl ? nl + 1 : end;
        int to[2], mask[2], copies = 1;
        to[0] = tab_find(&tab, name_hash(p, query_name_len(p, le, nl)), 0)->owner;
        mask[0] = 1;
        const char *tn = NULL;
        size_t tlen = 0;
        if (sides == PART_BOTH_SIDES && target_name(p, nl ? nl : le, &tn, &tlen)) {
            to[1] = tab_find(&tab, name_hash(tn, tlen), 0)->owner;
            mask[1] = 2;
            if (to[1] == to[0]) mask[0] = 3; /* one copy, both sides counted where it lies */
            else copies = 2;
        }
        for (int c = 0; c < copies; c++) {
            const int r = to[c];
            fwrite(p, 1, (size_t)(le - p), fin[r]);
            if (!nl) fputc('\n', fin[r]); /* a last line without its newline is a record all the same (impl/paf.c:213) */
            fwrite(&line_no, sizeof(line_no), 1, fidx[r]);
            if (fsides[r]) fputc(mask[c], fsides[r]);
            spooled[r]++;
        }
        p = le;
    }
    int werr = 0;
    for (int r = 0; r < n; r++) werr |= fclose(fin[r]) | fclose(fidx[r]) | (fsides[r] ? fclose(fsides[r]) : 0);
    if (in_len) munmap((void *)in, in_len);
    free(tab.slot);
    if (werr) {
        fprintf(stderr, "paffy %s: writing the spools under %s failed\n", cmd, g_tmpdir);
        return 1;
    }
    return 0;
}

static int partition_by_query(const char *cmd, int n, const char *in_path, int64_t *spooled) { return partition_lines(cmd, n, in_path, spooled, PART_BY_QUERY); }

static int run_tile(const CmdLine *cl, int n, int one_device, const char *in_path, const char *out_path) {
    int64_t spooled[MAX_RANKS]; /* lines routed to each worker */
    if (partition_by_query("tile", n, in_path, spooled) != 0) return 1;
    /* the workers: one per GPU that has lines to tile. Fewer query names than GPUs (one per-contig split of the input is the reference's
       own workflow, tests/paf_pipeline_test.sh:42-67) or an empty input leave workers without a line: they are not started, and the
       merge below has nothing to take from them -- the reference writes an empty output and exits 0 for an empty input */
    pid_t pids[MAX_RANKS];
    for (int r = 0; r < n; r++) {
        pids[r] = 0;
        if (spooled[r] == 0) continue;
        char **wv = worker_argv("tile", cl, g_spool[r][SP_IN], g_spool[r][SP_OUT]);
        pids[r] = spawn(wv, r, n, one_device, NULL, g_spool[r][SP_ROWS], NULL);
        free(wv);
        if (pids[r] < 0) {
            fprintf(stderr, "paffy: fork failed\n");
            for (int q = 0; q < r; q++)
                if (pids[q] > 0) kill(pids[q], SIGTERM);
            for (int q = 0; q < r; q++)
                if (pids[q] > 0) waitpid(pids[q], NULL, 0);
            return 1;
        }
        g_pids[r] = pids[r];
    }
    int bad_st = 0, any_bad = 0;
    for (int r = 0; r < n; r++) {
        if (pids[r] <= 0) continue;
        int st = 0;
        while (waitpid(pids[r], &st, 0) < 0 && errno == EINTR) {}
        g_pids[r] = 0;
        if (!any_bad && (WIFSIGNALED(st) || WEXITSTATUS(st) != 0)) {
            any_bad = 1;
            bad_st = st;
        }
    }
    if (any_bad) return status_of(bad_st); /* a failing record: nothing is written (impl/paf_tile.c:156-178 writes last) */
    /* merge: every worker's lines are in (s1 desc, AS desc, input order) order already */
    Cursor cur[MAX_RANKS];
    memset(cur, 0, sizeof(cur));
    for (int r = 0; r < n; r++) {
        Cursor *c = &cur[r];
        if (pids[r] <= 0) continue; /* no lines, no worker: line_end stays NULL */
        c->out = (const char *)map_file(g_spool[r][SP_OUT], &c->out_len);
        c->rows = (const uint32_t *)map_file(g_spool[r][SP_ROWS], &c->rows_len);
        c->idx = (const uint64_t *)map_file(g_spool[r][SP_IDX], &c->idx_len);
        if (c->out && c->out_len == 0 && !c->rows) { /* a worker that ended well and wrote nothing had nothing to list either */
            c->rows = (const uint32_t *)"";
            c->rows_len = 0;
        }
        if (!c->out || !c->rows || !c->idx) {
            fprintf(stderr, "paffy tile: worker %d left no output\n", r);
            return 1;
        }
        c->p = c->out;
        c->end = c->out + c->out_len;
        c->n_rows = (int64_t)(c->rows_len / sizeof(uint32_t));
        cursor_load(c);
    }
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) {
        fprintf(stderr, "paffy tile: cannot open %s\n", out_path);
        return 1;
    }
    setvbuf(out, NULL, _IOFBF, 1 << 22);
    for (;;) {
        int best = -1;
        for (int r = 0; r < n; r++) {
            const Cursor *c = &cur[r];
            if (!c->line_end) continue;
            if (best < 0) {
                best = r;
                continue;
            }
            const Cursor *b = &cur[best];
            if (c->s1 != b->s1 ? c->s1 > b->s1 : (c->as != b->as ? c->as > b->as : c->gidx < b->gidx)) best = r;
        }
        if (best < 0) break;
        Cursor *c = &cur[best];
        fwrite(c->p, 1, (size_t)(c->line_end - c->p), out);
        c->p = c->line_end;
        c->k++;
        cursor_load(c);
    }
    int rc = fflush(out) != 0;
    if (out != stdout) rc |= fclose(out) != 0;
    return rc;
}

/* ---------------- chain ---------------- */

enum { V_GO_ON = 0, V_YOU_FAILED = 1, V_END = 2 }; /* the verdicts */

typedef struct {
    pid_t pid;         /* 0: not started, or reaped */
    int to_fd, from_fd; /* our ends: verdicts down, reports up (-1: closed) */
    int dead, st;      /* ended without reporting; its wait status */
    int64_t rep[8];    /* the last report: phase, failed, key x 3, count, 0, 0 */
} ChainWorker;

static int read_all(int fd, void *buf, size_t n) { /* 0: n bytes; -1: end-of-file or an error before that */
    for (size_t got = 0; got < n;) {
        ssize_t k = read(fd, (char *)buf + got, n - got);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return -1;
        got += (size_t)k;
    }
    return 0;
}

static void reap(ChainWorker *w, int r) {
    if (w->pid <= 0) return;
    while (waitpid(w->pid, &w->st, 0) < 0 && errno == EINTR) {}
    g_pids[r] = 0;
    w->pid = 0;
}

static void hang_up(ChainWorker *w) {
    if (w->to_fd >= 0) close(w->to_fd);
    if (w->from_fd >= 0) close(w->from_fd);
    w->to_fd = w->from_fd = -1;
}

/* a verdict to a worker that may be gone already: the write must not end us with SIGPIPE */
static void send_verdict(ChainWorker *w, int64_t verdict) {
    if (w->to_fd < 0) return;
    struct sigaction ign, old;
    memset(&ign, 0, sizeof(ign));
    ign.sa_handler = SIG_IGN;
    sigaction(SIGPIPE, &ign, &old);
    while (write(w->to_fd, &verdict, sizeof(verdict)) < 0 && errno == EINTR) {}
    sigaction(SIGPIPE, &old, NULL);
}

/*
 * One phase's reports from every running worker (chain, to_bed or dedupe), in rank order (each of them either reports or ends: nothing here can wait for ever on a
 * dead peer). Returns -1 when all go on; else the rank whose failure ends the run -- a worker that ended without a report (the first
 * by rank) before any reported failure, among those the least sort key -- after that worker has been told to speak, every other one to
 * end, and all of them have been reaped. *st: the wait status to end with.
 */
static int chain_phase(ChainWorker *w, int n, int64_t phase, int *st) {
    int loser = -1, dead = -1;
    for (int r = 0; r < n; r++) {
        if (w[r].pid <= 0) continue;
        if (read_all(w[r].from_fd, w[r].rep, sizeof(w[r].rep)) != 0 || w[r].rep[0] != phase) {
            w[r].dead = 1;
            if (dead < 0) dead = r;
            continue;
        }
        if (!w[r].rep[1]) continue;
        if (loser < 0) { loser = r; continue; }
        const int64_t *a = w[r].rep + 2, *b = w[loser].rep + 2;
        if (a[0] != b[0] ? a[0] < b[0] : (a[1] != b[1] ? a[1] < b[1] : a[2] < b[2])) loser = r;
    }
    if (dead < 0 && loser < 0) return -1;
    if (dead >= 0) loser = dead;
    for (int r = 0; r < n; r++)
        if (w[r].pid > 0 && !w[r].dead) send_verdict(&w[r], r == loser ? V_YOU_FAILED : V_END);
    for (int r = 0; r < n; r++) {
        hang_up(&w[r]); /* whoever still waits for a verdict reads end-of-file and exits */
        reap(&w[r], r);
    }
    *st = w[loser].st;
    return loser;
}

typedef struct {
    int64_t cls, score, key, number; /* a chain's tail key */
    int32_t part;
    int64_t at; /* its place in the part's chain order */
} ChainTail;

/* the order one process pulls the chains out in (impl/chaining.c:213-230, '+' before '-', :304-305): shard.global_chain_ids */
static int by_chain_rank(const void *a, const void *b) {
    const ChainTail *x = (const ChainTail *)a, *y = (const ChainTail *)b;
    if (x->cls != y->cls) return x->cls < y->cls ? -1 : 1;
    if (x->score != y->score) return x->score > y->score ? -1 : 1;
    if (x->key != y->key) return x->key > y->key ? -1 : 1;
    if (x->number != y->number) return x->number > y->number ? -1 : 1;
    return 0;
}

/* every worker's <rank>.tails -> every worker's <rank>.ids */
static int number_chains(const ChainWorker *w, int n) {
    int64_t total = 0;
    for (int r = 0; r < n; r++)
        if (w[r].pid > 0) total += w[r].rep[5];
    if (total >= ((int64_t)1 << 31)) {
        fprintf(stderr, "paffy chain: %lld chains: more than a cn tag of the worker holds\n", (long long)total);
        return 1;
    }
    ChainTail *all = (ChainTail *)malloc(sizeof(ChainTail) * (size_t)(total + 1));
    int64_t *ids = (int64_t *)malloc(sizeof(int64_t) * (size_t)(total + 1));
    int64_t first[MAX_RANKS + 1], m = 0;
    int rc = !all || !ids;
    for (int r = 0; r < n && !rc; r++) {
        first[r] = m;
        if (w[r].pid <= 0) continue;
        size_t len = 0;
        const int64_t *t = (const int64_t *)map_file(g_spool[r][SP_TAILS], &len);
        if (!t || w[r].rep[5] < 0 || len != (size_t)w[r].rep[5] * 32) {
            fprintf(stderr, "paffy chain: worker %d left no chain keys\n", r);
            rc = 1;
            break;
        }
        for (int64_t c = 0; c < w[r].rep[5]; c++, m++) {
            ChainTail e = {t[4 * c], t[4 * c + 1], t[4 * c + 2], t[4 * c + 3], r, m};
            all[m] = e;
        }
        if (len) munmap((void *)t, len);
    }
    first[n] = m;
    if (!rc) {
        qsort(all, (size_t)m, sizeof(ChainTail), by_chain_rank);
        for (int64_t k = 0; k < m; k++) ids[all[k].at] = k; /* `at` runs over the parts one after the other */
        for (int r = 0; r < n && !rc; r++) {
            if (w[r].pid <= 0) continue;
            FILE *f = fopen(g_spool[r][SP_IDS], "wx");
            const size_t cnt = (size_t)(first[r + 1] - first[r]);
            if (!f || fwrite(ids + first[r], sizeof(int64_t), cnt, f) != cnt || fclose(f) != 0) {
                fprintf(stderr, "paffy chain: cannot write under %s\n", g_tmpdir);
                rc = 1;
            }
        }
    }
    free(all);
    free(ids);
    return rc;
}

typedef struct {
    const char *p, *end;   /* the worker's output lines */
    const int64_t *key;    /* (own score, chain id, link, bytes) of the next line; NULL: none left */
    const int64_t *key_end;
} ChainCursor;

/* the K-way merge of the workers' outputs by (own score desc, chain id asc, link asc): paf_cmp_by_score over the chains as they were
   written out (impl/chaining.c:337), shard.chain_line_offsets. A line's length is column 3 of its key. */
static int merge_chain_lines(const ChainWorker *w, int n, FILE *out) {
    ChainCursor cur[MAX_RANKS];
    memset(cur, 0, sizeof(cur));
    for (int r = 0; r < n; r++) {
        if (w[r].rep[5] <= 0) continue; /* no worker, or no line */
        size_t out_len = 0, key_len = 0;
        const char *text = (const char *)map_file(g_spool[r][SP_OUT], &out_len);
        const int64_t *keys = (const int64_t *)map_file(g_spool[r][SP_LKEYS], &key_len);
        int64_t bytes = 0;
        int ok = text && keys && key_len == (size_t)w[r].rep[5] * 32;
        for (int64_t k = 0; ok && k < w[r].rep[5]; k++) {
            if (keys[4 * k + 3] <= 0 || keys[4 * k + 3] > (int64_t)out_len - bytes) ok = 0;
            else bytes += keys[4 * k + 3];
        }
        if (!ok || bytes != (int64_t)out_len) {
            fprintf(stderr, "paffy chain: worker %d left no output\n", r);
            return 1;
        }
        cur[r].p = text;
        cur[r].end = text + out_len;
        cur[r].key = keys;
        cur[r].key_end = keys + 4 * w[r].rep[5];
    }
    for (;;) {
        int best = -1;
        for (int r = 0; r < n; r++) {
            const int64_t *a = cur[r].key;
            if (!a) continue;
            if (best < 0) {
                best = r;
                continue;
            }
            const int64_t *b = cur[best].key;
            if (a[0] != b[0] ? a[0] > b[0] : (a[1] != b[1] ? a[1] < b[1] : a[2] < b[2])) best = r;
        }
        if (best < 0) break;
        ChainCursor *c = &cur[best];
        if (fwrite(c->p, 1, (size_t)c->key[3], out) != (size_t)c->key[3]) return 1;
        c->p += c->key[3];
        c->key += 4;
        if (c->key == c->key_end) c->key = NULL;
    }
    return 0;
}

static double seconds_now(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* one worker per part that has lines (a worker without a line is not started), each with its two pipes; kind: LINK_CHAIN, LINK_BED or
   LINK_DEDUPE; in_path: the input every worker reads (dedupe), or NULL: worker r reads its own <r>.in. Returns the number of workers
   started, or -1 after a message, with those already started told to end and reaped */
static int start_part_workers(const char *cmd, const CmdLine *cl, int n, int one_device, const int64_t *spooled, ChainWorker *w, int kind, const char *in_path) {
    memset(w, 0, sizeof(ChainWorker) * MAX_RANKS);
    int started = 0;
    for (int r = 0; r < n; r++) w[r].to_fd = w[r].from_fd = -1;
    for (int r = 0; r < n; r++) {
        if (spooled[r] == 0) continue;
        int down[2], up[2];
        char part[PATH_MAX];
        snprintf(part, sizeof(part), "%s/%d", g_spooldir, r);
        if (pipe2(down, O_CLOEXEC) != 0) down[0] = down[1] = -1;
        if (down[0] < 0 || pipe2(up, O_CLOEXEC) != 0) up[0] = up[1] = -1;
        pid_t pid = -1;
        if (up[0] >= 0) {
            const ChainLink link = {part, down[0], up[1], kind};
            char **wv = worker_argv(cmd, cl, in_path ? in_path : g_spool[r][SP_IN], g_spool[r][SP_OUT]);
            pid = spawn(wv, r, n, one_device, NULL, NULL, &link);
            free(wv);
        }
        if (down[0] >= 0) close(down[0]);
        if (up[0] >= 0) close(up[1]);
        if (pid < 0) {
            fprintf(stderr, "paffy: cannot start worker %d: %s\n", r, strerror(errno));
            if (down[0] >= 0) close(down[1]);
            if (up[0] >= 0) close(up[0]);
            for (int q = 0; q < r; q++) {
                send_verdict(&w[q], V_END);
                hang_up(&w[q]);
                reap(&w[q], q);
            }
            return -1;
        }
        w[r].pid = g_pids[r] = pid;
        w[r].to_fd = down[1];
        w[r].from_fd = up[0];
        started++;
    }
    return started;
}

static int run_chain(const CmdLine *cl, int n, int one_device, const char *in_path, const char *out_path) {
    int info = 0; /* -l INFO / DEBUG: our own steps' times go to stderr */
    for (int i = 0; i + 1 < cl->n_opts; i++)
        if (!strcmp(cl->opts[i], "-l")) {
            info = !strcasecmp(cl->opts[i + 1], "INFO") || !strcasecmp(cl->opts[i + 1], "DEBUG");
            i++;
        }
    double t0 = seconds_now(), t_number = 0.0;
    int64_t spooled[MAX_RANKS];
    if (partition_by_query("chain", n, in_path, spooled) != 0) return 1;
    /* where one worker opens it (impl/paf_chain.c:125-126): a run that fails leaves the same empty file */
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) {
        fprintf(stderr, "paffy chain: cannot open %s\n", out_path);
        return 1;
    }
    const double t_partition = seconds_now() - t0;
    ChainWorker w[MAX_RANKS];
    const int started = start_part_workers("chain", cl, n, one_device, spooled, w, LINK_CHAIN, NULL);
    if (started < 0) return 1;
    int st = 0;
    for (int64_t phase = 1; phase <= 2; phase++) {
        const int loser = chain_phase(w, n, phase, &st);
        if (loser >= 0) { /* nothing is written; we end the way that worker ended */
            if (!WIFSIGNALED(st) && WEXITSTATUS(st) == 0) {
                fprintf(stderr, "paffy chain: worker %d ended without a result\n", loser);
                return 1;
            }
            return status_of(st);
        }
        if (phase == 1) {
            t0 = seconds_now();
            if (number_chains(w, n) != 0) {
                for (int r = 0; r < n; r++) {
                    send_verdict(&w[r], V_END);
                    hang_up(&w[r]);
                    reap(&w[r], r);
                }
                return 1;
            }
            t_number = seconds_now() - t0;
        }
        for (int r = 0; r < n; r++)
            if (w[r].pid > 0) send_verdict(&w[r], V_GO_ON);
    }
    int any_bad = 0;
    for (int r = 0; r < n; r++) { /* the workers write their lines and end */
        if (w[r].pid <= 0) {
            w[r].rep[5] = 0;
            continue;
        }
        hang_up(&w[r]);
        reap(&w[r], r);
        if (!any_bad && (WIFSIGNALED(w[r].st) || WEXITSTATUS(w[r].st) != 0)) {
            any_bad = 1;
            st = w[r].st;
        }
    }
    if (any_bad) return status_of(st);
    t0 = seconds_now();
    setvbuf(out, NULL, _IOFBF, 1 << 22);
    int rc = merge_chain_lines(w, n, out);
    rc |= fflush(out) != 0;
    if (out != stdout) rc |= fclose(out) != 0;
    if (info)
        fprintf(stderr, "paffy chain: %d workers; launcher: partition %.3f s, chain numbers %.3f s, merge %.3f s\n", started, t_partition, t_number,
                seconds_now() - t0);
    return rc;
}

/* ---------------- to_bed ---------------- */

/* whether the parsed command line has the flag -<key>; takes_value: the options of this command that are followed by their value */
static int has_flag(const CmdLine *cl, char key, const char *takes_value) {
    int found = 0;
    for (int i = 0; i < cl->n_opts; i++) {
        const char k = cl->opts[i][1];
        if (k == key) found = 1;
        if (strchr(takes_value, k)) i++;
    }
    return found;
}

static void end_all(ChainWorker *w, int n) {
    for (int r = 0; r < n; r++) {
        send_verdict(&w[r], V_END);
        hang_up(&w[r]);
        reap(&w[r], r);
    }
}

/* the union of the started workers' <rank>.seen (one byte per FASTA record, the same count everywhere) -> <first>.seen_all */
static int unite_seen(const ChainWorker *w, int n, int first) {
    uint8_t *all = NULL;
    size_t n_rec = 0;
    int rc = 0;
    for (int r = 0; r < n && !rc; r++) {
        if (w[r].pid <= 0) continue;
        size_t len = 0;
        const uint8_t *seen = (const uint8_t *)map_file(g_spool[r][SP_SEEN], &len);
        if (!seen || (all && len != n_rec)) {
            fprintf(stderr, "paffy to_bed: worker %d left no sequence flags\n", r);
            rc = 1;
        } else {
            if (!all) all = (uint8_t *)calloc((n_rec = len) + 1, 1);
            for (size_t k = 0; k < len; k++) all[k] |= seen[k];
        }
        if (seen && len) munmap((void *)seen, len);
    }
    if (!rc) {
        FILE *f = fopen(g_spool[first][SP_SEEN_ALL], "wx");
        if (!f || fwrite(all, 1, n_rec, f) != n_rec || fclose(f) != 0) {
            fprintf(stderr, "paffy to_bed: cannot write under %s\n", g_tmpdir);
            rc = 1;
        }
    }
    free(all);
    return rc;
}

typedef struct {
    int64_t key, bytes, from; /* 2 * global record of first appearance + side; the block's bytes; where they start in its worker's output */
    int32_t part;
} BedBlock;

static int by_block_key(const void *a, const void *b) {
    const BedBlock *x = (const BedBlock *)a, *y = (const BedBlock *)b;
    if (x->key != y->key) return x->key < y->key ? -1 : 1;
    return x->part < y->part ? -1 : (x->part > y->part ? 1 : 0);
}

/* the blocks of all workers in the order one process writes them: ascending key of first appearance (shard.bed_block_offsets). A worker's
   blocks lie back to back in its output in the order of its keys; a block of no bytes is legal (-e on an uncovered sequence) */
static int merge_bed_blocks(const ChainWorker *w, int n, FILE *out) {
    int64_t total = 0;
    for (int r = 0; r < n; r++) total += w[r].rep[5];
    BedBlock *all = (BedBlock *)malloc(sizeof(BedBlock) * (size_t)(total + 1));
    const char *text[MAX_RANKS];
    memset(text, 0, sizeof(text));
    int64_t m = 0;
    int rc = !all;
    for (int r = 0; r < n && !rc; r++) {
        if (w[r].rep[5] <= 0) continue; /* no worker, or no sequence */
        size_t out_len = 0, key_len = 0;
        text[r] = (const char *)map_file(g_spool[r][SP_OUT], &out_len);
        const int64_t *keys = (const int64_t *)map_file(g_spool[r][SP_BKEYS], &key_len);
        int64_t bytes = 0;
        int ok = text[r] && keys && key_len == (size_t)w[r].rep[5] * 24;
        for (int64_t k = 0; ok && k < w[r].rep[5]; k++, m++) {
            const int64_t len = keys[3 * k + 1];
            if (len < 0 || len > (int64_t)out_len - bytes) ok = 0;
            const BedBlock e = {keys[3 * k], len, bytes, r};
            all[m] = e;
            bytes += len;
        }
        if (!ok || bytes != (int64_t)out_len) {
            fprintf(stderr, "paffy to_bed: the output of worker %d is not what its block keys say\n", r);
            rc = 1;
        }
        if (keys && key_len) munmap((void *)keys, key_len);
    }
    if (!rc) {
        qsort(all, (size_t)m, sizeof(BedBlock), by_block_key);
        for (int64_t k = 0; k < m && !rc; k++)
            if (all[k].bytes && fwrite(text[all[k].part] + all[k].from, 1, (size_t)all[k].bytes, out) != (size_t)all[k].bytes) rc = 1;
    }
    free(all);
    return rc;
}

static int run_to_bed(const CmdLine *cl, int n, int one_device, const char *in_path, const char *out_path) {
    int log_info = 0; /* -l INFO / DEBUG: our own steps' times go to stderr */
    for (int i = 0; i < cl->n_opts; i++) {
        const char k = cl->opts[i][1];
        if (k == 'l' && i + 1 < cl->n_opts) log_info = !strcasecmp(cl->opts[i + 1], "INFO") || !strcasecmp(cl->opts[i + 1], "DEBUG");
        if (strchr("lmq", k)) i++;
    }
    const int with_target = has_flag(cl, 'n', "lmq");
    const int tail = has_flag(cl, 'f', "lmq") && has_flag(cl, 'q', "lmq"); /* impl/paf_to_bed.c:187-190: -q counts under -f only */
    double t0 = seconds_now();
    int64_t spooled[MAX_RANKS];
    if (partition_lines("to_bed", n, in_path, spooled, with_target ? PART_BOTH_SIDES : PART_QUERY_SIDE) != 0) return 1;
    /* where one worker opens it (impl/paf_to_bed.c:163): a run that fails leaves the same empty file */
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) {
        fprintf(stderr, "paffy to_bed: cannot open %s\n", out_path);
        return 1;
    }
    const double t_partition = seconds_now() - t0;
    ChainWorker w[MAX_RANKS];
    const int started = start_part_workers("to_bed", cl, n, one_device, spooled, w, LINK_BED, NULL);
    if (started < 0) return 1;
    int first = -1; /* the lowest started rank: it writes the -q tail */
    for (int r = n - 1; r >= 0; r--)
        if (w[r].pid > 0) first = r;
    int st = 0;
    int loser = chain_phase(w, n, 1, &st);
    if (loser < 0 && tail && unite_seen(w, n, first) != 0) {
        end_all(w, n);
        return 1;
    }
    if (loser < 0) {
        for (int r = 0; r < n; r++) /* every worker writes its blocks; under -f -q the next verdict waits in its pipe until it has */
            if (w[r].pid > 0) {
                send_verdict(&w[r], V_GO_ON);
                if (tail) send_verdict(&w[r], r == first ? V_GO_ON : V_END);
            }
        int any_bad = 0;
        for (int r = 0; r < n; r++) {
            if (w[r].pid <= 0) {
                w[r].rep[5] = 0;
                continue;
            }
            if (tail && r == first) continue;
            hang_up(&w[r]);
            reap(&w[r], r);
            if (!any_bad && (WIFSIGNALED(w[r].st) || WEXITSTATUS(w[r].st) != 0)) {
                any_bad = 1;
                st = w[r].st;
            }
        }
        if (any_bad) {
            end_all(w, n);
            return status_of(st);
        }
        if (tail) { /* the one worker that is left writes the tail and says so */
            const int64_t sequences = w[first].rep[5];
            loser = chain_phase(w, n, 2, &st);
            if (loser < 0) {
                w[first].rep[5] = sequences;
                send_verdict(&w[first], V_GO_ON);
                hang_up(&w[first]);
                reap(&w[first], first);
                if (WIFSIGNALED(w[first].st) || WEXITSTATUS(w[first].st) != 0) return status_of(w[first].st);
            }
        }
    }
    if (loser >= 0) { /* nothing is written; we end the way that worker ended */
        if (!WIFSIGNALED(st) && WEXITSTATUS(st) == 0) {
            fprintf(stderr, "paffy to_bed: worker %d ended without a result\n", loser);
            return 1;
        }
        return status_of(st);
    }
    t0 = seconds_now();
    setvbuf(out, NULL, _IOFBF, 1 << 22);
    int rc = merge_bed_blocks(w, n, out);
    if (!rc && tail) {
        size_t len = 0;
        const char *t = (const char *)map_file(g_spool[first][SP_TAIL], &len);
        if (!t || (len && fwrite(t, 1, len, out) != len)) {
            fprintf(stderr, "paffy to_bed: worker %d left no list of the sequences without alignments\n", first);
            rc = 1;
        }
    }
    rc |= fflush(out) != 0;
    if (out != stdout) rc |= fclose(out) != 0;
    if (log_info) fprintf(stderr, "paffy to_bed: %d workers; launcher: partition %.3f s, merge %.3f s\n", started, t_partition, seconds_now() - t0);
    return rc;
}

/* ---------------- dedupe ---------------- */

/* the share size C: PAFFY_DEDUPE_SHARE_BYTES (the rehearsal knob, at least 1), else PAFFY_CHUNK_MB as the worker's chunk_bytes() reads it */
static int64_t dedupe_share_bytes(void) {
    const char *e = getenv("PAFFY_DEDUPE_SHARE_BYTES");
    if (e && *e) {
        const long long v = atoll(e);
        return v < 1 ? 1 : (int64_t)v;
    }
    e = getenv("PAFFY_CHUNK_MB");
    long mb = e ? atol(e) : 256;
    if (mb < 1) mb = 1;
    if (mb > 1900) mb = 1900;
    return (int64_t)mb << 20;
}

/* `n` bytes of `from`, from byte `at` on, to `to` */
static int copy_range(int from, int64_t at, int64_t n, int to) {
    static char buf[1 << 22];
    while (n > 0) {
        const ssize_t got = pread(from, buf, n < (int64_t)sizeof(buf) ? (size_t)n : sizeof(buf), (off_t)at);
        if (got < 0 && errno == EINTR) continue;
        if (got <= 0) return -1;
        for (ssize_t o = 0; o < got;) {
            const ssize_t k = write(to, buf + o, (size_t)(got - o));
            if (k < 0 && errno == EINTR) continue;
            if (k < 0) return -1;
            o += k;
        }
        at += got;
        n -= got;
    }
    return 0;
}

/* A verdict to a dedupe worker: the code in the two low bits, a number above them */
static int64_t dedupe_verdict(int64_t code, int64_t number) { return (int64_t)(((uint64_t)number << 2) | (uint64_t)code); }

static int run_dedupe(const CmdLine *cl, int n, int one_device, const char *in_path, const char *out_path) {
    struct stat sb;
    if (stat(in_path, &sb) != 0) {
        fprintf(stderr, "paffy dedupe: cannot open %s\n", in_path);
        return 1;
    }
    int info = 0; /* -l INFO / DEBUG: our own steps' times go to stderr */
    for (int i = 0; i + 1 < cl->n_opts; i++)
        if (!strcmp(cl->opts[i], "-l")) {
            info = !strcasecmp(cl->opts[i + 1], "INFO") || !strcasecmp(cl->opts[i + 1], "DEBUG");
            i++;
        }
    const double t_start = seconds_now();
    double t_copy = 0.0;
    const int64_t size = (int64_t)sb.st_size, share = dedupe_share_bytes();
    const int64_t shares = size / share + (size % share != 0), rounds = (shares + n - 1) / n;
    {
        char b[32];
        snprintf(b, sizeof(b), "%lld", (long long)share);
        setenv("PAFFY_DEDUPE_SHARE_BYTES", b, 1); /* every worker cuts with the share size we count the rounds with */
    }
    /* where one worker opens it (host/paffy_cmds.c, run_stream_cmd): after the input, before the first record */
    const int out_fd = out_path ? open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0666) : 1;
    if (out_fd < 0) {
        fprintf(stderr, "paffy dedupe: cannot open %s\n", out_path);
        return 1;
    }
    int64_t spooled[MAX_RANKS];
    for (int r = 0; r < n; r++) { /* every worker is an owner in every round, whatever its shares hold */
        for (int k = 0; k < SPOOL_KINDS; k++) snprintf(g_spool[r][k], PATH_MAX, "%s/%d.%s", g_spooldir, r, k_spool_ext[k]);
        spooled[r] = 1;
    }
    ChainWorker w[MAX_RANKS];
    if (start_part_workers("dedupe", cl, n, one_device, spooled, w, LINK_DEDUPE, in_path) < 0) return 1;
    int src[MAX_RANKS], st = 0, dead = -1;
    int64_t at[MAX_RANKS], before[MAX_RANKS], records = 0;
    for (int r = 0; r < n; r++) {
        src[r] = -1;
        at[r] = 0;
    }
    for (int64_t round = 0; round < rounds; round++) {
        int64_t first_bad = -1;
        for (int64_t phase = 1; phase <= 4; phase++) {
            if ((dead = chain_phase(w, n, phase, &st)) >= 0) break; /* a worker is gone: what earlier rounds wrote stays */
            int64_t number = 0;
            if (phase == 1)
                for (int r = 0; r < n; r++) { /* the true record number of a share's first record: for the message only */
                    before[r] = records;
                    records += w[r].rep[5] > 0 ? w[r].rep[5] : 0;
                }
            if (phase == 3) { /* the run's first failing record, as its pseudo number: cut + index, which rises with the input order */
                for (int r = 0; r < n; r++)
                    if (w[r].rep[2] >= 0 && (first_bad < 0 || w[r].rep[2] < first_bad)) first_bad = w[r].rep[2];
                number = first_bad + 1;
            }
            if (phase == 4) { /* the round's output: the workers' new bytes in rank order */
                int bad = 0;
                const double t0 = seconds_now();
                for (int r = 0; r < n && !bad; r++) {
                    if (w[r].rep[5] <= 0) continue;
                    if (src[r] < 0) src[r] = open(g_spool[r][SP_OUT], O_RDONLY | O_NOFOLLOW);
                    if (src[r] < 0 || copy_range(src[r], at[r], w[r].rep[5], out_fd) != 0) bad = 1;
                    at[r] += w[r].rep[5];
                }
                t_copy += seconds_now() - t0;
                int holder = -1;
                for (int r = n - 1; r >= 0; r--)
                    if (w[r].rep[2]) holder = r;
                if (bad || (first_bad >= 0 && holder < 0)) {
                    fprintf(stderr, bad ? "paffy dedupe: cannot copy the output of a worker\n" : "paffy dedupe: no worker holds the failing record\n");
                    end_all(w, n);
                    return 1;
                }
                if (first_bad >= 0) { /* the worker that holds the record speaks, with the records in front of its share; the run ends here */
                    for (int r = 0; r < n; r++) send_verdict(&w[r], r == holder ? dedupe_verdict(V_YOU_FAILED, before[holder]) : dedupe_verdict(V_END, 0));
                    for (int r = 0; r < n; r++) {
                        hang_up(&w[r]);
                        reap(&w[r], r);
                    }
                    if (!WIFSIGNALED(w[holder].st) && WEXITSTATUS(w[holder].st) == 0) {
                        fprintf(stderr, "paffy dedupe: worker %d ended without a result\n", holder);
                        return 1;
                    }
                    return status_of(w[holder].st);
                }
            }
            for (int r = 0; r < n; r++) send_verdict(&w[r], dedupe_verdict(V_GO_ON, number));
        }
        if (dead >= 0) break;
    }
    if (dead >= 0) {
        if (!WIFSIGNALED(st) && WEXITSTATUS(st) == 0) {
            fprintf(stderr, "paffy dedupe: worker %d ended without a result\n", dead);
            return 1;
        }
        return status_of(st);
    }
    int any_bad = 0;
    for (int r = 0; r < n; r++) {
        hang_up(&w[r]);
        reap(&w[r], r);
        if (!any_bad && (WIFSIGNALED(w[r].st) || WEXITSTATUS(w[r].st) != 0)) {
            any_bad = 1;
            st = w[r].st;
        }
        if (src[r] >= 0) close(src[r]);
    }
    if (out_fd != 1 && close(out_fd) != 0) return 1;
    if (info)
        fprintf(stderr, "paffy dedupe: %d workers, %lld rounds; launcher: copy %.3f s of %.3f s\n", n, (long long)rounds, t_copy, seconds_now() - t_start);
    return any_bad ? status_of(st) : 0;
}

int main(int argc, char **argv) {
    find_worker();
    const char *g = getenv("PAFFY_GPUS");
    int n = g ? atoi(g) : 1;
    if (n > MAX_RANKS) n = MAX_RANKS;
    const int is_chain = argc >= 2 && !strcmp(argv[1], "chain");
    const int is_bed = argc >= 2 && !strcmp(argv[1], "to_bed");
    const int is_dedupe = argc >= 2 && !strcmp(argv[1], "dedupe");
    const int is_view = argc >= 2 && !strcmp(argv[1], "view");
    int shard = n > 1 && argc >= 2 && (is_stream_cmd(argv[1]) || !strcmp(argv[1], "tile") || is_chain || is_bed || is_dedupe || is_view);
    CmdLine cl;
    memset(&cl, 0, sizeof(cl));
    if (shard) {
        parse_cmdline(argc, argv, &cl);
        shard = cl.ok; /* -h, or something getopt_long would reject: the one worker says what the reference says */
        if (is_view && cl.n_pos == 0) shard = 0; /* no sequence file: it says that too (impl/paf_view.c:108-111) */
        if (shard && (is_chain || is_bed || is_dedupe) && cl.in_path) { /* and so it does for an input that cannot be opened */
            const int fd = open(cl.in_path, O_RDONLY);
            if (fd < 0) shard = 0;
            else close(fd);
        }
    }
    if (shard && is_chain && getenv("PAFFY_CHAIN_FRESH_WALK") && atoi(getenv("PAFFY_CHAIN_FRESH_WALK")) != 0) {
        /* the walk from a fresh iterator depends on a strand's leading single-group run, a property of the whole input and not of a part
           (DESIGN 3): one worker chains it, as for the commands that are not cut */
        for (int i = 0; i + 1 < cl.n_opts; i++)
            if (!strcmp(cl.opts[i], "-l") && (!strcasecmp(cl.opts[i + 1], "INFO") || !strcasecmp(cl.opts[i + 1], "DEBUG")))
                fprintf(stderr, "paffy chain: PAFFY_CHAIN_FRESH_WALK is set: chain in parts does not restate the fresh-iterator walk, running on one worker (PAFFY_GPUS=%d ignored)\n", n);
        shard = 0;
    }
    if (!shard) { /* one GPU (or a command that does not shard): this process becomes the worker; it has not touched a GPU */
        free(cl.copy);
        argv[0] = g_worker;
        execv(g_worker, argv);
        fprintf(stderr, "paffy: cannot start %s: %s\n", g_worker, strerror(errno));
        return 127;
    }
    find_tmpdir();
    if (make_spooldir() != 0) {
        fprintf(stderr, "paffy: cannot make a spool directory under %s\n", g_tmpdir);
        return 1;
    }
    g_n = n;
    atexit(cleanup);
    {
        struct sigaction sa;
        memset(&sa, 0, sizeof(sa));
        sa.sa_handler = on_signal;
        sigaction(SIGINT, &sa, NULL);
        sigaction(SIGTERM, &sa, NULL);
        sigaction(SIGHUP, &sa, NULL);
    }
    const int one_device = getenv("PAFFY_ONE_DEVICE") && atoi(getenv("PAFFY_ONE_DEVICE")) != 0;
    const char *in_path = cl.in_path, *out_path = cl.out_path;
    if (!in_path) { /* stdin: to a spool file first, the workers read ranges of it */
        snprintf(g_stdin_spool, sizeof(g_stdin_spool), "%s/stdin", g_spooldir);
        int fd = open(g_stdin_spool, O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW, 0600);
        if (fd < 0 || copy_fd(0, fd) != 0) {
            fprintf(stderr, "paffy: cannot spool the input under %s\n", g_tmpdir);
            return 1;
        }
        close(fd);
        in_path = g_stdin_spool;
    }
    if (is_bed || is_dedupe) { /* an input without a line: under to_bed -f -q one worker still lists every FASTA record, and dedupe has no round to run, so it is
                                  one plain worker's (stdin is at its end) */
        struct stat sb;
        if (stat(in_path, &sb) == 0 && sb.st_size == 0) {
            cleanup();
            free(cl.copy);
            argv[0] = g_worker;
            execv(g_worker, argv);
            fprintf(stderr, "paffy: cannot start %s: %s\n", g_worker, strerror(errno));
            return 127;
        }
    }
    ViewTotals view_totals;
    memset(&view_totals, 0, sizeof(view_totals));
    const int rc = !strcmp(argv[1], "tile") ? run_tile(&cl, n, one_device, in_path, out_path)
                   : (is_chain ? run_chain(&cl, n, one_device, in_path, out_path)
                               : (is_bed ? run_to_bed(&cl, n, one_device, in_path, out_path)
                                         : (is_dedupe ? run_dedupe(&cl, n, one_device, in_path, out_path)
                                                      : run_stream(argv[1], &cl, n, one_device, in_path, out_path, is_view ? &view_totals : NULL))));
    free(cl.copy);
    return rc;
}

#!/bin/bash
# End-to-end CLI timing of the FASTA load on the GPU box: `paffy add_mismatches` with a one-record PAF file, so that reading and loading
# the FASTA files dominates, and `paffy to_bed -f -q` with many names. Prints one JSON line per case.
# usage: tools/seqload_cli_bench.sh [genome Gb per file] [columns] [scaffolds] [to_bed names]
set -e -o pipefail
fail() { echo "$1 failed" >&2; exit 1; }
gb=${1:-3.1}; cols=${2:-60}; scaf=${3:-1000000}; names=${4:-100000}
d=$(mktemp -d)
trap 'rm -rf "$d"' EXIT
python3 - "$d" "$gb" "$cols" "$scaf" "$names" <<'PY'
import os, sys
import numpy as np
d, gb, cols, scaf, names = sys.argv[1], float(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
rng = np.random.default_rng(5)
lut = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
def genome(path, n, k=24):
    with open(path, "wb") as fh:
        for c in range(k):
            fh.write(b">chr%d\n" % c)
            left = (n // k) // cols * cols  # whole lines
            while left:
                m = min(left, cols * (1 << 16))
                b = lut[rng.integers(0, 9, m)]
                pad = (-m) % cols
                rows = np.concatenate([b, np.zeros(pad, np.uint8)]).reshape(-1, cols)
                out = np.concatenate([rows, np.full((rows.shape[0], 1), 10, np.uint8)], axis=1).reshape(-1)
                fh.write(out[:m + (m + cols - 1) // cols].tobytes())
                left -= m
genome(os.path.join(d, "a.fa"), int(gb * 1e9))
genome(os.path.join(d, "b.fa"), int(gb * 1e9))
with open(os.path.join(d, "scaf.fa"), "wb") as fh:
    for i, n in enumerate(rng.integers(1, 2001, scaf).tolist()):
        fh.write(b">scaffold_%d\n%s\n" % (i, lut[rng.integers(0, 9, n)].tobytes()))
with open(os.path.join(d, "one.paf"), "wb") as fh:
    fh.write(b"chr0\t%d\t0\t100\t+\tchr1\t%d\t0\t100\t100\t100\t60\tcg:Z:100M\n" % (int(gb * 1e9) // 24, int(gb * 1e9) // 24))
with open(os.path.join(d, "one_scaf.paf"), "wb") as fh:
    fh.write(b"scaffold_0\t1\t0\t1\t+\tscaffold_0\t1\t0\t1\t1\t1\t60\tcg:Z:1M\n")
with open(os.path.join(d, "names.fa"), "wb") as fh:
    fh.write(b"".join(b">n%d\nACGT\n" % i for i in range(names)))
with open(os.path.join(d, "names.paf"), "wb") as fh:
    fh.write(b"".join(b"n%d\t4\t0\t4\t+\tn%d\t4\t0\t4\t4\t4\t60\tcg:Z:4M\n" % (i, i + 1) for i in range(0, 2 * names, 3)))
PY
t() { local s e; s=$(date +%s.%N); "$@" > /dev/null || fail "$1"; e=$(date +%s.%N); python3 -c "print(round($e - $s, 3))"; }
ta=$(t ./bin/paffy add_mismatches -i "$d/one.paf" "$d/a.fa" "$d/b.fa")
echo "{\"cmd\": \"add_mismatches\", \"fasta\": \"2 x ${gb} Gb, ${cols} columns\", \"seconds\": $ta}"
ts=$(t ./bin/paffy add_mismatches -i "$d/one_scaf.paf" "$d/scaf.fa")
echo "{\"cmd\": \"add_mismatches\", \"fasta\": \"${scaf} scaffolds\", \"seconds\": $ts}"
tb=$(t ./bin/paffy to_bed -f -q "$d/names.fa" -i "$d/names.paf")
echo "{\"cmd\": \"to_bed -f -q\", \"fasta\": \"${names} names\", \"seconds\": $tb}"

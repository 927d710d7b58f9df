#!/usr/bin/env python3
"""Stand-in for `bin/paffy_gpu chain` in the CPU tests of the N-GPU launcher (tests/test_launcher_chain.py). The CPU oracle has no keys
to export, so this honours the part-mode contract of host/paffy_launch.c -- PAFFY_CHAIN_PART=<prefix> (reads <prefix>.idx and
<prefix>.ids, writes <prefix>.tails and <prefix>.lkeys), PAFFY_CHAIN_FDS=<from_launcher>,<to_launcher> (a report of eight int64 after each
phase, one int64 verdict back: 0 go on, 1 you are the failure, 2 end silently) -- with a deliberately trivial "chaining":

  every record is a chain of its own; its tail key is (0 for '+' / 1 for '-', AS, query start, global record number);
  its output line is the input line with "\\tcn:i:<id>" appended, own score = AS, link 0; a part's lines come by (AS desc, id asc);
  a line with strand '*' is a phase-1 failure: stage -1, exit status 1, a message that names the global record.

Switches (environment): STANDIN_CHAIN_FAIL2="g,g,..." -- a part that holds one of these global records fails phase 2 on it, with key
(chain id, 0) and exit status 1; STANDIN_CHAIN_EXIT_RANK=r -- worker r exits with status 7 before it reports; STANDIN_CHAIN_LOG=path --
every worker appends "<rank>/<world> <its arguments>". Test infrastructure only."""
import os
import struct
import sys

GO_ON, YOU_FAILED, END = 0, 1, 2


def as_of(line):
    i = line.find(b"\tAS:i:")
    return 0 if i < 0 else int(line[i + 6:].split(b"\t")[0])


def tail_key(line, number):
    f = line.split(b"\t")
    return (0 if f[4] == b"+" else 1, as_of(line), int(f[2]), number)


def main():
    args = sys.argv[1:]
    assert args[0] == "chain", args
    at = len(args) - 1 - args[::-1].index("-o")
    assert args[at - 2] == "-i", args
    inp, out = args[at - 1], args[at + 1]
    rank, world = os.environ.get("PAFFY_RANK", ""), os.environ.get("PAFFY_WORLD", "")
    if os.environ.get("STANDIN_CHAIN_LOG"):
        with open(os.environ["STANDIN_CHAIN_LOG"], "a") as fh:
            fh.write(f"{rank}/{world} {' '.join(args)}\n")
    part = os.environ["PAFFY_CHAIN_PART"]
    from_fd, to_fd = (int(x) for x in os.environ["PAFFY_CHAIN_FDS"].split(","))
    if os.environ.get("STANDIN_CHAIN_EXIT_RANK") == rank:
        sys.exit(7)

    def report(phase, failed, key, count):
        os.write(to_fd, struct.pack("<8q", phase, 1 if failed else 0, key[0], key[1], key[2], count, 0, 0))
        got = os.read(from_fd, 8)
        if len(got) < 8:
            sys.exit(1)  # end-of-file in place of a verdict
        return struct.unpack("<q", got)[0]

    def settle(phase, message, key, count):
        """report; returns on "go on", ends the process otherwise"""
        verdict = report(phase, message is not None, key, count)
        if verdict == GO_ON and message is None:
            return
        if verdict == YOU_FAILED and message is not None:
            sys.stderr.write(message + "\n")
            sys.exit(1)
        sys.exit(0 if verdict == END else 1)

    with open(inp, "rb") as fh:
        lines = fh.read().splitlines()
    with open(part + ".idx", "rb") as fh:
        raw = fh.read()
    numbers = list(struct.unpack(f"<{len(raw) // 8}q", raw))
    assert len(numbers) == len(lines), (len(numbers), len(lines))
    # phase 1
    bad = [g for ln, g in zip(lines, numbers) if ln.split(b"\t")[4] == b"*"]
    if bad:
        settle(1, f"stand-in chain: unexpected strand in record {min(bad)}", (-1, min(bad), 0), 0)
    tails = [tail_key(ln, g) for ln, g in zip(lines, numbers)]
    with open(part + ".tails", "wb") as fh:
        for t in tails:
            fh.write(struct.pack("<4q", *t))
    settle(1, None, (0, 0, 0), len(tails))
    # phase 2
    with open(part + ".ids", "rb") as fh:
        raw = fh.read()
    ids = list(struct.unpack(f"<{len(raw) // 8}q", raw))
    assert len(ids) == len(lines), (len(ids), len(lines))
    fail2 = {int(x) for x in os.environ.get("STANDIN_CHAIN_FAIL2", "").split(",") if x}
    hit = sorted((ids[k], numbers[k]) for k in range(len(lines)) if numbers[k] in fail2)
    if hit:
        settle(2, f"stand-in chain: check failed in record {hit[0][1]} (chain {hit[0][0]})", (hit[0][0], 0, 0), 0)
    order = sorted(range(len(lines)), key=lambda k: (-tails[k][1], ids[k]))
    written = [lines[k] + b"\tcn:i:%d\n" % ids[k] for k in order]
    with open(part + ".lkeys", "wb") as fh:
        for k, w in zip(order, written):
            fh.write(struct.pack("<4q", tails[k][1], ids[k], 0, len(w)))
    settle(2, None, (0, 0, 0), len(written))
    with open(out, "wb") as fh:
        fh.write(b"".join(written))


if __name__ == "__main__":
    main()

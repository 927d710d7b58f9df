"""Inputs of the device name sort (paffy_amd/csrc/name_sort_kernel.h), its decomposition restated in Python (the CPU model) and the checker.

A case is a list of FASTA headers in input order. A record's key is its header up to the first NUL byte. The checker orders the records by
(key, input index): Python compares bytes as memcmp does, then the shorter first. The model takes the same steps as the kernels -- runs,
the common-prefix skip, 8-byte words, a stable sort by (run, word), new run heads -- and counts the rounds the way the library reports them.
"""
import random

BLOCK_A, BLOCK_B = b"0000000a", b"0000000b"
SHARED = b"sharedprefix_0123"  # 17 bytes


def key_of(header):
    return header.split(b"\0", 1)[0]


def check(headers):
    """(order, name_of, n_names, name_rec) as the name table defines them"""
    keys = [key_of(h) for h in headers]
    n = len(keys)
    order = sorted(range(n), key=lambda r: (keys[r], r))
    name_of, name_rec = [0] * n, []
    for k, r in enumerate(order):
        if k == 0 or keys[r] != keys[order[k - 1]]:
            name_rec.append(-1)
        name_of[r] = len(name_rec) - 1
        if len(keys[r]) == len(headers[r]):
            name_rec[-1] = r  # the records of a name come in input order: the last whole header stays
    return order, name_of, len(name_rec), name_rec


def model(headers):
    """(order, flags, rounds, tied_after_first): the decomposition of name_sort_kernel.h, step by step"""
    keys = [key_of(h) for h in headers]
    n = len(keys)
    order = list(range(n))
    flag = [1 if k == 0 else 0 for k in range(n)]
    pos, run, depth = (list(range(n)), [0] * n, [0] * n) if n >= 2 else ([], [], [])
    rounds = tied = 0
    while pos:
        m = len(pos)
        skip = {}
        for j in range(1, m):  # (a) the common prefix of neighbours, from the run's depth on
            if run[j] == run[j - 1]:
                a, b, d = keys[order[pos[j - 1]]], keys[order[pos[j]]], depth[j]
                k = 0
                while d + k < min(len(a), len(b)) and a[d + k] == b[d + k]:
                    k += 1
                skip[run[j]] = min(skip.get(run[j], k), k)
        depth = [depth[j] + skip[run[j]] for j in range(m)]
        rec = [order[pos[j]] for j in range(m)]
        word = [keys[rec[j]][depth[j]:depth[j] + 8].ljust(8, b"\0") for j in range(m)]
        idx = sorted(range(m), key=lambda j: word[j])  # (b) two stable passes: word, then run
        idx = sorted(idx, key=lambda j: run[j])
        assert [run[j] for j in idx] == run  # the runs keep their stretches
        head = [i == 0 or run[i - 1] != run[i] or word[idx[i - 1]] != word[idx[i]] for i in range(m)] + [True]
        pos2, run2, depth2 = [], [], []
        start = 0
        for i in range(m):  # (c) new run heads
            order[pos[i]] = rec[idx[i]]
            if head[i]:
                flag[pos[i]] = 1
                start = i
            single = head[i] and (i + 1 == m or run[i + 1] != run[i] or head[i + 1])
            if not single and word[idx[i]][7] != 0:
                pos2.append(pos[i])
                run2.append(pos[start])
                depth2.append(depth[i] + 8)
        pos, run, depth = pos2, run2, depth2
        rounds += 1
        if rounds == 1:
            tied = len(pos)
    return order, flag, rounds, tied


def fasta(headers, bases=None):
    """one FASTA file of the headers; bases[r] (default: one base) on one line"""
    return b"".join(b">" + h + b"\n" + (bases[r] if bases else b"A") + b"\n" for r, h in enumerate(headers))


def distinct_bases(n, length=12, seed=17):
    rnd = random.Random(seed)
    return [bytes(rnd.choice(b"ACGT") for _ in range(length)) for _ in range(n)]


# ---- the named cases ----

EDGE_LENGTHS = (1, 7, 8, 9, 15, 16, 17)
DUP8, DUP16 = b"dup8dup8", b"dup16dup16dup16d"


def edges():
    base = [b""]
    for n in EDGE_LENGTHS:  # keys that share all but their last byte
        base += [SHARED[:n - 1] + b"x", SHARED[:n - 1] + b"y"]
    base += [b"ab", b"abc", b"pre8byte", b"pre8byteZ", b"pre16bytes_key__", b"pre16bytes_key__Z"]  # a key and its extension
    base += [b"hi\x7f", b"hi\x80", b"hi\xff"]  # unsigned order decides
    base += [b"a b", b"a\tb"]
    base += [b"cut\0one", b"cut\0two"]  # the name "cut" has no whole header
    base += [b"ab"]  # with the "ab" above and the "ab\0zz" below: one name of three records
    random.Random(5).shuffle(base)
    # a key that ends exactly at a word boundary, three times over and apart: its word has no zero byte although the key ends
    for at8, at16 in ((1, 5), (14, 20), (27, 33)):
        base.insert(at8, DUP8)
        base.insert(at16, DUP16)
    base.append(b"ab\0zz")  # the last record of the name "ab", and not a whole header
    return base


def long_names():
    x = b"x" * 4999
    y = b"y" * 4096
    return [x + b"b", y + b"1tail", x + b"a", x, y + b"2tail"]


def nested():
    keys = []
    for n in range(1, 6):
        for bits in range(1 << n):
            keys.append(b"".join(BLOCK_B if bits >> k & 1 else BLOCK_A for k in range(n)))
    rnd = random.Random(3)
    longer = [k for k in keys if len(k) > 8]
    keys += [BLOCK_A] + rnd.sample(longer, 6)  # 7 repeats; one of them a one-block key
    rnd.shuffle(keys)
    return keys


def scaffolds_plain(n=100000):
    return [b"scaffold_%d" % i for i in range(n)]


def scaffolds_spread(n=100000):
    return [b"scaffold_%d" % (i * 9973) for i in range(n)]


def all_equal(n=1000):
    return [b"one_name"] * n


def genome():
    return [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrY", b"chrM"]


RANDOM_SIZES = (0, 1, 2, 63, 64, 65, 1000, 20000)


def random_names(n, seed=None):
    rnd = random.Random(1000 + n if seed is None else seed)
    alphabet = [b"\xff", b"\x80", b"a", b"b"][:rnd.randrange(2, 5)]  # two to four letters, 0x80 and 0xff among them
    pool = [b"".join(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 41))) for _ in range(n // 3 + 1)]
    return [rnd.choice(pool) for _ in range(n)]


def named_cases():
    cases = {"edges": edges(), "long": long_names(), "nested": nested(), "scaffolds_plain": scaffolds_plain(), "scaffolds_spread": scaffolds_spread(),
             "all_equal": all_equal(), "genome": genome()}
    for n in RANDOM_SIZES:
        cases["random_%d" % n] = random_names(n)
    return cases

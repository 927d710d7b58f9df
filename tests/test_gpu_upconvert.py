"""`paffy upconvert` on the GPU (k_upconvert + the verbatim line writer) against the checker of chunk_lib (the oracle writes the bytes)."""
import os
import random
import subprocess

import pytest

import chunk_lib as K
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")

# extracted subsequences: several per name, adjacent ones sharing an endpoint (ends are inclusive), given out of order
FASTA_A = [(b"chrB|50000|20000", 5000), (b"chrA|100000|0", 1000), (b"chrA|100000|2000", 1000), (b"chrA|100000|1000", 1000),
           (b"chrC|9000|100", 800)]
FASTA_B = [(b"chrB|50000|10000", 10000), (b"chrA|100000|40000", 30000), (b"chrA|100000|3000", 500), (b"x|y|70|0x10", 20)]
FASTA = FASTA_A + FASTA_B


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def record(qn, ql, qs, qe, tn, tl, ts, te, cg=b"", strand=b"+", tags=b"\ttp:A:P\tAS:i:7"):
    cgt = b"" if cg is None else b"\tcg:Z:" + cg
    return b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t5\t9\t60%s%s\n" % (qn, ql, qs, qe, strand, tn, tl, ts, te, tags, cgt)


def records(seed, n):
    """records whose sides fall inside intervals, between them, on their shared ends, on names without intervals"""
    rnd = random.Random(seed)
    out, seen = [], set()
    names = [(b"chrA", 100000), (b"chrB", 50000), (b"chrC", 9000), (b"chrD", 7000), (b"x|y", 70)]
    while len(out) < n:
        side = []
        for _ in range(2):
            nm, ln = rnd.choice(names)
            pick = rnd.random()
            if pick < 0.3:  # on an endpoint shared by two intervals
                s = rnd.choice([1000, 2000, 3000, 0, 20000]) if nm != b"x|y" else 16
            else:
                s = rnd.randrange(0, ln - 1)
            e = min(ln, s + rnd.choice([0, 1, 5, 50, 400]))
            side.append((nm, ln, s, e))
        (qn, ql, qs, qe), (tn, tl, ts, te) = side
        key = (qn, tn, qs, qe, ts, te)
        if key in seen:
            continue
        seen.add(key)
        line = record(qn, ql, qs, qe, tn, tl, ts, te, cg=b"%dM" % max(1, qe - qs), strand=rnd.choice([b"+", b"-"]))
        exp = K.upconvert(b"".join(out) + line, FASTA)[1]
        if exp is not None:  # keep the bulk valid; the failing cases have tests of their own
            continue
        out.append(line)
    return b"".join(out)


def run(eng, data, fasta=FASTA):
    import paffy_amd

    eng.set_intervals([h for h, _ in fasta], [n for _, n in fasta])
    out, info = eng.run([paffy_amd.stage(paffy_amd.UPCONVERT)], data, raise_on_error=False)
    return out, ((info.error.code, info.error.record) if info.error.code else None), info


def test_hits_misses_and_shared_ends(eng):
    data = records(7, 600)
    want, fail = K.upconvert(data, FASTA)
    got, gfail, _ = run(eng, data)
    assert fail is None and gfail is None and got == want
    assert b"chrA|100000|1000\t" in got and b"chrD\t" in got  # renamed sides and untouched ones


def test_probe_order(eng):
    # a start of 2000 lies in [1000, 2000] and in [2000, 3000]: the bsearch probe order picks one
    data = record(b"chrA", 100000, 2000, 2000, b"chrA", 100000, 1000, 1000, cg=b"")
    want, fail = K.upconvert(data, FASTA)
    got, gfail, _ = run(eng, data)
    assert fail is None and gfail is None and got == want


def test_containment_assert(eng, tmp_path):
    good = records(3, 40)
    bad = record(b"chrA", 100000, 1500, 2600, b"chrB", 50000, 100, 200, cg=b"1100M")  # starts in [1000, 2000], ends beyond it
    data = good + bad + good[:200]
    want, fail = K.upconvert(data, FASTA)
    assert fail == (K.UPCONVERT_ASSERT, 40)
    got, gfail, info = run(eng, data)
    assert gfail == fail and info.error.stage == 0 and got == want
    fa = write_fasta(tmp_path, FASTA)
    p = subprocess.run([PAFFY, "upconvert"] + fa, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode in (134, -6) and p.stdout == want


def test_no_intervals(eng):
    data = records(5, 50)
    want, fail = K.upconvert(data, [])
    got, gfail, _ = run(eng, data, [])
    assert fail is None and gfail is None and got == want == O.dedupe(data)[0]


def test_cigar_verbatim(eng):
    data = (record(b"chrA", 100000, 10, 20, b"chrB", 50000, 20010, 20020, cg=b"10Q?9") +
            record(b"chrA", 100000, 30, 40, b"chrB", 50000, 20030, 20040, cg=None) +
            record(b"chrA", 100000, 50, 60, b"chrB", 50000, 20050, 20060, cg=b""))
    want, fail = K.upconvert(data, FASTA)
    got, gfail, _ = run(eng, data)
    assert fail is None and gfail is None and got == want and b"cg:Z:10Q?9" in got


def test_check_after_upconvert(eng):
    # the query is renamed into [0, 1000]; the target has no interval and its end passes its length: paf_check on the new coordinates
    data = records(9, 20) + record(b"chrA", 100000, 10, 20, b"chrD", 7000, 10, 7001)
    want, fail = K.upconvert(data, FASTA)
    got, gfail, _ = run(eng, data)
    assert fail == (K.CHECK_TEND, 20) and gfail == fail and got == want


def write_fasta(tmp_path, fasta, split=True):
    rnd = random.Random(1)
    files = [[], []]
    for k, (h, n) in enumerate(fasta):
        files[k % 2 if split else 0].append(b">%s\n%s\n" % (h, bytes(rnd.choice(b"ACGT") for _ in range(n))))
    paths = []
    for k, recs in enumerate(files):
        if recs:
            p = tmp_path / f"iv{k}.fa"
            p.write_bytes(b"".join(recs))
            paths.append(str(p))
    return paths


def test_cli(tmp_path):
    data = records(11, 300)
    want, _ = K.upconvert(data, FASTA)
    fa = write_fasta(tmp_path, FASTA)
    p = subprocess.run([PAFFY, "upconvert"] + fa, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == want
    inp = tmp_path / "in.paf"
    inp.write_bytes(data)
    env = dict(os.environ, PAFFY_GPUS="2", PAFFY_ONE_DEVICE="1")
    two = subprocess.run([PAFFY, "upconvert", "--inFile", str(inp)] + fa, stdout=subprocess.PIPE, env=env, timeout=300)
    assert two.returncode == 0 and two.stdout == want


def test_cli_bad_header(tmp_path):
    fa = write_fasta(tmp_path, FASTA + [(b"noheader", 10)], split=False)
    p = subprocess.run([PAFFY, "upconvert"] + fa, input=records(2, 5), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode in (134, -6) and p.stdout == b""


def test_engine_bad_header(eng):
    import paffy_amd

    with pytest.raises(RuntimeError):
        eng.set_intervals([b"a|5"], [3])
    eng.set_intervals([], [])
    assert isinstance(paffy_amd.upconvert(b"", {}), bytes)

"""`paffy dechunk` on the GPU (k_dechunk + the flat pass) against the checker of chunk_lib (the oracle writes the bytes)."""
import os
import subprocess

import pytest

import chunk_lib as K
import oracle_lib as O
import synth_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
STYLES = (b"%d", b"0x%x", b"0%o", b"+%d", b" %d", b"0X%X")


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def cfgs():
    return {"cfg1": synth_lib.generate(0x5EED0001, 64, 0, 400), "cfg2": synth_lib.generate(0x5EED0002, 512, 0, 200),
            "cfg3": synth_lib.generate(0x5EED0003, 2048, 0, 120)}


def stage_dechunk(q=True, t=True):
    import paffy_amd

    return paffy_amd.stage_dechunk(q, t)


def run(eng, stages, data):
    out, info = eng.run(stages, data, raise_on_error=False)
    fail = (info.error.code, info.error.record) if info.error.code else None
    return out, fail, info


def lines(data):
    return data.split(b"\n")[:-1]


@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg3"])
def test_round_trip(eng, cfgs, cfg):
    x = cfgs[cfg]
    want, fail = K.dechunk(x, query=False, target=False)  # PASS + paf_check of the original
    assert fail is None
    enc = K.chunk_encode(x, styles=STYLES)
    got, gfail, info = run(eng, [stage_dechunk()], enc)
    assert gfail is None and got == want
    assert K.dechunk(enc) == (want, None)


@pytest.mark.parametrize("q,t", [(True, False), (False, True), (False, False)])
def test_flags(eng, cfgs, q, t):
    x = cfgs["cfg2"]
    enc = K.chunk_encode(x, styles=STYLES)
    part = lines(enc)
    # only the fixed side is encoded: the other keeps its plain name
    src = lines(x)
    mixed = []
    for a, b in zip(part, src):
        fa, fb = a.split(b"\t"), b.split(b"\t")
        for on, idx in ((q, (0, 1, 2, 3)), (t, (5, 6, 7, 8))):
            if not on:
                for k in idx:
                    fa[k] = fb[k]
        mixed.append(b"\t".join(fa) + b"\n")
    data = b"".join(mixed)
    want, fail = K.dechunk(data, q, t)
    got, gfail, _ = run(eng, [stage_dechunk(q, t)], data)
    assert fail is None and gfail is None and got == want
    if not (q or t):
        assert got == O.run([O.stage(O.PASS)], data)[0]


BAD_NAMES = [b"plain", b"x|5", b"x||5", b"x|abc|5", b"x|100|zz", b"x|100|"]


@pytest.mark.parametrize("bad", BAD_NAMES)
@pytest.mark.parametrize("side", [0, 5])
def test_malformed_names(eng, cfgs, bad, side):
    enc = lines(K.chunk_encode(cfgs["cfg1"]))
    at = 37
    f = enc[at].split(b"\t")
    f[side] = bad
    enc[at] = b"\t".join(f)
    data = b"\n".join(enc) + b"\n"
    want, fail = K.dechunk(data)
    assert fail == (K.DECHUNK_HEADER, at)
    got, gfail, info = run(eng, [stage_dechunk()], data)
    assert gfail == fail and info.error.stage == 0 and got == want


def test_twenty_digits(eng, cfgs):
    # 20 digits do not fit int64: sscanf saturates, and the record then fails paf_check where the checker says it does
    enc = lines(K.chunk_encode(cfgs["cfg1"]))
    for at, tok in ((11, b"99999999999999999999"), (23, b"-99999999999999999999")):
        f = enc[at].split(b"\t")
        f[0] = f[0].rsplit(b"|", 1)[0] + b"|" + tok
        enc[at] = b"\t".join(f)
        data = b"\n".join(enc) + b"\n"
        want, fail = K.dechunk(data)
        got, gfail, _ = run(eng, [stage_dechunk()], data)
        assert fail is not None and gfail == fail and got == want
        enc[at] = lines(K.chunk_encode(cfgs["cfg1"]))[at]
    f = enc[5].split(b"\t")
    f[5] = f[5].split(b"|")[0] + b"|12345678901234567890|" + f[5].split(b"|")[2]  # the length saturates: a valid record
    enc[5] = b"\t".join(f)
    data = b"\n".join(enc) + b"\n"
    want, fail = K.dechunk(data)
    got, gfail, _ = run(eng, [stage_dechunk()], data)
    assert fail is None and gfail is None and got == want and b"9223372036854775807" in got


def test_checks_after_dechunk(eng, cfgs):
    enc = lines(K.chunk_encode(cfgs["cfg1"]))
    # the start moved past the decoded length
    f = enc[9].split(b"\t")
    name, _, c = f[0].rsplit(b"|", 2)
    f[0] = name + b"|%d|%s" % (int(c) + int(f[2]) + 1, c)  # length = chunk start + local start + 1: the end passes it
    enc[9] = b"\t".join(f)
    data = b"\n".join(enc) + b"\n"
    want, fail = K.dechunk(data)
    got, gfail, _ = run(eng, [stage_dechunk()], data)
    assert fail is not None and fail[1] == 9 and gfail == fail and got == want
    # a cigar-span mismatch: the target chunk start moves the end, not the span -- so change the span itself
    enc = lines(K.chunk_encode(cfgs["cfg1"]))
    f = enc[14].split(b"\t")
    f[8] = b"%d" % (int(f[8]) + 1)
    enc[14] = b"\t".join(f)
    data = b"\n".join(enc) + b"\n"
    want, fail = K.dechunk(data)
    got, gfail, _ = run(eng, [stage_dechunk()], data)
    assert fail == (K.CHECK_CIGAR_T, 14) and gfail == fail and got == want


def test_parse_error_first(eng, cfgs):
    # a bad cigar character and a bad name in one record: the cigar is parsed while reading, before the dechunk
    enc = lines(K.chunk_encode(cfgs["cfg1"]))
    f = enc[3].split(b"\t")
    f[0] = b"nopipes"
    f[-1] = f[-1][:20] + b"Q" + f[-1][21:]
    enc[3] = b"\t".join(f)
    data = b"\n".join(enc) + b"\n"
    want, fail = K.dechunk(data)
    got, gfail, info = run(eng, [stage_dechunk()], data)
    assert fail == (4, 3) and gfail == fail and info.error.stage == -1 and got == want


@pytest.mark.parametrize("rest", [[O.INVERT, O.TRIM_IDENTITY, O.SHATTER], [O.FILTER], [O.INVERT]])
def test_fused(eng, cfgs, rest):
    import paffy_amd

    O.set_filter(min_identity=0.95)
    eng.set_filter(min_identity=0.95)
    x = cfgs["cfg3"]
    enc = K.chunk_encode(x, styles=STYLES)
    mid, fail = K.dechunk(enc)
    assert fail is None
    want, err = O.run([O.stage(k) for k in rest], mid)
    assert err.code == 0
    got, gfail, _ = run(eng, [stage_dechunk()] + [paffy_amd.stage(k) for k in rest], enc)
    O.set_filter()
    eng.set_filter()
    assert gfail is None and got == want


def test_flat_pass_takes_it(eng):
    x = synth_lib.generate(0x5EED0003, 2048, 0, 2000)
    enc = K.chunk_encode(x)
    want, _ = K.dechunk(enc)
    got, gfail, _ = run(eng, [stage_dechunk()], enc)
    assert gfail is None and got == want
    assert eng.flat_stats()[0] == 0
    import paffy_amd

    got, gfail, _ = run(eng, [stage_dechunk(), paffy_amd.stage(paffy_amd.INVERT)], enc)
    assert gfail is None and got == O.run([O.stage(O.INVERT)], want)[0]
    assert eng.flat_stats()[0] == 0


def test_long_record(eng):
    n = 100_001
    cg = b"".join(b"%dM%dI" % (3 + k % 5, 1 + k % 2) if k % 2 else b"%dM%dD" % (2 + k % 7, 1 + k % 3) for k in range(n // 2)) + b"7M"
    ops = O.cigar_parse(cg)
    qs = sum(m for op, m in ops if op != K.OP_D)
    ts = sum(m for op, m in ops if op != K.OP_I)
    line = b"q|5000000|4000000\t%d\t%d\t%d\t+\tt|6000000|0x3d0900\t%d\t%d\t%d\t10\t20\t60\tcg:Z:%s\n" % (
        1000000, 100, 100 + qs, 2000000, 7, 7 + ts, cg)
    want, fail = K.dechunk(line)
    got, gfail, _ = run(eng, [stage_dechunk()], line)
    assert fail is None and gfail is None and got == want


def test_cli(cfgs, tmp_path):
    enc = K.chunk_encode(cfgs["cfg2"], styles=STYLES)
    want, _ = K.dechunk(enc)
    p = subprocess.run([PAFFY, "dechunk"], input=enc, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == want
    # the Cactus order: dechunk | dedupe, as a real shell pipe
    dup = enc + enc[: len(enc) // 3].rsplit(b"\n", 1)[0] + b"\n"
    p = subprocess.run(f"{PAFFY} dechunk | {PAFFY} dedupe", shell=True, input=dup, stdout=subprocess.PIPE, timeout=300)
    mid, fail = K.dechunk(dup)
    assert fail is None and p.returncode == 0 and p.stdout == O.dedupe(mid)[0]
    # the malformed name ends the process with the reference's SIGABRT, everything before it written
    bad = lines(enc)
    f = bad[7].split(b"\t")
    f[0] = b"plain"
    bad[7] = b"\t".join(f)
    data = b"\n".join(bad) + b"\n"
    p = subprocess.run([PAFFY, "dechunk"], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode in (134, -6) and p.stdout == K.dechunk(data)[0]


def test_cli_two_gpus(cfgs):
    enc = K.chunk_encode(cfgs["cfg3"], styles=STYLES)
    one = subprocess.run([PAFFY, "dechunk", "-q"], input=enc, stdout=subprocess.PIPE, timeout=300)
    env = dict(os.environ, PAFFY_GPUS="2", PAFFY_ONE_DEVICE="1")
    two = subprocess.run([PAFFY, "dechunk", "-q"], input=enc, stdout=subprocess.PIPE, env=env, timeout=300)
    assert one.returncode == 0 and two.returncode == 0 and one.stdout == two.stdout == K.dechunk(enc, True, False)[0]

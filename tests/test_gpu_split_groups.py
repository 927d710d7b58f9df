"""paffy split_file grouped on the device (split_kernel.h, split_host.h): paffy_amd.split_file against the files the CPU oracle writes
(oracle_lib.split_file, impl/paf_split_file.c:131-173), byte for byte, with the small_<k> numbering -- the part of the oracle's
opening order that its directory shows -- and, where the lines are distinct, the opening order itself."""
import ctypes as C
import os
import random
import re

import pytest

import oracle_lib as O
from test_split_file import R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def line(q, qlen, t, tlen, i, cigar="5M", tabs="\t"):
    """One record; AS:i:<i> makes the line distinct, so a file's content shows the input order of its lines."""
    return (f"{q}\t{qlen}\t0\t5\t+\t{t}\t{tlen}\t{i % 7}\t{i % 7 + 5}\t5\t5\t60\tAS:i:{i}\tcg:Z:{cigar}\n".replace("\t", tabs)).encode()


def oracle_files(tmp_path, data, **kw):
    """{file name without prefix and ".paf": bytes} of the oracle, and its Error."""
    d = tmp_path / f"want{len(os.listdir(tmp_path))}"
    d.mkdir()
    err = O.split_file(data, str(d) + "/s_", **kw)
    out = {}
    for n in os.listdir(d):
        assert n.startswith("s_") and n.endswith(".paf")
        with open(os.path.join(d, n), "rb") as fh:
            out[n[2:-4]] = fh.read()
    return out, err


def small_order_ok(keys):
    """small_<k> files open in the order of k."""
    ks = [int(m.group(1)) for m in (re.fullmatch(r"small_(\d+)", k) for k in keys) if m]
    return ks == list(range(len(ks)))


def first_line_order(files, data_norm_lines):
    """The files ordered by where their first line stands in the normalised input (distinct lines only)."""
    pos = {ln: i for i, ln in reversed(list(enumerate(data_norm_lines)))}
    return sorted(files, key=lambda k: pos[files[k].split(b"\n", 1)[0] + b"\n"])


def check(eng, tmp_path, data, distinct=True, **kw):
    want, err = oracle_files(tmp_path, data, **kw)
    assert err.code == 0
    got, info = eng.split_file(data, **kw)
    assert info.error.code == 0
    assert got == want
    assert small_order_ok(list(got)), list(got)
    if distinct and got:
        norm = O.dedupe(data)[0].splitlines(keepends=True)  # paf_read(.., 0) -> paf_write of every record
        assert len(set(norm)) == len(norm)
        assert list(got) == first_line_order(want, norm)
    return got, info


OPTION_SETS = [dict(), dict(by_query=True), dict(min_length=100000000), dict(by_query=True, min_length=60000000)]


@pytest.mark.parametrize("kw", OPTION_SETS, ids=["default", "by_query", "min_length", "both"])
def test_existing_inputs(eng, tmp_path, human_chimp, kw):
    check(eng, tmp_path, human_chimp, distinct=False, **kw)
    small = dict(kw)
    if "min_length" in small:
        small["min_length"] = 100  # the six records: tiny1 40, tiny2 70, tiny3 50 against 100
    check(eng, tmp_path, b"".join(R), **small)
    if "min_length" in small:
        check(eng, tmp_path, b"".join(R), **dict(small, min_length=120))


def test_module_level_split_file(tmp_path):
    import paffy_amd

    data = b"".join(R)
    got = paffy_amd.split_file(data, min_length=100)
    want, err = oracle_files(tmp_path, data, min_length=100)
    assert err.code == 0 and got == want and list(got) == ["chr_1", "small_0", "small_1", "small_2"]


def test_empty_and_tiny_inputs(eng, tmp_path):
    got, info = eng.split_file(b"")
    assert got == {} and info.error.code == 0 and info.n_records == 0
    one = line("q", 100, "t", 200, 0)
    assert check(eng, tmp_path, one)[0] == {"t": O.dedupe(one)[0]}
    two = one + line("q2", 100, "u", 200, 1)
    assert two.endswith(b"\n")
    got, _ = check(eng, tmp_path, two[:-1])  # a last line without a newline
    assert list(got) == ["t", "u"] and got["u"].endswith(b"\n")


@pytest.mark.parametrize("n_names", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_distinct_names_at_block_boundaries(eng, tmp_path, n_names):
    """Interleaved: line i belongs to name i % n_names, three rounds, so no group is contiguous in the input (but for one name)."""
    data = b"".join(line(f"q{i}", 500, f"ctg{i % n_names}", 1000 + i % n_names, i) for i in range(3 * n_names))
    got, _ = check(eng, tmp_path, data)
    assert len(got) == n_names and all(v.count(b"\n") == 3 for v in got.values())
    got, _ = check(eng, tmp_path, data, min_length=1000 + n_names // 2)  # the first half of the names is small
    assert len([k for k in got if not k.startswith("small_")]) == n_names - n_names // 2


def test_one_large_group(eng, tmp_path):
    data = b"".join(line(f"q{i}", 500, "only", 9000, i) for i in range(5000))
    got, info = check(eng, tmp_path, data)
    assert list(got) == ["only"] and info.n_records == 5000


def test_names_that_are_prefixes_of_each_other(eng, tmp_path):
    names = ["chr1", "chr10", "chr1 ", "chr", "chr100", "chr1_", " chr1", "c"]
    rng = random.Random(5)
    data = b"".join(line(f"q{i}", 500, rng.choice(names), 4000, i) for i in range(400))
    got, _ = check(eng, tmp_path, data)
    assert set(got) == set(names)
    check(eng, tmp_path, b"".join(line(rng.choice(names), 4000, f"t{i}", 500, i) for i in range(400)), by_query=True)


def test_a_long_name(eng, tmp_path):
    """A 5 000-byte name is no file name (NAME_MAX): the oracle's fopen fails and it drops the lines, so its directory holds the other
    files only; the long name's lines are checked against the oracle's normalised lines (paf_read -> paf_write)."""
    long_name = "L" * 5000
    lines = [line(f"q{i}", 500, long_name if i % 3 == 1 else f"s{i % 2}", 7000, i) for i in range(30)]
    data = b"".join(lines)
    want, err = oracle_files(tmp_path, data)
    assert err.code == 0 and set(want) == {"s0", "s1"}
    got, info = eng.split_file(data)
    assert info.error.code == 0 and list(got) == ["s0", long_name, "s1"]
    assert {k: v for k, v in got.items() if k != long_name} == want
    assert got[long_name] == O.dedupe(b"".join(ln for i, ln in enumerate(lines) if i % 3 == 1))[0]


def test_names_with_slashes(eng, tmp_path):
    names = ["a/b", "a/b/c", "/lead", "trail/", "x//y", "plain"]
    d = tmp_path / "w"
    d.mkdir()
    data = b"".join(line(f"q{i}", 500, names[i % len(names)], 4000, i) for i in range(60))
    assert O.split_file(data, str(d) + "/s_").code == 0
    want = {n[2:-4]: open(os.path.join(d, n), "rb").read() for n in os.listdir(d)}
    assert set(want) == {n.replace("/", "_") for n in names}
    got, info = eng.split_file(data)
    assert info.error.code == 0 and got == want and list(got) == [n.replace("/", "_") for n in names]


def test_small_and_big_at_once(eng, tmp_path):
    """The same name with lengths on both sides of min_length: the small bit is taken from every record's own line
    (impl/paf_split_file.c:143-146), so the name has a small file and a file of its own."""
    data = b"".join(line(f"q{i}", 500, "both", 50 if i % 2 else 5000, i) for i in range(20)) + line("q", 500, "other", 60, 99)
    got, _ = check(eng, tmp_path, data, min_length=100)
    assert list(got) == ["both", "small_0", "small_1"]
    assert got["both"].count(b"\n") == 10 and got["small_0"].count(b"\n") == 10 and got["small_1"].count(b"\n") == 1


def test_small_bins(eng, tmp_path):
    # fills exactly: 40 + 60 == 100 stays in small_0; the next contig (1) opens small_1
    data = line("q", 500, "a", 40, 0) + line("q", 500, "b", 60, 1) + line("q", 500, "c", 1, 2) + line("q", 500, "a", 40, 3)
    got, _ = check(eng, tmp_path, data, min_length=100)
    assert list(got) == ["small_0", "small_1"] and got["small_0"].count(b"\n") == 3
    # overflows by 1: 40 + 61 == 101 > 100
    data = line("q", 500, "a", 40, 0) + line("q", 500, "b", 61, 1) + line("q", 500, "c", 39, 2)
    got, _ = check(eng, tmp_path, data, min_length=100)
    assert list(got) == ["small_0", "small_1"] and got["small_0"].count(b"\n") == 1 and got["small_1"].count(b"\n") == 2


def test_runs_of_tabs(eng, tmp_path):
    data = line("q0", 500, "t", 4000, 0) + line("q1", 500, "t", 4000, 1, tabs="\t\t\t") + line("q2", 500, "u", 30, 2, tabs="\t\t") + line("q3", 500, "t", 4000, 3)
    check(eng, tmp_path, data)
    check(eng, tmp_path, data, min_length=100)
    check(eng, tmp_path, data, by_query=True)


def test_lines_of_one_name_keep_input_order(eng, tmp_path):
    """Lines that differ only in their cigar: a sort that is not stable would show."""
    cigars = ["5M", "2M1X2M", "1X4M", "4M1X", "5X", "3M2X", "2X3M", "1M1X1M1X1M"]
    rng = random.Random(3)
    recs = []
    for i in range(600):
        t = f"t{rng.randrange(5)}"
        recs.append(f"q\t500\t0\t5\t+\t{t}\t4000\t0\t5\t5\t5\t60\tcg:Z:{rng.choice(cigars)}\n".encode())
    data = b"".join(recs)
    got, _ = check(eng, tmp_path, data, distinct=False)
    for t in range(5):
        assert got[f"t{t}"] == b"".join(O.dedupe(r)[0] for r in recs if f"\tt{t}\t".encode() in r)  # every line normalised on its own


def plan_batch(eng, data):
    d_in = eng.to_device(data)
    info = eng.split_plan(d_in, len(data))
    out = b""
    if info.out_bytes:
        d_out = eng.alloc_out(info.out_bytes)
        eng.emit(d_out)
        eng.sync()
        out = d_out[: info.out_bytes].cpu().numpy().tobytes()
    return info, out, eng.split_groups()


def test_two_batches_on_one_context(eng, tmp_path):
    b1 = line("q", 500, "big", 5000, 0) + line("q", 500, "s1", 40, 1) + line("q", 500, "big", 5000, 2)
    b2 = line("q", 500, "s2", 50, 3) + line("q", 500, "big", 5000, 4) + line("q", 500, "s3", 20, 5) + line("q", 500, "new", 7000, 6) + line("q", 500, "s1", 40, 7)
    eng.split_begin(False, 100)
    files = {}
    i1, o1, g1 = plan_batch(eng, b1)
    assert [(g.file, g.new_file, g.is_small, g.lines, g.first_record) for g in g1] == [(0, 1, 0, 2, 0), (1, 1, 1, 1, 1)]
    i2, o2, g2 = plan_batch(eng, b2)
    # s2 (40 + 50 <= 100) continues batch 1's small file and s1 is known: one stretch, lines in input order; big comes back;
    # s3 (90 + 20 > 100) opens small_1
    assert [(g.file, g.new_file, g.is_small, g.lines, g.first_record) for g in g2] == [(1, 0, 1, 2, 0), (0, 0, 0, 1, 1), (2, 1, 1, 1, 2), (3, 1, 0, 1, 3)]
    assert [eng.split_file_name(f) for f in range(4)] == [b"big", b"small_0", b"small_1", b"new"]
    for out, groups in ((o1, g1), (o2, g2)):
        at = 0
        for g in groups:
            assert g.out_off == at  # the groups tile the output
            at += g.bytes
            files.setdefault(eng.split_file_name(g.file).decode(), []).append(out[g.out_off : g.out_off + g.bytes])
        assert at == len(out)
    want, err = oracle_files(tmp_path, b1 + b2, min_length=100)
    assert err.code == 0 and {k: b"".join(v) for k, v in files.items()} == want
    assert eng.split_file(b1 + b2, min_length=100, batch_bytes=len(b1))[0] == want
    # split_begin again starts from nothing
    eng.split_begin(False, 100)
    _, _, g = plan_batch(eng, b2)
    # s2 opens small_0, s3 joins it (50 + 20), s1 is new to this run and does not fit (70 + 40 > 100)
    assert [(x.file, x.new_file, x.lines) for x in g] == [(0, 1, 2), (1, 1, 1), (2, 1, 1), (3, 1, 1)]
    assert [eng.split_file_name(f) for f in range(4)] == [b"small_0", b"big", b"new", b"small_1"]


def test_a_failing_record_in_the_middle(eng, tmp_path):
    from paffy_amd.engine import PlanInfo, lib

    good = [line(f"q{i}", 500, f"t{i % 3}", 4000, i) for i in range(12)]
    bad = b"q\t500\t0\t5\t+\tt1\t4000\t0\t5\t5\n"  # fewer than 12 columns
    data = b"".join(good[:7]) + bad + b"".join(good[7:])
    want, werr = oracle_files(tmp_path, data)
    assert werr.code != 0 and werr.record == 7
    got, info = eng.split_file(data, raise_on_error=False)
    assert got == want and sum(v.count(b"\n") for v in got.values()) == 7
    # the code and the record of paffy_hip_dedupe_plan(.., PAFFY_DEDUPE_KEEP_ALL, ..) on the same input, which are the oracle's
    d_in = eng.to_device(data)
    dinfo = PlanInfo()
    assert lib().paffy_hip_dedupe_plan(eng._ctx, C.c_void_p(d_in.data_ptr()), len(data), 2, C.byref(dinfo)) == 0
    assert (info.error.code, info.error.record, info.error.stage) == (dinfo.error.code, dinfo.error.record, dinfo.error.stage)
    assert (info.error.code, info.error.record) == (werr.code, werr.record)
    import paffy_amd

    with pytest.raises(paffy_amd.PafError) as e:
        eng.split_file(data)
    assert e.value.args[0].startswith("record 7:")
    # in the second piece of a text that goes in pieces: the record counts over the whole text
    got, info = eng.split_file(data, raise_on_error=False, batch_bytes=len(b"".join(good[:4])))
    assert got == want and (info.error.code, info.error.record) == (werr.code, 7)


def test_the_collision_knob(eng, tmp_path, monkeypatch):
    """PAFFY_SPLIT_NARROW_SALT0 cuts salt 0's hash to two bits: 40 names cannot keep apart, the byte check finds it and the grouping
    runs again with the next salt."""
    data = b"".join(line(f"q{i}", 500, f"name{i % 40}", 4000 if i % 40 % 2 else 30, i) for i in range(200))
    want, err = oracle_files(tmp_path, data, min_length=100)
    assert err.code == 0
    monkeypatch.setenv("PAFFY_SPLIT_NARROW_SALT0", "1")
    got, info = eng.split_file(data, min_length=100)
    assert eng.split_salt() > 0
    assert info.error.code == 0 and got == want and small_order_ok(list(got))
    monkeypatch.delenv("PAFFY_SPLIT_NARROW_SALT0")
    got, info = eng.split_file(data, min_length=100)
    assert eng.split_salt() == 0 and got == want

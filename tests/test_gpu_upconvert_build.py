"""The device build of upconvert's interval table (paffy_hip_set_intervals_fasta) against the CPU predictor of upconvert_build_cases.py and
against the table paffy_hip_set_intervals builds from the same headers and lengths as host strings, entry by entry and byte by byte."""
import ctypes as C
import os
import subprocess

import pytest

import chunk_lib as K
import name_sort_cases as NS
import upconvert_build_cases as UC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAFFY = os.path.join(ROOT, "bin", "paffy")
GOOD, BAD = UC.good_cases(), UC.bad_cases()
MESSAGE = "upconvert: a FASTA header does not end in |length|start"


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


def set_host(eng, recs):
    eng.set_intervals([UC.key_of(h) for h, _ in recs], [n for _, n in recs])


def upconvert(eng, data):
    import paffy_amd

    out, info = eng.run([paffy_amd.stage(paffy_amd.UPCONVERT)], data, raise_on_error=False)
    return out, ((info.error.code, info.error.record) if info.error.code else None)


@pytest.mark.parametrize("key", sorted(GOOD))
def test_device_table_equals_predictor_and_host_path(eng, key):
    case = GOOD[key]
    recs = UC.flat(case)
    want = UC.expected(recs)
    assert eng.set_intervals_fasta(UC.texts(case)) == len(recs)
    dev, dev_info = eng.intervals(), eng.intervals_info()
    sort_stats = eng.name_sort_stats()
    set_host(eng, recs)
    host, host_info = eng.intervals(), eng.intervals_info()
    assert dev == want and host == want
    assert dev_info["on_device"] == 1 and host_info["on_device"] == 0 and host_info["rounds"] == 0
    assert dev_info["intervals"] == host_info["intervals"] == len(recs)
    assert dev_info["blob_bytes"] == host_info["blob_bytes"] == sum(len(t[0]) + len(t[4]) for t in want)
    rounds = NS.model(UC.names_of(recs))[2]
    assert dev_info["rounds"] == rounds
    if recs:  # the sort was the build's: its keys are the decoded names
        assert (sort_stats["records"], sort_stats["rounds"], sort_stats["names"]) == (len(recs), rounds, len(set(UC.names_of(recs))))


@pytest.mark.parametrize("case,found", [(UC.TIE_SMALL_FIRST, True), (UC.TIE_LARGE_FIRST, False)])
def test_tie_keeps_input_order_under_upconvert(eng, case, found):
    recs = UC.flat(case)
    table = UC.expected(recs)
    k = K.bsearch([t[:4] for t in table], b"c", 5, 50)
    assert (k == 1) if found else (k == -2)
    want = UC.expected_upconvert(UC.TIE_PROBE, table)
    assert (want[1] is None) == found and (found or want[1] == (K.UPCONVERT_ASSERT, 0))
    eng.set_intervals_fasta(UC.texts(case))
    dev = upconvert(eng, UC.TIE_PROBE)
    set_host(eng, recs)
    host = upconvert(eng, UC.TIE_PROBE)
    assert dev == want and host == want


@pytest.mark.parametrize("key", sorted(BAD))
def test_failing_header(eng, key):
    eng.set_intervals_fasta(UC.texts(GOOD["two_files"]))
    assert eng.intervals_info()["intervals"] == 5
    with pytest.raises(RuntimeError) as err:
        eng.set_intervals_fasta(UC.texts(BAD[key]))
    assert "(-6)" in str(err.value) and MESSAGE in str(err.value)  # PAFFY_E_HEADER
    with pytest.raises(RuntimeError) as host_err:
        set_host(eng, UC.flat(BAD[key]))
    assert str(host_err.value).split(": ", 1)[1] == str(err.value).split(": ", 1)[1]
    assert eng.intervals_info()["intervals"] == 0 and eng.intervals() == []
    assert upconvert(eng, UC.TIE_PROBE) == UC.expected_upconvert(UC.TIE_PROBE, [])  # no side is renamed
    assert eng.set_intervals_fasta(UC.texts(GOOD["styles"])) == len(UC.STYLES)
    assert eng.intervals() == UC.expected(UC.flat(GOOD["styles"]))


def test_records_are_counted_on_failure(eng):
    import paffy_amd.engine as E

    data, starts = eng._fasta_text(UC.texts(BAD["bad0_among_256"]))
    d_text = eng.to_device(data)
    n = C.c_int64(-1)
    st = (C.c_int64 * len(starts))(*starts)
    rc = E.lib().paffy_hip_set_intervals_fasta(eng._ctx, C.c_void_p(d_text.data_ptr()), len(data), st, len(starts), C.byref(n))
    assert rc == -6 and n.value == 257


def test_read_capacity(eng):
    import paffy_amd.engine as E

    case = GOOD["name_prefix"]
    eng.set_intervals_fasta(UC.texts(case))
    info = eng.intervals_info()
    n, nb = info["intervals"], info["blob_bytes"]
    assert n == 4 and nb > 0
    for cap, blob_cap in ((n - 1, nb), (n, nb - 1)):
        nums = (C.c_int64 * (3 * n))(*[-7] * (3 * n))
        slices = (C.c_uint32 * (4 * n))(*[77] * (4 * n))
        blob = C.create_string_buffer(b"\xee" * nb, nb)
        assert E.lib().paffy_hip_intervals_read(eng._ctx, cap, blob_cap, nums, slices, blob) == -4  # PAFFY_E_CAPACITY
        assert list(nums) == [-7] * (3 * n) and list(slices) == [77] * (4 * n) and blob.raw == b"\xee" * nb
    assert E.lib().paffy_hip_intervals_read(eng._ctx, n, nb, None, None, None) == 0
    nums = (C.c_int64 * (3 * n))()
    assert E.lib().paffy_hip_intervals_read(eng._ctx, n, nb, nums, None, None) == 0
    assert [nums[3 * k] for k in range(n)] == [t[1] for t in UC.expected(UC.flat(case))]


def test_a_smaller_table_after_a_larger_one(eng):
    eng.set_intervals_fasta(UC.texts(GOOD["shared_prefix"]))
    assert eng.intervals_info()["intervals"] == 600
    small = GOOD["empty_name"]
    eng.set_intervals_fasta(UC.texts(small))
    want = UC.expected(UC.flat(small))
    assert eng.intervals() == want
    assert eng.intervals_info() == {"intervals": 4, "blob_bytes": sum(len(t[0]) + len(t[4]) for t in want), "on_device": 1,
                                    "rounds": NS.model(UC.names_of(UC.flat(small)))[2]}
    eng.set_intervals_fasta(UC.texts(GOOD["empty"]))
    assert eng.intervals() == [] and eng.intervals_info() == {"intervals": 0, "blob_bytes": 0, "on_device": 1, "rounds": 0}


def test_cli(tmp_path):
    files = [UC.flat(GOOD["styles"])[:3] + UC.flat(UC.TIE_SMALL_FIRST), UC.flat(GOOD["styles"])[3:]]
    recs = UC.flat(files)
    table = UC.expected(recs)
    sides = [(b"st", 100, 16, 17), (b"st", 100, 32, 35), (b"st", 100, 0, 1), (b"st", 100, 8, 9), (b"c", 1000, 5, 50), (b"c", 1000, 0, 3), (b"none", 70, 1, 2)]
    data = b"".join(b"%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t5\t9\t60\ttp:A:P\n" % (q + t) for q in sides for t in sides if q != t)
    want, fail = UC.expected_upconvert(data, table)
    assert fail is None and b"st|31|15\t" in want and b"st|12|-3\t" in want and b"c|1000|0\t" in want
    paths = []
    for k, text in enumerate(UC.texts(files)):
        p = tmp_path / ("iv%d.fa" % k)
        p.write_bytes(text)
        paths.append(str(p))
    p = subprocess.run([PAFFY, "upconvert", "-l", "INFO"] + paths, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stdout == want
    assert b"Read %d sequences from sequence files\n" % len(recs) in p.stderr

"""`faffy extract` with the BED text parsed, sorted and merged on the device: the host form (paffy_hip_faffy_extract_plan, now one copy
plus the device plan) and the device form (paffy_hip_faffy_extract_plan_device, Engine.faffy_extract_device) against the checker
(tests/faffy_lib.py) over the inputs of tests/extract_device_lib.py: output bytes, or code and record of the failing plan."""
import ctypes as C
import functools

import pytest

import extract_device_lib as X
import faffy_lib as F

pytestmark = pytest.mark.gpu

FORMS = ("host", "device")
E_ARG, E_STATE = -2, -5


@pytest.fixture(scope="module")
def eng():
    import paffy_amd

    e = paffy_amd.Engine()
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def checker(cid):
    c = next(c for c in X.CASES + [X.big_case()] if c[0] == cid)
    return F.extract(X.FILES, c[1], c[2], c[3], skip_missing=c[4])


def extract(eng, form, files, bed, flank, min_size, skip):
    """the output, or (code, record, exit status) of the plan's failure"""
    import paffy_amd

    try:
        if form == "host":
            return eng.faffy_extract(files, bed, flank, min_size, skip)
        return eng.faffy_extract_device(files, eng.to_device(bed), len(bed), flank, min_size, skip)
    except paffy_amd.PafError as e:
        return e.info.error.code, e.info.error.record, e.exit_status


OK_CASES = [c for c in X.CASES if c not in X.ERROR_CASES]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", OK_CASES, ids=lambda c: c[0])
def test_output_equals_the_checkers(eng, form, c):
    want, status, _ = checker(c[0])
    assert status == 0
    assert extract(eng, form, X.FILES, *c[1:]) == want


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", X.ERROR_CASES, ids=lambda c: c[0])
def test_a_failing_plan_gives_code_and_record(eng, form, c):
    code, record = X.expected(X.FILES, *c[1:])
    assert checker(c[0])[1] == {X.ASSERT: 134, X.MISSING: 1}[code]
    got = extract(eng, form, X.FILES, *c[1:])
    print(c[0], "expected", (code, record), "got", got)
    assert got == (code, record, {X.ASSERT: 134, X.MISSING: 1}[code])


@pytest.mark.parametrize("form", FORMS)
def test_100001_lines(eng, form):
    c = X.big_case()
    want, status, _ = checker(c[0])
    assert status == 0 and len(want) > 100000
    assert extract(eng, form, X.FILES, *c[1:]) == want


@pytest.mark.parametrize("form", FORMS)
def test_after_a_failing_plan_nothing_is_planned(eng, form):
    from paffy_amd import engine as E

    d_text = eng._files(X.FILES)
    bed = b"chr1 10 200\nchr10 5 300\nchr1 7\n"
    info = E.PlanInfo()
    if form == "host":
        rc = E.lib().paffy_hip_faffy_extract_plan(eng._ctx, bed, len(bed), 0, 1, 0, C.byref(info))
    else:
        d_bed = eng.to_device(bed)
        rc = E.lib().paffy_hip_faffy_extract_plan_device(eng._ctx, C.c_void_p(d_bed.data_ptr()), len(bed), 0, 1, 0, C.byref(info))
    assert rc == 0 and (info.error.code, info.error.record) == (X.ASSERT, 2)
    assert info.n_rows == 0 and info.out_bytes == 0
    del d_text


@pytest.mark.parametrize("form", FORMS)
def test_plan_info_of_a_plan(eng, form):
    from paffy_amd import engine as E

    d_text = eng._files(X.FILES)
    bed = b"chr1 10 200\nchr10 5 300\nchr1 150 400\nnope 1 2\n"
    want, status, _ = F.extract(X.FILES, bed, 0, 1, skip_missing=True)
    info = E.PlanInfo()
    if form == "host":
        rc = E.lib().paffy_hip_faffy_extract_plan(eng._ctx, bed, len(bed), 0, 1, 1, C.byref(info))
    else:
        d_bed = eng.to_device(bed)
        rc = E.lib().paffy_hip_faffy_extract_plan_device(eng._ctx, C.c_void_p(d_bed.data_ptr()), len(bed), 0, 1, 1, C.byref(info))
    assert rc == 0 and info.error.code == 0
    assert (info.n_rows, info.out_bytes, info.n_records, info.in_bytes) == (2, len(want), len(X.RECORDS), len(X.GENOME))
    assert eng._faffy_emit(info) == want
    del d_text


@pytest.mark.parametrize("form", FORMS)
def test_hand_over_from_to_bed(eng, form):
    """the BED that to_bed writes for a small PAF, put into a device tensor (or handed over as host text)"""
    import oracle_lib as O

    def paf(qn, ql, qs, qe, tn, tl, ts, te):
        return b"%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t5\t9\t60\ttp:A:P\tcg:Z:%dM\n" % (qn, ql, qs, qe, tn, tl, ts, te, qe - qs)

    data = b"".join([paf(b"chr1", 3000, 100, 400, b"big", 200000, 5000, 5300), paf(b"chr1", 3000, 350, 900, b"big", 200000, 9000, 9550),
                     paf(b"chr10", 2500, 0, 2500, b"big", 200000, 100, 2600), paf(b"s12", 5000, 1200, 1900, b"chr1", 3000, 10, 710),
                     paf(b"chr1", 3000, 2000, 2100, b"chr10", 2500, 0, 100)])
    want_bed, err = O.to_bed(data)
    assert err.code == 0 and len(F.bed_lines(want_bed)) >= 4
    bed, _ = eng.to_bed(data)
    want, status, _ = F.extract(X.FILES, want_bed, 10, 50)
    assert status == 0 and len(X.items(want)) >= 3
    if form == "host":
        assert eng.faffy_extract(X.FILES, bed, 10, 50) == want
    else:
        assert eng.faffy_extract_device(X.FILES, eng.to_device(bed), len(bed), 10, 50) == want


@pytest.mark.parametrize("form", FORMS)
def test_the_profile_names_the_plans_kernels(eng, form):
    bed = b"chr1 10 200\nchr10 5 300\nchr1 150 400\n"
    eng.profile(True)
    try:
        out = extract(eng, form, X.FILES, bed, 0, 1, False)
        prof = eng.profile_read()
    finally:
        eng.profile(False)
    assert out == F.extract(X.FILES, bed, 0, 1)[0]
    assert "k_bed_parse" in prof and "k_bed_items" in prof, sorted(prof)
    assert prof["k_bed_parse"][1] == 1 and prof["k_bed_items"][1] == 1


@pytest.mark.parametrize("form", FORMS)
def test_the_plan_keeps_nothing_of_the_bed(eng, form):
    """the BED text is overwritten between plan and emit"""
    from paffy_amd import engine as E

    c = next(c for c in X.CASES if c[0] == "pmax-run-of-5000")
    want = checker(c[0])[0]
    d_text = eng._files(X.FILES)
    info = E.PlanInfo()
    if form == "host":
        h_bed = C.create_string_buffer(c[1], len(c[1]))
        rc = E.lib().paffy_hip_faffy_extract_plan(eng._ctx, C.cast(h_bed, C.c_char_p), len(c[1]), c[2], c[3], 0, C.byref(info))
        C.memset(h_bed, 0xff, len(c[1]))
    else:
        d_bed = eng.to_device(c[1])
        rc = E.lib().paffy_hip_faffy_extract_plan_device(eng._ctx, C.c_void_p(d_bed.data_ptr()), len(c[1]), c[2], c[3], 0, C.byref(info))
        d_bed.fill_(0xff)
        eng.torch.cuda.synchronize(eng.device)
    assert rc == 0 and info.error.code == 0
    assert eng._faffy_emit(info) == want
    del d_text


@pytest.mark.parametrize("form", FORMS)
def test_argument_and_state_errors(form):
    import paffy_amd
    from paffy_amd import engine as E

    L = E.lib()
    e = paffy_amd.Engine()
    try:
        info = E.PlanInfo()
        bed = b"chr1 10 200\n"
        d_bed = e.to_device(b"x" + bed)

        def plan(ptr, n):
            if form == "host":
                return L.paffy_hip_faffy_extract_plan(e._ctx, ptr, n, 0, 1, 0, C.byref(info))
            return L.paffy_hip_faffy_extract_plan_device(e._ctx, ptr, n, 0, 1, 0, C.byref(info))

        good = bed if form == "host" else C.c_void_p(d_bed.data_ptr())
        assert plan(good, len(bed)) == E_STATE  # no index
        e.fasta_seen(X.FILES, b"")              # an index without bases
        assert plan(good, len(bed)) == E_STATE
        d_text = e._files(X.FILES)
        assert plan(None, len(bed)) == E_ARG
        assert plan(good, -1) == E_ARG
        if form == "device":
            assert plan(C.c_void_p(d_bed.data_ptr() + 1), len(bed)) == E_ARG  # not 16-byte aligned
        assert plan(None, 0) == 0 and (info.error.code, info.n_rows, info.out_bytes) == (0, 0, 0)
        assert e._faffy_emit(info) == b""
        del d_text
    finally:
        e.close()

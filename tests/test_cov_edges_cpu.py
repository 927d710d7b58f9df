"""The inputs of test_gpu_cov_edges.py (cov_edges_lib) hit their cases: shown on the oracle and on the library's predictor of k_cov_bitmap
alone. The predictor restates the kernel's geometry (rounds of TEXT bytes from cg_off & ~15 on, an op list of TEXT / 2 letters, a window of
WIN words, the one-wave shape up to COV_WAVE_BYTES); test_constants reads those values out of the headers, so a changed constant fails
here instead of silently moving the cases off their edges. Nothing below is skipped or counted: every case must be placed."""
import os
import re

import pytest

import cov_edges_lib as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "paffy_amd", "csrc")


def test_constants():
    h = L.header_constants(CSRC)
    for g in L.SHAPES:
        assert h["NT_%d" % g] == g and h["TEXT_%d" % g] == L.TEXT[g] == 16 * g and h["WIN_%d" % g] == L.WIN[g] and h["OPS_%d" % g] == L.OPS[g]
    assert h["COV_WAVE_BYTES"] == L.COV_WAVE_BYTES and h["COV_SLICE"] == L.COV_SLICE and h["BED_PER"] == L.BED_PER and h["BED_STAGE"] == L.BED_STAGE
    assert h["serial_digits"] == 8


def test_the_predictor_on_a_hand_made_line():
    b = L.Batch("hand")
    b.add("5M" + "0I" * 600 + "12345678M", 14, strand="-", qs=1)  # 1 215 bytes from byte 14 of a chunk: rounds of 1 010 and 205 bytes
    p = L.predict(b.data, sides=2)[0]
    assert (p["shape"], p["rounds"], p["lead"], p["boundary"]) == (64, 2, 14, [-14, 1010])
    assert p["letters"] == [505, 97] and p["serial"] == ("digits", 1) and p["straddles"] == []
    assert p["sides"][0]["lds"] == [True] and p["sides"][2]["lds"] == [True] and p["sides"][0]["words"] == [1]


def number_around(cg, i):
    """(digits in front of cigar byte i, digits) of the number that byte i lies in"""
    s = e = i
    while s > 0 and cg[s - 1:s].isdigit():
        s -= 1
    while e < len(cg) and cg[e:e + 1].isdigit():
        e += 1
    return i - s, e - s


@pytest.mark.parametrize("batch", L.error_free_batches(), ids=lambda b: b.name)
def test_error_free_cases_hit_what_they_are_named_for(batch):
    data = batch.data
    for mode in L.MODES:
        code, rec, out = L.oracle(mode, data)
        assert code == 0 and (out or mode == "tile"), (mode, code, rec)
    pred = L.predict(data, sides=2)
    assert len(pred) == len(batch.lines)
    for i, (want, p) in enumerate(zip(batch.expect, pred)):
        where = (batch.name, i, want)
        if "shape" in want:
            assert p["shape"] == want["shape"] and (p["cg_len"] <= L.COV_WAVE_BYTES) == (want["shape"] == 64), where
        for key in ("lead", "cg_len", "serial"):
            if key in want:
                assert p[key] == want[key], (where, p[key])
        if want.get("serial") and want["serial"][1] == 2:  # two parallel rounds have set bits before the serial walk starts again
            assert [x is not None for x in p["sides"][0]["lds"]] == [True, True], (where, p["sides"][0])
        if "last_at" in want:
            assert (p["cg_off"] + p["cg_len"] - 1) % 16 == want["last_at"], where
        if "straddle" in want:
            assert want["straddle"] in p["straddles"] and p["serial"] is None, (where, p["straddles"])
        if "lane" in want:
            at, j, n = want["lane"]
            cg = batch.lines[i].split("cg:Z:")[1].rstrip("\n").encode()
            assert (p["cg_off"] + (at - p["lead"])) % 16 == 0 and at % L.TEXT[p["shape"]] and number_around(cg, at - p["lead"]) == (j, n), where
        if "first_letter" in want:
            assert want["first_letter"] in p["first_letter"], (where, p["first_letter"])
        if "last_letter" in want:
            assert want["last_letter"] in p["last_letter"], (where, p["last_letter"])
        if "letters" in want:
            k, n = want["letters"]
            assert p["letters"][k] == n and all(x <= L.OPS[p["shape"]] for x in p["letters"][:k]), (where, p["letters"])
        if "idle_round" in want:
            for side in p["sides"].values():
                k = want["idle_round"]
                assert side["lds"][k] is None and side["lds"][k - 1] is not None and side["lds"][k + 1] is not None, (where, side["lds"])
        if "lds0" in want:
            assert p["sides"][0]["lds"][0] == want["lds0"] and p["sides"][0]["words"][0] == want["words0"] and p["sides"][0]["lds"][1] is True, (where, p["sides"][0])
        if "lds" in want:
            assert p["sides"][0]["lds"][:len(want["lds"])] == want["lds"], (where, p["sides"][0])
    if batch.name.startswith("window_alternating"):  # neighbouring rounds on different paths meet inside a word: the op boundary is not on one
        for ln in batch.lines:
            f = ln.split("\t")
            at, g = int(f[2]), 64 if len(f[-1]) - 6 <= L.COV_WAVE_BYTES else 256
            for k in range(4):
                text = f[-1][5:].rstrip("\n")
                at += L.spans(text[:L.TEXT[g] * (k + 1) - 9][L.TEXT[g] * k - 9 if k else 0:])[0]
                assert at % 32, (batch.name, k, at)


def test_every_group_has_both_shapes_and_the_exact_threshold():
    shapes = {}
    for b in L.error_free_batches() + L.failing_batches():
        for p in L.predict(b.data)[slice(None) if b.error_free else slice(1, 2)]:  # of a failing batch the line that fails
            if p["has_cg"]:
                shapes.setdefault(re.sub(r"_(64|256)(?=_|$)", "", b.name), set()).add(p["shape"])
    one_shape = {"align_tiny", "bed_runs", "bed_lines", "median"}  # cigars of 1 to 17 bytes; inputs of the kernels behind the bitmaps
    assert all(v == set(L.SHAPES) for k, v in shapes.items() if k not in one_shape), {k: v for k, v in shapes.items() if len(v) < 2}
    b = L.threshold_batch()
    lens = [p["cg_len"] for p in L.predict(b.data)]
    assert sorted(set(lens)) == [L.COV_WAVE_BYTES, L.COV_WAVE_BYTES + 1] and [p["shape"] for p in L.predict(b.data)] == [64 if n == 9000 else 256 for n in lens]
    for mode in L.MODES:
        assert L.oracle(mode, b.data)[0] == 0


@pytest.mark.parametrize("batch", L.failing_batches(), ids=lambda b: b.name)
def test_failing_cases_fail_as_named(batch):
    data = batch.data
    want = batch.expect[1]
    p = L.predict(data, sides=2)[1]
    assert p["shape"] == want["shape"]
    if "serial" in want:
        assert p["serial"] == want["serial"]
    for mode in L.MODES:
        code, rec, out = L.oracle(mode, data)
        assert code == want["err"][mode], (batch.name, mode, code)
        if code:
            assert rec == 1 and out == b"", (batch.name, mode, rec)
    # the lines in front and behind are error-free on their own
    ok = (batch.lines[0] + batch.lines[2]).encode()
    assert all(L.oracle(mode, ok)[0] == 0 for mode in L.MODES)
    if "bad_letter_first_of_round" in batch.name:
        assert p["first_letter"] == [1] and batch.lines[1].split("cg:Z:")[1][p["boundary"][1]] == "Q"
    if "bad_letter_last_of_round" in batch.name:
        assert 0 in p["last_letter"] and batch.lines[1].split("cg:Z:")[1][p["boundary"][1] - 1] == "S"
    if "on_round_boundary" in batch.name:
        assert (p["lead"] + p["cg_len"]) % L.TEXT[p["shape"]] == 0
    if "after_overrun" in batch.name:  # without the bad letter the same line fails the walk's assert
        good = batch.lines[1].replace("5Q\n", "5M\n").encode()
        assert L.oracle("bed", good)[0] == L.ERR_ASSERT


def test_trailing_digits_end_at_every_offset():
    seen = {g: set() for g in L.SHAPES}
    for b in L.failing_batches():
        if "trailing_digits_" in b.name and "boundary" not in b.name:
            p = L.predict(b.data)[1]
            seen[p["shape"]].add((p["cg_off"] + p["cg_len"] - 1) % 16)
    assert all(seen[g] == set(range(16)) for g in L.SHAPES)


def reline(ln, cg):
    """the line with another cigar, its ends moved to fit (the sequence lengths stay)"""
    f = ln.rstrip("\n").split("\t")
    q, t, a = L.spans(cg)
    f[3], f[8], f[9], f[10] = str(int(f[2]) + q), str(int(f[7]) + t), str(a), str(max(q, t))
    assert int(f[3]) <= int(f[1]) and int(f[8]) <= int(f[6])
    return ("\t".join(f[:12] + [x if not x.startswith("cg:Z:") else "cg:Z:" + cg for x in f[12:]]) + "\n").encode()


@pytest.mark.parametrize("batch", [b for b in L.error_free_batches() if b.name.startswith("straddle")], ids=lambda b: b.name)
def test_straddles_are_sharp(batch):
    """the same line without the digits in front of the boundary (what a lost halo makes of it) gives another output"""
    pred = L.predict(batch.data)
    for ln, want, p in zip(batch.lines, batch.expect, pred):
        k_j_n = want.get("straddle") or want.get("lane")
        cg = ln.split("cg:Z:")[1].rstrip("\n")
        lost = L.without_front_digits(cg, want["at"], p["lead"], k_j_n[1])
        assert len(lost) == len(cg) - k_j_n[1] and L.spans(lost) != L.spans(cg)
        for mode in ("bed", "bed_n"):
            c0, _, out0 = L.oracle(mode, ln.encode())
            c1, _, out1 = L.oracle(mode, reline(ln, lost))
            assert c0 == 0 and c1 == 0 and out0 != out1, (batch.name, want)
        assert L.oracle("bed_n", ln.encode().replace(cg.encode(), lost.encode()))[0] == L.ERR_ASSERT  # with the ends left alone the walk misses them


def test_boundaries_are_sharp():
    """every record of group 7, moved by one base, changes the runs of its own sequences"""
    for g in L.SHAPES:
        at, moved = L.boundary_batch(g), L.boundary_batch(g, moved=True)
        c0, _, out0 = L.oracle("bed_n", at.data)
        c1, _, out1 = L.oracle("bed_n", moved.data)
        assert c0 == 0 and c1 == 0
        b0, b1 = L.bed_by_name(out0), L.bed_by_name(out1)
        for want in at.expect:
            name = want["name"]
            q, t = ("q_" + name).encode(), ("t_" + name).encode()
            if name.startswith("start_equals_end"):  # nothing to move: the sequence is one unaligned run on the empty side
                assert len(b0[q]) == 1 and b0[q][0].endswith(b" 0") and len(b0[t]) == 1 and b0[t][0].endswith(b" 0")  # a D or I op covers nothing
                continue
            assert b0[q] != b1[q] and b0[t] != b1[t], name
    lengths = {int(ln.split("\t")[1]) for ln in L.boundary_batch(64).lines}
    assert set(L.SEQ_LENGTHS) <= lengths


def test_runs_and_lines_cases():
    b = L.runs_batch()
    out = L.oracle("bed", b.data)[2]
    by = L.bed_by_name(out)
    # sequences are laid at multiples of 8 counters with 8 to 15 of padding: their ends fall on every position of a lane's sixteen
    pos, ends, seen = 0, set(), set()
    for ln in b.lines:
        f = ln.split("\t")
        if f[0] not in seen:
            seen.add(f[0])
            ends.add((pos + int(f[1])) % L.BED_PER)
            pos += (int(f[1]) + 15) & ~7
    assert ends == set(range(L.BED_PER))
    assert len(by[b"r64_last"]) == 2 and len(by[b"r4096_all"]) == 1 and len(by[b"r4096_none"]) == 1 and sum(len(v) == 1 for k, v in by.items() if k.startswith(b"one")) == 300
    assert by[b"r4096_last"][-1].endswith(b" 1") and by[b"r4096_first"][0].endswith(b" 1")  # non-zero counters on both sides of a sequence boundary
    lines = L.lines_batch()
    out = L.oracle("bed", lines.data)[2]
    by = L.bed_by_name(out)
    for n in (1, 95, 97, 300):
        assert len(by[b"N" * n]) >= 64
    # a wave's 64 lines well below the stage, within its last 16 bytes (staged or not by the output's alignment), and beyond it
    spans = L.wave_spans(lines, out)
    assert any(L.BED_STAGE - 200 <= x <= L.BED_STAGE - 15 for x in spans) and any(L.BED_STAGE - 15 < x <= L.BED_STAGE for x in spans), spans
    assert any(L.BED_STAGE < x <= L.BED_STAGE + 400 for x in spans) and any(x > 2 * L.BED_STAGE for x in spans), spans
    digits = {len(x.split(b" ")[1]) for x in out.splitlines()} | {len(x.split(b" ")[1]) for x in L.oracle("bed", L.ten_digit_batch().data)[2].splitlines()}
    assert {1, 7, 8, 10} <= digits
    kept = [L.oracle("bed", lines.data, **kw)[2].count(b"\n") for kw in L.LINE_OPTS]
    assert kept[0] == max(kept) and 0 in kept and len(set(kept)) >= 6, kept


def test_median_cases():
    b = L.median_batch()
    code, _, out = L.oracle("tile", b.data)
    assert code == 0
    level = {}
    for ln in out.splitlines():
        f = ln.split(b"\t")
        level.setdefault(f[0].decode(), []).append(int(ln.split(b"tl:i:")[1].split(b"\t")[0]))
    want = {"one": 5, "two_meets": 1, "two_equal": 3, "three_misses": 3, "three_meets": 1, "four_meets": 1, "four_misses": 3, "four_late": 2}
    for name, lv in want.items():
        assert level["m_" + name][-1] == lv, (name, level["m_" + name])
    assert level["m_slices"][-3:] == [6, 7, 8] and level["m_stairs"][-2] > 64 and level["m_stairs"][-1] > 1, (level["m_slices"][-3:], level["m_stairs"][-2:])

"""`paffy view` as a stream (paffy_hip_stream_open_view) and the device-side layout under it (paffy_hip_plan_view_layout /
_view_emit_range): the batches of test_gpu_view_text.py, streamed in chunks cut at several line ends and fetched in ranges of every size
that changes a cut, against the oracle's paf_pretty_print of every line and the oracle's sums. What a range holds is decided by the
greedy rule on the ORACLE's sizes (ranges_of below), never by the code under test."""
import random

import pytest

import oracle_lib as O
from test_gpu_alignment_rows import make_seq, sequences
from test_gpu_flat import cigar_of, record
from test_gpu_view_text import name_lines, name_sequences, oracle_text, ratio_lines, row_case, width_lines

pytestmark = pytest.mark.gpu
STATS = 10
ERR_MISSING_QUERY, ERR_SEQ_RANGE = 17, 21
E_STATE = -5
GUARD = 256


def ranges_of(sizes, range_bytes):
    """the greedy cut: a range takes records while their bytes stay within range_bytes, and one record at least -> [(first, end)]"""
    out, first = [], 0
    while first < len(sizes):
        end, held = first + 1, sizes[first]
        while end < len(sizes) and held + sizes[end] <= range_bytes:
            held += sizes[end]
            end += 1
        out.append((first, end))
        first = end
    return out


def sums_of(lines):
    tot = [0] * 6
    for ln in lines:
        if b"cg:Z:" in ln:
            tot = O.cigar_stats(cigar_of(ln).decode(), tot, zero=False)
    return tot


def chunks_of(lines, cuts):
    at = [0] + list(cuts) + [len(lines)]
    return [b"".join(lines[a:b]) for a, b in zip(at, at[1:])]


_CASES = {}


def rows_batch():
    """(lines, the oracle's blocks, the oracle's sums): row_case() under text = 2"""
    if "rows" not in _CASES:
        lines, blocks, _ = row_case()
        enc = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines), sequences())[0].splitlines(keepends=True)
        _CASES["rows"] = (lines, blocks, sums_of(enc))
    return _CASES["rows"]


def lines_batch():
    """the ratio / width / name batch under text = 1 (no record has an M op: the sums are those of the cigars as written)"""
    if "lines" not in _CASES:
        lines = ([c[0] for c in ratio_lines()] + width_lines() + name_lines()) * 2
        _CASES["lines"] = (lines, oracle_text(lines), sums_of(lines), name_sequences(lines))
    return _CASES["lines"]


def range_sizes(sizes, need_between=True):
    """the range_bytes of the issue: the whole text, exactly one block's size and that +- 1, 1, and a value with one record longer than the
    range between shorter ones"""
    block = sizes[len(sizes) // 2]
    between = None
    for i in range(1, len(sizes) - 1):
        if sizes[i] > max(sizes[i - 1], sizes[i + 1]):
            between = max(sizes[i - 1], sizes[i + 1])
            break
    assert between is not None or not need_between
    return [sum(sizes), block, block - 1, block + 1, 1] + ([between] if between is not None else [])


@pytest.fixture(scope="module")
def rows_eng():
    import paffy_amd

    e = paffy_amd.Engine()
    e.keep_raw_sequences(True)
    e.set_sequences(sequences())
    yield e
    e.close()


@pytest.fixture(scope="module")
def lines_eng():
    import paffy_amd

    e = paffy_amd.Engine()
    e.stats_only(True)
    e.set_sequences(lines_batch()[3])
    yield e
    e.close()


def check_stream(e, text, lines, want, tot, cut_sets):
    sizes = [len(w) for w in want]
    for cuts in cut_sets:
        chunks = chunks_of(lines, cuts)
        at = [0] + list(cuts) + [len(lines)]
        for rb in range_sizes(sizes):
            got = e.view_stream(chunks, text=text, range_bytes=rb)
            assert got["error"] is None, (cuts, rb, got["error"])
            assert got["text"] == b"".join(want), (cuts, rb)
            assert got["sums"] == tot and got["records"] == len(lines), (cuts, rb)
            # a chunk of more than one range, with another chunk behind it, had to be read out before the next buffer was to be had
            n_open = sum(1 for a, b in list(zip(at, at[1:]))[:-1] if len(ranges_of(sizes[a:b], rb)) > 1)
            assert got["open_chunks"] == n_open, (cuts, rb)


def test_rows_streamed_in_every_range_size(rows_eng):
    lines, blocks, tot = rows_batch()
    check_stream(rows_eng, 2, lines, blocks, tot, [(), (1,), (5, 9), (1, 2, 12)])


def test_lines_streamed_in_every_range_size(lines_eng):
    lines, want, tot, _ = lines_batch()
    n = len(lines)
    check_stream(lines_eng, 1, lines, want, tot, [(), (n // 2,), (1, 70, n - 1)])


@pytest.mark.parametrize("with_rows", [False, True], ids=["lines", "rows"])
def test_the_layout_is_the_greedy_cut_of_the_oracles_sizes(rows_eng, with_rows):
    """the range table of paffy_hip_plan_view_layout (first record, first byte) for range sizes on both sides of every kind of cut, on a
    batch long enough that the cut kernel's search takes more than one step of 64 probes; every range written between guards"""
    import paffy_amd

    e = rows_eng
    lines, blocks, _ = row_case()
    lines, blocks = lines * 40, blocks * 40  # 520 records
    enc = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(lines[:13]), sequences())[0].splitlines(keepends=True)
    want = blocks if with_rows else oracle_text(enc) * 40
    sizes = [len(w) for w in want]
    off = [0]
    for b in sizes:
        off.append(off[-1] + b)
    data = b"".join(lines)
    d_in = e.to_device(data)
    info = e.plan([paffy_amd.stage(O.ADD_MISMATCHES, 0.05, 1.0), paffy_amd.stage(STATS, 0.0, 0.0)], d_in, len(data))
    assert info.error.code == 0 and info.n_records == len(lines)
    for rb in range_sizes(sizes, need_between=with_rows) + [off[100], off[100] - 1, off[400], sum(sizes) - 1, sum(sizes) + 1, 1 << 62]:
        total, table = e.view_layout(with_rows, rb)
        model = ranges_of(sizes, rb)
        assert total == off[-1]
        assert table == [(a, off[a]) for a, _ in model] + [(len(sizes), off[-1])], rb
    # the ranges of one layout, each at the front of its own destination
    total, table = e.view_layout(with_rows, off[100])
    got = []
    for r, ((a, at), (b, end)) in enumerate(zip(table, table[1:])):
        text, err = e.view_emit_range(r, end - at, guard=GUARD)
        assert err is None
        got.append(text)
    assert len(got) > 3 and b"".join(got) == b"".join(want)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):  # PAFFY_E_CAPACITY
        e.view_emit_range(0, table[1][1], out_cap=table[1][1] - 1)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        e.view_emit_range(len(table) - 1, 16)
    # another plan since: the layout is gone with the plan it described
    assert e.plan([paffy_amd.stage(STATS, 0.0, 0.0)], d_in, len(data)).error.code == 0
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        e.view_emit_range(0, table[1][1])


def test_an_open_chunk_keeps_the_next_buffer_back(rows_eng):
    lines, blocks, tot = rows_batch()
    first, second = b"".join(lines[:6]), b"".join(lines[6:])
    st = rows_eng.open_view_stream(text=2, chunk_bytes=len(first) + len(second), range_bytes=1)
    try:
        assert st.input(first)
        info = st.submit(len(first))
        assert info.error.code == 0 and info.n_records == 6 and info.out_bytes == sum(len(b) for b in blocks[:6])
        assert not st.input(second) and not st.input(second)  # six ranges: the plan stays until they are read
        got = b"".join(st.pieces())
        assert got == b"".join(blocks[:6])
        assert st.input(second)
        assert st.submit(len(second)).error.code == 0
        assert b"".join(st.pieces()) == b"".join(blocks[6:])
        assert st.status() == (tot, len(lines), None)
    finally:
        st.close()
    # one range per chunk: the next buffer is there at once, and the chunk before is read while the next one is planned
    st = rows_eng.open_view_stream(text=2, chunk_bytes=len(first) + len(second), range_bytes=1 << 30)
    try:
        assert st.input(first) and st.submit(len(first)).error.code == 0
        assert st.input(second) and st.submit(len(second)).error.code == 0
        assert b"".join(st.pieces()) == b"".join(blocks[:6]) and b"".join(st.pieces()) == b"".join(blocks[6:])
    finally:
        st.close()


def test_an_empty_chunk_and_no_chunk(lines_eng):
    lines, want, tot, _ = lines_batch()
    got = lines_eng.view_stream([b"".join(lines[:10]), b"", b"".join(lines[10:])], text=1)
    assert (got["text"], got["sums"], got["records"], got["error"]) == (b"".join(want), tot, len(lines), None)
    got = lines_eng.view_stream([], text=1)
    assert (got["text"], got["sums"], got["records"], got["error"]) == (b"", [0] * 6, 0, None)


def test_text_0_gives_the_sums_alone(lines_eng, rows_eng):
    lines, want, tot, _ = lines_batch()
    got = lines_eng.view_stream(chunks_of(lines, (3, 50)), text=0)
    assert (got["text"], got["sums"], got["records"], got["error"]) == (b"", tot, len(lines), None)
    lines, blocks, tot = rows_batch()
    got = rows_eng.view_stream(chunks_of(lines, (4,)), text=0)
    assert (got["text"], got["sums"], got["records"], got["error"]) == (b"", tot, len(lines), None)


def test_a_chunk_with_a_failing_record_gives_nothing_and_the_oracles_error(rows_eng):
    lines, blocks, _ = rows_batch()
    seqs = sequences()
    kw = dict(qlen=len(seqs["qb"]), tlen=len(seqs["tb"]), qs=12_000, ts=13_000)
    lost = record([(20, "M")], "+", qname="nobody", tname="tb", **kw).encode()
    torn = b"qb\t30000\t5\t9\tx\ttb\t30000\t5\t9\t4\t4\t60\n"  # no such strand
    for bad_chunk, fail_at in (([lines[4], lost, lines[5]], 1), ([lines[4], lost, torn], 2), ([torn, lost], 0)):
        data = b"".join(lines[:4])
        _, err = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(bad_chunk), seqs)
        _, parse = O.run([O.stage(O.PASS)], b"".join(bad_chunk))
        want = parse if parse.code else err  # a line that does not parse is met before the stages run
        assert want.code and want.record == fail_at
        for rb in (1, 1 << 30):
            got = rows_eng.view_stream([data, b"".join(bad_chunk), b"".join(lines[6:])], text=2, range_bytes=rb)
            assert got["text"] == b"".join(blocks[:4]), (fail_at, rb)
            assert got["error"][:2] == (want.code, 4 + want.record), (got["error"], want.code, want.record)


# ---- the rows' own failure: a record of = / I ops whose coordinates pass the end of a loaded sequence ----
def short_case():
    if "short" not in _CASES:
        rng = random.Random(0x5407)
        seqs = {"q1": make_seq(rng, 1000), "t1": make_seq(rng, 1000), "qshort": make_seq(rng, 300)}

        def rec(qn, qs, k):
            return record([(40 + k, "="), (2, "I"), (60, "=")], "+-"[k % 2], qname=qn, tname="t1", qlen=1000, tlen=1000, qs=qs, ts=200 + k).encode()

        good = [rec("q1", 100 + k, k) for k in range(7)]
        far = rec("qshort", 250, 3)  # query_end 355 > the 300 bases loaded: the plan passes (no M op), the rows do not
        enc = O.run([O.stage(O.ADD_MISMATCHES)], b"".join(good), seqs)[0].splitlines(keepends=True)
        assert len(enc) == len(good)
        _CASES["short"] = (seqs, good, far, oracle_text(enc, seqs, True), oracle_text([far])[0])
    return _CASES["short"]


@pytest.fixture(scope="module")
def short_eng():
    import paffy_amd

    e = paffy_amd.Engine()
    e.keep_raw_sequences(True)
    e.set_sequences(short_case()[0])
    yield e
    e.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("later_range", [False, True], ids=["range0", "later_range"])
def test_a_rows_failure_ends_the_text_with_the_records_stats_line(short_eng, where, later_range):
    seqs, good, far, blocks, far_line = short_case()
    # the failing record's range holds three records: it and two good ones, in the place asked for
    k = {"first": 0, "middle": 1, "last": 2}[where]
    trio = good[3:5]
    trio.insert(k, far)
    trio_blocks = blocks[3:5]
    head = good[:3] if later_range else []
    head_blocks = blocks[:3] if later_range else []
    chunk = head + trio + good[5:]
    # ranges of three good blocks: the model on the oracle's sizes (the failing record's block: its line and rows as long as a good one's)
    rb = 3 * max(len(b) for b in blocks)
    far_block = len(far_line) + 3 * 105 + 3  # its 105 columns in one window of three rows
    sizes = [len(b) for b in head_blocks + trio_blocks[:k]] + [far_block] + [len(b) for b in trio_blocks[k:] + blocks[5:]]
    assert (len(head), len(head) + 3) in ranges_of(sizes, rb)
    want = b"".join(head_blocks) + b"".join(trio_blocks[:k]) + far_line
    first_chunk = b"".join(good[5:7])
    st = short_eng.open_view_stream(text=2, chunk_bytes=1 << 16, range_bytes=rb)
    try:
        assert st.input(first_chunk) and st.submit(len(first_chunk)).error.code == 0
        data = b"".join(chunk)
        assert st.input(data)
        info = st.submit(len(data))
        assert info.error.code == 0  # the plan passes: the record has no M op
        assert b"".join(st.pieces()) == b"".join(blocks[5:7]) and st.status()[2] is None
        assert b"".join(st.pieces()) == want
        assert st.status()[2] == (ERR_SEQ_RANGE, len(head) + k)  # counted from the chunk's first record
        assert st.input(first_chunk)
        rc, _ = st.submit_rc(len(first_chunk))
        assert rc == E_STATE
    finally:
        st.close()
    got = short_eng.view_stream([first_chunk, b"".join(chunk), first_chunk], text=2, range_bytes=rb)
    assert got["text"] == b"".join(blocks[5:7]) + want
    assert got["error"] == (ERR_SEQ_RANGE, 2 + len(head) + k, 0, -1)


def test_emit_range_reports_a_missing_sequence_and_what_was_printed(rows_eng):
    """a name that is among no sequences fails the plan of `view` itself, so the rows' own report of it is reached behind a plan of STATS
    alone, as in test_gpu_view_text.py"""
    import paffy_amd

    e = rows_eng
    seqs = sequences()
    kw = dict(qlen=len(seqs["qb"]), tlen=len(seqs["tb"]), qs=12_000, ts=13_000)
    good = record([(20, "M")], "+", qname="qb", tname="tb", **kw).encode()
    lost = record([(20, "M")], "+", qname="nobody", tname="tb", **kw).encode()
    batch = [good, good, good, lost, good, good]
    data = b"".join(batch)
    d_in = e.to_device(data)
    assert e.plan([paffy_amd.stage(STATS, 0.0, 0.0)], d_in, len(data)).error.code == 0
    block, line = oracle_text([good], seqs, True)[0], oracle_text([lost])[0]
    assert len(line) == len(oracle_text([good])[0]) + 4  # "nobody" for "qb"
    sizes = [len(block)] * 3 + [len(block) + 4] + [len(block)] * 2  # the lost record's rows would be as long as a good one's
    rb = 2 * len(block) + 4
    assert ranges_of(sizes, rb) == [(0, 2), (2, 4), (4, 6)]
    total, table = e.view_layout(True, rb)
    assert [a for a, _ in table] == [0, 2, 4, 6]
    assert e.view_emit_range(0, table[1][1], guard=GUARD) == (block * 2, None)
    assert e.view_emit_range(1, table[2][1] - table[1][1], guard=GUARD) == (block + line, (ERR_MISSING_QUERY, 3))
    assert e.view_emit_range(2, table[3][1] - table[2][1], guard=GUARD) == (block * 2, None)


@pytest.mark.parametrize("text", [1, 2])
def test_view_in_parts_equals_one_part(text):
    from paffy_amd import shard

    if text == 2:
        lines, want, tot = rows_batch()
        seqs = sequences()
    else:
        lines, want, tot, seqs = lines_batch()
    data = b"".join(lines)
    one = shard.view_in_parts(data, seqs, 1, text=text)
    assert (one["text"], one["sums"], one["records"], one["error"]) == (b"".join(want), tot, len(lines), None)
    for n in (2, 3, 5):
        got = shard.view_in_parts(data, seqs, n, text=text, chunk_bytes=4096)
        assert (got["text"], got["sums"], got["records"], got["error"]) == (one["text"], one["sums"], one["records"], None), n
        assert len(got["parts"]) == n and sum(got["parts"]) == len(lines)


def test_a_record_without_a_cigar_where_the_batch_before_had_one(rows_eng):
    """under [ADD_MISMATCHES, STATS] without paffy_hip_stats_only nobody sizes a record that has no cigar, so its RecPlan is what the batch
    before left at that index; the rows' kernels must not read it. Two plans on one context, the record without a cigar at an
    index where the first batch had 150 and 451 columns: the sizes and the text with rows are the oracle's, through both pairs of calls,
    and two chunks of one stream with the record first in the second"""
    import paffy_amd

    e = rows_eng
    lines, blocks, tot = rows_batch()
    bare = [i for i, ln in enumerate(lines) if b"cg:Z:" not in ln]
    assert bare == [5]
    stages = [paffy_amd.stage(O.ADD_MISMATCHES, 0.05, 1.0), paffy_amd.stage(STATS, 0.0, 0.0)]
    for at in (0, 4, 7):  # where the record without a cigar lands in the second batch
        first = b"".join(lines[6:] + lines[:5])  # every index holds a record with a cigar
        d_in = e.to_device(first)
        assert e.plan(stages, d_in, len(first)).error.code == 0
        order = [i for i in range(len(lines)) if i != 5]
        order.insert(at, 5)
        data = b"".join(lines[i] for i in order)
        want = [blocks[i] for i in order]
        d_in2 = e.to_device(data)
        info = e.plan(stages, d_in2, len(data))
        assert info.error.code == 0 and info.n_records == len(lines)
        assert e.view_sizes(0, len(lines), with_rows=True) == [len(w) for w in want], at
        assert e.view_text(0, len(lines), with_rows=True, guard=GUARD) == b"".join(want), at
        total, table = e.view_layout(True, 1 << 30)
        assert (total, table) == (sum(len(w) for w in want), [(0, 0), (len(lines), sum(len(w) for w in want))]), at
        assert e.view_emit_range(0, total, guard=GUARD) == (b"".join(want), None), at
    got = e.view_stream([b"".join(lines[:5]), b"".join(lines[5:])], text=2)
    assert (got["text"], got["sums"], got["error"]) == (b"".join(blocks), tot, None)

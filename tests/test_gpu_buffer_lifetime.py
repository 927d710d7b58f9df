"""Device buffers free themselves (paffy_amd/csrc/device_buffer.h): the library's tally of the buffers it owns (paffy_hip_device_buffers)
is, after everything a case made has been closed, exactly what it was before the case made anything -- whichever command states a
context allocated, whoever of a stream and its context goes first. The counters are compared with their values at the start, not with
zero: the module-level engine of paffy_amd.engine, or another test's, may be alive. Inputs of a few records; what the commands write is
the business of their own tests."""
import gc

import pytest
import torch

import synth_lib
from paffy_amd import shard
from test_gpu_upconvert import FASTA as INTERVALS, record as upconvert_record

pytestmark = pytest.mark.gpu

FASTA_TEXT = b">a\n" + b"ACGTTGCAAC" * 90 + b"\n>b some words\n" + b"GGCATNNNTA" * 70 + b"\n"


@pytest.fixture(scope="module")
def P():
    import paffy_amd

    return paffy_amd


@pytest.fixture(scope="module")
def E():
    import paffy_amd.engine as E

    return E


@pytest.fixture(scope="module")
def aligned():
    """a dozen records on their two genomes: (PAF text, {name: bases})"""
    host = synth_lib.Synth4(0x5EED0004, 512, n_contigs=8, tlen_min=60_000, tlen_span=90_000)
    return host.records(0, 12), host.genomes()


def counters(E):
    gc.collect()  # an engine another test dropped without closing it goes now, not in the middle of the case
    return E.device_buffers()


def lines_of(data, n):
    return b"".join(data.splitlines(keepends=True)[:n])


def test_every_command_state_of_one_engine(P, E, human_chimp, aligned):
    start = counters(E)
    e = P.Engine()
    created = E.device_buffers()
    assert created[0] > start[0] and created[1] > start[1]
    paf, seqs = aligned
    few = lines_of(human_chimp, 40)

    assert e.run([P.stage(P.INVERT)], few)[0]  # a lean pipe
    assert e.run([P.stage(P.SHATTER)], few)[0]
    e.keep_raw_sequences(True)
    e.set_sequences(seqs)
    assert e.run([P.stage(P.ADD_MISMATCHES)], paf)[0]
    d_in = e.to_device(paf)  # view with rows: the text of a plan at once, and laid out in ranges
    info = e.plan([P.stage(P.ADD_MISMATCHES), P.stage(P.STATS)], d_in, len(paf))
    assert info.error.code == 0 and e.view_text(0, info.n_records, True)
    total, ranges = e.view_layout(True)
    assert total > 0 and e.view_emit_range(0, ranges[1][1] - ranges[0][1])[1] is None
    assert e.tile(few)[0] and e.chain(few)[0]
    assert e.to_bed(few)[0]
    d_few = e.to_device(few)  # to_bed in parts: every line with a side mask
    n_few = few.count(b"\n")
    info = e.bed_part([(d_few, len(few))], sides=[torch.ones(n_few, dtype=torch.uint8, device=e.device)])
    assert info.error.code == 0 and info.out_bytes > 0
    e.emit(e.alloc_out(info.out_bytes))
    e.sync()
    assert e.dedupe(few + lines_of(few, 20))[0]
    res = shard.dedupe_in_parts([shard.GpuDedupeWorker(e)], [[(d_few, len(few))], [(d_few, len(few))]], False)  # two rounds: the owner's memory swaps
    assert res["error"] is None and res["records"] == 2 * n_few
    assert e.split_file(few)[0]
    e.set_intervals([h for h, _ in INTERVALS], [n for _, n in INTERVALS])
    up = upconvert_record(b"chrA", 100000, 1100, 1200, b"chrB", 50000, 21000, 21100, cg=b"100M")
    assert e.run([P.stage(P.UPCONVERT)], up)[0]
    assert e.set_sequences_fasta([FASTA_TEXT]) == 2  # the loader's own index; its bases are swapped into the store
    assert e.set_intervals_fasta([b">chrA|100000|0\n" + b"ACGT" * 25 + b"\n"]) == 1
    assert len(e.fasta_seen([FASTA_TEXT], b"a\t900\t0\t10\t+\tb\t700\t0\t10\t10\t10\t60\n")) == 2
    chunks = e.faffy_chunk([FASTA_TEXT], 300, 20)
    assert len(chunks) > 2
    assert e.faffy_merge([c for _, c in chunks])
    assert e.faffy_extract([FASTA_TEXT], b"a\t100\t400\na\t500\t880\n")
    batches = [e.to_device(x) for x in (few, lines_of(human_chimp, 25))]  # the names of two batches before the first is split: two kept indexes
    sizes = [len(few), len(lines_of(human_chimp, 25))]
    owner_of = {}
    for b, n in zip(batches, sizes):
        owner_of.update({h: k % 2 for k, h in enumerate(sorted(e.query_names(b, n)))})
    for b, n in zip(batches, sizes):
        out, pb, pr, _ = e.split_by_owner(b, n, 2, owner_of)  # the entry goes to the pool
        assert sum(pb) == n
    assert e.query_names(batches[1], sizes[1])  # an entry from the pool again, never split: it goes with the context

    alive = E.device_buffers()
    assert alive[0] > created[0] and alive[1] > created[1]
    e.close()
    assert E.device_buffers() == start


def test_kept_slot_buffers_of_streams(P, E, human_chimp):
    start = counters(E)
    e = P.Engine()
    chunks = [lines_of(human_chimp, 30)] * 3
    got = []
    assert e.stream_host([P.stage(P.INVERT)], chunks, sink=got.append)[0] == 90
    assert b"".join(got) == e.run([P.stage(P.INVERT)], chunks[0])[0] * 3
    closed = E.device_buffers()
    assert E.lib().paffy_hip_stream_trim(e._ctx) == 0
    trimmed = E.device_buffers()
    assert trimmed[0] == closed[0] - 4 and trimmed[1] < closed[1]  # two slots, input and output: the stream left them with the context
    e.close()
    assert E.device_buffers() == start


def test_second_stream_adopts_the_buffers_of_the_first(P, E, human_chimp):
    start = counters(E)
    e = P.Engine()
    chunk = lines_of(human_chimp, 30)
    during = []

    def sink(piece):
        during.append(E.device_buffers()[0])

    e.stream_host([P.stage(P.INVERT)], [chunk] * 3, sink=sink)
    first = max(during)
    del during[:]
    e.stream_host([P.stage(P.INVERT)], [chunk], sink=sink)  # one chunk: what the count is after the stream's first chunk
    assert during and max(during) <= first
    e.close()
    assert E.device_buffers() == start


def test_engine_closed_before_its_view_stream(P, E, aligned):
    start = counters(E)
    paf, seqs = aligned
    e = P.Engine()
    e.keep_raw_sequences(True)
    e.set_sequences(seqs)
    st = e.open_view_stream(text=2, chunk_bytes=len(paf))
    assert st.input(paf)
    assert st.submit(len(paf)).error.code == 0  # every call raises on a status other than 0
    assert b"".join(st.pieces())
    assert st.status()[1] == paf.count(b"\n")
    during = E.device_buffers()
    e.close()  # detaches the stream: its slots' buffers are its own now
    left = E.device_buffers()
    assert start[0] < left[0] < during[0]
    st.close()
    assert E.device_buffers() == start


def test_two_engines_closed_in_the_opposite_order(P, E, human_chimp):
    start = counters(E)
    a, b = P.Engine(), P.Engine()
    few = lines_of(human_chimp, 40)
    want = None
    for k in range(3):
        for e in (a, b):
            out = (e.run([P.stage(P.SHATTER)], few)[0], e.tile(few)[0], e.dedupe(few)[0])
            assert want is None or out == want
            want = out
    b.close()
    assert E.device_buffers()[0] > start[0]
    a.close()
    assert E.device_buffers() == start

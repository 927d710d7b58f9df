"""`paffy view` as a stream, without a GPU: the library cross-compiled for gfx950 exports and declares the layout calls and the view
mode of the stream, the Python mirrors exist, and the compiler's resource remarks show that the kernels of the layout -- and the two
writers, which now read their offsets rebased -- use no scratch memory and spill no register."""
import os
import re
import subprocess

from paffy_amd import engine, shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("k_view_range_cut", "k_view_range_verdict")
WRITERS = ("k_view_line_size", "k_view_line_emit")
DECLARATIONS = (
    r"int paffy_hip_plan_view_layout\(paffy_hip_ctx \*ctx, int with_rows, int64_t range_bytes, int64_t \*total_bytes, int64_t \*n_ranges\);",
    r"int64_t paffy_hip_plan_view_ranges\(paffy_hip_ctx \*ctx, int64_t cap_ranges, int64_t \*first_record, int64_t \*first_byte\);",
    r"int paffy_hip_plan_view_emit_range\(paffy_hip_ctx \*ctx, int64_t range, void \*d_out, int64_t out_cap, int64_t \*bytes, paffy_error \*err\);",
    r"int paffy_hip_stream_open_view\(paffy_hip_ctx \*ctx, int text, int64_t chunk_bytes, int64_t piece_bytes, int64_t range_bytes, "
    r"paffy_hip_stream \*\*stream\);",
    r"int paffy_hip_stream_view_status\(paffy_hip_stream \*stream, int64_t sums\[6\], int64_t \*n_records, paffy_error \*rows_err\);",
)


def test_the_view_stream_calls_are_exported_and_declared():
    lib = engine.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert {"paffy_hip_plan_view_layout", "paffy_hip_plan_view_ranges", "paffy_hip_plan_view_emit_range", "paffy_hip_stream_open_view",
            "paffy_hip_stream_view_status"} <= names
    assert {"paffy_hip_plan_view_sizes", "paffy_hip_plan_view_text"} <= names  # the two calls the layout stands beside stay
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        header = " ".join(fh.read().split())  # a declaration may be broken over lines
    for d in DECLARATIONS:
        assert re.search(r"\b" + d, header), d
    for name in ("view_layout", "view_emit_range", "open_view_stream", "view_stream"):
        assert callable(getattr(engine.Engine, name, None)), name
    assert callable(shard.view_in_parts) and callable(shard.stream_cuts)


def test_the_launchers_cut_in_python():
    data = b"a\nbb\nccc\ndddd\n"
    assert shard.stream_cuts(data, 1) == [0, len(data)]
    assert shard.stream_cuts(data, 2) == [0, 9, len(data)]  # 14 // 2 = 7 lies inside "ccc\n": the first line end at or after it
    assert shard.stream_cuts(b"x\ny\n", 5) == [0, 2, 4, 4, 4, 4]  # fewer lines than parts: a cut never lies in front of the one before, empty parts
    assert shard.stream_cuts(b"", 3) == [0, 0, 0, 0]
    assert shard.stream_cuts(b"no line end", 2) == [0, 11, 11]


def test_the_view_layout_kernels_use_no_scratch():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "paffy_amd", "csrc"), "resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    name = None
    for ln in (r.stdout + r.stderr).splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", ln)
        if m and name:
            found.setdefault(name, {})[m.group(1)] = int(m.group(2))
    for k in NEW_KERNELS + WRITERS:
        tail = r"\d+ViewLineParams\w*" if k in WRITERS else r"P\w+"
        mine = [v for n, v in found.items() if re.fullmatch(r"_Z\d+%s%s" % (k, tail), n)]
        assert len(mine) == 1, (k, sorted(found)[:5])
        print(k, mine[0])
        assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0 and mine[0]["SGPRs Spill"] == 0, (k, mine[0])

"""`paffy view`'s text on the device without a GPU: the library cross-compiled for gfx950 exports and declares paffy_hip_plan_view_sizes
and paffy_hip_plan_view_text, and the compiler's resource remarks show that the kernels of view_line_kernel.h use no scratch memory and
spill no register."""
import os
import re
import subprocess

from paffy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_view_line_size", "k_view_line_emit")


def test_the_view_text_calls_are_exported_and_declared():
    lib = engine.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert {"paffy_hip_plan_view_sizes", "paffy_hip_plan_view_text"} <= names
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        header = " ".join(fh.read().split())  # a declaration may be broken over lines
    assert re.search(r"\bint paffy_hip_plan_view_sizes\(paffy_hip_ctx \*ctx, int64_t first, int64_t count, int with_rows, int64_t \*h_bytes\);", header)
    assert re.search(r"\bint paffy_hip_plan_view_text\(paffy_hip_ctx \*ctx, int64_t first, int64_t count, int with_rows, const int64_t \*h_off, "
                     r"void \*d_out, int64_t out_cap, paffy_error \*err\);", header)
    assert callable(getattr(engine.Engine, "view_sizes", None)) and callable(getattr(engine.Engine, "view_text", None)) and callable(engine.view)


def test_the_view_line_kernels_use_no_scratch():
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
    for k in KERNELS:
        mine = [v for n, v in found.items() if re.fullmatch(r"_Z\d+%s\d+ViewLineParams\w*" % k, n)]
        assert len(mine) == 1, (k, sorted(found)[:5])
        print(k, mine[0])
        assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0 and mine[0]["SGPRs Spill"] == 0, (k, mine[0])

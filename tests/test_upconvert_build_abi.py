"""The device build of upconvert's interval table without a GPU: the two calls that show the table are exported and declared, the Python
methods exist, the library is still one translation unit, and the compiler's resource remarks show that the kernels of
upconvert_build_kernel.h use no scratch memory and spill no register."""
import os
import re
import subprocess

from paffy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_up_decode", "k_up_gather", "k_up_lens", "k_up_table")
DECLS = ("int paffy_hip_intervals_info(paffy_hip_ctx *ctx, int64_t out[4]);",
         "int paffy_hip_intervals_read(paffy_hip_ctx *ctx, int64_t cap, int64_t blob_cap, int64_t *nums, uint32_t *slices, void *blob);")


def test_the_calls_are_exported_and_declared():
    lib = engine.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in ("paffy_hip_intervals_info", "paffy_hip_intervals_read"):
        assert re.search(r" T %s$" % name, syms, re.M), name
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        header = fh.read()
    for decl in DECLS:
        assert decl in header, decl


def test_the_python_methods_exist():
    assert callable(getattr(engine.Engine, "intervals_info", None)) and callable(getattr(engine.Engine, "intervals", None))


def test_the_library_is_one_translation_unit_with_the_new_headers():
    csrc = os.path.join(ROOT, "paffy_amd", "csrc")
    with open(os.path.join(csrc, "seqload_host.h")) as fh:
        assert '#include "upconvert_build_host.h"' in fh.read()
    with open(os.path.join(csrc, "upconvert_build_host.h")) as fh:
        assert '#include "upconvert_build_kernel.h"' in fh.read()
    with open(os.path.join(csrc, "paffy_hip.hip")) as fh:
        assert '#include "seqload_host.h"' in fh.read()
    with open(os.path.join(csrc, "Makefile")) as fh:
        make = fh.read()
    assert "upconvert_build_kernel.h" in make and "upconvert_build_host.h" in make
    assert [f for f in os.listdir(csrc) if f.endswith(".hip")] == ["paffy_hip.hip"]


def test_the_new_kernels_use_no_scratch_and_spill_nothing():
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
        mine = [v for n, v in found.items() if re.fullmatch(r"_Z%d%s[A-Za-z].*" % (len(k), k), n)]
        assert len(mine) == 1, (k, sorted(found)[:5])
        print(k, mine[0])
        assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0 and mine[0]["SGPRs Spill"] == 0, (k, mine[0])

"""The flat pass's `add_mismatches | trim | filter` mode without a GPU: the library cross-compiled for gfx950 builds with the kernels of
flat_add_pipe_kernel.h, and the compiler's resource remarks show that they use no scratch memory and spill no register."""
import os
import re
import subprocess

from paffy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_addp_fill", "k_addp_size")


def test_the_library_builds_with_the_new_mode():
    lib = engine.build_library()
    assert os.path.exists(lib)
    with open(os.path.join(ROOT, "paffy_amd", "csrc", "paffy_hip.hip")) as fh:
        src = fh.read()
    assert "FLAT_MODE_ADD_PIPE" in src and '#include "flat_add_pipe_kernel.h"' in src


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
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", ln)
        if m and name:
            found.setdefault(name, {})[m.group(1)] = int(m.group(2))
    for k in KERNELS:
        mine = [v for n, v in found.items() if re.fullmatch(r"_Z\d+%s\d+AddPipeParams" % k, n)]
        assert len(mine) == 1, (k, sorted(found)[:5])
        print(k, mine[0])
        assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0, (k, mine[0])

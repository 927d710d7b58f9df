"""The device plan of `faffy extract` without a GPU: the library cross-compiled for gfx950 builds with the kernels of
fasta_extract_kernel.h and exports the plan that takes device text, the host loop is gone, and the compiler's resource remarks show
that the new kernels use no scratch memory and spill no register (rocPRIM's own kernels are not judged)."""
import os
import re
import subprocess

from paffy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paffy_amd", "csrc")
KERNELS = ("k_bed_index", "k_bed_parse", "k_bed_bounds", "k_bed_compact", "k_bed_heads", "k_bed_items")


def test_the_library_builds_with_the_device_plan():
    lib = engine.build_library()
    assert os.path.exists(lib)
    with open(os.path.join(CSRC, "fasta_host.h")) as fh:
        src = fh.read()
    assert '#include "fasta_extract_kernel.h"' in src
    assert "paffy_hip_faffy_extract_plan_device" in src
    assert "unordered_map" not in src and "atol(tok" not in src and "strcmp(" not in src and "std::sort(ivs" not in src  # the host loop
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    assert re.search(r"\bT paffy_hip_faffy_extract_plan_device\b", nm.stdout)
    assert re.search(r"\bT paffy_hip_faffy_extract_plan\b", nm.stdout)


def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    r = subprocess.run(["make", "-C", CSRC, "resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    name = where = None
    for ln in (r.stdout + r.stderr).splitlines():
        m = re.search(r"(\S+?):\d+:\d+: remark: Function Name: (\S+)", ln)
        if m:
            where, name = os.path.basename(m.group(1)), m.group(2)
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)", ln)
        if m and name:
            found.setdefault((where, name), {})[m.group(1)] = int(m.group(2))
    for k in KERNELS:
        mine = [v for (w, n), v in found.items() if w == "fasta_extract_kernel.h" and re.fullmatch(r"_Z\d+%s\w+" % k, n)]
        assert len(mine) == 1, (k, sorted(found)[:5])
        print(k, mine[0])
        assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0 and mine[0]["SGPRs Spill"] == 0, (k, mine[0])

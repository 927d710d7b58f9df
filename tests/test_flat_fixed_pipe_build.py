"""The flat pass with a fixed trim at any place of a stage list, without a GPU: the library cross-compiled for gfx950 builds, and the
compiler's resource remarks show that every instantiation of k_flat_size uses no scratch memory and spills no register -- what the
flat-pass kernels had before (the wave kernel of `trim -f` before this, k_flat_size<true>: 86 VGPRs, 0 bytes of scratch, 0 spilled)."""
import os
import re
import subprocess

from paffy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_builds_and_the_host_takes_the_lists():
    lib = engine.build_library()
    assert os.path.exists(lib)
    with open(os.path.join(ROOT, "paffy_amd", "csrc", "paffy_hip.hip")) as fh:
        src = fh.read()
    assert "has_fixed" in src and "fixed_last" not in src
    with open(os.path.join(ROOT, "paffy_amd", "csrc", "flat_kernel.h")) as fh:
        assert "struct FlatCuts" in fh.read()


def test_the_sizing_kernels_use_no_scratch_and_spill_nothing():
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
    mine = {n: v for n, v in found.items() if re.fullmatch(r"_Z\d+k_flat_sizeILi[012]EEv\d+FlatSizeParams", n)}
    assert len(mine) == 3, sorted(found)[:5]  # no fixed trim, one as the last stage, at any place
    for n, v in sorted(mine.items()):
        print(n, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (n, v)

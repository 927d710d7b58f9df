"""The sums-only mode of `paffy view` without a GPU: the library cross-compiled for gfx950 exports and declares paffy_hip_stats_only, and
the compiler's resource remarks show that the kernels of flat_view_kernel.h use no scratch memory."""
import os
import re
import subprocess

from paffy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_view_prep", "k_view_count", "k_view_final")


def test_stats_only_is_exported_and_declared():
    lib = engine.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "paffy_hip_stats_only" in {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        assert re.search(r"\bint paffy_hip_stats_only\(paffy_hip_ctx \*ctx, int on\);", fh.read())
    assert callable(getattr(engine.Engine, "stats_only", None))


def test_the_view_kernels_use_no_scratch():
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
        mine = [v for n, v in found.items() if re.fullmatch(r"_Z\d+%s\d+ViewParams" % k, n)]
        assert len(mine) == 1, (k, sorted(found)[:5])
        print(k, mine[0])
        assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0, (k, mine[0])

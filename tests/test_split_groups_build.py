"""split_file's grouping without a GPU: the library cross-compiled for gfx950 exports and declares the four split calls, the engine has
split_file, and the compiler's resource remarks show that the kernels of split_kernel.h use no scratch memory and spill nothing."""
import os
import re
import subprocess

from paffy_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_split_keys", "k_split_heads", "k_split_verify", "k_split_counts", "k_split_place", "k_split_table", "k_split_names")
DECLS = (r"int paffy_hip_split_begin\(paffy_hip_ctx \*ctx, int by_query, int64_t min_length\);",
         r"int paffy_hip_split_plan\(paffy_hip_ctx \*ctx, const void \*d_in, int64_t in_len, paffy_plan_info \*info\);",
         r"int64_t paffy_hip_split_groups\(paffy_hip_ctx \*ctx, int64_t cap, paffy_split_group \*groups\);",
         r"int64_t paffy_hip_split_file_name\(paffy_hip_ctx \*ctx, int64_t file, char \*buf, int64_t cap\);")


def test_the_split_calls_are_exported_and_declared():
    lib = engine.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for name in ("paffy_hip_split_begin", "paffy_hip_split_plan", "paffy_hip_split_groups", "paffy_hip_split_file_name"):
        assert name in exported, name
    with open(os.path.join(ROOT, "include", "paffy_hip.h")) as fh:
        header = fh.read()
    for decl in DECLS:
        assert re.search(r"(?m)^" + decl, header), decl
    assert re.search(r"int64_t file, out_off, bytes, lines, first_record;\s+int32_t new_file, is_small;\s+} paffy_split_group;", header)
    for name in ("split_file", "split_begin", "split_plan", "split_groups", "split_file_name"):
        assert callable(getattr(engine.Engine, name, None)), name
    import paffy_amd

    assert callable(paffy_amd.split_file)


def test_the_split_kernels_use_no_scratch_and_spill_nothing():
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
        mine = [v for n, v in found.items() if n == k]  # extern "C" in paffy_hip.hip: the names are not mangled
        assert len(mine) == 1, (k, sorted(found)[:5])
        print(k, mine[0])
        assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0, (k, mine[0])

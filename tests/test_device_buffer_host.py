"""paffy_amd/csrc/device_buffer.h without a GPU: tests/host/device_buffer_check.cpp is a stand-alone program with its own hipMalloc / hipFree
(malloc and free behind a tally), built with AddressSanitizer + UBSan and run as a subprocess. It moves buffers the ways the library does
(kept indexes between two vectors, stream slots to the context and back, std::swap, the exact-size fallback of a failed allocation) and
ends with status 0 only if every check held and both its tally and the library's counters are back at zero; a buffer freed twice or not at
all is the sanitizer's report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SAN = dict(ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_device_buffer_moves_frees_and_counts(tmp_path):
    exe = str(tmp_path / "device_buffer_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"),
                           "-I", os.path.join(ROOT, "paffy_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "host", "device_buffer_check.cpp"), "-o", exe])
    p = subprocess.run([exe], env=dict(os.environ, **SAN), capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith(b"device_buffer_check: ok") and p.stderr == b"", (p.returncode, p.stdout, p.stderr[-4000:])

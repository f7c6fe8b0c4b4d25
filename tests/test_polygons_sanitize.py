"""Host-only AddressSanitizer + UndefinedBehaviorSanitizer run of amp_polygons_to_rle's argument check and host evaluation (polygon_runs_host.hip and
the routines of rle_host.hip are plain C++): random polygon instances against the composition of amp_rle_from_polygon and amp_rle_merge2, every
buffer of exactly the capacity asked for, the closed-form edge walk the device kernels use against the routine's crossings, and the refusals
(tests/sanitize/polygons_sanitize_main.cpp).  The device kernels index only what the check lets through."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_polygons_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "polygons_sanitize")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-o", exe,
           os.path.join(ROOT, "tests", "sanitize", "polygons_sanitize_main.cpp"), os.path.join(ROOT, "ampis_amd", "csrc", "rle_host.hip"),
           os.path.join(ROOT, "ampis_amd", "csrc", "polygon_runs_host.hip")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "POLYGONS SANITIZE OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

"""Host-only AddressSanitizer + UndefinedBehaviorSanitizer run of what the four mask analyses share (ampis_amd/csrc/run_list.h is plain C++):
the bit-plane painter against a per-pixel loop on the sizes of the shared case set and on random crops, the walk over a run list with its
refusals, and hostile off / len through the four argument checks (tests/sanitize/run_list_sanitize_main.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_shared_run_list_layer_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "run_list_sanitize")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-o", exe,
           os.path.join(ROOT, "tests", "sanitize", "run_list_sanitize_main.cpp"), os.path.join(ROOT, "ampis_amd", "csrc", "mask_analysis_host.hip")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "RUN LIST SANITIZE OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

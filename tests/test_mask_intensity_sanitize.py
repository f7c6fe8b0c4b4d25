"""Host-only AddressSanitizer + UndefinedBehaviorSanitizer run of amp_mask_intensity's argument check and host evaluation (mask_intensity.h and
mask_intensity_host.hip are plain C++): hand shapes and random masks, tight and with zero-length runs, under random images of both depths and
1 .. 4 channels, every value and every bin checked against a loop over all pixels, every buffer of exactly the capacity asked for, one word
less refused, and the refusals (tests/sanitize/mask_intensity_sanitize_main.cpp).  The device kernels index only what the check lets through."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_intensity_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "mask_intensity_sanitize")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    cmd = ["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-o", exe,
           os.path.join(ROOT, "tests", "sanitize", "mask_intensity_sanitize_main.cpp"), os.path.join(ROOT, "ampis_amd", "csrc", "mask_intensity_host.hip")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "MASK INTENSITY SANITIZE OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

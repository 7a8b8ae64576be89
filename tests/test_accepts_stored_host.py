"""The host side of the stored Accept encoder (mpx_encode_accepts_stored and its _reserve / _dev
forms) under AddressSanitizer + UndefinedBehaviorSanitizer: engine.cpp and accepts_stored.cpp over
the host-memory stand-in for the HIP runtime (tests/san/hip_stub.cpp, unchanged) and a stand-in
for the launcher that really encodes (tests/san/accepts_stored_stub.cpp), driven by the
stand-alone program tests/san/accepts_stored_driver.cpp. Every argument-validation path of both
forms answers its code before anything is staged; valid MIN and CLASSIC calls bring the
hand-worked bytes back through the staging arena on guarded buffers, and of a 2^20-entry arena
only the referenced commands are staged. Nothing is loaded into Python: the program is compiled
with the sanitizers and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CSRC = os.path.join(ROOT, "minpaxos_amd", "csrc")


def test_accepts_stored_host_paths_asan_ubsan(tmp_path):
    exe = str(tmp_path / "accepts_stored_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(CSRC, "engine.cpp"),
           os.path.join(CSRC, "accepts_stored.cpp"), os.path.join(SAN, "hip_stub.cpp"),
           os.path.join(SAN, "accepts_stored_stub.cpp"),
           os.path.join(SAN, "accepts_stored_driver.cpp"), "-ldl", "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

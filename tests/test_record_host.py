"""The host side of record assembly (mpx_record_log and its _reserve / _dev forms) under
AddressSanitizer + UndefinedBehaviorSanitizer: engine.cpp and record.cpp over the host-memory
stand-in for the HIP runtime (tests/san/hip_stub.cpp) and a stand-in for the record launcher that
really encodes (tests/san/record_stub.cpp), driven by the stand-alone program
tests/san/record_driver.cpp. Every argument-validation path of both forms answers its code before
anything is staged; valid calls bring the run's bytes, item_off and res back through the staging
arena on guarded buffers. Nothing is loaded into Python: the program is compiled with the
sanitizers and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CSRC = os.path.join(ROOT, "minpaxos_amd", "csrc")


def test_record_host_paths_asan_ubsan(tmp_path):
    exe = str(tmp_path / "record_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(CSRC, "engine.cpp"),
           os.path.join(CSRC, "record.cpp"), os.path.join(SAN, "hip_stub.cpp"),
           os.path.join(SAN, "record_stub.cpp"), os.path.join(SAN, "record_driver.cpp"), "-ldl",
           "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

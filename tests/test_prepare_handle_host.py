"""The host side of the prepare side (mpx_gather_prepares, mpx_prepare_handle,
mpx_encode_prepare_replies and their _reserve / _dev forms) under AddressSanitizer +
UndefinedBehaviorSanitizer: engine.cpp and prepare_handle.cpp over the host-memory stand-in for the
HIP runtime (tests/san/hip_stub.cpp, unchanged) and stand-ins for the launchers that really do the
work (tests/san/prepare_handle_stub.cpp), driven by the stand-alone program
tests/san/prepare_handle_driver.cpp. Every argument-validation path of the three calls answers its
code before anything is staged; valid MIN and CLASSIC calls bring the hand-worked bytes back
through the staging arena on guarded buffers, only the touched groups' span of the window is
staged, and of a 2^20-entry arena only the referenced commands. Nothing is loaded into Python: the
program is compiled with the sanitizers and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CSRC = os.path.join(ROOT, "minpaxos_amd", "csrc")


def test_prepare_handle_host_paths_asan_ubsan(tmp_path):
    exe = str(tmp_path / "prepare_handle_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(CSRC, "engine.cpp"),
           os.path.join(CSRC, "prepare_handle.cpp"), os.path.join(SAN, "hip_stub.cpp"),
           os.path.join(SAN, "prepare_handle_stub.cpp"),
           os.path.join(SAN, "prepare_handle_driver.cpp"), "-ldl", "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

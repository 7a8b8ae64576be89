"""The host side of the commit entry points under AddressSanitizer + UndefinedBehaviorSanitizer:
engine.cpp over the host-memory stand-in for the HIP runtime (tests/san/hip_stub.cpp), driven by
the stand-alone program tests/san/commit_driver.cpp. The stand-in has no commit launchers, so the
weak symbols stay null: the driver checks that every argument-validation path of
mpx_commit_handle, mpx_encode_commits and mpx_gather_commit_shorts answers first (MPX_E_INVAL) and
that valid calls answer MPX_E_UNSUPPORTED."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")


def test_commit_host_paths_asan_ubsan(tmp_path):
    exe = str(tmp_path / "commit_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "minpaxos_amd", "csrc", "engine.cpp"),
           os.path.join(SAN, "hip_stub.cpp"), os.path.join(SAN, "commit_driver.cpp"), "-ldl",
           "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

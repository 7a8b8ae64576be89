"""The host side of the proposer, unmarshal and commit entry points under AddressSanitizer +
UndefinedBehaviorSanitizer: engine.cpp over the host-memory stand-in for the HIP runtime
(tests/san/hip_stub.cpp), driven by the stand-alone programs tests/san/<family>_driver.cpp. Each
driver checks that every argument-validation path answers its code before anything is staged
(MPX_E_INVAL, MPX_E_NIL_INSTANCE, MPX_E_UNSUPPORTED for a size limit) and that valid calls answer
MPX_OK and stage their arrays whole and apart over the stand-ins for the family's launchers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")


@pytest.mark.parametrize("family", ["proposer", "unmarshal", "commit"])
def test_family_host_paths_asan_ubsan(tmp_path, family):
    exe = str(tmp_path / (family + "_driver"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "minpaxos_amd", "csrc", "engine.cpp"),
           os.path.join(SAN, "hip_stub.cpp"), os.path.join(SAN, family + "_driver.cpp"), "-ldl",
           "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

"""The host side of store assembly (mpx_store_commands, mpx_store_compact and their _reserve / _dev
forms) under AddressSanitizer + UndefinedBehaviorSanitizer: engine.cpp and store.cpp over the
host-memory stand-in for the HIP runtime (tests/san/hip_stub.cpp) and stand-ins for the store
launchers that really store and compact (tests/san/store_stub.cpp), driven by the stand-alone
program tests/san/store_driver.cpp. Every argument-validation path of both forms of both calls
answers its code before anything is staged; valid calls bring the appended commands, the winners'
slots, the cursor and the counts back through the staging arena on guarded buffers and leave the
rest of the arena and of the window alone. Nothing is loaded into Python: the program is compiled
with the sanitizers and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CSRC = os.path.join(ROOT, "minpaxos_amd", "csrc")


def test_store_host_paths_asan_ubsan(tmp_path):
    exe = str(tmp_path / "store_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(CSRC, "engine.cpp"),
           os.path.join(CSRC, "store.cpp"), os.path.join(SAN, "hip_stub.cpp"),
           os.path.join(SAN, "store_stub.cpp"), os.path.join(SAN, "store_driver.cpp"), "-ldl",
           "-o", exe]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout

"""Host-side check of the families' scratch sizes (tools/check/work_bytes_check.cpp): over every
size 0..70000, a geometric ladder with its neighbours up to 2^31 - 2 and 2^k +- 2, no
x_work_bytes decreases (a reservation for a maximum covers every smaller call),
apply_reserve_bytes covers every smaller call on every pipeline, and the regions each family
carves from a base lie inside [base, base + work_bytes), in order, 256-byte aligned. Host code
only: the program links libmpx.so and calls no HIP function."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_work_bytes_cover_their_carve_ups(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    libdir = os.path.join(ROOT, "minpaxos_amd")
    assert os.path.exists(os.path.join(libdir, "libmpx.so")), "libmpx.so is not built"
    exe = str(tmp_path / "work_bytes_check")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950",
                    "-I", os.path.join(libdir, "csrc"),
                    os.path.join(ROOT, "tools", "check", "work_bytes_check.cpp"),
                    "-L", libdir, "-lmpx", "-Wl,-rpath," + libdir, "-o", exe],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "region check on" in r.stdout and "work_bytes ok" in r.stdout, r.stdout

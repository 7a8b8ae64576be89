"""CPU-side checks of record assembly's boundary: libmpx.so exports mpx_record_log[_reserve|_dev] and
mpx_record_bound, the package binds them, the record layouts agree between the header, numpy and
ctypes, and the calls fail cleanly without a device."""
import ctypes as C
import os
import re
import subprocess

from minpaxos_amd import _lib
from minpaxos_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpx_record_log", "mpx_record_log_reserve", "mpx_record_log_dev", "mpx_record_bound")


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mpx_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in exported and hasattr(lib, name), name
    assert lib.mpx_abi_version() == 8


def test_the_bound_serves_both_formats():
    lib = _lib.load()
    for n, m in ((0, 0), (1, 0), (3, 7), (1 << 20, 1 << 22)):
        assert lib.mpx_record_bound(n, m) == 12 * n + 17 * m == R.record_bound(n, m)


def test_struct_sizes_and_constants_match_header(tmp_path):
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "mpx.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mpx_record_batch), sizeof(mpx_record_result),
        offsetof(mpx_record_batch, items), offsetof(mpx_record_batch, src),
        offsetof(mpx_record_batch, inst_base), offsetof(mpx_record_result, n_bytes));
      printf("%u %u %u %u %d %d %u %u %d %d\n", MPX_LR_ACCEPTS, MPX_LR_COMMITS, MPX_LR_SENDS,
        MPX_LR_DECIDED, MPX_LOG_DURABLE, MPX_LOG_DURABLE_CLASSIC, MPX_LR_GENERAL, MPX_LR_FULL,
        MPX_LR_ONE_LAUNCH_ITEMS, MPX_LR_ONE_LAUNCH_CMDS);
      return 0;
    }"""
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [
        C.sizeof(_lib.MpxRecordBatch), C.sizeof(_lib.MpxRecordResult), _lib.MpxRecordBatch.items.offset,
        _lib.MpxRecordBatch.src.offset, _lib.MpxRecordBatch.inst_base.offset,
        R.RECORD_RESULT.fields["n_bytes"][1]]
    assert C.sizeof(_lib.MpxRecordResult) == R.RECORD_RESULT.itemsize == 32
    assert [int(x) for x in lines[1].split()] == [
        R.LR_ACCEPTS, R.LR_COMMITS, R.LR_SENDS, R.LR_DECIDED, R.LOG_DURABLE, R.LOG_DURABLE_CLASSIC,
        R.LR_GENERAL, R.LR_FULL, R.LR_ONE_LAUNCH_ITEMS, R.LR_ONE_LAUNCH_CMDS]


def test_no_device_calls_fail_cleanly():
    lib = _lib.load()
    b, res = _lib.MpxRecordBatch(), _lib.MpxRecordResult()
    assert lib.mpx_record_log(None, C.byref(b), None, 0, None, C.byref(res)) == R.E_INVAL
    assert lib.mpx_record_log_reserve(None, 1) == R.E_INVAL
    assert lib.mpx_record_log_dev(None, C.byref(b), None, 0, None, None, None) == R.E_INVAL

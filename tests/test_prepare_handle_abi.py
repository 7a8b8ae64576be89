"""CPU-side checks of the prepare side's boundary: libmpx.so exports the three calls and their
_reserve / _dev forms, the package binds them, mpx_prepare_msg and mpx_prepare_reply_batch have one
layout in the header, in numpy and in ctypes, and the calls fail cleanly without a device."""
import ctypes as C
import os
import re
import subprocess

from minpaxos_amd import _lib
from minpaxos_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpx_gather_prepares", "mpx_gather_prepares_dev", "mpx_prepare_handle",
         "mpx_prepare_handle_dev", "mpx_encode_prepare_replies",
         "mpx_encode_prepare_replies_reserve", "mpx_encode_prepare_replies_dev")
FIELDS = [name for name, _ in _lib.MpxPrepareReplyBatch._fields_]
MSG = ["key", "ballot", "leader_id", "arg"]


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mpx_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in exported and hasattr(lib, name), name
    assert lib.mpx_abi_version() == 8


def test_struct_sizes_and_every_offset_match_header(tmp_path):
    assert FIELDS == ["replies", "reply_to", "log_from", "n", "n_dest", "inst_base", "n_inst", "st",
                      "lb", "inst", "src_op", "src_key", "src_val", "n_src", "reserved"]
    offs = ", ".join(f"offsetof(mpx_prepare_reply_batch, {f})" for f in FIELDS)
    moffs = ", ".join(f"offsetof(mpx_prepare_msg, {f})" for f in MSG)
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "mpx.h"
    int main(void) {
      size_t v[] = {sizeof(mpx_prepare_reply_batch), %s};
      size_t m[] = {sizeof(mpx_prepare_msg), %s};
      for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%zu ", v[i]);
      printf("\n");
      for (size_t i = 0; i < sizeof m / sizeof m[0]; ++i) printf("%%zu ", m[i]);
      printf("\n%%zu %%zu %%u %%u %%u %%u %%d\n", sizeof(mpx_prepare_reply),
             sizeof(mpx_prepare_reply_min), MPX_PRH_OK, MPX_PRH_RAISED, MPX_PRH_LOG, MPX_VALUE_KEEP,
             MPX_PEER_PREPARE);
      return 0;
    }""" % (offs, moffs)
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.MpxPrepareReplyBatch)] + [
        getattr(_lib.MpxPrepareReplyBatch, f).offset for f in FIELDS]
    assert [int(x) for x in lines[1].split()] == [R.PREPARE_MSG.itemsize] + [
        R.PREPARE_MSG.fields[f][1] for f in MSG]
    assert R.PREPARE_MSG.itemsize == 16 and list(R.PREPARE_MSG.names) == MSG
    assert [int(x) for x in lines[2].split()] == [
        R.PREPARE_REPLY.itemsize, R.PREPARE_REPLY_MIN.itemsize, R.PRH_OK, R.PRH_RAISED, R.PRH_LOG,
        R.VALUE_KEEP, R.PEER_PREPARE]


def test_no_device_calls_fail_cleanly():
    lib = _lib.load()
    b = _lib.MpxPrepareReplyBatch()
    off = (C.c_uint64 * 17)()
    assert lib.mpx_encode_prepare_replies(None, C.byref(b), None, 0, off) == R.E_INVAL
    assert lib.mpx_encode_prepare_replies_reserve(None, 1, 1, 1) == R.E_INVAL
    assert lib.mpx_encode_prepare_replies_dev(None, C.byref(b), None, 0, off, None) == R.E_INVAL
    assert lib.mpx_gather_prepares(None, None, 0, None, 0, 0, None, None, 0, off) == R.E_INVAL
    assert lib.mpx_gather_prepares_dev(None, None, 0, None, 0, None, 0, None, None, 0, off,
                                       None) == R.E_INVAL
    assert lib.mpx_prepare_handle(None, None, 0, None, 0, 0, None, 0, 0, None, None, None, None,
                                  None, None) == R.E_INVAL
    assert lib.mpx_prepare_handle_dev(None, None, 0, None, 0, 0, None, 0, 0, None, None, None, None,
                                      None, None, None) == R.E_INVAL

"""CPU-side checks of the stored Accept encoder's boundary: libmpx.so exports
mpx_encode_accepts_stored[_reserve|_dev], the package binds them, mpx_accept_store_batch has one
layout in the header and in ctypes, and the calls fail cleanly without a device."""
import ctypes as C
import os
import re
import subprocess

from minpaxos_amd import _lib
from minpaxos_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpx_encode_accepts_stored", "mpx_encode_accepts_stored_reserve",
         "mpx_encode_accepts_stored_dev")
FIELDS = [name for name, _ in _lib.MpxAcceptStoreBatch._fields_]


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (mpx_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in exported and hasattr(lib, name), name
    assert lib.mpx_abi_version() == 8


def test_struct_size_and_every_offset_match_header(tmp_path):
    assert FIELDS == ["sends", "n_sends", "inst_base", "ipg", "n_groups", "groups", "peer_commits",
                      "cmd_op", "cmd_key", "cmd_val", "n_cmds", "st", "lb", "inst", "src_op",
                      "src_key", "src_val", "n_src", "flags", "alive_mask", "reserved"]
    offs = ", ".join(f"offsetof(mpx_accept_store_batch, {f})" for f in FIELDS)
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "mpx.h"
    int main(void) {
      size_t v[] = {sizeof(mpx_accept_store_batch), %s};
      for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%zu ", v[i]);
      printf("\n%%zu %%zu %%zu %%u %%d\n", sizeof(mpx_acceptor_state), sizeof(mpx_inst_state),
             sizeof(mpx_inst_cmds), MPX_IC_HAS_CMDS, MPX_STATUS_NIL);
      return 0;
    }""" % offs
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.MpxAcceptStoreBatch)] + [
        getattr(_lib.MpxAcceptStoreBatch, f).offset for f in FIELDS]
    assert [int(x) for x in lines[1].split()] == [
        R.ACCEPTOR_STATE.itemsize, R.INST_STATE.itemsize, R.INST_CMDS.itemsize, R.IC_HAS_CMDS, -1]
    # the fields it shares with mpx_accept_batch sit where they sit there, up to the log
    for f in FIELDS[:FIELDS.index("st")]:
        assert getattr(_lib.MpxAcceptStoreBatch, f).offset == getattr(_lib.MpxAcceptBatch, f).offset


def test_no_device_calls_fail_cleanly():
    lib = _lib.load()
    b = _lib.MpxAcceptStoreBatch()
    off = (C.c_uint64 * 17)()
    assert lib.mpx_encode_accepts_stored(None, C.byref(b), None, 0, off) == R.E_INVAL
    assert lib.mpx_encode_accepts_stored_reserve(None, 1, 1) == R.E_INVAL
    assert lib.mpx_encode_accepts_stored_dev(None, C.byref(b), None, 0, off, None) == R.E_INVAL

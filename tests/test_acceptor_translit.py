"""CPU checks of the acceptor side: the hand-traced known answers against the transliteration
(tests/acceptor_translit.py), the new records against the header, the new entry points on a NULL
engine, and the fuzz generator's branch coverage (so the GPU fuzz is known to reach every branch
before it runs)."""
import collections
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import acceptor_translit as A
from go_translit import GoPanic
from minpaxos_amd import _lib
from minpaxos_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5


def same(got, want):
    return all(np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("case", A.KAT_MIN, ids=[c[0] for c in A.KAT_MIN])
def test_min_known_answers(case):
    msgs, st, groups, base = A.kat_inputs(case)
    got = A.accept_handle(R.MODE_MIN, N, msgs, st, groups, base)
    assert same(got, A.kat_expected(R.MODE_MIN, case)), got


@pytest.mark.parametrize("case", A.KAT_CLASSIC, ids=[c[0] for c in A.KAT_CLASSIC])
def test_classic_known_answers(case):
    msgs, st, groups, base = A.kat_inputs(case)
    got = A.accept_handle(R.MODE_CLASSIC, N, msgs, st, groups, base)
    assert same(got, A.kat_expected(R.MODE_CLASSIC, case)), got


def test_min_nil_stays_nil_and_unreplied_slots_are_zero():
    msgs, st, groups, base = A.kat_inputs(A.KAT_MIN[1])
    st_out, rep, to, eff = A.accept_handle(R.MODE_MIN, N, msgs, st, groups, base)
    assert st_out.tobytes() == st.tobytes()
    assert rep.tobytes() == bytes(16) and to[0] == -1 and eff[0] == 0


def test_translit_panics_where_go_panics():
    g = A.mk_groups([(16, 1)])
    st = A.mk_state([(A.NIL, 0, 0, 0)] * 4)
    for mode in (R.MODE_MIN, R.MODE_CLASSIC):
        with pytest.raises(GoPanic) as e:  # instanceSpace index out of range
            A.accept_handle(mode, N, A.mk_msgs([(4, 16, 0, 1)]), st, g)
        assert e.value.code == R.E_NIL_INSTANCE
        with pytest.raises(GoPanic) as e:  # PeerWriters[LeaderId]
            A.accept_handle(mode, N, A.mk_msgs([(1, 16, N, 1)]), st, g)
        assert e.value.code == R.E_BAD_ID
        with pytest.raises(GoPanic) as e:  # the batch contract
            A.accept_handle(mode, N, A.mk_msgs([(2, 16, 0, 1), (1, 16, 0, 1)]), st, g)
        assert e.value.code == R.E_INVAL
    # MIN: a message that does not reply never indexes PeerWriters
    out = A.accept_handle(R.MODE_MIN, N, A.mk_msgs([(1, 32, N, 1)]), st, g)
    assert out[2][0] == -1


def test_marshal_restatement_bytes():
    t = A.AcceptReply(0x01020304, 1, -2, 3)
    assert A.send_msg_bytes(R.MODE_MIN, t) == bytes(
        [13, 4, 3, 2, 1, 1, 0xFE, 0xFF, 0xFF, 0xFF, 3, 0, 0, 0])
    assert A.send_msg_bytes(R.MODE_CLASSIC, t) == bytes([13, 4, 3, 2, 1, 1, 0xFE, 0xFF, 0xFF, 0xFF])
    assert len(A.send_msg_bytes(R.MODE_MIN, t)) == R.ACCEPT_REPLY_FRAME[R.MODE_MIN]
    assert len(A.send_msg_bytes(R.MODE_CLASSIC, t)) == R.ACCEPT_REPLY_FRAME[R.MODE_CLASSIC]
    rep = np.zeros(3, R.ACCEPT_REPLY)
    rep["instance"], rep["ok"], rep["ballot"], rep["id"] = [5, 6, 7], 1, 16, [1, 2, 1]
    out, off = A.encode_accept_replies(R.MODE_MIN, rep, [1, -1, 1], 3)
    assert list(off) == [0, 0, 28, 28]
    assert out.tobytes() == b"".join(b"\x0d" + struct.pack("<iBii", i, 1, 16, 1) for i in (5, 7))


def test_new_struct_sizes_match_header():
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "mpx.h"
    int main(void) {
      printf("%zu %zu %zu\n", sizeof(mpx_accept_msg), sizeof(mpx_acceptor_state),
        sizeof(mpx_acceptor_group));
      printf("%zu %zu %zu %zu\n", offsetof(mpx_accept_msg, instance),
        offsetof(mpx_accept_msg, ballot), offsetof(mpx_accept_msg, leader_id),
        offsetof(mpx_accept_msg, value_id));
      printf("%zu %zu %zu %zu\n", offsetof(mpx_acceptor_state, status),
        offsetof(mpx_acceptor_state, ballot), offsetof(mpx_acceptor_state, value_id),
        offsetof(mpx_acceptor_state, flags));
      printf("%zu %zu\n", offsetof(mpx_acceptor_group, default_ballot),
        offsetof(mpx_acceptor_group, self_id));
      printf("%u %u %u %d %d\n", MPX_AH_REPLIED, MPX_AH_STORED, MPX_AH_REQUEUE,
        MPX_ACCEPT_REPLY_FRAME_MIN, MPX_ACCEPT_REPLY_FRAME_CLASSIC);
      return 0;
    }"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [[int(x) for x in ln.split()] for ln in lines[:5]]
    assert rows[0] == [R.ACCEPT_MSG.itemsize, R.ACCEPTOR_STATE.itemsize, R.ACCEPTOR_GROUP.itemsize]
    assert rows[0] == [16, 16, 8]
    assert rows[1] == [R.ACCEPT_MSG.fields[f][1]
                       for f in ("instance", "ballot", "leader_id", "value_id")]
    assert rows[2] == [R.ACCEPTOR_STATE.fields[f][1]
                       for f in ("status", "ballot", "value_id", "flags")]
    assert rows[3] == [R.ACCEPTOR_GROUP.fields[f][1] for f in ("default_ballot", "self_id")]
    assert rows[4] == [R.AH_REPLIED, R.AH_STORED, R.AH_REQUEUE, R.ACCEPT_REPLY_FRAME[R.MODE_MIN],
                       R.ACCEPT_REPLY_FRAME[R.MODE_CLASSIC]]


def test_new_entry_points_reject_a_null_engine():
    lib = _lib.load()
    assert lib.mpx_accept_handle(None, None, 0, None, 0, 0, None, 0, 0, None, None, None) == \
        R.E_INVAL
    assert lib.mpx_accept_handle_dev(None, None, 0, None, None, 0, 0, None, 0, 0, None, None,
                                     None, None) == R.E_INVAL
    assert lib.mpx_encode_accept_replies(None, None, None, 0, 5, None, None) == R.E_INVAL
    assert lib.mpx_encode_accept_replies_reserve(None, 16) == R.E_INVAL
    assert lib.mpx_encode_accept_replies_dev(None, None, None, 0, 5, None, None, None) == R.E_INVAL


def test_stub_build_exports_the_entry_points_without_the_kernels(stub_lib):
    """the CPU build of engine.cpp (the stub's stand-ins for the acceptor launchers linked, no
    weak symbol left) loads and exports them"""
    lib = C.CDLL(stub_lib)
    for name in ("mpx_accept_handle", "mpx_accept_handle_dev", "mpx_encode_accept_replies",
                 "mpx_encode_accept_replies_reserve", "mpx_encode_accept_replies_dev"):
        assert hasattr(lib, name), name
    lib.mpx_encode_accept_replies_reserve.argtypes = [C.c_void_p, C.c_size_t]
    assert lib.mpx_encode_accept_replies_reserve(None, 16) == R.E_INVAL


def test_stub_build_exports_the_newer_families_entry_points(stub_lib):
    """... and the proposer, unmarshal and commit entry points: their launchers have stand-ins in
    the stub too, so the library loads with every symbol bound"""
    lib = C.CDLL(stub_lib)
    for name in ("mpx_propose_handle", "mpx_propose_handle_dev", "mpx_encode_accepts",
                 "mpx_encode_accepts_reserve", "mpx_encode_accepts_dev",
                 "mpx_unmarshal_frames", "mpx_unmarshal_frames_reserve", "mpx_unmarshal_frames_dev",
                 "mpx_commit_handle", "mpx_commit_handle_dev", "mpx_encode_commits",
                 "mpx_encode_commits_reserve", "mpx_encode_commits_dev",
                 "mpx_gather_commit_shorts", "mpx_gather_commit_shorts_dev"):
        assert hasattr(lib, name), name
    lib.mpx_unmarshal_frames_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    assert lib.mpx_unmarshal_frames_reserve(None, 16, 16) == R.E_INVAL
    lib.mpx_encode_commits_reserve.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    assert lib.mpx_encode_commits_reserve(None, 16, 16) == R.E_INVAL


@pytest.mark.parametrize("mode", [R.MODE_MIN, R.MODE_CLASSIC], ids=["min", "classic"])
def test_fuzz_generator_reaches_every_branch(mode):
    """every branch of the handler (and CLASSIC's requeue) is taken by at least 2 % of the
    fuzz's records, and the long-run seeds carry a run longer than a tile"""
    cnt = collections.Counter()
    total = requeue = 0
    long_runs = 0
    for seed in A.FUZZ_SEEDS:
        msgs, st, groups, base, ipg = A.fuzz_case(seed, N)
        assert 1 <= len(msgs)
        assert np.all(np.diff(msgs["instance"]) >= 0)
        _, runs = np.unique(msgs["instance"], return_counts=True)
        if seed % 4 == 3:
            assert runs.max() > 1024
            long_runs += 1
        else:
            assert len(msgs) <= 5000 and runs.max() <= 5
        *_, eff, br = A.accept_handle(mode, N, msgs, st, groups, base, ipg, want_branches=True)
        cnt.update(br)
        total += len(msgs)
        requeue += int(np.count_nonzero(eff & R.AH_REQUEUE))
    assert long_runs == 6
    frac = {b: cnt[b] / total for b in A.BRANCHES[mode]}
    assert set(cnt) == set(A.BRANCHES[mode]), cnt
    assert min(frac.values()) >= 0.02, frac
    if mode == R.MODE_CLASSIC:
        assert requeue / total >= 0.02, requeue / total

"""CPU checks of the proposer side: hand-traced known answers (worked out from the Go text, written
here as literals) against the transliteration (tests/proposer_translit.py), its frames against
wire.accept, the new records against the header, the new entry points on a NULL engine, and the
fuzz generator's branch coverage (so the GPU fuzz is known to reach every branch before it runs)."""
import collections
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import proposer_translit as P
from go_translit import GoPanic
from minpaxos_amd import _lib, wire
from minpaxos_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
HAS = R.PF_HAS_PROPOSALS
NILROW = (P.NIL, 0, 0, 0)
USED = (P.COMMITTED, 17, 7, 0)


def run(mode, grp, n_props, st_rows, base=100, lb=False):
    st = P.mk_state(st_rows)
    lb0 = np.zeros(len(st), R.INST_STATE) if lb else None
    return P.propose_handle(mode, N, P.mk_groups([grp]), [0, n_props], st, base, len(st), lb0)


def rows(a):
    return [tuple(int(x) for x in r)[:6] for r in a.tolist()]


# (default_ballot, self_id, leader, prepare_oks, crt_instance, committed_upto)
def test_kat_min_not_leader():
    g, st, _, sends, off, false = run(MIN, (17, 1, 2, 5, 100, 99), 3, [NILROW] * 4)
    assert rows(sends) == [(-1, 0, 0, R.PH_NOT_LEADER, 0, 3)] and list(off) == [0, 1]
    assert list(false) == [0, 1, 2]          # :622-623, one by one
    assert g["crt_instance"][0] == 100 and st.tobytes() == P.mk_state([NILROW] * 4).tobytes()


def test_kat_min_prepare_oks_equal_half_is_not_enough():
    g, st, _, sends, _, false = run(MIN, (17, 1, 1, N >> 1, 100, 99), 2, [NILROW] * 4)
    assert rows(sends) == [(-1, 0, 0, R.PH_NOT_LEADER, 0, 2)] and list(false) == [0, 1]
    *_, sends, _, false = run(MIN, (17, 1, 1, (N >> 1) + 1, 100, 99), 2, [NILROW] * 4)
    assert rows(sends) == [(100, 17, 99, R.PH_ACCEPT, 0, 2)] and list(false) == []


def test_kat_min_crt_advances_over_three_non_nil_slots():
    g, st, lb, sends, _, false = run(MIN, (17, 1, 1, 3, 100, 102), 2, [USED] * 3 + [NILROW] * 2,
                                     lb=True)
    assert rows(sends) == [(103, 17, 102, R.PH_ACCEPT, 0, 2)] and list(false) == []
    assert g["crt_instance"][0] == 104
    assert st.tolist() == [USED] * 3 + [(P.PREPARED, 17, 0, HAS), NILROW]
    assert lb.tolist() == [(0, 0, 0, 0)] * 3 + [(P.PREPARED, 0, 0, 0), (0, 0, 0, 0)]


def test_kat_min_refused_keeps_the_advanced_crt():
    st0 = [USED] * 3 + [NILROW] * 2
    g, st, _, sends, _, false = run(MIN, (17, 1, 1, 3, 100, 100), 4, st0)
    assert rows(sends) == [(103, 17, 100, R.PH_REFUSED, 0, 4)]
    assert list(false) == [0]                # only `propose` is answered (:682-683)
    assert g["crt_instance"][0] == 103 and st.tolist() == st0


def test_kat_min_5001_proposals_accept_then_refused():
    g, st, _, sends, off, false = run(MIN, (17, 1, 1, 3, 100, 99), 5001, [NILROW] * 4)
    assert rows(sends) == [(100, 17, 99, R.PH_ACCEPT, 0, 5000),
                           (101, 17, 99, R.PH_REFUSED, 5000, 1)]
    assert list(off) == [0, 2] and list(false) == [5000] and g["crt_instance"][0] == 101
    assert st.tolist() == [(P.PREPARED, 17, 0, HAS)] + [NILROW] * 3


def test_kat_classic_10001_proposals_three_instances():
    g, st, _, sends, off, false = run(CLASSIC, (17, 1, 1, 0, 100, 99), 10001, [NILROW] * 4)
    assert rows(sends) == [(100, 17, 99, R.PH_ACCEPT, 0, 5000),
                           (101, 17, 99, R.PH_ACCEPT, 5000, 5000),
                           (102, 17, 99, R.PH_ACCEPT, 10000, 1)]
    assert list(off) == [0, 3] and list(false) == [] and g["crt_instance"][0] == 103
    assert st.tolist() == [(P.PREPARED, 17, 0, HAS), (P.PREPARED, 17, 5000, HAS),
                           (P.PREPARED, 17, 10000, HAS), NILROW]


def test_kat_classic_default_ballot_minus_one_prepares():
    g, st, lb, sends, _, _ = run(CLASSIC, (-1, 3, 3, 0, 100, 99), 2, [NILROW] * 2, lb=True)
    assert rows(sends) == [(100, 3, 99, R.PH_PREPARE, 0, 2)]   # makeUniqueBallot(0) = r.Id
    assert st.tolist() == [(P.PREPARING, 3, 0, HAS), NILROW]
    assert lb.tolist() == [(P.PREPARING, 0, 0, 0), (0, 0, 0, 0)]


def test_kat_classic_not_leader():
    g, st, _, sends, _, false = run(CLASSIC, (17, 1, 0, 0, 100, 99), 2, [NILROW] * 2)
    assert rows(sends) == [(-1, 0, 0, R.PH_NOT_LEADER, 0, 2)] and list(false) == [0, 1]


@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_kat_window_overflow_panics(mode):
    with pytest.raises(GoPanic) as e:
        run(mode, (17, 1, 1, 3, 100, 101), 1, [USED] * 2)
    assert e.value.code == R.E_NIL_INSTANCE
    with pytest.raises(GoPanic):             # crt already outside its window
        run(mode, (17, 1, 1, 3, 99, 101), 1, [NILROW] * 2)


# ---- bcastAccept -----------------------------------------------------------------------------------
def cmd_bytes(op, k, v):
    return bytes([op]) + struct.pack("<q", k) + struct.pack("<q", v)


LOG3 = (np.array([(5, 3, 0, 0), (6, 3, 0, 0), (0, P.NIL, 0, 0), (0, P.NIL, 0, 0)],
                 R.LOG_REC), np.array([0, 1, 1, 1, 1], np.uint64), np.array([1], np.uint8),
        np.array([2], np.int64), np.array([3], np.int64))
CMD1 = (np.array([1], np.uint8), np.array([10], np.int64), np.array([20], np.int64))


def test_kat_min_catch_up_from_first_and_from_peer_commits():
    grp = P.mk_groups([(32, 0, 0, 2, 103, 101)])
    sends = P.mk_sends([(102, 32, 101, R.PH_ACCEPT, 0, 1)])
    out, off = P.encode_accepts(MIN, 3, sends, grp, CMD1, 100, 4, [[0, 50, 100]], LOG3)
    head = bytes([9]) + struct.pack("<iiii", 0, 102, 32, 101) + b"\x02" + cmd_bytes(1, 10, 20)
    i100 = struct.pack("<ii", 5, 3) + b"\x02" + cmd_bytes(1, 2, 3)
    i101 = struct.pack("<ii", 6, 3) + b"\x00"
    to1 = head + b"\x04" + i100 + i101       # peerCommits[1] = 50 < first: from instance `first`
    to2 = head + b"\x02" + i101              # peerCommits[2] = 100: from 101
    assert out.tobytes() == to1 + to2
    assert list(off) == [0, 0, len(to1), len(to1) + len(to2)]
    assert len(to1) == R.accept_frame_bytes(MIN, 1, [1, 0])


def test_kat_min_empty_catch_up_range():
    grp = P.mk_groups([(32, 0, 0, 2, 103, 101)])
    sends = P.mk_sends([(102, 32, 101, R.PH_ACCEPT, 0, 1)])
    out, off = P.encode_accepts(MIN, 3, sends, grp, CMD1, 100, 4, [[0, 101, 102]], LOG3)
    f = bytes([9]) + struct.pack("<iiii", 0, 102, 32, 101) + b"\x02" + cmd_bytes(1, 10, 20) + b"\0"
    assert out.tobytes() == f + f and list(off) == [0, 0, len(f), 2 * len(f)]


def test_kat_min_nothing_committed_and_nil_in_range():
    grp = P.mk_groups([(32, 0, 0, 2, 101, 99)])
    sends = P.mk_sends([(100, 32, 99, R.PH_ACCEPT, 0, 0)])     # LastCommitted = first - 1
    out, _ = P.encode_accepts(MIN, 3, sends, grp, CMD1, 100, 4, [[0, -1, -1]], LOG3)
    f = bytes([9]) + struct.pack("<iiii", 0, 100, 32, 99) + b"\0\0"
    assert out.tobytes() == f + f
    sends = P.mk_sends([(103, 32, 102, R.PH_ACCEPT, 0, 0)])     # 102 is nil in LOG3
    with pytest.raises(GoPanic) as e:
        P.encode_accepts(MIN, 3, sends, grp, CMD1, 100, 4, [[0, 101, 102]], LOG3)
    assert e.value.code == R.E_NIL_INSTANCE


def dests(mode, n, self_id, thrifty, alive=0xFFFF):
    grp = P.mk_groups([(32, self_id, self_id, n, 1, -1)])
    sends = P.mk_sends([(0, 32, -1, R.PH_ACCEPT, 0, 0)])
    log = (np.array([(0, P.NIL, 0, 0)] * 2, R.LOG_REC), np.zeros(3, np.uint64),
           np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64))
    _, off = P.encode_accepts(mode, n, sends, grp, CMD1, 0, 2, np.full((1, n), -1), log,
                              thrifty=thrifty, alive_mask=alive)
    return [q for q in range(n) if off[q + 1] > off[q]]


def test_kat_thrifty_rings():
    assert dests(MIN, 3, 2, True) == [0]             # n = 3>>1 = 1: q = (2+1)%3
    assert dests(MIN, 3, 2, False) == [0, 1]
    assert dests(MIN, 5, 3, True) == [0, 4]          # n = 2: q = 4, 0
    assert dests(CLASSIC, 5, 3, True) == [0, 4]
    assert dests(MIN, 5, 3, False) == [0, 1, 2, 4]


def test_kat_dead_peers():
    alive = 0b11010                                  # 0 and 2 are dead
    assert dests(CLASSIC, 5, 1, False, alive) == [3, 4]   # :323-326 passes over 2 and 0
    assert dests(CLASSIC, 5, 1, True, alive) == [3, 4]    # n = 2 alive successors
    assert dests(CLASSIC, 5, 4, True, alive) == [1, 3]
    assert dests(MIN, 5, 1, True, alive) == [2, 3]        # MIN counts the dead peer (:476-482)
    assert dests(CLASSIC, 5, 1, False, 0) == []


def test_kat_one_replica_sends_nothing():
    for mode in (MIN, CLASSIC):
        grp = P.mk_groups([(16, 0, 0, 1, 1, -1)])
        out, off = P.encode_accepts(mode, 1, P.mk_sends([(0, 16, -1, R.PH_ACCEPT, 0, 1)]), grp,
                                    CMD1, 0, 2, [[-1]], LOG3[:1] + (np.zeros(3, np.uint64),) +
                                    LOG3[2:])
        assert len(out) == 0 and list(off) == [0, 0]


def test_kat_classic_frame_and_skipped_slots():
    grp = P.mk_groups([(33, 1, 1, 0, 7, 0)])
    sends = P.mk_sends([(5, 33, 0, R.PH_PREPARE, 0, 1), (6, 33, 0, R.PH_ACCEPT, 0, 1),
                        (-1, 0, 0, R.PH_NOT_LEADER, 0, 1)])
    out, off = P.encode_accepts(CLASSIC, 2, sends, grp, CMD1, 0, 8)
    f = bytes([9]) + struct.pack("<iii", 1, 6, 33) + b"\x02" + cmd_bytes(1, 10, 20)
    assert out.tobytes() == f and list(off) == [0, len(f), len(f)]
    assert len(f) == R.accept_frame_bytes(CLASSIC, 1) == 31


@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_translit_frames_equal_wire_accept(mode, seed):
    a = P.fuzz_encode(seed, N, mode)
    _, _, per = P.encode_accepts(mode, N, want_frames=True, **a)
    op, key, val = a["cmds"]
    lrec, lcoff, lop, lkey, lval = a["log"]
    G, ipg, base = len(a["groups"]), a["ipg"], a["inst_base"]
    total = 0
    for q in range(N):
        # rebuild with wire.accept from the frames' own headers: leader, instance, ballot
        for f in per[q]:
            leader, inst, ballot = struct.unpack_from("<iii", f, 1)
            s = a["sends"][[i for i, x in enumerate(a["sends"]) if x["flags"] & R.PH_ACCEPT and
                            x["instance"] == inst][0]]
            c0, nc = int(s["first_cmd"]), int(s["n_cmds"])
            cmds = [(int(op[j]), int(key[j]), int(val[j])) for j in range(c0, c0 + nc)]
            g = (inst - base) // ipg
            first, lc = base + g * ipg, int(s["last_committed"])
            pc = int(a["peer_commits"][g, q])
            lo = first if pc < first else pc + 1
            log = []
            for i in range(lo, lc + 1):
                k = i - base
                log.append((int(lrec[k]["ballot"]), int(lrec[k]["status"]),
                            [(int(lop[j]), int(lkey[j]), int(lval[j]))
                             for j in range(int(lcoff[k]), int(lcoff[k + 1]))]))
            w = wire.accept(mode, leader, inst, ballot, cmds, lc, log)
            assert f == w
            total += 1
    assert total > 0


def test_new_struct_sizes_match_header():
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "mpx.h"
    int main(void) {
      printf("%zu %zu\n", sizeof(mpx_proposer_group), sizeof(mpx_accept_send));
      printf("%zu %zu %zu %zu %zu %zu\n", offsetof(mpx_proposer_group, default_ballot),
        offsetof(mpx_proposer_group, self_id), offsetof(mpx_proposer_group, leader),
        offsetof(mpx_proposer_group, prepare_oks), offsetof(mpx_proposer_group, crt_instance),
        offsetof(mpx_proposer_group, committed_upto));
      printf("%zu %zu %zu %zu %zu %zu\n", offsetof(mpx_accept_send, instance),
        offsetof(mpx_accept_send, ballot), offsetof(mpx_accept_send, last_committed),
        offsetof(mpx_accept_send, flags), offsetof(mpx_accept_send, first_cmd),
        offsetof(mpx_accept_send, n_cmds));
      printf("%u %u %u %u %u %d %d\n", MPX_PH_ACCEPT, MPX_PH_NOT_LEADER, MPX_PH_REFUSED,
        MPX_PH_PREPARE, MPX_AB_THRIFTY, MPX_PROPOSE_MAX_BATCH, MPX_ABI_VERSION);
      printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mpx_accept_batch),
        offsetof(mpx_accept_batch, n_sends), offsetof(mpx_accept_batch, ipg),
        offsetof(mpx_accept_batch, groups), offsetof(mpx_accept_batch, n_log_cmds),
        offsetof(mpx_accept_batch, alive_mask));
      return 0;
    }"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = [[int(x) for x in ln.split()] for ln in lines[:5]]
    assert got[0] == [R.PROPOSER_GROUP.itemsize, R.ACCEPT_SEND.itemsize] == [32, 32]
    assert got[1] == [R.PROPOSER_GROUP.fields[f][1] for f in (
        "default_ballot", "self_id", "leader", "prepare_oks", "crt_instance", "committed_upto")]
    assert got[2] == [R.ACCEPT_SEND.fields[f][1] for f in (
        "instance", "ballot", "last_committed", "flags", "first_cmd", "n_cmds")]
    assert got[3] == [R.PH_ACCEPT, R.PH_NOT_LEADER, R.PH_REFUSED, R.PH_PREPARE, R.AB_THRIFTY,
                      R.PROPOSE_MAX_BATCH, 8]
    B = _lib.MpxAcceptBatch
    assert got[4] == [__import__("ctypes").sizeof(B), B.n_sends.offset, B.ipg.offset,
                      B.groups.offset, B.n_log_cmds.offset, B.alive_mask.offset]


def test_frame_size_helpers():
    assert [R.varint_len(x) for x in (0, 63, 64, 8191, 8192, 1 << 20)] == [1, 1, 2, 2, 3, 4]
    assert R.accept_frame_bytes(MIN, 0) == 19 and R.accept_frame_bytes(CLASSIC, 0) == 14
    assert R.accept_frame_bytes(MIN, 5000, [0, 64]) == 17 + 2 + 85000 + 1 + 9 + 10 + 64 * 17
    assert R.log_instance_bytes(3) == len(P.instance_marshal(1, 2, [(0, 0, 0)] * 3))


def test_new_entry_points_reject_a_null_engine():
    lib = _lib.load()
    assert lib.mpx_propose_handle(None, None, 0, None, None, None, 0, 0, 0, None, None, 0) == \
        R.E_INVAL
    assert lib.mpx_propose_handle_dev(None, None, 0, None, None, None, None, 0, 0, 0, None,
                                      None) == R.E_INVAL
    assert lib.mpx_encode_accepts(None, None, None, 0, None) == R.E_INVAL
    assert lib.mpx_encode_accepts_reserve(None, 16, 16, 16) == R.E_INVAL
    assert lib.mpx_encode_accepts_dev(None, None, None, 0, None, None) == R.E_INVAL


@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_fuzz_generator_reaches_every_branch(mode):
    """every branch of the handler is taken in at least 2 % of the fuzz's groups, and (MIN) both
    catch-up cases and the empty range in at least 2 % of its frames"""
    cnt, kinds = collections.Counter(), collections.Counter()
    groups_total = frames = 0
    for seed in P.FUZZ_SEEDS:
        groups, prop_off, st, base, ipg = P.fuzz_propose(seed, N, mode)
        *_, br = P.propose_handle(mode, N, groups, prop_off, st, base, ipg, want_branches=True)
        groups_total += len(groups)
        for b in br:
            cnt.update(set(b))
        if mode == MIN:
            note = []
            P.encode_accepts(mode, N, note=note, **P.fuzz_encode(seed, N, mode))
            frames += len(note)
            kinds.update(k for k, _ in note)
            kinds["empty"] += sum(1 for _, n in note if n == 0)
    frac = {b: cnt[b] / groups_total for b in P.BRANCHES[mode]}
    print("handler branch fractions of groups:", mode, frac)
    assert min(frac.values()) >= 0.02, frac
    if mode == MIN:
        kf = {k: kinds[k] / frames for k in P.CATCHUP_KINDS}
        print("catch-up fractions of frames:", kf, "frames", frames)
        assert min(kf.values()) >= 0.02, kf


def test_boundary_sweep_inputs_sit_on_the_window_boundary():
    """the GPU sweep (test_gpu_proposer.py) is only as good as its inputs: walked through the
    transliteration's frames, case d has the header of the record under test at byte 8192 + d, and
    over the sweep d = -30 .. 2 a record header starts on every byte of 8192 - 30 .. 8192 + 2 (the
    sweep's own range: the neighbouring headers are 60 bytes and more away) and a log command on
    every byte of 8192 - 47 .. 8192 + 11"""
    heads, cmds = set(), set()
    for d in P.SWEEP:
        a, k = P.boundary_case(d)
        _, _, per = P.encode_accepts(MIN, 2, want_frames=True, **a)
        assert not per[0] and len(per[1]) == 1
        recs, starts = P.log_starts(per[1][0], 17)
        assert recs[k] == P.WINDOW + d and len(per[1][0]) > P.WINDOW
        heads.update(recs)
        cmds.update(starts)
    assert heads >= set(range(P.WINDOW - 30, P.WINDOW + 3))
    assert cmds >= set(range(P.WINDOW - 47, P.WINDOW + 12))

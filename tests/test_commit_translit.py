"""Known answers for tests/commit_translit.py, hand-traced from the Go text (the line numbers are
bareminpaxos.go's; paxos.go:522-575 and :336-386 are the same code), the property the engine's
design rests on (updateCommittedUpTo after every message == once after the batch) and the reach of
the fuzz generators. CPU only."""
import struct

import numpy as np
import pytest

import commit_translit as T
from go_translit import GoPanic
from minpaxos_amd import records as R
from proposer_translit import mk_state

NIL, KEEP, C = T.NIL, T.KEEP, T.COMMITTED
HAS, REQ = R.PF_HAS_PROPOSALS, R.PF_REQUEUED
NILROW = (NIL, 0, 0, 0)


def run(rows, msgs, cu, base=100, ipg=None):
    st, cu2, eff, log = T.commit_handle(T.mk_msgs(msgs), mk_state(rows), cu, base, ipg)
    return [tuple(int(x) for x in r) for r in st.tolist()], cu2.tolist(), eff.tolist(), \
        [tuple(int(x) for x in r) for r in log.tolist()]


# ---- the handlers --------------------------------------------------------------------------------
def test_nil_commit():
    """:861-866: a fresh Instance{Ballot, COMMITTED, nil, Command}; :879 the prefix takes it"""
    st, cu, eff, log = run([NILROW, NILROW], [(100, 17, 2, 55)], [99])
    assert st == [(C, 17, 55, 0), NILROW] and cu == [100]
    assert eff == [R.CH_INSTALLED | R.CH_CMDS] and log == [(17, C, 100, 0)]


def test_nil_commit_short():
    """:890-895: Instance{Ballot, COMMITTED, nil, nil}: Cmds stay nil (VALUE_KEEP)"""
    st, cu, eff, log = run([NILROW], [(100, 9, 0, KEEP)], [99])
    assert st == [(C, 9, KEEP, 0)] and cu == [100]
    assert eff == [R.CH_INSTALLED] and log == [(9, C, 100, 0)]


def test_commit_then_short_keeps_commands_last_ballot_wins():
    st, cu, eff, log = run([NILROW], [(100, 17, 0, 55), (100, 33, 0, KEEP)], [99])
    assert st == [(C, 33, 55, 0)] and eff == [R.CH_INSTALLED | R.CH_CMDS, 0]
    assert log == [(17, C, 100, 0), (33, C, 100, 0)]


def test_short_then_commit_takes_commands():
    st, _, eff, _ = run([(T.ACCEPTED, 17, 44, 0)], [(100, 17, 0, KEEP), (100, 17, 0, 55)], [99])
    assert st == [(C, 17, 55, 0)] and eff == [0, R.CH_CMDS]


def test_lower_ballot_overwrites():
    """no ballot is compared anywhere (:868-870 / :897-898)"""
    st, _, eff, _ = run([(T.ACCEPTED, 49, 44, 0), (C, 49, 45, 0)],
                        [(100, 17, 0, 55), (101, 3, 0, KEEP)], [99])
    assert st == [(C, 17, 55, 0), (C, 3, 45, 0)] and eff == [R.CH_CMDS, 0]


def test_requeue_once():
    """:871-876: the proposals go back and ClientProposals = nil, so the second message on the
    instance finds none"""
    st, _, eff, _ = run([(T.PREPARED, 17, 44, HAS)], [(100, 18, 0, 55), (100, 18, 0, KEEP)], [99])
    assert st == [(C, 18, 55, REQ)] and eff == [R.CH_CMDS | R.CH_REQUEUE, 0]
    st, _, eff, _ = run([(T.PREPARED, 17, 44, HAS)], [(100, 18, 0, KEEP), (100, 19, 0, 55)], [99])
    assert st == [(C, 19, 55, REQ)] and eff == [R.CH_REQUEUE, R.CH_CMDS]


def test_nil_gap_stops_the_prefix():
    st, cu, _, _ = run([NILROW] * 4, [(100, 1, 0, 5), (101, 1, 0, KEEP), (103, 1, 0, 6)], [99])
    assert cu == [101] and st[2] == NILROW and st[3] == (C, 1, 6, 0)


def test_uncommitted_instance_stops_the_prefix():
    _, cu, _, _ = run([NILROW, (T.ACCEPTED, 1, 2, 0), NILROW], [(100, 1, 0, 5), (102, 1, 0, 5)], [99])
    assert cu == [100]


def test_out_of_order_commit_jumps_by_two():
    """instance 5 before 4 in time is 4 before 5 in the sorted batch; per message the prefix stays
    at 3 after (the earlier) 5 and jumps to 5 after 4. Here both orders, through the handlers."""
    r = T.Replica(0, 8, mk_state([(C, 1, 1, 0)] * 4 + [NILROW] * 4), 3)
    out = {"branch": [], "log": [], "effect": []}
    T.handle_commit(r, 5, 7, 50, out)
    assert r.committedUpTo == 3
    T.handle_commit_short(r, 4, 7, out)
    assert r.committedUpTo == 5
    _, cu, _, _ = run([(C, 1, 1, 0)] * 4 + [NILROW] * 4, [(4, 7, 0, KEEP), (5, 7, 0, 50)], [3], base=0)
    assert cu == [5]


def test_untouched_group_does_not_advance():
    """group 1's states allow an advance, but the reference only advances inside a handler"""
    rows = [NILROW, NILROW, (C, 1, 1, 0), (C, 1, 1, 0)]
    _, cu, _, _ = run(rows, [(100, 1, 0, 5)], [99, 101], ipg=2)
    assert cu == [100, 101]
    _, cu, _, _ = run(rows, [(100, 1, 0, 5), (103, 2, 0, KEEP)], [99, 101], ipg=2)
    assert cu == [100, 103]


def test_prefix_stops_at_the_windows_end():
    """the stated deviation: group 0's prefix does not run on into group 1's slots"""
    rows = [(C, 1, 1, 0), NILROW, (C, 1, 1, 0), (C, 1, 1, 0)]
    _, cu, _, _ = run(rows, [(101, 1, 0, 5)], [99, 101], ipg=2)
    assert cu == [101, 101]
    _, cu, _, _ = run([(C, 1, 1, 0)], [(100, 2, 0, KEEP)], [100])  # already at the end
    assert cu == [100]


def test_prefix_takes_instances_committed_earlier():
    """a touched group advances over what earlier batches left COMMITTED beyond its watermark"""
    _, cu, _, _ = run([NILROW] + [(C, 1, 1, 0)] * 3 + [NILROW], [(100, 1, 0, 5)], [99])
    assert cu == [103]


def test_errors():
    with pytest.raises(GoPanic) as e:
        run([NILROW], [(101, 1, 0, 5)], [99])
    assert e.value.code == R.E_NIL_INSTANCE
    with pytest.raises(GoPanic) as e:
        run([NILROW], [(99, 1, 0, 5)], [99])
    assert e.value.code == R.E_NIL_INSTANCE
    with pytest.raises(GoPanic) as e:
        run([NILROW] * 2, [(101, 1, 0, 5), (100, 1, 0, 5)], [99])
    assert e.value.code == R.E_INVAL
    for bad in (98, 102):
        with pytest.raises(GoPanic) as e:
            run([NILROW] * 2, [(100, 1, 0, 5)], [bad])
        assert e.value.code == R.E_INVAL


# ---- bcastCommit ---------------------------------------------------------------------------------
def dests(N, Id, thrifty, alive):
    out = T.bcast_commit(N, Id, thrifty, [(alive >> q) & 1 == 1 for q in range(N)], 7, 3, [])
    return [(q, b[0]) for q, b in out]


S, F = T.COMMIT_SHORT_RPC, T.COMMIT_RPC


def test_bcast_n3():
    assert dests(3, 0, False, 0b111) == [(1, S), (2, S)]
    assert dests(3, 2, False, 0b111) == [(0, S), (1, S)]
    assert dests(3, 0, True, 0b111) == [(1, S), (2, F)]         # n = 1, then the second loop
    assert dests(3, 1, True, 0b111) == [(2, S), (0, F)]
    assert dests(3, 0, False, 0b101) == [(2, S)]                # 1 is dead: the ring wraps
    assert dests(3, 0, True, 0b101) == [(2, S)]                 # loop 1 ends on 2, loop 2 wraps at once
    assert dests(3, 0, True, 0b011) == [(1, S)]                 # dead peer in the second loop
    assert dests(3, 0, True, 0b001) == []                       # none alive: q == Id, no second loop


def test_bcast_n5():
    assert dests(5, 0, False, 0b11111) == [(1, S), (2, S), (3, S), (4, S)]
    assert dests(5, 3, True, 0b11111) == [(4, S), (0, S), (1, F), (2, F)]
    assert dests(5, 0, True, 0b11101) == [(2, S), (3, S), (4, F)]   # dead peer in the first loop
    assert dests(5, 0, True, 0b10111) == [(1, S), (2, S), (4, F)]   # ... in the second
    assert dests(5, 0, True, 0b00011) == [(1, S)]                    # wraps before n is reached
    assert dests(5, 0, False, 0b01011) == [(1, S), (3, S)]
    assert dests(5, 4, True, 0b11111) == [(0, S), (1, S), (2, F), (3, F)]


def test_bcast_n1_and_n2():
    assert dests(1, 0, False, 1) == [] and dests(1, 0, True, 1) == []
    assert dests(2, 0, False, 3) == [(1, S)] and dests(2, 1, True, 3) == [(0, S)]


# ---- the bytes ------------------------------------------------------------------------------------
def test_commit_short_bytes():
    b = T.send_msg(S, T.commit_short_marshal(2, 0x01020304, 5000, -1))
    assert b == bytes([11, 2, 0, 0, 0, 4, 3, 2, 1, 0x88, 0x13, 0, 0, 255, 255, 255, 255])
    assert len(b) == R.COMMIT_SHORT_FRAME
    assert T.commit_short_unmarshal(b[1:]) == (2, 0x01020304, 5000, -1)


def test_commit_bytes_0_and_64_commands():
    b = T.send_msg(F, T.commit_marshal(1, 7, 33, []))
    assert b == bytes([10, 1, 0, 0, 0, 7, 0, 0, 0, 33, 0, 0, 0, 0]) and len(b) == R.commit_frame_bytes(0)
    cmds = [(1, k, -k) for k in range(64)]
    b = T.send_msg(F, T.commit_marshal(1, 7, 33, cmds))
    assert b[13:15] == bytes([0x80, 0x01])  # PutVarint(64): zig-zag 128, two bytes
    assert len(b) == R.commit_frame_bytes(64) == 13 + 2 + 64 * 17
    assert b[15:32] == struct.pack("<Bqq", 1, 0, 0) and b[-17:] == struct.pack("<Bqq", 1, 63, -63)
    b = T.send_msg(F, T.commit_marshal(1, 7, 33, cmds[:63]))
    assert b[13] == 126 and len(b) == 14 + 63 * 17


def test_encode_commits_layout():
    """destination by destination, each in send-array order; skipped slots leave nothing"""
    sends = T.mk_commit_sends([(10, 5, 0, 1, R.CS_SEND), (11, 5, 1, 0, 0), (12, 6, 1, 2, R.CS_SEND)])
    cmds = (np.array([1, 2, 3], np.uint8), np.array([4, 5, 6], np.int64), np.array([7, 8, 9], np.int64))
    by, off, per = T.encode_commits(3, sends, T.mk_self([0, 2]), cmds, 10, 2, thrifty=True,
                                    want_frames=True)
    # instances 10, 11 are led by 0 (-> 1 short, 2 full), 12 by 2 (-> 0 short, 1 full)
    assert [[f[0] for f in q] for q in per] == [[S], [S, F], [F]]
    assert off.tolist() == [0, 17, 17 + 17 + 14 + 34, 17 + 17 + 14 + 34 + 14 + 17]
    assert by.tobytes() == b"".join(b"".join(q) for q in per)
    for bad, field in ((9, "instance"), (14, "instance")):
        s2 = sends.copy()
        s2[field][0] = bad
        with pytest.raises(GoPanic):
            T.encode_commits(3, s2, T.mk_self([0, 2]), cmds, 10, 2)


def test_gather_translit():
    buf, ns = T.mixed_stream(0, R.MODE_MIN, 50)
    other = np.zeros(2, R.PEER_FRAME)
    body = T.commit_short_marshal(3, 41, 2, 17)
    buf = b"\x06" + b"\0" * 8 + T.send_msg(S, body)
    other[0] = (0, 6, (0, 0, 0))
    other[1] = (9, 11, (0, 0, 0))
    m, c, i = T.gather_commit_shorts(buf, other)
    assert m.tolist() == [(41, 17, 3, KEEP)] and c.tolist() == [2] and i.tolist() == [1]
    assert ns > 0


# ---- the property the engine's design rests on -----------------------------------------------------
@pytest.mark.parametrize("seed", T.FUZZ_SEEDS)
def test_per_message_and_end_of_batch_prefix_agree(seed):
    a = T.fuzz_commit(seed)
    one = T.commit_handle(**a, per_message=True)
    two = T.commit_handle(**a, per_message=False)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()


def test_fuzz_reach():
    """every branch of the table, and each of bcastCommit's loops, takes at least 0.02 of the fuzz
    messages (the bar of the acceptor's reach test)"""
    n, count = 0, {b: 0 for b in T.BRANCHES}
    advanced = untouched_kept = 0
    for seed in T.FUZZ_SEEDS:
        a = T.fuzz_commit(seed)
        st, cu, eff, log, br = T.commit_handle(**a, want_branches=True)
        n += len(a["msgs"])
        for b in br:
            count[b] += 1
        advanced += int((cu > a["committed_upto"]).sum())
        untouched_kept += int((cu == a["committed_upto"]).sum())
    assert n > 500  # (so that a share of 0.02 is at least ten messages)
    for b, c in count.items():
        assert c / n >= 0.02, (b, c, n)
    assert advanced >= 10 and untouched_kept >= 10
    loops, frames = [0, 0], 0
    for seed in T.FUZZ_SEEDS:
        for N in (3, 5):
            by, off, per = T.encode_commits(N, **T.fuzz_bcast(seed, N), want_frames=True, loops=loops)
            frames += sum(len(q) for q in per)
    assert frames == sum(loops) and frames > 300
    assert loops[0] / frames >= 0.02 and loops[1] / frames >= 0.02, loops

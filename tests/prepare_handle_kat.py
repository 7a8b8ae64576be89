"""Hand-worked PrepareReply frames, one per frame shape, with the store and the Prepare that
produce them. The bytes were written out by hand from the Marshals' field order
(minpaxosprotomarsh.go:308-350, paxosprotomarsh.go:126-150; little endian, V = binary.PutVarint,
so V(0) = 00, V(1) = 02, V(2) = 04; a Command is Op u8, K i64, V i64), not produced by any code.

Every case is (mode, kwargs of prepare_handle_translit.run_batch, expected): expected holds the
frame bytes, the reply record, effect, log_from and the group scalars after the call.
"""
import numpy as np

from minpaxos_amd import records as R

NIL = R.STATUS_NIL


def _hex(s):
    return bytes.fromhex(s.replace("|", " "))


def _cmd(op, k, v):
    """for readability only: the 17 bytes of one Command as the hex the cases spell out"""
    return f"{op:02x} " + k.to_bytes(8, "little").hex() + " " + v.to_bytes(8, "little").hex()


def _window(n, base_ballot=-1):
    st = np.zeros(n, R.ACCEPTOR_STATE)
    st["status"], st["ballot"], st["value_id"] = NIL, base_ballot, R.VALUE_KEEP
    return st, np.zeros(n, R.INST_CMDS)


def min_no_log():
    """Follower 1 of N = 3, window [0, 8), slots 0..4 full, crtInstance 5, committedUpTo 4. The
    Prepare {leader 2, ballot 0x21, LastCommitted 4}: 0x10 < 0x21 raises; 4 <= 4: no log."""
    st, inst = _window(8)
    st["status"][:5], st["ballot"][:5] = R.COMMITTED, 0x10
    groups = np.array([(0x10, 1, 0, 2, 5, 4, (0, 0))], R.PROPOSER_GROUP)
    msgs = np.array([(0, 0x21, 2, 4)], R.PREPARE_MSG)
    frame = _hex("0c | 01 00 00 00 | 04 00 00 00 | 01 | 21 00 00 00 | 04 00 00 00 | 00 | 00")
    return R.MODE_MIN, dict(N=3, msgs=msgs, groups=groups, st=st, inst_base=0, ipg=8, inst=inst,
                            arena=(np.zeros(0, np.uint8), np.zeros(0, np.int64),
                                   np.zeros(0, np.int64))), \
        dict(frame=frame, reply=(1, 4, 0x21, 4, 1, R.VALUE_KEEP), reply_to=2,
             effect=R.PRH_OK | R.PRH_RAISED, log_from=5,
             group=(0x21, 1, 2, 0, 5, 4))


def min_command_and_log():
    """Follower 2 of N = 3, window [10, 18): 10 {COMMITTED, 0x11, [(PUT 5 6)]}, 11 {COMMITTED,
    0x12, Cmds nil: made by a CommitShort}, 12 {ACCEPTED, 0x13, [(PUT 7 8), (GET 9 0)]}, the rest
    nil; crtInstance 12, committedUpTo 11. The Prepare {leader 0, ballot 0x20, LastCommitted 9}
    raises, crtInstance moves to 13, Command = slot 12's, CatchUpLog = instances 10 and 11. The
    arena holds slot 12's commands first, one dead command, then slot 10's."""
    st, inst = _window(8)
    st["status"][:3] = (R.COMMITTED, R.COMMITTED, R.ACCEPTED)
    st["ballot"][:3] = (0x11, 0x12, 0x13)
    inst[0] = (3, 1, R.IC_HAS_CMDS)
    inst[2] = (0, 2, R.IC_HAS_CMDS)
    arena = (np.array([1, 2, 4, 1], np.uint8), np.array([7, 9, -1, 5], np.int64),
             np.array([8, 0, -1, 6], np.int64))
    groups = np.array([(0x13, 2, 1, 2, 12, 11, (0, 0))], R.PROPOSER_GROUP)
    msgs = np.array([(0, 0x20, 0, 9)], R.PREPARE_MSG)
    frame = _hex("0c | 02 00 00 00 | 0c 00 00 00 | 01 | 20 00 00 00 | 0b 00 00 00 | 04 |"
                 + _cmd(1, 7, 8) + _cmd(2, 9, 0) + "| 04 |"
                 "11 00 00 00 | 03 00 00 00 | 02 |" + _cmd(1, 5, 6) +
                 "| 12 00 00 00 | 03 00 00 00 | 00")
    return R.MODE_MIN, dict(N=3, msgs=msgs, groups=groups, st=st, inst_base=10, ipg=8, inst=inst,
                            arena=arena), \
        dict(frame=frame, reply=(2, 12, 0x20, 11, 1, 2), reply_to=0,
             effect=R.PRH_OK | R.PRH_RAISED | R.PRH_LOG, log_from=10,
             group=(0x20, 2, 0, 0, 13, 11))


def classic_nil():
    """Instance 7 is nil, defaultBallot 5; the Prepare {leader 1, Instance 7, ballot 5,
    ToInfinity 1}: !(5 > 5) is TRUE, Command is the empty slice; 5 > 5 is false: nothing raised."""
    st, inst = _window(8)
    groups = np.array([(5, 0, 0, 0, 0, -1, (0, 0))], R.PROPOSER_GROUP)
    msgs = np.array([(7, 5, 1, 1)], R.PREPARE_MSG)
    frame = _hex("0c | 07 00 00 00 | 01 | 05 00 00 00 | 00")
    return R.MODE_CLASSIC, dict(N=3, msgs=msgs, groups=groups, st=st, inst_base=0, ipg=8,
                                inst=inst, arena=(np.zeros(0, np.uint8), np.zeros(0, np.int64),
                                                  np.zeros(0, np.int64))), \
        dict(frame=frame, reply=(7, 5, 1, R.VALUE_KEEP), reply_to=1, effect=R.PRH_OK,
             log_from=None, group=(5, 0, 0, 0, 0, -1))


def classic_inst():
    """Instance 8 (window [4, 12), index 4) is {ACCEPTED, ballot 9, [(PUT 2 3)]}; the Prepare
    {leader 2, Instance 8, ballot 8, ToInfinity 1}: 8 < 9 refuses, the reply carries ballot 9 and
    the commands; 8 > defaultBallot 3 raises it to 8."""
    st, inst = _window(8)
    st["status"][4], st["ballot"][4] = R.ACCEPTED, 9
    inst[4] = (1, 1, R.IC_HAS_CMDS)
    arena = (np.array([0, 1], np.uint8), np.array([0, 2], np.int64), np.array([0, 3], np.int64))
    groups = np.array([(3, 0, 0, 0, 4, 3, (0, 0))], R.PROPOSER_GROUP)
    msgs = np.array([(8, 8, 2, 1)], R.PREPARE_MSG)
    frame = _hex("0c | 08 00 00 00 | 00 | 09 00 00 00 | 02 |" + _cmd(1, 2, 3))
    return R.MODE_CLASSIC, dict(N=3, msgs=msgs, groups=groups, st=st, inst_base=4, ipg=8,
                                inst=inst, arena=arena), \
        dict(frame=frame, reply=(8, 9, 0, 4), reply_to=2, effect=R.PRH_RAISED, log_from=None,
             group=(8, 0, 0, 0, 4, 3))


CASES = {"min_no_log": min_no_log, "min_command_and_log": min_command_and_log,
         "classic_nil": classic_nil, "classic_inst": classic_inst}

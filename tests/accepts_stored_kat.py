"""Known answers of mpx_encode_accepts_stored, worked by hand from the Go's Marshals
(minpaxosprotomarsh.go:425-468 Accept, :100-124 Instance; statemarsh.go:8-19 Command; the code
byte 9 of genericsmr.go:499-512). Shared by the CPU and the GPU tests.

N = 3, one group, ipg = 8, inst_base = 100. The leader sends instance 103 at ballot 33 with two new
commands and last_committed = 102. peer_commits = [98, 101, 102]: a peer below first_g gets the log
from first_g (three records), a peer at 101 one record, a peer at 102 an empty log; which two of
them are destinations follows from self_id (the ring walk starts at self_id + 1).

The three log instances hold 0, 1 and 3 commands; their arena ranges lie in reverse window order
with dead commands (op 0xEE) between them:

    arena   0     1     2 3 4        5     6        7
            dead  dead  instance 2   dead  inst. 1  dead
"""
import numpy as np

import proposer_translit as P
from minpaxos_amd import records as R

N, IPG, BASE = 3, 8, 100
NILROW = (P.NIL, 0, 0, 0)
DEAD = (0xEE, -1, -1)
ARENA_ROWS = [DEAD, DEAD, (1, 0x20, 0x21), (1, 0x22, 0x23), (3, 0x24, 0), DEAD, (2, 0x10, 0), DEAD]
NEW_ROWS = [(1, 5, 6), (2, 7, 0)]

# Command.Marshal: Op u8, K i64, V i64, little endian
NEW = ("01 0500000000000000 0600000000000000"
       "02 0700000000000000 0000000000000000")
A2_4 = ("01 2000000000000000 2100000000000000"
        "01 2200000000000000 2300000000000000"
        "03 2400000000000000 0000000000000000")
A6 = "02 1000000000000000 0000000000000000"


def head(leader):
    """[9][LeaderId][Instance 103][Ballot 33][LastCommitted 102][V(2) = 04][2 commands]"""
    return f"09 {leader:02x}000000 67000000 21000000 66000000 04" + NEW


# Instance.Marshal: Ballot, Status, V(len(Cmds)), Cmds. Ballots 16, 17, 18 from st.
REC0 = "10000000 03000000 00"                  # COMMITTED, V(0)
REC1 = "11000000 02000000 02" + A6             # ACCEPTED, V(1)
REC2 = "12000000 01000000 06" + A2_4           # PREPARED, V(3)
REC2_COMMITTED = "12000000 03000000 06" + A2_4   # ... once lb says COMMITTED
REC0_ONE = "10000000 03000000 02" + A6         # instance 0 sharing instance 1's range


def rows(dtype, rs):
    a = np.zeros(len(rs), dtype)
    for i, r in enumerate(rs):
        a[i] = r
    return a


def cols(rs):
    return (np.array([r[0] for r in rs], np.uint8), np.array([r[1] for r in rs], np.int64),
            np.array([r[2] for r in rs], np.int64))


def case(self_id, lb, inst_rows):
    st = rows(R.ACCEPTOR_STATE, [(P.COMMITTED, 16, 0, 0), (P.ACCEPTED, 17, 0, 0),
                                 (P.PREPARED, 18, 0, 0), (P.PREPARED, 33, 0, R.PF_HAS_PROPOSALS)] +
              [NILROW] * 4)
    return dict(sends=P.mk_sends([(103, 33, 102, R.PH_ACCEPT, 0, 2)]),
                groups=P.mk_groups([(33, self_id, self_id, 2, 104, 102)]), cmds=cols(NEW_ROWS),
                inst_base=BASE, ipg=IPG, peer_commits=np.array([[98, 101, 102]], np.int32), st=st,
                lb=None if lb is None else rows(R.INST_STATE, lb),
                inst=rows(R.INST_CMDS, inst_rows), arena=cols(ARENA_ROWS))


HAS = R.IC_HAS_CMDS
# slot 0 unflagged (its first_cmd / n_cmds are not read: Cmds == nil marshals as V(0)); slots 1 and 2
# in reverse arena order; slot 5, outside every range and nil, names slot 1's range too
INST = [(99, 7, 0), (6, 1, HAS), (2, 3, HAS), (0, 0, 0), (0, 0, 0), (6, 1, HAS), (0, 0, 0), (0, 0, 0)]
# slots 0 and 1 share one range; the log instances then hold 1, 1 and 3 commands
INST_SHARED = [(6, 1, HAS)] + INST[1:]
# lb: NIL at slot 0 (st's COMMITTED stands), ACCEPTED at slot 1, COMMITTED over st's PREPARED at 2
LB = [(P.NIL, 0, 0, 0), (P.ACCEPTED, 1, 0, 0), (P.COMMITTED, 2, 0, 17), (P.PREPARED, 0, 0, 0)] + \
     [(P.NIL, 0, 0, 0)] * 4


def hexes(*per_dest):
    """destination by destination, the frames' hex -> (bytes, dest_off)"""
    runs = [bytes.fromhex("".join(x)) for x in per_dest]
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in runs])
    return np.frombuffer(b"".join(runs), np.uint8), off


# name -> (arguments, bytes, dest_off). The ring walk from self_id 2 reaches 0 then 1; from 0, 1 then 2.
CASES = {
    # peer 0 (98 < first_g): V(3) and the three records; peer 1 (101): V(1) and record 2
    "self2_lb_null": (case(2, None, INST),
                      *hexes((head(2), "06", REC0, REC1, REC2), (head(2), "02", REC2), ())),
    # peer 1: one record; peer 2 (102 = last_committed): V(0), an empty log
    "self0_lb_null": (case(0, None, INST),
                      *hexes((), (head(0), "02", REC2), (head(0), "00"))),
    "self2_lb": (case(2, LB, INST),
                 *hexes((head(2), "06", REC0, REC1, REC2_COMMITTED),
                        (head(2), "02", REC2_COMMITTED), ())),
    "self2_shared": (case(2, LB, INST_SHARED),
                     *hexes((head(2), "06", REC0_ONE, REC1, REC2_COMMITTED),
                            (head(2), "02", REC2_COMMITTED), ())),
}
# frame lengths: head 17 + V(2) 1 + 34 = 52; V(m) 1; records 9, 9 + 17, 9 + 51
LENGTHS = {"self2_lb_null": [0, 148, 261, 261], "self0_lb_null": [0, 0, 113, 166],
           "self2_lb": [0, 148, 261, 261], "self2_shared": [0, 165, 278, 278]}

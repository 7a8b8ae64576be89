"""Known answers of record assembly, worked by hand from the reference's record sites
(recordInstanceMetadata + recordCommands, bareminpaxos.go:164-188 / paxos.go:107-130): for each kind
and format the exact bytes of a small batch. TEST INFRASTRUCTURE.

The three commands every case draws from, as state.(*Command).Marshal writes them (Op u8, K i64 LE,
V i64 LE):
  c0 = PUT  0x11                 5        01 1100000000000000 0500000000000000
  c1 = GET  0x2233              -1        02 3322000000000000 ffffffffffffffff
  c2 = PUT  -2   0x0102030405060708       01 feffffffffffffff 0807060504030201"""
import numpy as np

import record_translit as T
from minpaxos_amd import records as R

C0 = "01" "1100000000000000" "0500000000000000"
C1 = "02" "3322000000000000" "ffffffffffffffff"
C2 = "01" "feffffffffffffff" "0807060504030201"
OP = np.array([1, 2, 1], np.uint8)
KEY = np.array([0x11, 0x2233, -2], np.int64)
VAL = np.array([5, -1, 0x0102030405060708], np.int64)


def source(cmd_off, n_recs):
    return dict(cmd_off=None if cmd_off is None else np.array(cmd_off, np.uint64), op=OP.copy(),
                key=KEY.copy(), val=VAL.copy(), n_recs=n_recs)


# a Commit of two commands, a CommitShort, a Commit of one command with ballot -1
_COMMITS = dict(kind=R.LR_COMMITS, items=T.mk_msgs([(7, 0x21, 0), (8, 0x22, R.VALUE_KEEP), (9, -1, 1)]),
                effect=np.array([R.CH_CMDS, R.CH_INSTALLED, R.CH_CMDS | R.CH_REQUEUE], np.uint8),
                sources=[source([0, 2, 3], 3)])
# a stored Accept of zero commands (12 bytes only), one that was answered but not stored, a stored
# Accept of two commands
_ACCEPTS = dict(kind=R.LR_ACCEPTS, items=T.mk_msgs([(4, 0x10, 0), (4, 0x11, 1), (5, 0x12, 2)]),
                effect=np.array([R.AH_STORED | R.AH_REPLIED, R.AH_REPLIED, R.AH_STORED], np.uint8),
                sources=[source([0, 0, 1, 3], 3)])
# ACCEPT, REFUSED, PREPARE, ACCEPT (and for DECIDED one more ACCEPT)
_SLOTS = [(30, 5, R.PH_ACCEPT, 0, 1), (31, 5, R.PH_REFUSED, 1, 1), (31, 2, R.PH_PREPARE, 1, 1),
          (32, 5, R.PH_ACCEPT, 1, 2)]
_SENDS = dict(kind=R.LR_SENDS, items=T.mk_sends(_SLOTS), sources=[source(None, 4)])
# the window from instance 30: 30 and 33 decided, 32 accepted but not decided, 31 never accepted
_DECIDED = dict(kind=R.LR_DECIDED, items=T.mk_sends(_SLOTS + [(33, 6, R.PH_ACCEPT, 3, 0)]),
                mask=np.array([1, 1, 0, 1], np.uint8), inst_base=30)

KAT = [
    dict(name="commits_min", args=dict(_COMMITS, fmt=R.LOG_DURABLE),
         out="21000000" "03000000" "07000000" + C0 + C1 +
             "22000000" "03000000" "08000000" +
             "ffffffff" "03000000" "09000000" + C2,
         item_off=[0, 46, 58, 87], n_recs=3, n_cmds=3),
    dict(name="commits_classic", args=dict(_COMMITS, fmt=R.LOG_DURABLE_CLASSIC),
         out="21000000" "03" + C0 + C1 + "22000000" "03" + "ffffffff" "03" + C2,
         item_off=[0, 39, 44, 66], n_recs=3, n_cmds=3),
    dict(name="accepts_min", args=dict(_ACCEPTS, fmt=R.LOG_DURABLE),
         out="10000000" "02000000" "04000000" + "12000000" "02000000" "05000000" + C1 + C2,
         item_off=[0, 12, 12, 58], n_recs=2, n_cmds=2),
    dict(name="sends_min", args=dict(_SENDS, fmt=R.LOG_DURABLE),
         out="05000000" "01000000" "1e000000" + C0 + "05000000" "01000000" "20000000" + C1 + C2,
         item_off=[0, 29, 29, 29, 75], n_recs=2, n_cmds=3),
    dict(name="sends_classic", args=dict(_SENDS, fmt=R.LOG_DURABLE_CLASSIC),
         out="05000000" "01" + C0 + "05000000" "01" + C1 + C2,
         item_off=[0, 22, 22, 22, 61], n_recs=2, n_cmds=3),
    dict(name="decided_min", args=dict(_DECIDED, fmt=R.LOG_DURABLE),
         out="05000000" "03000000" "1e000000" + "06000000" "03000000" "21000000",
         item_off=[0, 12, 12, 12, 12, 24], n_recs=2, n_cmds=0),
    dict(name="decided_classic", args=dict(_DECIDED, fmt=R.LOG_DURABLE_CLASSIC),
         out="05000000" "03" + "06000000" "03",
         item_off=[0, 5, 5, 5, 5, 10], n_recs=2, n_cmds=0),
]


def check(case, got):
    """got: out (uint8 array), item_off, res"""
    want = bytes.fromhex(case["out"])
    assert bytes(np.asarray(got["out"])) == want, case["name"]
    assert np.asarray(got["item_off"]).tolist() == case["item_off"], case["name"]
    res = got["res"]
    assert (int(res["n_recs"]), int(res["n_cmds"]), int(res["n_bytes"]), int(res["flags"])) == \
        (case["n_recs"], case["n_cmds"], len(want), 0), case["name"]

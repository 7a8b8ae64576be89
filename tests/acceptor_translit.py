"""TEST INFRASTRUCTURE ONLY — the acceptor's half of Phase 2, restated from the Go text.

A literal transliteration of the two handleAccept functions over Go-shaped objects, in the style
of go_translit.py (whose Instance, LeaderBookkeeping, Slice and panic helpers it reuses), plus a
struct.pack restatement of the two AcceptReply.Marshal functions behind SendMsg's code byte:

  bareminpaxos.(*Replica).handleAccept   src/bareminpaxos/bareminpaxos.go:753-806
  paxos.(*Replica).handleAccept          src/paxos/paxos.go:470-520
  genericsmr.(*Replica).SendMsg          src/genericsmr/genericsmr.go:499-512
  minpaxosproto.(*AcceptReply).Marshal   src/minpaxosproto/minpaxosprotomarsh.go:545-566
  paxosproto.(*AcceptReply).Marshal      src/paxosproto/paxosprotomarsh.go:306-322

This path has ONE restatement (the C oracle does not cover it), so it is pinned by this module
plus the hand-traced known answers below (KAT_MIN / KAT_CLASSIC), which were worked out from the
Go text by hand and are checked against this module and against the engine.

Only the adapter functions at the bottom (accept_handle, encode_accept_replies) know the engine's
record layouts.
"""
import struct

import numpy as np

from go_translit import (ACCEPTED, COMMITTED, PREPARED, PREPARING, GoPanic, Instance,  # noqa: F401
                         LeaderBookkeeping, Slice)
from minpaxos_amd import records as R

TRUE, FALSE = 1, 0  # bareminpaxos.go:19-20, paxos.go `const TRUE/FALSE`
ACCEPT_REPLY_CODE = 13  # the RPC code RegisterRPC hands AcceptReply (the sixth registration after
#                         genericsmrproto's codes: bareminpaxos.go:108-113, paxos.go:93-98)


class Accept:
    """minpaxosproto.Accept {LeaderId, Instance, Ballot, LastCommitted, Command, CatchUpLog}
    (minpaxosproto.go:66-73) / paxosproto.Accept {LeaderId, Instance, Ballot, Command}
    (paxosproto.go:30-35); the fields handleAccept's live code reads"""

    def __init__(self, LeaderId, Instance, Ballot, Command):
        self.LeaderId, self.Instance, self.Ballot, self.Command = LeaderId, Instance, Ballot, Command


class AcceptReply:
    """minpaxosproto.AcceptReply {Instance, OK, Ballot, Id} / paxosproto.AcceptReply (no Id)"""

    def __init__(self, Instance, OK, Ballot, Id=None):
        self.Instance, self.OK, self.Ballot, self.Id = Instance, OK, Ballot, Id


class Acceptor:
    """the fields of bareminpaxos.Replica / paxos.Replica that handleAccept touches, plus logs
    standing in for its side effects: `sent` for replyAccept -> SendMsg, `events` for the stable
    store writes and ProposeChan, `branch` for the path the last message took"""

    def __init__(self, N, Id, defaultBallot, instanceSpace):
        self.N, self.Id, self.defaultBallot = N, Id, defaultBallot
        self.instanceSpace = instanceSpace
        self.sent, self.events, self.branch = [], [], None

    def replyAccept(self, replicaId, reply):  # bareminpaxos.go / paxos.go replyAccept -> SendMsg
        if replicaId < 0 or replicaId >= self.N:  # genericsmr.go:501 r.PeerWriters[peerId]
            raise GoPanic(R.E_BAD_ID, f"index {replicaId} out of range [0:{self.N}]")
        self.sent.append((replicaId, reply))

    # ---- MIN  src/bareminpaxos/bareminpaxos.go:753-806 ----
    def min_handleAccept(self, accept):
        self.branch = "mismatch"
        if self.instanceSpace[accept.Instance] is not None:                        # :757
            if self.instanceSpace[accept.Instance].Status == ACCEPTED and \
                    self.instanceSpace[accept.Instance].Ballot == accept.Ballot:   # :758
                self.branch = "resend"
                return                                                             # :760
        # :764-784 a dlog line and commented-out code
        if self.defaultBallot == accept.Ballot:                                    # :786
            inst = Instance(ACCEPTED, accept.Ballot, accept.Command,
                            LeaderBookkeeping(0, 0, 0, clientProposals=None))      # :787-791
            self.instanceSpace[accept.Instance] = inst                             # :793
            areply = AcceptReply(accept.Instance, TRUE, accept.Ballot, self.Id)    # :794
            self.replyAccept(accept.LeaderId, areply)                              # :796
            self.events.append("stored")                                           # :798-800
            self.branch = "acted"
        # :803-805 a loop around a commented-out dlog line

    # ---- CLASSIC  src/paxos/paxos.go:470-520 ----
    def classic_handleAccept(self, accept):
        inst = self.instanceSpace[accept.Instance]                                 # :471
        if inst is None:                                                           # :474
            if accept.Ballot < self.defaultBallot:                                 # :476
                areply = AcceptReply(accept.Instance, FALSE, self.defaultBallot)   # :477
                self.branch = "nil_low"
            else:
                self.instanceSpace[accept.Instance] = Instance(
                    ACCEPTED, accept.Ballot, accept.Command, None)                 # :479-483
                areply = AcceptReply(accept.Instance, TRUE, self.defaultBallot)    # :484
                self.branch = "nil_install"
        elif inst.Ballot > accept.Ballot:                                          # :486
            areply = AcceptReply(accept.Instance, FALSE, inst.Ballot)              # :488
            self.branch = "higher"
        elif inst.Ballot < accept.Ballot:                                          # :489
            inst.Cmds = accept.Command                                             # :491
            inst.Ballot = accept.Ballot                                            # :492
            inst.Status = ACCEPTED                                                 # :493
            areply = AcceptReply(accept.Instance, TRUE, inst.Ballot)               # :494
            self.branch = "lower"
            if inst.Lb is not None and inst.Lb.ClientProposals is not None:        # :495
                self.events.append("requeue")                                      # :498-500
                inst.Lb.ClientProposals = None                                     # :501
        else:                                                                      # :503
            self.instanceSpace[accept.Instance].Cmds = accept.Command              # :506
            if self.instanceSpace[accept.Instance].Status != COMMITTED:            # :507
                self.instanceSpace[accept.Instance].Status = ACCEPTED              # :508
            areply = AcceptReply(accept.Instance, TRUE, self.defaultBallot)        # :510
            self.branch = "equal"
        if areply.OK == TRUE:                                                      # :513
            self.events.append("stored")                                           # :514-516
        self.replyAccept(accept.LeaderId, areply)                                  # :519


# ---- the bytes SendMsg writes for one AcceptReply ------------------------------------------------
def marshal_min(t):  # minpaxosprotomarsh.go:545-566: Instance, OK, Ballot, Id (13 bytes)
    return struct.pack("<iBii", t.Instance, t.OK, t.Ballot, t.Id)


def marshal_classic(t):  # paxosprotomarsh.go:306-322: Instance, OK, Ballot (9 bytes)
    return struct.pack("<iBi", t.Instance, t.OK, t.Ballot)


def send_msg_bytes(mode, t):  # genericsmr.go:503-504: WriteByte(code), msg.Marshal(w)
    return bytes([ACCEPT_REPLY_CODE]) + (marshal_min(t) if mode == R.MODE_MIN
                                         else marshal_classic(t))


# ---- adapter: the engine's records <-> the objects above -----------------------------------------
def _inst_from(s):
    if int(s["status"]) == R.STATUS_NIL:
        return None
    props = [object()] if int(s["flags"]) & R.PF_HAS_PROPOSALS else None
    return Instance(int(s["status"]), int(s["ballot"]), int(s["value_id"]),
                    LeaderBookkeeping(clientProposals=props))


def accept_handle(mode, N, msgs, st, groups, inst_base=0, ipg=None, want_branches=False):
    """the Engine.accept_handle surface over the transliteration (GoPanic where Go panics, and
    E_INVAL where the batch contract is broken: CONTRACT records grouped by instance, ascending)"""
    st = np.array(st, R.ACCEPTOR_STATE, copy=True)
    groups = np.atleast_1d(np.asarray(groups, R.ACCEPTOR_GROUP))
    ipg = len(st) // len(groups) if ipg is None else ipg
    if ipg < 1 or ipg * len(groups) != len(st):
        raise GoPanic(R.E_INVAL, "n_inst != n_groups * ipg")
    n = len(msgs)
    replies = np.zeros(n, R.ACCEPT_REPLY)
    reply_to = np.full(n, -1, np.int32)
    effect = np.zeros(n, np.uint8)
    branches = []
    items = [_inst_from(s) for s in st]
    orig = list(items)
    space = Slice(inst_base, items)
    reps = [Acceptor(N, int(g["self_id"]), int(g["default_ballot"]), space) for g in groups]
    requeued, touched = set(), set()
    prev = None
    for i, m in enumerate(msgs):
        inst_no = int(m["instance"])
        if prev is not None and inst_no < prev:
            raise GoPanic(R.E_INVAL, "records not in ascending instance order")
        prev = inst_no
        j = inst_no - inst_base
        if j < 0 or j >= len(st):
            raise GoPanic(R.E_NIL_INSTANCE, f"index {inst_no} out of range")
        rep = reps[j // ipg]  # CONTRACT: window index j belongs to group j / ipg
        rep.sent, rep.events = [], []
        a = Accept(int(m["leader_id"]), inst_no, int(m["ballot"]), int(m["value_id"]))
        (rep.min_handleAccept if mode == R.MODE_MIN else rep.classic_handleAccept)(a)
        touched.add(j)
        branches.append(rep.branch)
        fl = 0
        for to, ar in rep.sent:
            fl |= R.AH_REPLIED
            reply_to[i] = to
            replies[i]["instance"], replies[i]["ok"] = ar.Instance, ar.OK
            replies[i]["ballot"] = ar.Ballot
            replies[i]["id"] = ar.Id if mode == R.MODE_MIN else -1  # CLASSIC: no Id on the wire
        if "stored" in rep.events:
            fl |= R.AH_STORED
        if "requeue" in rep.events:
            fl |= R.AH_REQUEUE
            requeued.add(j)
        effect[i] = fl
    for j in touched:
        inst, s = items[j], st[j]
        if inst is None:
            continue  # still nil: the slot is left as it was
        s["status"], s["ballot"], s["value_id"] = inst.Status, inst.Ballot, inst.Cmds
        has = inst.Lb is not None and inst.Lb.ClientProposals is not None
        if inst is orig[j]:  # the same *Instance: its other flag bits stay
            fl = int(s["flags"]) & ~R.PF_HAS_PROPOSALS
        else:                # a fresh Instance replaced it
            fl = 0
        fl |= R.PF_HAS_PROPOSALS if has else 0
        fl |= R.PF_REQUEUED if j in requeued else 0
        s["flags"] = fl
    out = (st, replies, reply_to, effect)
    return out + (branches,) if want_branches else out


def encode_accept_replies(mode, replies, reply_to, n_dest):
    """per destination, the frames SendMsg writes for its replies in array order"""
    runs = [bytearray() for _ in range(n_dest)]
    for r, to in zip(replies, reply_to):
        to = int(to)
        if to < 0:
            continue
        if to >= n_dest:
            raise GoPanic(R.E_INVAL, "destination")
        runs[to] += send_msg_bytes(mode, AcceptReply(int(r["instance"]), int(r["ok"]),
                                                     int(r["ballot"]), int(r["id"])))
    off = np.zeros(n_dest + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in runs])
    return np.frombuffer(b"".join(bytes(x) for x in runs), np.uint8), off


# ---- small builders shared by the tests ----------------------------------------------------------
NIL = R.STATUS_NIL


def mk_state(rows):
    """rows of (status, ballot, value_id, flags)"""
    st = np.zeros(len(rows), R.ACCEPTOR_STATE)
    for s, row in zip(st, rows):
        s["status"], s["ballot"], s["value_id"], s["flags"] = row
    return st


def mk_msgs(rows):
    """rows of (instance, ballot, leader_id, value_id)"""
    m = np.zeros(len(rows), R.ACCEPT_MSG)
    for x, row in zip(m, rows):
        x["instance"], x["ballot"], x["leader_id"], x["value_id"] = row
    return m


def mk_groups(rows):
    g = np.zeros(len(rows), R.ACCEPTOR_GROUP)
    for x, row in zip(g, rows):
        x["default_ballot"], x["self_id"] = row
    return g


# ---- hand-traced known answers (N = 5, D = 16 unless stated, self_id = 3, leader 0) --------------
# Each case: (name, D, state in (status, ballot, value, flags), messages (ballot, value), then the
# expected state out and per message (replied, ok, reply ballot, effect)). Worked out from the Go
# text by hand, not by running this module.
SELF = 3
_RS = R.AH_REPLIED | R.AH_STORED
KAT_MIN = [
    # 1 + 2: nil + Accept(16) installs and replies; the same Accept again is a resend: ignored
    ("install_then_resend", 16, (NIL, 0, 0, 0), [(16, 7), (16, 7)],
     (ACCEPTED, 16, 7, 0), [(1, 1, 16, _RS), (0, 0, 0, 0)]),
    # 3: nil + Accept(32) at D = 16: ballot mismatch, nothing happens, stays nil
    ("nil_other_ballot", 16, (NIL, 0, 0, 0), [(32, 7)],
     (NIL, 0, 0, 0), [(0, 0, 0, 0)]),
    # 4: status is not checked: COMMITTED is demoted, the fresh Lb drops the proposals silently
    ("committed_demoted", 16, (COMMITTED, 16, 5, R.PF_HAS_PROPOSALS), [(16, 9)],
     (ACCEPTED, 16, 9, 0), [(1, 1, 16, _RS)]),
    # 5: ACCEPTED at an older ballot is not a resend
    ("accepted_older", 16, (ACCEPTED, 0, 5, 0), [(16, 9)],
     (ACCEPTED, 16, 9, 0), [(1, 1, 16, _RS)]),
    # 6: ACCEPTED at the same ballot: ignored, state untouched
    ("accepted_same", 16, (ACCEPTED, 16, 5, 0), [(16, 9)],
     (ACCEPTED, 16, 5, 0), [(0, 0, 0, 0)]),
    # 7: after a leader change (D = 32) the instance accepted at 16 accepts again
    ("new_default_ballot", 32, (ACCEPTED, 16, 5, 0), [(32, 9)],
     (ACCEPTED, 32, 9, 0), [(1, 1, 32, _RS)]),
]
KAT_CLASSIC = [
    ("nil_low", 16, (NIL, 0, 0, 0), [(0, 7)],
     (NIL, 0, 0, 0), [(1, 0, 16, R.AH_REPLIED)]),
    ("nil_install", 16, (NIL, 0, 0, 0), [(32, 7)],
     (ACCEPTED, 32, 7, 0), [(1, 1, 16, _RS)]),  # the reply carries D, not the Accept's ballot
    ("higher_refuses", 16, (PREPARED, 32, 5, 0), [(16, 7)],
     (PREPARED, 32, 5, 0), [(1, 0, 32, R.AH_REPLIED)]),
    ("lower_requeues", 16, (PREPARED, 16, 5, R.PF_HAS_PROPOSALS), [(32, 9)],
     (ACCEPTED, 32, 9, R.PF_REQUEUED), [(1, 1, 32, _RS | R.AH_REQUEUE)]),
    ("equal_committed_stays", 16, (COMMITTED, 16, 5, 0), [(16, 9)],
     (COMMITTED, 16, 9, 0), [(1, 1, 16, _RS)]),
    ("committed_demoted", 16, (COMMITTED, 16, 5, 0), [(32, 9)],
     (ACCEPTED, 32, 9, 0), [(1, 1, 32, _RS)]),
    # 7: a run on a nil instance: install at 32 (reply D), 16 refused with 32, 32 again is the
    # equal branch (reply D) and takes the last value
    ("run_on_nil", 16, (NIL, 0, 0, 0), [(32, 7), (16, 8), (32, 9)],
     (ACCEPTED, 32, 9, 0), [(1, 1, 16, _RS), (1, 0, 32, R.AH_REPLIED), (1, 1, 16, _RS)]),
]


def kat_inputs(case, inst=40, inst_base=40):
    """(msgs, st, groups) of a known-answer case: one instance, one group"""
    _, D, s, ms, _, _ = case
    return (mk_msgs([(inst, b, 0, v) for b, v in ms]), mk_state([s]), mk_groups([(D, SELF)]),
            inst_base)


def kat_expected(mode, case, inst=40):
    """(st, replies, reply_to, effect) a known-answer case must produce"""
    _, _, _, ms, s_out, outs = case
    replies = np.zeros(len(ms), R.ACCEPT_REPLY)
    reply_to = np.full(len(ms), -1, np.int32)
    effect = np.zeros(len(ms), np.uint8)
    for i, (replied, ok, rb, eff) in enumerate(outs):
        effect[i] = eff
        if replied:
            reply_to[i] = 0
            replies[i]["instance"], replies[i]["ok"], replies[i]["ballot"] = inst, ok, rb
            replies[i]["id"] = SELF if mode == R.MODE_MIN else -1
    return mk_state([s_out]), replies, reply_to, effect


# ---- the fuzz generator --------------------------------------------------------------------------
FUZZ_SEEDS = range(24)
BRANCHES = {R.MODE_MIN: ("resend", "acted", "mismatch"),
            R.MODE_CLASSIC: ("nil_low", "nil_install", "higher", "lower", "equal")}


def fuzz_case(seed, N=5):
    """One seeded batch: 1 to 5000 messages in runs of 1 to 5 per instance (every fourth seed
    also one run longer than a 1024-record tile), ballots of messages and states from
    {D-16, D, D+16} of the instance's group, states uniform over nil and the four statuses.
    Returns (msgs, st, groups, inst_base, ipg)."""
    rng = np.random.default_rng(1000 + seed)
    n_target = int(rng.integers(1, 5001))
    ipg = int(rng.choice([8, 64, 1 << 20]))
    inst_base = int(rng.choice([0, 977]))
    runs = []
    total = 0
    while total < n_target:
        k = int(rng.integers(1, 6))
        k = min(k, n_target - total)
        runs.append(k)
        total += k
    if seed % 4 == 3:
        runs[len(runs) // 2] = 1024 + int(rng.integers(1, 400))
    gaps = rng.integers(0, 3, len(runs))  # instances without messages between the runs
    idx = np.cumsum(gaps + 1) - 1 + int(rng.integers(0, 4))
    n_inst = int(idx[-1]) + 1 + int(rng.integers(0, 4))
    return case_from_runs(rng, idx, runs, n_inst, ipg, inst_base, N)


def case_from_runs(rng, idx, runs, n_inst, ipg, inst_base=0, N=5):
    """the fuzz's mix over a given shape: window index idx[k] receives runs[k] messages (idx
    ascending); groups of ipg instances (one group when ipg covers the window, the window
    rounded up to whole groups otherwise). Returns (msgs, st, groups, inst_base, ipg)."""
    idx = np.asarray(idx, np.int64)
    if ipg >= n_inst:
        ipg, n_groups = n_inst, 1
    else:
        n_groups = (n_inst + ipg - 1) // ipg
        n_inst = n_groups * ipg
    groups = mk_groups([(16 * (2 + g % 3), (g * 7 + 1) % N) for g in range(n_groups)])
    Dof = groups["default_ballot"][np.arange(n_inst) // ipg].astype(np.int64)
    st = np.zeros(n_inst, R.ACCEPTOR_STATE)
    st["status"] = rng.integers(-1, 4, n_inst)
    st["ballot"] = Dof + 16 * rng.integers(-1, 2, n_inst)
    st["value_id"] = rng.integers(1, 1 << 31, n_inst)
    st["flags"] = np.where(st["status"] == NIL, 0, rng.integers(0, 2, n_inst) * R.PF_HAS_PROPOSALS)
    inst_of = np.repeat(idx, runs)
    n = len(inst_of)
    msgs = np.zeros(n, R.ACCEPT_MSG)
    msgs["instance"] = inst_of + inst_base
    msgs["ballot"] = Dof[inst_of] + 16 * rng.integers(-1, 2, n)
    msgs["leader_id"] = rng.integers(0, N, n)
    msgs["value_id"] = rng.integers(1, 1 << 31, n)
    return msgs, st, groups, inst_base, ipg

"""A whole-replica, message-at-a-time model of Phase 2 of both protocols, read from the Go one
handler at a time, and a scheduler that runs G independent reference clusters in turns.

TEST INFRASTRUCTURE: the reference of the closed-loop tests (test_cluster_model.py,
test_cluster_translit.py, test_gpu_cluster.py). It is a third reading of the Go, shaped unlike the
oracle (a C++ restatement of single handlers over records) and unlike the batch transliterations
(one handler each, over the engine's arrays): a Replica here holds the Go's fields, real command
lists and a real State map, and is not assembled from either.

  handlePropose        MIN  src/bareminpaxos/bareminpaxos.go:617-710   CLASSIC  src/paxos/paxos.go:388-443
  bcastAccept          MIN  :450-520                                   CLASSIC  :299-331
  handleAccept         MIN  :753-806                                   CLASSIC  :470-520
  handleAcceptReply    MIN  :1014-1064                                 CLASSIC  :631-673
  bcastCommit          MIN  :565-615                                   CLASSIC  :336-386
  handleCommit[Short]  MIN  :856-910                                   CLASSIC  :522-575
  updateCommittedUpTo  MIN  :387-392                                   CLASSIC  :259-264
  executeCommands      MIN  :1066-1098                                 CLASSIC  :675-706
  recordInstanceMetadata / recordCommands   MIN :164-188               CLASSIC  :107-130
  Command.Execute      src/state/state.go:77-103

The window. The engine gives group g the instance numbers [inst_base + g*ipg, inst_base +
(g+1)*ipg): `first` stands for the reference's instance 0 (as in proposer_translit), so the Go's
`< 0` reads `< first`, a fresh replica has committedUpTo = first - 1 and crtInstance = first, and
an index outside the window is the Go's index-out-of-range panic (GoPanic). A replica starts where
a finished Phase 1 leaves it (Phase 1 is out of scope here): every replica of a group holds the
group's defaultBallot and Leader, MIN's leader holds prepareOKs = N/2 + 1 and peerCommits =
first - 1 for every peer.

The schedule (Cluster). Go's `select` takes the ready channels in any order; this is one legal
schedule, and the handlers know nothing of it. A turn is walked station by station, every replica
at each station before any replica at the next:
  1 proposals      the turn's client bytes; the proposals of a group enter its ProposeChan in
                   connection order, then stream order, and handlePropose runs until it is empty
  2 Accepts        what the peers' station 1 wrote
  3 AcceptReplies  what the peers' station 2 wrote
  4 Commit[Short]s what the leaders' station 3 wrote
  5 one executeCommands pass from the executed cursor
so with every connection delivering, an instance is proposed, accepted, decided, committed and
executed inside one turn. Inside a station a replica handles its inbox in the order
mpx_order_records defines: instance ascending, arrival order kept, where arrival is the
connection's index (the peer's id) and then the stream offset. A seeded `hold[turn][p][q]` says
that connection p -> q delivers nothing in that turn: whatever p wrote on it stays in the stream
and is read, in front of the later bytes, at the same station of the next turn that delivers.
That gives lagging peers, MIN catch-up logs longer than one instance and late AcceptReplies.
Replicas talk only in bytes: an outbox is marshalled (minpaxos_amd.wire, proposer_translit) when
it is written and parsed again (unmarshal_translit) when it is read.

CLASSIC's ProposeReplyTS literals (paxos.go:390, :647, :686) name four fields of the five the
struct marshals (gsmrprotomarsh.go:702-732); Leader is then Go's zero value, 0.
"""
import struct
from collections import deque

import numpy as np

import proposer_translit as P
import unmarshal_translit as U
from go_translit import GoPanic
from minpaxos_amd import records as R
from minpaxos_amd import wire as W

MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
TRUE, FALSE = 1, 0
NIL_VALUE = 0                                   # state.NIL
PREPARING, PREPARED, ACCEPTED, COMMITTED = 0, 1, 2, 3
NONE, PUT, GET, DELETE, RLOCK, WLOCK = range(6)  # state.go:12-19
MAX_BATCH = 5000                                # bareminpaxos.go:22 / paxos.go:20
KINDS = ("accept", "accept_reply", "commit")


# ---- the Go's structs ------------------------------------------------------------------------------
class Propose:                                  # genericsmr.Propose
    def __init__(self, CommandId, Command, Timestamp, Reply):
        self.CommandId, self.Command, self.Timestamp, self.Reply = CommandId, Command, Timestamp, Reply


class ProposeReplyTS:                           # genericsmrproto.go:31-37
    def __init__(self, OK, CommandId, Value, Timestamp, Leader=0):
        self.OK, self.CommandId, self.Value, self.Timestamp, self.Leader = \
            OK, CommandId, Value, Timestamp, Leader

    def Marshal(self):                          # gsmrprotomarsh.go:702-732
        return struct.pack("<Biqqi", self.OK, self.CommandId, self.Value, self.Timestamp, self.Leader)


class LeaderBookkeeping:
    def __init__(self, ClientProposals):
        self.ClientProposals = ClientProposals
        self.MaxRecvBallot, self.AcceptOKs, self.Nacks = 0, 0, 0


class Instance:
    def __init__(self, Cmds, Ballot, Status, Lb):
        self.Cmds, self.Ballot, self.Status, self.Lb = Cmds, Ballot, Status, Lb


class Accept:
    def __init__(self, LeaderId, Instance, Ballot, Command, LastCommitted=None, CatchUpLog=None):
        self.LeaderId, self.Instance, self.Ballot, self.Command = LeaderId, Instance, Ballot, Command
        self.LastCommitted, self.CatchUpLog = LastCommitted, CatchUpLog


class AcceptReply:
    def __init__(self, Instance, OK, Ballot, Id=0):
        self.Instance, self.OK, self.Ballot, self.Id = Instance, OK, Ballot, Id


class Commit:
    def __init__(self, LeaderId, Instance, Ballot, Command):
        self.LeaderId, self.Instance, self.Ballot, self.Command = LeaderId, Instance, Ballot, Command


class CommitShort:
    def __init__(self, LeaderId, Instance, Count, Ballot):
        self.LeaderId, self.Instance, self.Count, self.Ballot = LeaderId, Instance, Count, Ballot


def execute(cmd, store):                        # state.go:77-103
    op, k, v = cmd
    if op == PUT:
        store[k] = v
        return v
    if op == GET:
        if k in store:
            return store[k]
    return NIL_VALUE


# ---- one replica of one group ----------------------------------------------------------------------
class Replica:
    """the fields of bareminpaxos.Replica / paxos.Replica (with genericsmr.Replica's) that Phase 2
    reads. `out` receives (kind, destination, message) in call order; `counts` what the tests'
    non-vacuity conditions ask about."""

    def __init__(self, mode, N, Id, leader, first, ipg, default_ballot, thrifty=False, dreply=False,
                 durable=True, out=None, store=None):
        self.mode, self.N, self.Id, self.first, self.ipg = mode, N, Id, first, ipg
        self.Leader, self.IsLeader = leader, leader == Id
        self.Thrifty, self.Dreply, self.Durable = thrifty, dreply, durable
        self.Alive = [True] * N
        self.defaultBallot = default_ballot
        self.crtInstance = first
        self.committedUpTo = first - 1
        self.space = [None] * ipg                               # instanceSpace[first ...]
        self.prepareOKs = (N >> 1) + 1 if self.IsLeader else 0  # prepareBookkeeping (MIN)
        self.peerCommits = [first - 1] * N
        self.State = {}
        self.executed = first                                   # executeCommands' i
        # one process serves a group each of many clusters: they share its file and its writers
        self.StableStore = bytearray() if store is None else store
        self.ProposeChan = deque()
        self.out = [] if out is None else out
        # unanswered: proposals MIN drains behind a refused head (:648, :684); late_ignored: CLASSIC,
        # an AcceptReply that finds its instance COMMITTED (:634-636), MIN, one past the quorum (it
        # still moves peerCommits, :1050); nil_install: a Commit that finds a nil slot; catchup: the
        # CatchUpLog length of every MIN Accept; get_hits: GETs that found their key
        self.counts = dict(unanswered=0, late_ignored=0, nil_install=0, catchup=[], get_hits=0)

    # instanceSpace[i], with the Go's bounds check
    def at(self, i):
        if i < self.first or i >= self.first + self.ipg:
            raise GoPanic(R.E_NIL_INSTANCE, f"instanceSpace[{i}]: index out of range")
        return i - self.first

    def get(self, i):
        return self.space[self.at(i)]

    def put(self, i, inst):
        self.space[self.at(i)] = inst

    def deref(self, i):
        inst = self.get(i)
        if inst is None:
            raise GoPanic(R.E_NIL_INSTANCE, f"instanceSpace[{i}] is nil")
        return inst

    # ---- stable storage ----
    def recordInstanceMetadata(self, inst, instNo):
        if not self.Durable:
            return
        if self.mode == MIN:                                    # bareminpaxos.go:164-174
            self.StableStore += struct.pack("<III", inst.Ballot & 0xFFFFFFFF,
                                            inst.Status & 0xFFFFFFFF, instNo & 0xFFFFFFFF)
        else:                                                   # paxos.go:107-116
            self.StableStore += struct.pack("<IB", inst.Ballot & 0xFFFFFFFF, inst.Status & 0xFF)

    def recordCommands(self, cmds):                             # :177-188 / :119-130
        if not self.Durable or cmds is None:
            return
        for c in cmds:
            self.StableStore += W.command(*c)

    # ---- sending ----
    def SendMsg(self, q, kind, msg):
        self.out.append((kind, q, msg))

    def ReplyProposeTS(self, reply, w):
        self.out.append(("client", w, reply))

    def _reply(self, ok, cid, value, ts):
        # MIN's literal names Leader (:622, :1035, :1077), CLASSIC's does not (:390, :647, :686)
        return ProposeReplyTS(ok, cid, value, ts, self.Leader if self.mode == MIN else 0)

    # ---- handlePropose ----
    def handlePropose(self, propose):
        if self.mode == MIN:
            return self._handlePropose_min(propose)
        return self._handlePropose_classic(propose)

    def _batch(self, propose):
        batchSize = len(self.ProposeChan) + 1                   # :634 / :402
        if batchSize > MAX_BATCH:
            batchSize = MAX_BATCH
        cmds, proposals = [propose.Command], [propose]
        for _ in range(1, batchSize):                           # :647-651 / :415-419
            prop = self.ProposeChan.popleft()
            cmds.append(prop.Command)
            proposals.append(prop)
        return cmds, proposals

    def _handlePropose_min(self, propose):                      # bareminpaxos.go:617-710
        if self.Leader != self.Id or self.prepareOKs <= self.N >> 1:      # :618
            self.ReplyProposeTS(self._reply(FALSE, -1, NIL_VALUE, 0), propose.Reply)  # :622-623
            return
        while self.get(self.crtInstance) is not None:           # :627
            self.crtInstance += 1
        instNo = self.crtInstance                               # :632
        cmds, proposals = self._batch(propose)                  # :634-651
        if self.committedUpTo < instNo - 1:                     # :671
            self.ReplyProposeTS(self._reply(FALSE, -1, NIL_VALUE, 0), propose.Reply)  # :682-683
            self.counts["unanswered"] += len(proposals) - 1     # drained at :648, never answered
            return                                              # :684
        if self.Leader == self.Id:                              # :687
            self.crtInstance += 1                               # :688
            if self.prepareOKs > self.N >> 1:                   # :689
                inst = Instance(cmds, self.defaultBallot, PREPARED, LeaderBookkeeping(proposals))
                self.put(instNo, inst)                          # :691-695
                self.recordInstanceMetadata(inst, instNo)       # :697
                self.recordCommands(cmds)                       # :698
                self.bcastAccept_min(instNo, self.defaultBallot, self.committedUpTo, cmds,
                                     self.peerCommits)          # :702

    def _handlePropose_classic(self, propose):                  # paxos.go:388-443
        if not self.IsLeader:                                   # :389
            self.ReplyProposeTS(self._reply(FALSE, -1, NIL_VALUE, 0), propose.Reply)  # :390-391
            return
        while self.get(self.crtInstance) is not None:           # :395
            self.crtInstance += 1
        instNo = self.crtInstance                               # :399
        self.crtInstance += 1                                   # :400
        cmds, proposals = self._batch(propose)                  # :402-419
        if self.defaultBallot == -1:                            # :421
            raise NotImplementedError("Phase 1 (paxos.go:422-427) is out of this model's scope")
        inst = Instance(cmds, self.defaultBallot, PREPARED, LeaderBookkeeping(proposals))
        self.put(instNo, inst)                                  # :430-434
        self.recordInstanceMetadata(inst, instNo)               # :436
        self.recordCommands(cmds)                               # :437
        self.bcastAccept_classic(instNo, self.defaultBallot, cmds)  # :440

    # ---- bcastAccept ----
    def bcastAccept_min(self, instance, ballot, lastcommitted, command, peercommits):  # :450-520
        n = self.N - 1                                          # :465
        if self.Thrifty:
            n = self.N >> 1                                     # :467
        q = self.Id
        sent = 0
        while sent < n:                                         # :471
            q = (q + 1) % self.N                                # :472
            if q == self.Id:                                    # :473
                break
            # :476-480: a dead peer is reconnected; it is sent to either way
            sent += 1                                           # :482
            partiallog = []
            if peercommits[q] < self.first and self.crtInstance >= self.first:  # :496 (`< 0`)
                for i in range(self.first, lastcommitted + 1):  # :498
                    partiallog.append(self.deref(i))            # :499
            elif self.crtInstance >= self.first:                # :502
                for i in range(peercommits[q] + 1, lastcommitted + 1):  # :504
                    partiallog.append(self.deref(i))            # :505
            log = [(x.Ballot, x.Status, list(x.Cmds or [])) for x in partiallog]
            self.counts["catchup"].append(len(log))
            self.SendMsg(q, "accept", Accept(self.Id, instance, ballot, command, lastcommitted, log))  # :515

    def bcastAccept_classic(self, instance, ballot, command):   # paxos.go:299-331
        n = self.N - 1
        if self.Thrifty:
            n = self.N >> 1
        q = self.Id
        sent = 0
        while sent < n:                                         # :318
            q = (q + 1) % self.N
            if q == self.Id:
                break
            if not self.Alive[q]:                               # :323
                continue
            sent += 1
            self.SendMsg(q, "accept", Accept(self.Id, instance, ballot, command))  # :329

    # ---- bcastCommit: the two texts are the same ----
    def bcastCommit(self, instance, ballot, command):           # :565-615 / :336-386
        args = Commit(self.Id, instance, ballot, command)
        argsShort = CommitShort(self.Id, instance, len(command), ballot)
        n = self.N - 1
        if self.Thrifty:
            n = self.N >> 1
        q = self.Id
        sent = 0
        while sent < n:                                         # :591 / :362
            q = (q + 1) % self.N
            if q == self.Id:
                break
            if not self.Alive[q]:
                continue
            sent += 1
            self.SendMsg(q, "commit", argsShort)                # :600 / :371
        if self.Thrifty and q != self.Id:                       # :602 / :373
            while sent < self.N - 1:
                q = (q + 1) % self.N
                if q == self.Id:
                    break
                if not self.Alive[q]:
                    continue
                sent += 1
                self.SendMsg(q, "commit", args)                 # :612 / :383

    # ---- handleAccept ----
    def handleAccept(self, accept):
        if self.mode == MIN:                                    # bareminpaxos.go:753-806
            inst = self.get(accept.Instance)                    # :757
            if inst is not None:
                if inst.Status == ACCEPTED and inst.Ballot == accept.Ballot:  # :758
                    return                                      # :760
            if self.defaultBallot == accept.Ballot:             # :786
                inst = Instance(accept.Command, accept.Ballot, ACCEPTED, LeaderBookkeeping(None))
                self.put(accept.Instance, inst)                 # :793
                areply = AcceptReply(accept.Instance, TRUE, accept.Ballot, self.Id)  # :794
                self.SendMsg(accept.LeaderId, "accept_reply", areply)  # :796
                self.recordInstanceMetadata(inst, accept.Instance)  # :798
                self.recordCommands(accept.Command)             # :799
            return
        inst = self.get(accept.Instance)                        # paxos.go:470-520
        if inst is None:                                        # :474
            if accept.Ballot < self.defaultBallot:              # :476
                areply = AcceptReply(accept.Instance, FALSE, self.defaultBallot)
            else:
                self.put(accept.Instance, Instance(accept.Command, accept.Ballot, ACCEPTED, None))
                areply = AcceptReply(accept.Instance, TRUE, self.defaultBallot)  # :484
        elif inst.Ballot > accept.Ballot:                       # :486
            areply = AcceptReply(accept.Instance, FALSE, inst.Ballot)
        elif inst.Ballot < accept.Ballot:                       # :489
            inst.Cmds = accept.Command
            inst.Ballot = accept.Ballot
            inst.Status = ACCEPTED
            areply = AcceptReply(accept.Instance, TRUE, inst.Ballot)
            self._requeue(inst)                                 # :495-502
        else:                                                   # :503
            inst.Cmds = accept.Command                          # :506
            if inst.Status != COMMITTED:                        # :507
                inst.Status = ACCEPTED
            areply = AcceptReply(accept.Instance, TRUE, self.defaultBallot)  # :510
        if areply.OK == TRUE:                                   # :513
            self.recordInstanceMetadata(self.get(accept.Instance), accept.Instance)  # :514
            self.recordCommands(accept.Command)                 # :515
        self.SendMsg(accept.LeaderId, "accept_reply", areply)   # :519

    def _requeue(self, inst):
        if inst.Lb is not None and inst.Lb.ClientProposals is not None:
            for p in inst.Lb.ClientProposals:
                self.ProposeChan.append(p)
            inst.Lb.ClientProposals = None

    # ---- handleAcceptReply ----
    def handleAcceptReply(self, areply):
        inst = self.deref(areply.Instance)
        if self.mode == MIN:                                    # bareminpaxos.go:1014-1064
            if areply.OK == TRUE:                               # :1023
                inst.Lb.AcceptOKs += 1                          # :1024
                if inst.Lb.AcceptOKs + 1 > self.N >> 1:         # :1025
                    if inst.Lb.AcceptOKs == self.N >> 1:        # :1026
                        inst.Status = COMMITTED                 # :1028
                        if inst.Lb.ClientProposals is not None and not self.Dreply:  # :1030
                            for i in range(len(inst.Cmds)):     # :1034
                                p = inst.Lb.ClientProposals[i]
                                self.ReplyProposeTS(self._reply(TRUE, p.CommandId, NIL_VALUE,
                                                                p.Timestamp), p.Reply)  # :1035-1041
                        self.recordInstanceMetadata(inst, areply.Instance)  # :1045
                        self.committedUpTo = areply.Instance    # :1048
                    else:
                        self.counts["late_ignored"] += 1
                    self.peerCommits[areply.Id] = areply.Instance - 1  # :1050
            return
        if inst.Status != PREPARED and inst.Status != ACCEPTED:  # paxos.go:634
            self.counts["late_ignored"] += 1
            return                                              # :636
        if areply.OK == TRUE:                                   # :639
            inst.Lb.AcceptOKs += 1                              # :640
            if inst.Lb.AcceptOKs + 1 > self.N >> 1:             # :641
                inst.Status = COMMITTED                         # :643
                if inst.Lb.ClientProposals is not None and not self.Dreply:  # :644
                    for i in range(len(inst.Cmds)):             # :646
                        p = inst.Lb.ClientProposals[i]
                        self.ReplyProposeTS(self._reply(TRUE, p.CommandId, NIL_VALUE, p.Timestamp),
                                            p.Reply)            # :647-652
                self.recordInstanceMetadata(inst, areply.Instance)  # :656
                self.updateCommittedUpTo()                      # :659
                self.bcastCommit(areply.Instance, inst.Ballot, inst.Cmds)  # :661
        else:
            inst.Lb.Nacks += 1                                  # :665
            if areply.Ballot > inst.Lb.MaxRecvBallot:           # :666
                inst.Lb.MaxRecvBallot = areply.Ballot

    def updateCommittedUpTo(self):                              # :387-392 / :259-264
        while self.committedUpTo + 1 < self.first + self.ipg and \
                self.get(self.committedUpTo + 1) is not None and \
                self.get(self.committedUpTo + 1).Status == COMMITTED:
            self.committedUpTo += 1

    # ---- handleCommit / handleCommitShort: the two texts are the same ----
    def handleCommit(self, commit):                             # :856-883 / :522-549
        inst = self.get(commit.Instance)
        if inst is None:
            self.counts["nil_install"] += 1
            self.put(commit.Instance, Instance(commit.Command, commit.Ballot, COMMITTED, None))
        else:
            inst.Cmds = commit.Command
            inst.Status = COMMITTED
            inst.Ballot = commit.Ballot
            self._requeue(inst)
        self.updateCommittedUpTo()
        self.recordInstanceMetadata(self.get(commit.Instance), commit.Instance)
        self.recordCommands(commit.Command)

    def handleCommitShort(self, commit):                        # :885-910 / :551-575
        inst = self.get(commit.Instance)
        if inst is None:
            self.put(commit.Instance, Instance(None, commit.Ballot, COMMITTED, None))
        else:
            inst.Status = COMMITTED
            inst.Ballot = commit.Ballot
            self._requeue(inst)
        self.updateCommittedUpTo()
        self.recordInstanceMetadata(self.get(commit.Instance), commit.Instance)

    # ---- executeCommands: one pass of the inner loop ----
    def executeCommands(self):                                  # :1071-1091 / :680-699
        i = self.executed
        while i <= self.committedUpTo:
            inst = self.deref(i)
            if inst.Cmds is None:                               # :1072 / :681
                break
            for j in range(len(inst.Cmds)):
                if inst.Cmds[j][0] == GET and inst.Cmds[j][1] in self.State:
                    self.counts["get_hits"] += 1
                val = execute(inst.Cmds[j], self.State)         # :1075 / :684
                if self.Dreply and inst.Lb is not None and inst.Lb.ClientProposals is not None:
                    p = inst.Lb.ClientProposals[j]
                    self.ReplyProposeTS(self._reply(TRUE, p.CommandId, val, p.Timestamp), p.Reply)
            i += 1
        self.executed = i


# ---- the wire ---------------------------------------------------------------------------------------
def marshal(mode, msg):
    """SendMsg (genericsmr.go:499-512): the code byte, then the message's Marshal"""
    if isinstance(msg, Accept):
        if mode == MIN:
            return P.send_msg(P.ACCEPT_RPC, P.accept_marshal_min(
                msg.LeaderId, msg.Instance, msg.Ballot, msg.LastCommitted, msg.Command, msg.CatchUpLog))
        return P.send_msg(P.ACCEPT_RPC, P.accept_marshal_classic(
            msg.LeaderId, msg.Instance, msg.Ballot, msg.Command))
    if isinstance(msg, AcceptReply):
        return W.accept_reply(mode, msg.Instance, msg.OK, msg.Ballot, msg.Id)
    if isinstance(msg, Commit):
        return W.commit(msg.LeaderId, msg.Instance, msg.Ballot, msg.Command)
    if isinstance(msg, CommitShort):                            # :710-735 / :465-490
        return bytes([R.PEER_COMMIT_SHORT]) + struct.pack("<iiii", msg.LeaderId, msg.Instance,
                                                          msg.Count, msg.Ballot)
    raise TypeError(msg)


def parse(mode, buf):
    """replicaListener (genericsmr.go:402-446) over a connection's bytes: [(offset, message)]"""
    buf = bytes(buf)
    pos, out = 0, []
    while pos < len(buf):
        code = buf[pos]
        if code in (R.PEER_ACCEPT, R.PEER_COMMIT):
            _, m, end = U.unmarshal(mode, buf, pos)
            if code == R.PEER_ACCEPT:
                msg = Accept(m["LeaderId"], m["Instance"], m["Ballot"], m["Command"],
                             m.get("LastCommitted"), m.get("CatchUpLog"))
            else:
                msg = Commit(m["LeaderId"], m["Instance"], m["Ballot"], m["Command"])
        elif code == R.PEER_ACCEPT_REPLY:
            if mode == MIN:                                     # minpaxosprotomarsh.go:568-580
                i, ok, b, rid = struct.unpack_from("<iBii", buf, pos + 1)
                end = pos + 14
            else:                                               # paxosprotomarsh.go:324-335
                i, ok, b = struct.unpack_from("<iBi", buf, pos + 1)
                rid, end = 0, pos + 10
            msg = AcceptReply(i, ok, b, rid)
        elif code == R.PEER_COMMIT_SHORT:                       # :737-749 / :492-503
            lid, i, cnt, b = struct.unpack_from("<iiii", buf, pos + 1)
            msg, end = CommitShort(lid, i, cnt, b), pos + 17
        else:
            raise ValueError(f"frame code {code} at {pos}")
        out.append((pos, msg))
        pos = end
    return out


# ---- the scheduler -----------------------------------------------------------------------------------
def default_ballot(g, N):
    """makeUniqueBallot(1) of the group's leader (bareminpaxos.go:383 / paxos.go:255)"""
    return (1 << 4) | (g % N)


class Cluster:
    """G reference clusters of N replicas; process p holds replica p of every cluster and leads
    the groups g % N == p. clients: [(replica, group)], replica r's connections being those that
    name it, in list order (a scenario keeps them sorted by group); a connection's index among
    them is the Reply handle its proposals carry."""

    def __init__(self, mode, N, G, ipg, clients, hold=None, inst_base=0, thrifty=False,
                 dreply=False, durable=True):
        self.mode, self.N, self.G, self.ipg, self.inst_base = mode, N, G, ipg, inst_base
        self.sink = [[] for _ in range(N)]
        self.store = [bytearray() for _ in range(N)]
        self.rep = [[Replica(mode, N, r, g % N, inst_base + g * ipg, ipg, default_ballot(g, N),
                             thrifty, dreply, durable, self.sink[r], self.store[r])
                     for r in range(N)] for g in range(G)]
        self.conns = [[g for (r2, g) in clients if r2 == r] for r in range(N)]
        self.hold = hold
        self.turn = 0
        self.wire = {k: {(p, q): bytearray() for p in range(N) for q in range(N) if p != q}
                     for k in KINDS}
        self.mark = [0] * N
        self.proposed = []      # (turn, replica, connection, group, command_id) as read

    def group_of(self, inst):
        g = (inst - self.inst_base) // self.ipg
        if not 0 <= g < self.G:
            raise GoPanic(R.E_NIL_INSTANCE, f"instance {inst} belongs to no group")
        return g

    def held(self, p, q):
        return self.hold is not None and bool(self.hold[self.turn][p][q])

    def _flush(self, r, log, station):
        """what replica r's handlers wrote at this station, marshalled onto its connections in
        call order, and the bytes they appended to its file"""
        for kind, dest, msg in self.sink[r]:
            if kind == "client":
                log["client"][station].setdefault((r, dest), bytearray()).extend(msg.Marshal())
            else:
                b = marshal(self.mode, msg)
                self.wire[kind][(r, dest)] += b
                log[kind].setdefault((r, dest), bytearray()).extend(b)
        del self.sink[r][:]
        log["durable"][station][r] = bytes(self.store[r][self.mark[r]:])
        self.mark[r] = len(self.store[r])

    def _read(self, r, kind, log):
        """replica r's inbox of `kind` from every delivering connection, in mpx_order_records'
        order: instance, then connection, then stream offset"""
        inbox = []
        for p in range(self.N):
            if p == r or self.held(p, r):
                continue
            buf = bytes(self.wire[kind][(p, r)])
            self.wire[kind][(p, r)] = bytearray()
            log["delivered"][kind][(p, r)] = buf
            inbox += [(msg.Instance, p, off, msg) for off, msg in parse(self.mode, buf)]
        inbox.sort(key=lambda t: t[:3])
        return [t[3] for t in inbox]

    STATIONS = ("propose", "accept", "tally", "commit", "execute")

    def begin(self, client_bytes):
        """open a turn. client_bytes[r][k]: the bytes client connection k of replica r delivers
        (whole Propose frames). Returns the turn's log, which the stations fill: what each put on
        every connection and file, and what every connection delivered."""
        log = {k: {} for k in KINDS}
        log["client"] = {s: {} for s in ("propose", "tally", "execute")}
        log["durable"] = {s: {} for s in self.STATIONS}
        log["delivered"] = {k: {} for k in KINDS}
        log["n_proposals"] = [0] * self.G
        self.log, self.client_bytes = log, client_bytes
        return log

    def station(self, name):
        """one station of the open turn, for every replica"""
        import client_translit
        log = self.log
        for r in range(self.N):
            if name == "propose":                               # 1 proposals
                for k, g in enumerate(self.conns[r]):
                    buf = self.client_bytes[r][k]
                    props, dropped, consumed, _, _ = client_translit.client_listener(buf)
                    assert dropped == 0 and consumed == len(buf)
                    for cid, op, kk, vv, ts in props:
                        self.rep[g][r].ProposeChan.append(Propose(cid, (op, kk, vv), ts, k))
                        self.proposed.append((self.turn, r, k, g, cid))
                    log["n_proposals"][g] += len(props)
                for g in range(self.G):
                    x = self.rep[g][r]
                    while x.ProposeChan:                        # run()'s proposal case
                        x.handlePropose(x.ProposeChan.popleft())
            elif name == "accept":                              # 2 Accepts
                for msg in self._read(r, "accept", log):
                    self.rep[self.group_of(msg.Instance)][r].handleAccept(msg)
            elif name == "tally":                               # 3 AcceptReplies
                for msg in self._read(r, "accept_reply", log):
                    self.rep[self.group_of(msg.Instance)][r].handleAcceptReply(msg)
            elif name == "commit":                              # 4 Commits and CommitShorts
                for msg in self._read(r, "commit", log):
                    x = self.rep[self.group_of(msg.Instance)][r]
                    if isinstance(msg, Commit):
                        x.handleCommit(msg)
                    else:
                        x.handleCommitShort(msg)
            else:                                               # 5 executeCommands
                for g in range(self.G):
                    self.rep[g][r].executeCommands()
            self._flush(r, log, name)

    def end(self):
        self.turn += 1
        return self.log

    def step(self, client_bytes):
        """one whole turn; returns its log"""
        self.begin(client_bytes)
        for name in self.STATIONS:
            self.station(name)
        return self.end()


# ---- the scenarios of the closed-loop tests ---------------------------------------------------------
def _hold(rng, turns, N, p):
    """hold[t][p][q]; the last turn delivers everything, so every instance can finish"""
    h = rng.random((turns, N, N)) < p
    h[-1] = False
    for q in range(N):
        h[:, q, q] = False
    return h


def scenario(case, mode, N, dreply=False, seed=0):
    """The inputs of one closed-loop case: a dict of Cluster's arguments (mode, N, G, ipg, clients,
    hold, thrifty, dreply), `turns` and client_bytes[t][r][k]. Nothing else enters a run.
      steady   G 8, ipg 16, 6 turns, 1-3 clients per group of which some talk to a non-leader, 0-5
               proposals per client and turn, keys disjoint per group and few per group (a GET meets an
               earlier PUT), every op, connections held with probability 0.15
      thrifty  steady with Thrifty
      wave     G 65 (one past a 64-lane wave of groups), ipg 8, 3 turns, one client per group
      batch    G 2, ipg 8, 2 turns: group 0 receives MAX_BATCH + 1 proposals in turn 0, one in turn 1
      window   G 2, ipg 4, 5 turns, one proposal per group and turn: the fifth finds no free slot
      replay   G 2, ipg 8, 3 turns, one proposal per group and turn: replica 2 of 3 leads nothing and
               accepts one command per instance, so its whole durable log is the 29-byte records
               getDataFromStableStore can read back (a leader's decide record, bareminpaxos.go:1045,
               carries no command: the Go cannot replay a leader's file)"""
    rng = np.random.default_rng([seed, N, mode, len(case)])
    G, ipg, turns, p_hold = {"steady": (8, 16, 6, 0.15), "thrifty": (8, 16, 6, 0.15),
                             "wave": (65, 8, 3, 0.1), "batch": (2, 8, 2, 0.0),
                             "window": (2, 4, 5, 0.0), "replay": (2, 8, 3, 0.0)}[case]
    clients = []
    for g in range(G):
        n_c = int(rng.integers(1, 4)) if case in ("steady", "thrifty") else 1
        for c in range(n_c):
            stray = case in ("steady", "thrifty") and c == 1 and g % 2 == 0
            clients.append(((g + 1) % N if stray else g % N, g))
    clients.sort(key=lambda rc: rc[1])                          # a replica's connections: by group
    conns = [[i for i, (r, _) in enumerate(clients) if r == r2] for r2 in range(N)]
    next_id = [1] * len(clients)
    idle = {(2, 3), (4, 5)} if case in ("steady", "thrifty") else set()   # (turn, group)
    ops = [PUT, PUT, PUT, GET, GET, GET, NONE, DELETE, RLOCK, WLOCK]
    client_bytes = []
    for t in range(turns):
        per = [[b"" for _ in conns[r]] for r in range(N)]
        for r in range(N):
            for k, i in enumerate(conns[r]):
                g = clients[i][1]
                lead = r == g % N
                first_of_group = lead and all(clients[j][1] != g or clients[j][0] != r
                                              for j in range(i))
                if case in ("steady", "thrifty"):
                    n = 0 if (t, g) in idle else int(rng.integers(1 if first_of_group else 0, 6))
                elif case == "batch":
                    n = (MAX_BATCH + 1 if t == 0 else 1) if g == 0 else 1
                else:
                    n = 1
                b = bytearray()
                for _ in range(n):
                    op = ops[int(rng.integers(0, len(ops)))]
                    key = g * 1000 + int(rng.integers(0, 4))
                    b += W.propose(next_id[i], op, key, int(rng.integers(1, 1 << 40)),
                                   int(rng.integers(0, 1 << 50)))
                    next_id[i] += 1
                per[r][k] = bytes(b)
        client_bytes.append(per)
    return dict(mode=mode, N=N, G=G, ipg=ipg, clients=clients, hold=_hold(rng, turns, N, p_hold),
                thrifty=case == "thrifty", dreply=dreply, turns=turns, client_bytes=client_bytes)


def cluster_of(sc):
    return Cluster(sc["mode"], sc["N"], sc["G"], sc["ipg"], sc["clients"], sc["hold"],
                   thrifty=sc["thrifty"], dreply=sc["dreply"])


# the cases the GPU test runs; test_cluster_model.py asserts the non-vacuity conditions on each
CASES = ([("steady", m, n, d) for m in (MIN, CLASSIC) for n in (3, 5) for d in (False, True)] +
         [("thrifty", CLASSIC, 5, False), ("wave", MIN, 3, False), ("batch", MIN, 3, True),
          ("batch", CLASSIC, 3, True), ("window", CLASSIC, 3, False), ("replay", MIN, 3, False)])


def case_id(c):
    return f"{c[0]}-{'min' if c[1] == MIN else 'classic'}-n{c[2]}-{'dreply' if c[3] else 'decide'}"


def run_model(sc):
    """every turn of a scenario. Returns (cluster, logs, commit_turns per group, panic): panic is
    None or (turn, GoPanic) where a handler panicked, the turns before it in logs."""
    cl = cluster_of(sc)
    N, G = sc["N"], sc["G"]
    logs, commit_turns, panic = [], [0] * G, None

    def committed(g):
        return [x is not None and x.Status == COMMITTED for x in cl.rep[g][g % N].space]
    for t in range(sc["turns"]):
        before = [committed(g) for g in range(G)]
        try:
            logs.append(cl.step(sc["client_bytes"][t]))
        except GoPanic as e:
            panic = (t, e)
            break
        for g in range(G):
            commit_turns[g] += committed(g) != before[g]
    return cl, logs, commit_turns, panic

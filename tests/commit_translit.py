"""The commit side of Phase 2, transliterated line by line from the Go reference (the single
restatement the commit tests compare against; the oracle does not cover this path).

  handleCommit         MIN      src/bareminpaxos/bareminpaxos.go:856-883
                       CLASSIC  src/paxos/paxos.go:522-549
  handleCommitShort    MIN      src/bareminpaxos/bareminpaxos.go:885-910
                       CLASSIC  src/paxos/paxos.go:551-575
  updateCommittedUpTo           src/paxos/paxos.go:259-264
  bcastCommit          MIN      src/bareminpaxos/bareminpaxos.go:565-615
                       CLASSIC  src/paxos/paxos.go:336-386
  SendMsg              src/genericsmr/genericsmr.go:499-512 (the code byte, then Marshal)
  Commit.Marshal       src/minpaxosproto/minpaxosprotomarsh.go:618-646 / paxosprotomarsh.go:373-401
  CommitShort.Marshal  src/minpaxosproto/minpaxosprotomarsh.go:710-735 / paxosprotomarsh.go:465-490
  CommitShort.Unmarshal  minpaxosprotomarsh.go:737-749 / paxosprotomarsh.go:492-503

The two protocols' handlers, broadcasts and wire formats are the same text, so there is one
transliteration of each (the line numbers cited in the bodies are bareminpaxos.go's).

A group's replica sees its own window of the engine's instance numbers: first = inst_base + g*ipg
stands for the reference's instance 0 and "nothing committed" is first - 1. Indexing instanceSpace
outside [first, first + ipg) is the Go's index-out-of-range panic, with one stated deviation:
updateCommittedUpTo stops at the window's end, where the reference would index the next slot.
"""
import struct

import numpy as np

from go_translit import GoPanic
from minpaxos_amd import records as R
from proposer_translit import command_marshal, put_varint, send_msg

NIL = -1  # MPX_STATUS_NIL
PREPARING, PREPARED, ACCEPTED, COMMITTED = 0, 1, 2, 3
COMMIT_RPC, COMMIT_SHORT_RPC = 10, 11  # the codes RegisterRPC hands commitRPC / commitShortRPC
KEEP = R.VALUE_KEEP


class Instance:
    """Ballot, Status, Lb, Cmds. Cmds is a handle (None: nil); of Lb only `Lb != nil &&
    Lb.ClientProposals != nil` matters: the MPX_PF_HAS_PROPOSALS bit of flags"""

    def __init__(self, ballot, status, flags, cmds):
        self.Ballot, self.Status, self.flags, self.Cmds = ballot, status, flags, cmds


class Replica:
    """the fields the commit handlers read, for one group"""

    def __init__(self, first, ipg, st_rows, committed_upto):
        self.first, self.ipg = first, ipg
        self.instanceSpace = [None if int(s["status"]) == NIL else
                              Instance(int(s["ballot"]), int(s["status"]), int(s["flags"]),
                                       None if int(s["value_id"]) == KEEP else int(s["value_id"]))
                              for s in st_rows]
        self.committedUpTo = committed_upto
        self.requeued = []  # instances whose clientProposals went back on ProposeChan

    def space(self, i):
        if i < self.first or i >= self.first + self.ipg:
            raise GoPanic(R.E_NIL_INSTANCE, f"instanceSpace[{i}] out of range")
        return i - self.first

    def get(self, i):
        return self.instanceSpace[self.space(i)]

    def rows(self):
        out = np.zeros(self.ipg, R.ACCEPTOR_STATE)
        for k, x in enumerate(self.instanceSpace):
            out[k] = (NIL, 0, 0, 0) if x is None else \
                (x.Status, x.Ballot, KEEP if x.Cmds is None else x.Cmds, x.flags)
        return out


def update_committed_upto(r):                                             # paxos.go:259-264
    while r.committedUpTo + 1 < r.first + r.ipg and \
            r.get(r.committedUpTo + 1) is not None and \
            r.get(r.committedUpTo + 1).Status == COMMITTED:               # :260-261
        r.committedUpTo += 1                                              # :262


def _requeue(r, inst, instance, out):
    if inst.flags & R.PF_HAS_PROPOSALS:                                   # :871 / :899
        r.requeued.append(instance)                                       # :872-874
        inst.flags = (inst.flags & ~R.PF_HAS_PROPOSALS) | R.PF_REQUEUED   # :875 (= nil)
        out["branch"].append("requeue")
        return R.CH_REQUEUE
    return 0


def handle_commit(r, instance, ballot, command, out, per_message=True):
    """bareminpaxos.go:856-883; command: the handle of commit.Command"""
    inst = r.get(instance)                                                # :857
    if inst is None:                                                      # :861
        r.instanceSpace[r.space(instance)] = Instance(ballot, COMMITTED, 0, command)  # :862-866
        eff = R.CH_INSTALLED | R.CH_CMDS
        out["branch"].append("nil_commit")
    else:
        inst.Cmds = command                                               # :868
        inst.Status = COMMITTED                                           # :869
        inst.Ballot = ballot                                              # :870
        eff = R.CH_CMDS | _requeue(r, inst, instance, out)                # :871-876
        out["branch"].append("commit")
    if per_message:
        update_committed_upto(r)                                          # :879
    x = r.get(instance)
    out["log"].append((x.Ballot, x.Status, instance, 0))                  # :881 recordInstanceMetadata
    out["effect"].append(eff)                                             # :882 recordCommands: host


def handle_commit_short(r, instance, ballot, out, per_message=True):
    """bareminpaxos.go:885-910"""
    inst = r.get(instance)                                                # :886
    if inst is None:                                                      # :890
        r.instanceSpace[r.space(instance)] = Instance(ballot, COMMITTED, 0, None)  # :891-895
        eff = R.CH_INSTALLED
        out["branch"].append("nil_short")
    else:
        inst.Status = COMMITTED                                           # :897
        inst.Ballot = ballot                                              # :898
        eff = _requeue(r, inst, instance, out)                            # :899-904
        out["branch"].append("short")
    if per_message:
        update_committed_upto(r)                                          # :907
    x = r.get(instance)
    out["log"].append((x.Ballot, x.Status, instance, 0))                  # :909
    out["effect"].append(eff)


def commit_handle(msgs, st, committed_upto, inst_base=0, ipg=None, per_message=True,
                  want_branches=False):
    """the handlers over a batch in array order (a message with value_id KEEP is a CommitShort).
    per_message=False: updateCommittedUpTo once per touched group after the last message instead
    of after every message (the form the engine computes). Returns (st, committed_upto, effect,
    log_recs[, branches])."""
    cu = np.array(np.atleast_1d(committed_upto), np.int32)
    G = len(cu)
    ipg = len(st) // G if ipg is None else ipg
    n_inst = G * ipg
    reps = {}
    out = {"branch": [], "log": [], "effect": []}
    prev = None
    for m in msgs:
        instance = int(m["instance"])
        idx = instance - inst_base
        if idx < 0 or idx >= n_inst:
            raise GoPanic(R.E_NIL_INSTANCE, f"instanceSpace[{instance}] out of range")
        if prev is not None and instance < prev:
            raise GoPanic(R.E_INVAL, "descending instances")
        prev = instance
        g = idx // ipg
        if g not in reps:
            first = inst_base + g * ipg
            if not first - 1 <= int(cu[g]) <= first + ipg - 1:
                raise GoPanic(R.E_INVAL, "committed_upto outside its window")
            reps[g] = Replica(first, ipg, st[g * ipg:(g + 1) * ipg], int(cu[g]))
        r = reps[g]
        if int(m["value_id"]) == KEEP:
            handle_commit_short(r, instance, int(m["ballot"]), out, per_message)
        else:
            handle_commit(r, instance, int(m["ballot"]), int(m["value_id"]), out, per_message)
    st2 = np.array(st, R.ACCEPTOR_STATE, copy=True)
    for g, r in reps.items():
        if not per_message:
            update_committed_upto(r)
        st2[g * ipg:(g + 1) * ipg] = r.rows()
        cu[g] = r.committedUpTo
    eff = np.array(out["effect"], np.uint8)
    log = np.zeros(len(msgs), R.LOG_REC)
    for i, row in enumerate(out["log"]):
        log[i] = row
    res = (st2, cu, eff, log)
    return res + (out["branch"],) if want_branches else res


# ---- the Marshals ---------------------------------------------------------------------------------
def commit_marshal(leader, inst, ballot, cmds):       # minpaxosprotomarsh.go:618-646
    return (struct.pack("<i", leader) + struct.pack("<i", inst) + struct.pack("<i", ballot) +
            put_varint(len(cmds)) + b"".join(command_marshal(*c) for c in cmds))


def commit_short_marshal(leader, inst, count, ballot):  # minpaxosprotomarsh.go:710-735
    return (struct.pack("<i", leader) + struct.pack("<i", inst) + struct.pack("<i", count) +
            struct.pack("<i", ballot))


def commit_short_unmarshal(bs):                         # minpaxosprotomarsh.go:737-749
    """-> (LeaderId, Instance, Count, Ballot)"""
    return struct.unpack("<iiii", bytes(bs[:16]))


# ---- bcastCommit ----------------------------------------------------------------------------------
def bcast_commit(N, Id, thrifty, alive, instance, ballot, command, loops=None):
    """bareminpaxos.go:565-615; alive: list of bool. Returns [(q, frame bytes)] in send order;
    loops (optional): a 2-list counting the sends of each loop."""
    sent_to = []
    short = commit_short_marshal(Id, instance, len(command), ballot)       # :576-580
    n = N - 1                                                              # :584
    if thrifty:
        n = N >> 1                                                         # :586
    q = Id
    sent = 0
    while sent < n:                                                        # :591
        q = (q + 1) % N
        if q == Id:
            break
        if not alive[q]:                                                   # :596
            continue
        sent += 1
        sent_to.append((q, send_msg(COMMIT_SHORT_RPC, short)))             # :600
        if loops is not None:
            loops[0] += 1
    if thrifty and q != Id:                                                # :602
        full = commit_marshal(Id, instance, ballot, command)               # :571-575
        while sent < N - 1:                                                # :603
            q = (q + 1) % N
            if q == Id:
                break
            if not alive[q]:                                               # :608
                continue
            sent += 1
            sent_to.append((q, send_msg(COMMIT_RPC, full)))                # :612
            if loops is not None:
                loops[1] += 1
    return sent_to


def encode_commits(N, sends, groups, cmds, inst_base=0, ipg=1, thrifty=False, alive_mask=0xFFFF,
                   want_frames=False, loops=None):
    """bcastCommit for every MPX_CS_SEND slot, in array order; what each peer's connection then
    holds. Returns (bytes uint8, dest_off u64[N+1]) [and per destination the list of frames]."""
    groups = np.atleast_1d(groups)
    n_inst = len(groups) * ipg
    op, key, val = cmds
    alive = [(alive_mask >> q) & 1 == 1 for q in range(N)]
    per = [[] for _ in range(N)]
    for s in sends:
        if not int(s["flags"]) & R.CS_SEND:
            continue
        inst = int(s["instance"])
        idx = inst - inst_base
        if idx < 0 or idx >= n_inst:
            raise GoPanic(R.E_INVAL, "send outside the window")
        c0, nc = int(s["first_cmd"]), int(s["n_cmds"])
        if c0 > len(op) or nc > len(op) - c0:
            raise GoPanic(R.E_INVAL, "commands outside the arrays")
        Id = int(groups[idx // ipg]["self_id"])
        if not 0 <= Id < N:
            raise GoPanic(R.E_INVAL, "self_id")
        command = [(int(op[j]), int(key[j]), int(val[j])) for j in range(c0, c0 + nc)]
        for q, b in bcast_commit(N, Id, thrifty, alive, inst, int(s["ballot"]), command, loops):
            per[q].append(b)
    dest_off = np.zeros(N + 1, np.uint64)
    for q in range(N):
        dest_off[q + 1] = int(dest_off[q]) + sum(len(b) for b in per[q])
    by = np.frombuffer(b"".join(b"".join(x) for x in per), np.uint8)
    return (by, dest_off, per) if want_frames else (by, dest_off)


def gather_commit_shorts(buf, other):
    """CommitShort.Unmarshal on every code-11 frame of `other`, in order. Returns (msgs ACCEPT_MSG,
    count int32, frame_index uint32)."""
    buf = bytes(buf)
    rows, cnt, idx = [], [], []
    for i, f in enumerate(other):
        if int(f["code"]) != COMMIT_SHORT_RPC:
            continue
        o = int(f["offset"])
        if o + 17 > len(buf):
            raise GoPanic(R.E_INVAL, "frame outside the buffer")
        leader, inst, count, ballot = commit_short_unmarshal(buf[o + 1:o + 17])
        rows.append((inst, ballot, leader, KEEP))
        cnt.append(count)
        idx.append(i)
    return mk_msgs(rows), np.array(cnt, np.int32), np.array(idx, np.uint32)


# ---- builders -------------------------------------------------------------------------------------
def mk_msgs(rows):
    """rows of (instance, ballot, leader_id, value_id)"""
    m = np.zeros(len(rows), R.ACCEPT_MSG)
    for i, row in enumerate(rows):
        m[i] = row
    return m


def mk_commit_sends(rows):
    """rows of (instance, ballot, first_cmd, n_cmds, flags)"""
    s = np.zeros(len(rows), R.COMMIT_SEND)
    for i, row in enumerate(rows):
        s[i] = tuple(row) + ((0, 0),)
    return s


def mk_self(ids):
    """PROPOSER_GROUP rows of which only self_id matters"""
    g = np.zeros(len(ids), R.PROPOSER_GROUP)
    g["self_id"] = ids
    g["leader"] = ids
    return g


# ---- the fuzz generators --------------------------------------------------------------------------
FUZZ_SEEDS = list(range(24))
BRANCHES = ("nil_commit", "nil_short", "commit", "short", "requeue")


def fuzz_commit(seed):
    """-> dict(msgs, st, committed_upto, inst_base, ipg): a few groups, some untouched, a committed
    prefix per group with committed_upto somewhere inside it, one to three messages on about
    half of the instances, half of them CommitShorts"""
    rng = np.random.default_rng(1000 + seed)
    G = int(rng.integers(1, 7))
    ipg = int(rng.choice([1, 3, 8, 40, 70]))
    base = int(rng.integers(-50, 1000))
    st = np.zeros(G * ipg, R.ACCEPTOR_STATE)
    st["status"] = np.where(rng.random(G * ipg) < 0.45, NIL, rng.integers(0, 4, G * ipg))
    live = st["status"] != NIL
    st["ballot"] = np.where(live, rng.integers(0, 1 << 10, G * ipg), 0)
    st["value_id"] = np.where(live, rng.integers(0, 1 << 20, G * ipg), 0)
    st["flags"] = np.where(live & (rng.random(G * ipg) < 0.4), R.PF_HAS_PROPOSALS, 0)
    cu = np.zeros(G, np.int32)
    rows = []
    for g in range(G):
        first = base + g * ipg
        p = int(rng.integers(0, ipg + 1)) if rng.random() < 0.7 else 0
        st["status"][g * ipg:g * ipg + p] = COMMITTED
        cu[g] = first - 1 + int(rng.integers(0, p + 1))
        if G > 1 and rng.random() < 0.25:
            continue  # an untouched group
        for k in range(ipg):
            if rng.random() < 0.5:
                for _ in range(int(rng.choice([1, 1, 2, 3]))):
                    short = rng.random() < 0.5
                    rows.append((first + k, int(rng.integers(0, 1 << 10)), int(rng.integers(0, 5)),
                                 KEEP if short else int(rng.integers(0, 1 << 20))))
    return dict(msgs=mk_msgs(rows), st=st, committed_upto=cu, inst_base=base, ipg=ipg)


def fuzz_bcast(seed, N):
    """-> kwargs of encode_commits: groups led by differing replicas, a third of the calls thrifty,
    random alive masks, some skipped slots, 0 to 70 commands per send"""
    rng = np.random.default_rng(2000 + seed)
    G = int(rng.integers(1, 9))
    ipg = int(rng.integers(1, 6))
    base = int(rng.integers(-20, 500))
    ids = rng.integers(0, N, G)
    rows, c0 = [], 0
    for idx in sorted(rng.choice(G * ipg, int(rng.integers(1, G * ipg + 1)), replace=False)):
        nc = int(rng.choice([0, 1, 2, 5, 63, 64, 70]))
        rows.append((base + int(idx), int(rng.integers(0, 1 << 12)), c0, nc,
                     R.CS_SEND if rng.random() < 0.85 else 0))
        c0 += nc
    from proposer_translit import mk_cmds
    alive = int(rng.integers(0, 1 << N)) if rng.random() < 0.6 else (1 << N) - 1
    return dict(sends=mk_commit_sends(rows), groups=mk_self(ids), cmds=mk_cmds(rng, c0),
                inst_base=base, ipg=ipg, thrifty=bool(seed % 3 != 0), alive_mask=alive)


def mixed_stream(seed, mode, n_frames, p_short=0.5):
    """a peer stream of CommitShorts among Beacons, AcceptReplies and full Commits (all fixed-size
    or self-describing under both framings). Returns (bytes, n_shorts)."""
    rng = np.random.default_rng(3000 + seed)
    ar_body = 13 if mode == R.MODE_MIN else 9
    out, ns = [], 0
    for _ in range(n_frames):
        x = rng.random()
        if x < p_short:
            out.append(send_msg(COMMIT_SHORT_RPC, commit_short_marshal(
                int(rng.integers(0, 5)), int(rng.integers(-5, 1 << 30)),
                int(rng.integers(0, 5001)), int(rng.integers(0, 1 << 30)))))
            ns += 1
        elif x < p_short + 0.2:
            out.append(bytes([6]) + rng.integers(0, 256, 8).astype(np.uint8).tobytes())
        elif x < p_short + 0.4:
            out.append(bytes([13]) + rng.integers(0, 256, ar_body).astype(np.uint8).tobytes())
        else:
            k = int(rng.integers(0, 4))
            cmds = [(int(rng.integers(0, 4)), int(rng.integers(-9, 9)), int(rng.integers(-9, 9)))
                    for _ in range(k)]
            out.append(send_msg(COMMIT_RPC, commit_marshal(1, int(rng.integers(0, 99)), 7, cmds)))
    return b"".join(out), ns

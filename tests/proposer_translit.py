"""The proposer's half of Phase 2, transliterated line by line from the Go reference (the single
restatement the proposer tests compare against; the oracle does not cover this path).

  handlePropose  MIN      src/bareminpaxos/bareminpaxos.go:617-710
                 CLASSIC  src/paxos/paxos.go:388-443
  bcastAccept    MIN      src/bareminpaxos/bareminpaxos.go:450-520
                 CLASSIC  src/paxos/paxos.go:299-331
  SendMsg        src/genericsmr/genericsmr.go:499-512 (the code byte, then Marshal)
  Accept.Marshal MIN      src/minpaxosproto/minpaxosprotomarsh.go:425-468
                 CLASSIC  src/paxosproto/paxosprotomarsh.go:214-242
  Instance.Marshal        src/minpaxosproto/minpaxosprotomarsh.go:100-124
  Command.Marshal         src/state/statemarsh.go:8-19

A group's replica sees its own window of the engine's instance numbers: first = inst_base + g*ipg
stands for the reference's instance 0, so `< 0` tests of the Go read `< first` here, and indexing
instanceSpace outside [first, first + ipg) is the Go's index-out-of-range panic.
"""
import struct

import numpy as np

from go_translit import GoPanic
from minpaxos_amd import records as R

MAX_BATCH = 5000  # bareminpaxos.go:22 / paxos.go:20
NIL = -1          # MPX_STATUS_NIL
PREPARING, PREPARED, ACCEPTED, COMMITTED = 0, 1, 2, 3
ACCEPT_RPC = 9    # the code RegisterRPC hands acceptRPC (MPX_PEER_ACCEPT)


class Replica:
    """the fields handlePropose and bcastAccept read, for one group"""

    def __init__(self, N, grp, first, ipg, st, lb=None, thrifty=False, alive=0xFFFF,
                 peer_commits=None):
        self.N, self.first, self.ipg = N, first, ipg
        self.Id, self.Leader = int(grp["self_id"]), int(grp["leader"])
        self.IsLeader = self.Leader == self.Id
        self.prepareOKs = int(grp["prepare_oks"])
        self.defaultBallot = int(grp["default_ballot"])
        self.crtInstance = int(grp["crt_instance"])
        self.committedUpTo = int(grp["committed_upto"])
        self.st, self.lb = st, lb  # views of the group's window
        self.Thrifty = thrifty
        self.Alive = [(alive >> q) & 1 == 1 for q in range(N)]
        self.peerCommits = peer_commits

    def space(self, i):
        """r.instanceSpace[i]: the window index, or the index panic"""
        if i < self.first or i >= self.first + self.ipg:
            raise GoPanic(R.E_NIL_INSTANCE, f"instanceSpace[{i}] out of range")
        return i - self.first

    def is_nil(self, i):
        return int(self.st["status"][self.space(i)]) == NIL

    def install(self, i, ballot, status, value_id):
        k = self.space(i)
        self.st[k] = (status, ballot, value_id & 0xFFFFFFFF, R.PF_HAS_PROPOSALS)
        if self.lb is not None:
            self.lb[k] = (status, 0, 0, 0)  # &LeaderBookkeeping{0, 0, 0, proposals}

    def make_unique_ballot(self, ballot):
        return (ballot << 4) | self.Id


def handle_propose_min(r, chan_len, head, out):
    """bareminpaxos.go:617-710. chan_len = len(r.ProposeChan) when the handler runs, head = the
    index of `propose`. Returns how many queued proposals it took besides the head."""
    if r.Leader != r.Id or r.prepareOKs <= r.N >> 1:                       # :618
        out["branch"].append("not_leader_id" if r.Leader != r.Id else "not_leader_oks")
        out["false"].append(head)                                          # :622-623
        out["event"].append((R.PH_NOT_LEADER, -1, 0, 0, head, 1))
        return 0                                                           # :624
    adv = 0
    while not r.is_nil(r.crtInstance):                                     # :627
        r.crtInstance += 1                                                 # :629
        adv += 1
    if adv:
        out["branch"].append("advance")
    instNo = r.crtInstance                                                 # :632
    batchSize = chan_len + 1                                               # :634
    if batchSize > MAX_BATCH:                                              # :636
        batchSize = MAX_BATCH
    # :642-651: cmds / proposals = the head and the next batchSize-1 of the channel
    if r.committedUpTo < instNo - 1:                                       # :671
        out["branch"].append("refused")
        out["false"].append(head)                                          # :682-683
        out["event"].append((R.PH_REFUSED, instNo, r.defaultBallot, r.committedUpTo, head,
                             batchSize))
        return batchSize - 1                                               # :684
    if r.Leader == r.Id:                                                   # :687
        r.crtInstance += 1                                                 # :688
        if r.prepareOKs > r.N >> 1:                                        # :689
            out["branch"].append("accept")
            r.install(instNo, r.defaultBallot, PREPARED, head)             # :691-695
            # :697-699 recordInstanceMetadata, recordCommands, sync: the host
            # :702 bcastAccept(instNo, r.defaultBallot, r.committedUpTo, cmds, peerCommits)
            out["event"].append((R.PH_ACCEPT, instNo, r.defaultBallot, r.committedUpTo, head,
                                 batchSize))
    return batchSize - 1


def handle_propose_classic(r, chan_len, head, out):
    """paxos.go:388-443"""
    if not r.IsLeader:                                                     # :389
        out["branch"].append("not_leader")
        out["false"].append(head)                                          # :390-391
        out["event"].append((R.PH_NOT_LEADER, -1, 0, 0, head, 1))
        return 0
    adv = 0
    while not r.is_nil(r.crtInstance):                                     # :395
        r.crtInstance += 1
        adv += 1
    if adv:
        out["branch"].append("advance")
    instNo = r.crtInstance                                                 # :399
    r.crtInstance += 1                                                     # :400
    batchSize = chan_len + 1                                               # :402
    if batchSize > MAX_BATCH:
        batchSize = MAX_BATCH
    if r.defaultBallot == -1:                                              # :421
        out["branch"].append("prepare")
        b = r.make_unique_ballot(0)
        r.install(instNo, b, PREPARING, head)                              # :422-426
        out["event"].append((R.PH_PREPARE, instNo, b, r.committedUpTo, head, batchSize))  # :427
    else:
        out["branch"].append("accept")
        r.install(instNo, r.defaultBallot, PREPARED, head)                 # :430-434
        out["event"].append((R.PH_ACCEPT, instNo, r.defaultBallot, r.committedUpTo, head,
                             batchSize))                                   # :440
    return batchSize - 1


def propose_handle(mode, N, groups, prop_off, st, inst_base=0, ipg=None, lb=None,
                   want_branches=False):
    """run()'s proposal case (bareminpaxos.go:296-307) until every group's channel is empty.
    Returns (groups, st, lb, sends, send_off, false_replies[, branches]): sends in the engine's
    slot layout (the NOT_LEADER calls of a slot's proposals merged into the slot), false_replies
    the proposal indices answered FALSE in order."""
    groups = np.array(np.atleast_1d(groups), dtype=R.PROPOSER_GROUP, copy=True)
    st = np.array(st, dtype=R.ACCEPTOR_STATE, copy=True)
    lb = None if lb is None else np.array(lb, dtype=R.INST_STATE, copy=True)
    G = len(groups)
    ipg = (len(st) // G if G else 0) if ipg is None else ipg
    handler = handle_propose_min if mode == R.MODE_MIN else handle_propose_classic
    send_off = np.zeros(G + 1, np.uint64)
    sends, falses, branches = [], [], []
    for g in range(G):
        p0, p1 = int(prop_off[g]), int(prop_off[g + 1])
        w = slice(g * ipg, (g + 1) * ipg)
        r = Replica(N, groups[g], inst_base + g * ipg, ipg, st[w], None if lb is None else lb[w])
        out = {"branch": [], "false": [], "event": []}
        head = p0
        while head < p1:
            took = handler(r, p1 - head - 1, head, out)
            head += 1 + took
        groups[g]["crt_instance"] = r.crtInstance
        # slots: one per MAX_BATCH proposals of the group
        ev = out["event"]
        k = 0
        for b in range(-(-(p1 - p0) // MAX_BATCH)):
            fc = p0 + b * MAX_BATCH
            nc = min(MAX_BATCH, p1 - fc)
            flags, inst, ballot, lc, first, n = ev[k]
            assert first == fc
            if flags == R.PH_NOT_LEADER:  # nc single-proposal calls
                assert all(e[0] == R.PH_NOT_LEADER for e in ev[k:k + nc])
                k += nc
            else:
                assert n == nc
                k += 1
            sends.append((inst, ballot, lc, flags, fc, nc, 0))
        assert k == len(ev)
        send_off[g + 1] = len(sends)
        falses += out["false"]
        branches.append(out["branch"])
    sends = np.array(sends, dtype=R.ACCEPT_SEND) if sends else np.zeros(0, R.ACCEPT_SEND)
    res = (groups, st, lb, sends, send_off, np.array(falses, np.int64))
    return res + (branches,) if want_branches else res


# ---- Marshal -------------------------------------------------------------------------------------
def put_varint(x):
    """encoding/binary.PutVarint"""
    ux = (x << 1) & 0xFFFFFFFFFFFFFFFF
    if x < 0:
        ux ^= 0xFFFFFFFFFFFFFFFF
    b = bytearray()
    while ux >= 0x80:
        b.append((ux & 0x7F) | 0x80)
        ux >>= 7
    b.append(ux)
    return bytes(b)


def command_marshal(op, k, v):                        # statemarsh.go:8-19
    return struct.pack("<B", op) + struct.pack("<q", k) + struct.pack("<q", v)


def instance_marshal(ballot, status, cmds):           # minpaxosprotomarsh.go:100-124
    return (struct.pack("<i", ballot) + struct.pack("<i", status) + put_varint(len(cmds)) +
            b"".join(command_marshal(*c) for c in cmds))


def accept_marshal_min(leader, inst, ballot, lc, cmds, log):   # minpaxosprotomarsh.go:425-468
    return (struct.pack("<i", leader) + struct.pack("<i", inst) + struct.pack("<i", ballot) +
            struct.pack("<i", lc) + put_varint(len(cmds)) +
            b"".join(command_marshal(*c) for c in cmds) + put_varint(len(log)) +
            b"".join(instance_marshal(*x) for x in log))


def accept_marshal_classic(leader, inst, ballot, cmds):        # paxosprotomarsh.go:214-242
    return (struct.pack("<i", leader) + struct.pack("<i", inst) + struct.pack("<i", ballot) +
            put_varint(len(cmds)) + b"".join(command_marshal(*c) for c in cmds))


def send_msg(code, body):                             # genericsmr.go:499-512
    return bytes([code]) + body


# ---- bcastAccept ---------------------------------------------------------------------------------
def bcast_accept_min(r, instance, ballot, lastcommitted, command, log_inst, note=None):
    """bareminpaxos.go:450-520. log_inst(i) -> (ballot, status, cmds) of *r.instanceSpace[i], or
    the nil dereference. Returns [(q, bytes)] in send order."""
    sent_to = []
    n = r.N - 1                                                            # :465
    if r.Thrifty:
        n = r.N >> 1                                                       # :467
    q = r.Id
    sent = 0
    while sent < n:                                                        # :471
        q = (q + 1) % r.N                                                  # :472
        if q == r.Id:                                                      # :473
            break
        # :476-480 a dead peer is reconnected, and counted either way
        sent += 1                                                          # :482
        partiallog = []
        if r.peerCommits[q] < r.first and r.crtInstance >= r.first:        # :496
            i = r.first
            while i <= lastcommitted:                                      # :498
                partiallog.append(log_inst(i))
                i += 1
            kind = "from_first"
        elif r.crtInstance >= r.first:                                     # :502
            i = r.peerCommits[q] + 1
            while i <= lastcommitted:                                      # :504
                partiallog.append(log_inst(i))
                i += 1
            kind = "from_pc"
        else:
            partiallog = []                                                # :508
            kind = "none"
        if note is not None:
            note.append((kind, len(partiallog)))
        sent_to.append((q, send_msg(ACCEPT_RPC, accept_marshal_min(     # :515
            r.Id, instance, ballot, lastcommitted, command, partiallog))))
    return sent_to


def bcast_accept_classic(r, instance, ballot, command):
    """paxos.go:299-331"""
    sent_to = []
    n = r.N - 1
    if r.Thrifty:
        n = r.N >> 1
    q = r.Id
    sent = 0
    while sent < n:                                                        # :318
        q = (q + 1) % r.N
        if q == r.Id:
            break
        if not r.Alive[q]:                                                 # :323
            continue
        sent += 1
        sent_to.append((q, send_msg(ACCEPT_RPC, accept_marshal_classic(
            r.Id, instance, ballot, command))))                            # :329
    return sent_to


def encode_accepts(mode, N, sends, groups, cmds, inst_base=0, ipg=None, peer_commits=None,
                   log=None, thrifty=False, alive_mask=0xFFFF, note=None, want_frames=False):
    """bcastAccept for every MPX_PH_ACCEPT slot, in array order; what each peer's connection then
    holds. Returns (bytes uint8, dest_off u64[N+1]) [and per destination the list of frames]."""
    groups = np.atleast_1d(groups)
    G = len(groups)
    op, key, val = cmds
    if log is not None:
        lrec, lcoff, lop, lkey, lval = log
        n_inst = len(lrec)
    if ipg is None:
        ipg = n_inst // G
    n_inst = G * ipg
    per = [[] for _ in range(N)]
    for s in sends:
        if not int(s["flags"]) & R.PH_ACCEPT:
            continue
        inst = int(s["instance"])
        idx = inst - inst_base
        if idx < 0 or idx >= n_inst:
            raise GoPanic(R.E_INVAL, "send outside the window")
        g = idx // ipg
        first = inst_base + g * ipg
        c0, nc = int(s["first_cmd"]), int(s["n_cmds"])
        command = [(int(op[j]), int(key[j]), int(val[j])) for j in range(c0, c0 + nc)]
        grp = groups[g]
        if not 0 <= int(grp["self_id"]) < N:
            raise GoPanic(R.E_INVAL, "self_id")
        r = Replica(N, grp, first, ipg, None, thrifty=thrifty, alive=alive_mask,
                    peer_commits=None if peer_commits is None else
                    [int(x) for x in np.asarray(peer_commits).reshape(G, N)[g]])
        r.crtInstance = inst + 1  # handlePropose has advanced it past instNo (:688)
        if mode == R.MODE_MIN:
            lc = int(s["last_committed"])
            if lc >= inst or lc < first - 1:
                raise GoPanic(R.E_INVAL, "last_committed")

            def log_inst(i):
                k = r.space(i) + g * ipg
                if int(lrec[k]["status"]) == NIL:
                    raise GoPanic(R.E_NIL_INSTANCE, f"*r.instanceSpace[{i}] is nil")
                a, b = int(lcoff[k]), int(lcoff[k + 1])
                return (int(lrec[k]["ballot"]), int(lrec[k]["status"]),
                        [(int(lop[j]), int(lkey[j]), int(lval[j])) for j in range(a, b)])
            out = bcast_accept_min(r, inst, int(s["ballot"]), lc, command, log_inst, note)
        else:
            out = bcast_accept_classic(r, inst, int(s["ballot"]), command)
        for q, b in out:
            per[q].append(b)
    dest_off = np.zeros(N + 1, np.uint64)
    for q in range(N):
        dest_off[q + 1] = int(dest_off[q]) + sum(len(b) for b in per[q])
    by = np.frombuffer(b"".join(b"".join(x) for x in per), np.uint8)
    return (by, dest_off, per) if want_frames else (by, dest_off)


# ---- builders ------------------------------------------------------------------------------------
def mk_groups(rows):
    """rows of (default_ballot, self_id, leader, prepare_oks, crt_instance, committed_upto)"""
    g = np.zeros(len(rows), R.PROPOSER_GROUP)
    for i, row in enumerate(rows):
        (g[i]["default_ballot"], g[i]["self_id"], g[i]["leader"], g[i]["prepare_oks"],
         g[i]["crt_instance"], g[i]["committed_upto"]) = row
    return g


def mk_state(rows):
    st = np.zeros(len(rows), R.ACCEPTOR_STATE)
    for i, row in enumerate(rows):
        st[i] = row
    return st


def nil_state(n):
    st = np.zeros(n, R.ACCEPTOR_STATE)
    st["status"] = NIL
    return st


def mk_sends(rows):
    """rows of (instance, ballot, last_committed, flags, first_cmd, n_cmds)"""
    s = np.zeros(len(rows), R.ACCEPT_SEND)
    for i, row in enumerate(rows):
        s[i] = tuple(row) + (0,)
    return s


def mk_cmds(rng, n):
    return (rng.integers(0, 4, n).astype(np.uint8),
            rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64),
            rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64))


def mk_log(rng, counts, nil_at=()):
    """a window's log: record i carries counts[i] commands (None: a nil record)"""
    n = len(counts)
    rec = np.zeros(n, R.LOG_REC)
    rec["ballot"] = rng.integers(0, 1 << 20, n)
    rec["status"] = rng.integers(1, 4, n)
    k = np.array([0 if c is None else c for c in counts], np.int64)
    for i, c in enumerate(counts):
        if c is None:
            rec["status"][i] = NIL
    coff = np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum(k)
    return (rec, coff) + mk_cmds(rng, int(k.sum()))



# ---- the window-boundary sweep -------------------------------------------------------------------
WINDOW = 8192
SWEEP = range(-30, 3)


def log_starts(frame, head):
    """walk a MIN frame (head bytes, V(n), n Commands, V(m), m Instances): the offsets at which its
    log's record headers and its log's commands start"""
    def varint(pos):
        u, k = 0, 0
        while True:
            x = frame[pos + k]
            u |= (x & 0x7F) << (7 * k)
            k += 1
            if x < 0x80:
                return u >> 1, pos + k
    n, pos = varint(head)
    m, pos = varint(pos + 17 * n)
    recs, cmds = [], []
    for _ in range(m):
        recs.append(pos)
        k, pos = varint(pos + 8)
        cmds += [pos + 17 * j for j in range(k)]
        pos += 17 * k
    assert pos == len(frame)
    return recs, cmds


def boundary_counts(T, fixed):
    """the command counts of a log whose record under test starts at byte T of a frame with `fixed`
    bytes ahead of the log's first record: z records of 9 bytes, one of 10 + 17 k0, the record
    under test (3 commands), one more (2)"""
    z = next(z for z in range(17) if (T - fixed - 10 - 9 * z) % 17 == 0)
    k0 = (T - fixed - 10 - 9 * z) // 17
    assert k0 >= 64 and z + 3 < 64  # V(k0) of two bytes, V(m) of one
    return [0] * z + [k0, 3, 2]


def boundary_case(d):
    """encode_accepts' arguments for one MIN frame (2 replicas, to peer 1) whose catch-up record
    z + 1 has its header at byte 8192 + d: 17 + V(0) + V(m) ahead of the log, the record's first
    command at 8192 + d + 9, the record before it ending with a command at 8192 + d - 17. Returns
    (arguments, that record's index)."""
    used = boundary_counts(WINDOW + d, 19)
    rng = np.random.default_rng(900 + d)
    base, ipg = 50, len(used) + 1
    inst, lc = base + len(used), base + len(used) - 1
    a = dict(sends=mk_sends([(inst, 16, lc, R.PH_ACCEPT, 0, 0)]),
             groups=mk_groups([(16, 0, 0, 2, inst + 1, lc)]), cmds=mk_cmds(rng, 0), inst_base=base,
             ipg=ipg, peer_commits=np.full((1, 2), base - 1, np.int32),
             log=mk_log(rng, used + [None]))
    return a, len(used) - 2

# ---- the fuzz generator --------------------------------------------------------------------------
FUZZ_SEEDS = list(range(24))
BRANCHES = {R.MODE_MIN: ("not_leader_id", "not_leader_oks", "advance", "refused", "accept"),
            R.MODE_CLASSIC: ("not_leader", "advance", "prepare", "accept")}
CATCHUP_KINDS = ("from_first", "from_pc", "empty")


def fuzz_propose(seed, N, mode):
    """groups with every handler branch. Returns (groups, prop_off, st, inst_base, ipg)."""
    rng = np.random.default_rng(1000 + seed)
    G = int(rng.integers(1, 200))
    ipg = int(rng.integers(8, 24))
    base = int(rng.integers(-50, 1000))
    rows, st = [], nil_state(G * ipg)
    n = np.zeros(G, np.int64)
    for g in range(G):
        first = base + g * ipg
        self_id = int(rng.integers(0, N))
        u = rng.random()
        leader = (self_id + 1) % N if (u < 0.2 and N > 1) else self_id
        oks = int(rng.integers(0, N >> 1) if N > 1 else 0) if 0.2 <= u < 0.4 else \
            int(rng.integers((N >> 1) + 1, N + 1))
        used = int(rng.integers(0, 5))          # instances the group has already
        skip = int(rng.integers(0, 4)) if rng.random() < 0.4 else 0
        crt = first + used
        for i in range(used + skip):            # non-nil: what crt advances over
            st[g * ipg + i] = (int(rng.integers(1, 4)), 16 + self_id, 7, 0)
        crt_in = first + used
        # committedUpTo: mostly right behind the next instance; sometimes lagging (REFUSED)
        nxt = crt + skip
        committed = nxt - 1 if rng.random() < 0.7 else nxt - 1 - int(rng.integers(1, 3))
        committed = max(committed, first - 1)
        D = -1 if (mode == R.MODE_CLASSIC and rng.random() < 0.25) else 16 * int(
            rng.integers(1, 9)) + self_id
        rows.append((D, self_id, leader, oks, crt_in, committed))
        v = rng.random()
        n[g] = 0 if v < 0.1 else (int(rng.integers(5001, 5200)) if v < 0.13 else
                                  int(rng.integers(1, 9)))
    prop_off = np.zeros(G + 1, np.uint64)
    prop_off[1:] = np.cumsum(n)
    return mk_groups(rows), prop_off, st, base, ipg


def fuzz_encode(seed, N, mode):
    """a proposer step's output plus the log and peer commits around it. Returns a dict of
    encode_accepts' arguments (sends from the transliterated handler)."""
    rng = np.random.default_rng(5000 + seed)
    groups, prop_off, st, base, ipg = fuzz_propose(seed, N, mode)
    G = len(groups)
    g2, st2, _, sends, send_off, _ = propose_handle(mode, N, groups, prop_off, st, base, ipg)
    cmds = mk_cmds(rng, int(prop_off[-1]))
    counts = []
    for g in range(G):
        for i in range(ipg):
            counts.append(int(rng.integers(0, 4)) if st["status"][g * ipg + i] != NIL else None)
    log = mk_log(rng, counts)
    pc = np.zeros((G, N), np.int32)
    for g in range(G):
        first, c = base + g * ipg, int(groups[g]["committed_upto"])
        for q in range(N):
            u = rng.random()
            pc[g, q] = first - 1 - int(rng.integers(0, 3)) if u < 0.25 else (
                c + int(rng.integers(0, 2)) if u < 0.5 else int(rng.integers(first - 1, c + 1)))
    return dict(sends=sends, groups=g2, cmds=cmds, inst_base=base, ipg=ipg, peer_commits=pc,
                log=log, thrifty=bool(seed & 1), alive_mask=int(rng.integers(0, 1 << N)) | 1)

"""The follower's half of Phase 1, transliterated line by line from the Go reference (the single
restatement the prepare-side tests compare against; nothing here is shared with the engine).

  handlePrepare          MIN      src/bareminpaxos/bareminpaxos.go:712-751
                         CLASSIC  src/paxos/paxos.go:445-468
  PrepareReply.Marshal   MIN      src/minpaxosproto/minpaxosprotomarsh.go:308-350
                         CLASSIC  src/paxosproto/paxosprotomarsh.go:126-150
  Prepare.Marshal        MIN      src/minpaxosproto/minpaxosprotomarsh.go:237-257
                         CLASSIC  src/paxosproto/paxosprotomarsh.go:53-74
  Instance.Marshal       src/minpaxosproto/minpaxosprotomarsh.go:100-124
  Command.Marshal        src/state/statemarsh.go
  replyPrepare / SendMsg src/genericsmr/genericsmr.go:499-512 (the code byte, then Marshal)

The :744 reading. bareminpaxos.go:742-745 declares `var culog []minpaxosproto.Instance` and then
assigns culog[i-(prepare.LastCommitted+1)] for i = LastCommitted+1 .. committedUpTo: an index into
a nil slice, which panics as written. Here (and in the engine) the loop builds the range that the
indexing names: culog has committedUpTo - LastCommitted entries, entry k is
*r.instanceSpace[LastCommitted + 1 + k]. It is the range handlePrepareReply (:936-938) consumes.

A group's window. The engine keeps instance numbers as window numbers: group g owns [first,
first + ipg), `first` plays the reference's instance 0 and first - 1 its -1 ("nothing committed").
instanceSpace indexing outside the window is the reference's index panic.
"""
import struct

import numpy as np

from go_translit import GoPanic
from minpaxos_amd import records as R

MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
TRUE, FALSE = 1, 0
NIL = R.STATUS_NIL


class Instance:
    def __init__(self, Cmds, Ballot, Status):
        self.Cmds, self.Ballot, self.Status = Cmds, Ballot, Status   # Cmds: list or None (nil)


class Replica:
    """the fields of one Replica the handlers touch; instanceSpace is the group's window"""

    def __init__(self, Id, N, first, ipg, space, defaultBallot, Leader=-1, crtInstance=None,
                 committedUpTo=None, prepareOKs=0):
        self.Id, self.N, self.first, self.ipg = Id, N, first, ipg
        self._space = space                                  # ipg entries: Instance or None
        self.defaultBallot, self.Leader = defaultBallot, Leader
        self.crtInstance = first if crtInstance is None else crtInstance
        self.committedUpTo = first - 1 if committedUpTo is None else committedUpTo
        self.prepareBookkeeping = None                       # set by a raised ballot (:719)
        self.prepareOKs = prepareOKs
        self.sent = []                                       # (LeaderId, preply)

    def instanceSpace(self, i):
        if i < self.first or i >= self.first + self.ipg:
            raise GoPanic(R.E_NIL_INSTANCE, f"instanceSpace[{i}]: index out of range")
        return self._space[i - self.first]

    def replyPrepare(self, replicaId, reply):                # bareminpaxos.go / paxos.go
        if replicaId < 0 or replicaId >= self.N:             # SendMsg: r.PeerWriters[peerId]
            raise GoPanic(R.E_BAD_ID, f"PeerWriters[{replicaId}]")
        self.sent.append((replicaId, reply))


def deref(p, what):
    if p is None:
        raise GoPanic(R.E_NIL_INSTANCE, f"nil pointer dereference ({what})")
    return p


# ---- handlePrepare -------------------------------------------------------------------------------
def handle_prepare_min(r, prepare):                          # bareminpaxos.go:712-751
    LeaderId, Ballot, LastCommitted = prepare
    ok = FALSE                                               # :716
    if r.defaultBallot < Ballot:                             # :718
        # :719 PrepareBookkeeping{prepare.Ballot, 0, 0, make([]int32, 3), 0, nil}; instance 0 of
        # the reference is `first` here, for peerCommits and highestInstanceNumber alike
        r.prepareBookkeeping = dict(maxRecvBallot=Ballot, prepareOKs=0, nacks=0,
                                    peerCommits=[r.first] * r.N, highestInstanceNumber=r.first,
                                    cmds=None)
        r.prepareOKs = 0
        ok = TRUE                                            # :720
        r.defaultBallot = Ballot                             # :721
        r.Leader = LeaderId                                  # :722
    while r.instanceSpace(r.crtInstance) is not None:        # :725
        r.crtInstance += 1                                   # :726
    if r.committedUpTo <= LastCommitted:                     # :731
        preply = dict(Id=r.Id, Instance=r.crtInstance - 1, OK=ok, Ballot=r.defaultBallot,
                      LastCommitted=r.committedUpTo, Command=None, CatchUpLog=None)   # :732
        preply["_from"], preply["_slot"] = r.committedUpTo + 1, None
    else:
        recentAccept, slot = None, None                      # :736
        if r.crtInstance > r.committedUpTo:                  # :737
            temp = deref(r.instanceSpace(r.committedUpTo + 1), "instanceSpace[committedUpTo+1]")
            recentAccept = temp.Cmds                         # :739
            slot = r.committedUpTo + 1
        culog = []                                           # :742 (see the :744 reading above)
        for i in range(LastCommitted + 1, r.committedUpTo + 1):                       # :743
            culog.append(deref(r.instanceSpace(i), f"instanceSpace[{i}]"))            # :744
        preply = dict(Id=r.Id, Instance=r.crtInstance - 1, OK=ok, Ballot=r.defaultBallot,
                      LastCommitted=r.committedUpTo, Command=recentAccept, CatchUpLog=culog)  # :747
        preply["_from"], preply["_slot"] = LastCommitted + 1, slot
    r.replyPrepare(LeaderId, preply)                         # :750
    return preply


def handle_prepare_classic(r, prepare):                      # paxos.go:445-468
    LeaderId, Instance_, Ballot, ToInfinity = prepare
    inst = r.instanceSpace(Instance_)                        # :446
    if inst is None:                                         # :449
        ok = TRUE
        if r.defaultBallot > Ballot:                         # :451
            ok = FALSE
        preply = dict(Instance=Instance_, OK=ok, Ballot=r.defaultBallot, Command=[],
                      _slot=None)                            # :454 make([]state.Command, 0)
    else:
        ok = TRUE
        if Ballot < inst.Ballot:                             # :457
            ok = FALSE
        preply = dict(Instance=Instance_, OK=ok, Ballot=inst.Ballot, Command=inst.Cmds,
                      _slot=Instance_)                       # :460
    r.replyPrepare(LeaderId, preply)                         # :463
    if ToInfinity == TRUE and Ballot > r.defaultBallot:      # :465 (TRUE = uint8(1))
        r.defaultBallot = Ballot                             # :466
    return preply


# ---- Marshal -------------------------------------------------------------------------------------
def put_varint(x):                                           # binary.PutVarint
    ux = ((x << 1) ^ (x >> 63)) & 0xFFFFFFFFFFFFFFFF
    out = bytearray()
    while ux >= 0x80:
        out.append((ux & 0x7F) | 0x80)
        ux >>= 7
    out.append(ux)
    return bytes(out)


def command_marshal(c):                                      # Op u8, K i64, V i64
    return struct.pack("<Bqq", c[0], c[1], c[2])


def commands_marshal(cmds):
    cmds = cmds or []                                        # len(nil) == 0
    return put_varint(len(cmds)) + b"".join(command_marshal(c) for c in cmds)


def instance_marshal(inst):                                  # minpaxosprotomarsh.go:100-124
    return struct.pack("<ii", inst.Ballot, inst.Status) + commands_marshal(inst.Cmds)


def prepare_reply_marshal_min(t):                            # minpaxosprotomarsh.go:308-350
    bs = struct.pack("<iiBii", t["Id"], t["Instance"], t["OK"] & 0xFF, t["Ballot"],
                     t["LastCommitted"])                     # :312-336
    bs += commands_marshal(t["Command"])                     # :337-343
    log = t["CatchUpLog"] or []
    bs += put_varint(len(log))                               # :344-347
    for inst in log:
        bs += instance_marshal(inst)                         # :348-350
    return bs


def prepare_reply_marshal_classic(t):                        # paxosprotomarsh.go:126-150
    return struct.pack("<iBi", t["Instance"], t["OK"] & 0xFF, t["Ballot"]) + \
        commands_marshal(t["Command"])


def send_msg(mode, t):
    """SendMsg: the code byte, then Marshal (genericsmr.go:499-512)"""
    m = prepare_reply_marshal_min(t) if mode == MIN else prepare_reply_marshal_classic(t)
    return bytes([R.PEER_PREPARE_REPLY]) + m


def prepare_frame(mode, leader, ballot, x, y=0):
    """Prepare.Marshal behind its code byte. MIN: x = LastCommitted. CLASSIC: x = Instance, y =
    ToInfinity."""
    if mode == MIN:
        return bytes([R.PEER_PREPARE]) + struct.pack("<iii", leader, ballot, x)
    return bytes([R.PEER_PREPARE]) + struct.pack("<iiiB", leader, x, ballot, y & 0xFF)


# ---- the engine's layout around the Go -----------------------------------------------------------
def build_replica(mode, N, g, groups, st, lb, inst, arena, inst_base, ipg):
    """the Replica of group g out of the engine's arrays (the store rule of
    mpx_encode_accepts_stored: nil when st is nil, Ballot from st, Status from lb where it has
    one, Cmds through inst; an unflagged slot has Cmds == nil)"""
    first = inst_base + g * ipg
    space = []
    for k in range(g * ipg, (g + 1) * ipg):
        if int(st["status"][k]) == NIL:
            space.append(None)
            continue
        status = int(st["status"][k])
        if lb is not None and int(lb["status"][k]) != NIL:
            status = int(lb["status"][k])
        cmds = None
        if inst is not None and int(inst["flags"][k]) & R.IC_HAS_CMDS:
            c0, nc = int(inst["first_cmd"][k]), int(inst["n_cmds"][k])
            if c0 > len(arena[0]) or nc > len(arena[0]) - c0:
                raise GoPanic(R.E_INVAL, f"slot {k}: commands [{c0}, {c0 + nc}) leave the arena")
            cmds = [(int(arena[0][j]), int(arena[1][j]), int(arena[2][j]))
                    for j in range(c0, c0 + nc)]
        space.append(Instance(cmds, int(st["ballot"][k]), status))
    grp = groups[g]
    return Replica(int(grp["self_id"]), N, first, ipg, space, int(grp["default_ballot"]),
                   int(grp["leader"]), int(grp["crt_instance"]), int(grp["committed_upto"]),
                   int(grp["prepare_oks"]))


def run_batch(mode, N, msgs, groups, st, inst_base=0, ipg=None, lb=None, inst=None, arena=None,
              gps=None, peer_commits=None, n_dest=None):
    """A batch of PREPARE_MSG in contract order through the handlers, group by group, each
    group's messages in slot order. Returns a dict: groups, gps, peer_commits (after), replies,
    reply_to, effect, log_from (MIN), frames (per message: bytes), bytes, dest_off, census.
    Raises GoPanic with the engine's code where the Go panics (or the batch is malformed)."""
    groups = np.array(np.atleast_1d(groups), dtype=R.PROPOSER_GROUP, copy=True)
    G = len(groups)
    if ipg is None:
        ipg = len(st) // G
    n_inst = G * ipg
    n = len(msgs)
    n_dest = N if n_dest is None else n_dest
    if gps is not None:
        gps = np.array(gps, dtype=R.GROUP_PREP_STATE, copy=True)
    if peer_commits is not None:
        peer_commits = np.array(peer_commits, dtype=np.int32, copy=True).reshape(G, N)
    keys = [int(m["key"]) for m in msgs]
    if any(a > b for a, b in zip(keys, keys[1:])):
        raise GoPanic(R.E_INVAL, "batch out of order")
    rep = np.zeros(n, R.PREPARE_REPLY_MIN if mode == MIN else R.PREPARE_REPLY)
    to = np.zeros(n, np.int32)
    eff = np.zeros(n, np.uint8)
    lf = np.zeros(n, np.int32) if mode == MIN else None
    frames = [b""] * n
    census = {}
    reps = {}

    def count(name):
        census[name] = census.get(name, 0) + 1

    for i, m in enumerate(msgs):
        key, ballot, leader, arg = (int(m[f]) for f in ("key", "ballot", "leader_id", "arg"))
        if mode == MIN:
            if key < 0 or key >= G:
                raise GoPanic(R.E_INVAL, "no such group")
            g = key
        else:
            idx = key - inst_base
            if idx < 0 or idx >= n_inst:
                raise GoPanic(R.E_NIL_INSTANCE, "instance outside the window")
            g = idx // ipg
        if g not in reps:
            reps[g] = build_replica(mode, N, g, groups, st, lb, inst, arena, inst_base, ipg)
        r = reps[g]
        before = r.defaultBallot
        if mode == MIN:
            p = handle_prepare_min(r, (leader, ballot, arg))
            rep[i] = (p["Id"], p["Instance"], p["Ballot"], p["LastCommitted"], p["OK"],
                      R.VALUE_KEEP if p["_slot"] is None else p["_slot"] - inst_base)
            lf[i] = p["_from"]
            logged = p["CatchUpLog"] is not None
            eff[i] = (R.PRH_OK if p["OK"] else 0) | (R.PRH_RAISED if r.defaultBallot != before else 0) \
                | (R.PRH_LOG if logged else 0)
            count("raised" if r.defaultBallot != before else "not_raised")
            count("log" if logged else "no_log")
            if p["Command"]:
                count("command")
            if r.defaultBallot != before and gps is not None:
                b = r.prepareBookkeeping
                for f, v in (("default_ballot", r.defaultBallot), ("prepare_oks", 0), ("nacks", 0),
                             ("max_recv_ballot", b["maxRecvBallot"]),
                             ("highest_instance", b["highestInstanceNumber"]),
                             ("value_id", R.VALUE_KEEP)):
                    gps[f][g] = v
            if r.defaultBallot != before and peer_commits is not None:
                peer_commits[g, :] = r.prepareBookkeeping["peerCommits"]
        else:
            nil = r.instanceSpace(key) is None
            p = handle_prepare_classic(r, (leader, key, ballot, arg))
            rep[i] = (p["Instance"], p["Ballot"], p["OK"],
                      R.VALUE_KEEP if p["_slot"] is None else p["_slot"] - inst_base)
            raised = r.defaultBallot != before
            eff[i] = (R.PRH_OK if p["OK"] else 0) | (R.PRH_RAISED if raised else 0)
            count(("nil_" if nil else "inst_") + ("ok" if p["OK"] else "refused"))
            if raised:
                count("raises")
            if arg != TRUE:
                count("not_true")
        to[i] = leader
        frames[i] = send_msg(mode, p)
    for g, r in reps.items():
        groups["default_ballot"][g] = r.defaultBallot
        if mode == MIN:
            groups["leader"][g] = r.Leader
            groups["prepare_oks"][g] = r.prepareOKs
            groups["crt_instance"][g] = r.crtInstance
    by, off = partition(frames, to, n_dest)
    return dict(groups=groups, gps=gps,
                peer_commits=None if peer_commits is None else peer_commits.reshape(-1),
                replies=rep, reply_to=to, effect=eff, log_from=lf, frames=frames, bytes=by,
                dest_off=off, census=census)


def partition(frames, reply_to, n_dest):
    """one Write per leader connection: destination by destination, frames in array order;
    reply_to < 0 is skipped"""
    per = [[] for _ in range(n_dest)]
    for f, d in zip(frames, reply_to):
        d = int(d)
        if d < 0:
            continue
        if d >= n_dest:
            raise GoPanic(R.E_INVAL, "reply_to outside [0, n_dest)")
        per[d].append(f)
    off = np.zeros(n_dest + 1, np.uint64)
    for q in range(n_dest):
        off[q + 1] = int(off[q]) + sum(len(b) for b in per[q])
    return np.frombuffer(b"".join(b"".join(x) for x in per), np.uint8), off



# ---- the window-boundary cases -------------------------------------------------------------------
def one_reply_case(counts, n_own, seed):
    """run_batch's arguments for one MIN Prepare to one group whose reply carries a log of
    len(counts) records (record i with counts[i] commands, every other empty one unflagged: Cmds ==
    nil marshals as V(0) too) and a Command of n_own commands"""
    rng = np.random.default_rng(seed)
    m = len(counts)
    big = dict(enumerate(counts))
    big[m], big[m + 1] = n_own, 1
    st, lb, inst, arena = make_store(rng, 1, m + 4, 0, [m + 2], lb_kind=1, big=big)
    inst["flags"][[i for i in range(1, m, 2) if counts[i] == 0]] = 0
    groups = np.zeros(1, R.PROPOSER_GROUP)
    groups[0] = (7, 0, 0, 2, 0, m - 1, (0, 0))
    msgs = np.zeros(1, R.PREPARE_MSG)
    msgs[0] = (0, 9, 1, -1)
    return dict(msgs=msgs, groups=groups, st=st, inst_base=0, ipg=m + 4, lb=lb, inst=inst,
                arena=arena)


def boundary_case(d):
    """one MIN PrepareReply frame whose log record z + 1 has its header at byte 8192 + d: the
    18-byte head, V(2), Command's two commands and V(m) ahead of the log, then the records of
    proposer_translit.boundary_counts. Returns (arguments, that record's index)."""
    from proposer_translit import WINDOW, boundary_counts
    used = boundary_counts(WINDOW + d, 18 + 1 + 34 + 1)
    return one_reply_case(used, 2, 7300 + d), len(used) - 2


def command_straddle_case():
    """one MIN PrepareReply frame whose Command slice lies across byte 8192 (482 commands behind 18
    + V(482) bytes: command 480 is bytes 8180 .. 8196), then a log of three records"""
    return one_reply_case([2, 0, 1], 482, 7400)

# ---- the fuzz generator --------------------------------------------------------------------------
FUZZ_SEEDS = list(range(24))
MIN_BRANCHES = ("raised", "not_raised", "no_log", "log", "command")
CLASSIC_BRANCHES = ("nil_ok", "nil_refused", "inst_ok", "inst_refused", "raises", "not_true")


def make_store(rng, G, ipg, inst_base, fill, p_unflag=0.25, max_cmds=4, lb_kind=0, dead=3,
               big=None):
    """A store of G groups: group g holds fill[g] non-nil slots from its first, then nil ones
    (a hole after them keeps crtInstance inside the window). Returns (st, lb, inst, arena): the
    arena in scrambled order with `dead` dead commands between ranges. big: {window index: n_cmds}."""
    n_inst = G * ipg
    st = np.zeros(n_inst, R.ACCEPTOR_STATE)
    st["status"] = NIL
    st["ballot"] = -1
    st["value_id"] = R.VALUE_KEEP
    inst = np.zeros(n_inst, R.INST_CMDS)
    lb = None
    if lb_kind:
        lb = np.zeros(n_inst, R.INST_STATE)
        lb["status"] = NIL
    want = []
    for g in range(G):
        for j in range(int(fill[g])):
            k = g * ipg + j
            st["status"][k] = int(rng.integers(1, 4))
            st["ballot"][k] = int(rng.integers(0, 1 << 20))
            if lb is not None and rng.random() < 0.5:
                lb["status"][k] = R.COMMITTED
            nc = (big or {}).get(k)
            if nc is None:
                if rng.random() < p_unflag:
                    continue                                 # made by a CommitShort: Cmds == nil
                nc = int(rng.integers(0, max_cmds + 1))
            want.append((k, nc))
    order = rng.permutation(len(want)) if want else []
    at = 0
    for x in order:
        k, nc = want[int(x)]
        at += int(rng.integers(0, dead + 1))
        inst[k] = (at, nc, R.IC_HAS_CMDS)
        at += nc
    at += dead
    arena = (rng.integers(0, 6, at).astype(np.uint8),
             rng.integers(-(1 << 62), 1 << 62, at).astype(np.int64),
             rng.integers(-(1 << 62), 1 << 62, at).astype(np.int64))
    return st, lb, inst, arena


def fuzz_case(seed, mode, N=3, G=12, ipg=8, n=96):
    """one legal batch over a random store: keyword arguments of run_batch (and of the engine)"""
    rng = np.random.default_rng(7100 + 2 * seed + (mode == CLASSIC))
    inst_base = int(rng.integers(-50, 50))
    fill = rng.integers(0, ipg - 1, G)                       # at least two nil slots at the end
    st, lb, inst, arena = make_store(rng, G, ipg, inst_base, fill, lb_kind=seed % 2)
    groups = np.zeros(G, R.PROPOSER_GROUP)
    for g in range(G):
        first = inst_base + g * ipg
        groups[g] = (int(rng.integers(0, 64)), int(rng.integers(0, N)), int(rng.integers(0, N)),
                     int(rng.integers(0, N)), first + int(rng.integers(0, int(fill[g]) + 1)),
                     first - 1 + int(rng.integers(0, max(int(fill[g]), 1))), (0, 0))
    msgs = np.zeros(n, R.PREPARE_MSG)
    for i in range(n):
        g = int(rng.integers(0, G))
        first = inst_base + g * ipg
        msgs["leader_id"][i] = int(rng.integers(0, N))
        if mode == MIN:
            msgs["key"][i] = g
            msgs["ballot"][i] = int(rng.integers(0, 96))
            cu = int(groups["committed_upto"][g])
            # LastCommitted around the follower's committedUpTo, inside [first - 1, ...)
            msgs["arg"][i] = max(first - 1, cu - int(rng.integers(-1, 4)))
        else:
            msgs["key"][i] = first + int(rng.integers(0, ipg))
            u = rng.random()
            k = int(msgs["key"][i]) - inst_base
            ref = int(st["ballot"][k]) if int(st["status"][k]) != NIL else \
                int(groups["default_ballot"][g])
            msgs["ballot"][i] = ref + int(rng.integers(-2, 3)) if u < 0.7 else \
                int(rng.integers(0, 1 << 20))
            msgs["arg"][i] = [0, 1, 1, 1, 2, 255][int(rng.integers(0, 6))]
    msgs = msgs[np.argsort(msgs["key"], kind="stable")]
    gps = pc = None
    if mode == MIN:
        gps = np.zeros(G, R.GROUP_PREP_STATE)
        gps["committed_upto"] = groups["committed_upto"]
        gps["triggered"] = rng.integers(0, 5, G)
        gps["prepare_oks"] = 2
        pc = rng.integers(-5, 100, G * N).astype(np.int32)
    return dict(msgs=msgs, groups=groups, st=st, inst_base=inst_base, ipg=ipg, lb=lb, inst=inst,
                arena=arena, gps=gps, peer_commits=pc)

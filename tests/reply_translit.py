"""Python transliteration of the three loops in which the reference answers its clients, over
Go-shaped objects (an Instance carries Cmds and Lb.ClientProposals; a per-client writer list
receives ProposeReplyTS structs in call order), for both protocols:

  refusals            bareminpaxos.go:617-624 and :671-685 (MIN), paxos.go:388-393 (CLASSIC)
  decide-time replies bareminpaxos.go:1023-1043 (MIN), paxos.go:639-654 (CLASSIC)
  execute-time        bareminpaxos.go:1071-1091 (MIN), paxos.go:680-699 (CLASSIC)

TEST INFRASTRUCTURE: the reference model of mpx_build_replies for the CPU and GPU tests.
build_replies() maps the call's records onto those objects (a slot of mpx_propose_handle is one
run of handlePropose: its proposals, and for an installed slot its instance), runs the Go loops
in send-array order and reads the writers back as mpx_reply_rec, with the engine's treatment of
capacity, padding and faulty slots (include/mpx.h)."""
import numpy as np

from minpaxos_amd import records as R

TRUE, FALSE = 1, 0   # genericsmr / bareminpaxos constants
NIL = 0              # state.NIL
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC


class Propose:                      # genericsmr.Propose: *genericsmrproto.Propose + Reply
    def __init__(self, command_id, timestamp, reply):
        self.CommandId, self.Timestamp, self.Reply = command_id, timestamp, reply


class ProposeReplyTS:               # genericsmrproto.go:31-37 (MIN's carries Leader as well)
    def __init__(self, ok, command_id, value, timestamp, leader=None):
        self.OK, self.CommandId, self.Value, self.Timestamp = ok, command_id, value, timestamp
        self.Leader = leader


class LeaderBookkeeping:
    def __init__(self, client_proposals):
        self.ClientProposals = client_proposals


class Instance:
    def __init__(self, cmds, ballot, lb):
        self.Cmds, self.Ballot, self.Lb = cmds, ballot, lb


class Replica:
    """what the three loops read of a replica, and where their calls land"""

    def __init__(self, proto, dreply, leader=0):
        self.proto, self.Dreply, self.Leader = proto, dreply, leader
        self.writers = {}    # client connection -> [ProposeReplyTS] in call order
        self.calls = []      # (client connection, ProposeReplyTS) in call order over all writers
        self.bcast = []      # CLASSIC: bcastCommit(instance, ballot, cmds) calls

    def ReplyProposeTS(self, reply, w):           # genericsmr.go: Marshal onto the client's writer
        self.writers.setdefault(w, []).append(reply)
        self.calls.append((w, reply))


def handle_propose_refuse(r, propose):
    """the refusing exits of handlePropose: not the leader (MIN :618-624, CLASSIC :389-392) and
    MIN's committedUpTo < instNo-1 (:671-685), which answers `propose`, the batch's first"""
    if r.proto == MIN:
        preply = ProposeReplyTS(FALSE, -1, NIL, 0, r.Leader)       # :622 / :682
    else:
        preply = ProposeReplyTS(FALSE, -1, NIL, 0)                 # :390
    r.ReplyProposeTS(preply, propose.Reply)                        # :623 / :683 / :391


def handle_accept_reply_commit(r, instance_no, inst):
    """the branch of handleAcceptReply that commits an instance (MIN :1026-1049, CLASSIC
    :641-662): the client replies, and CLASSIC's bcastCommit"""
    if inst.Lb.ClientProposals is not None and not r.Dreply:       # :1030 / :644
        for i in range(len(inst.Cmds)):                            # :1034 / :646
            p = inst.Lb.ClientProposals[i]
            if r.proto == MIN:
                propreply = ProposeReplyTS(TRUE, p.CommandId, NIL, p.Timestamp, r.Leader)  # :1035-1040
            else:
                propreply = ProposeReplyTS(TRUE, p.CommandId, NIL, p.Timestamp)            # :647-651
            r.ReplyProposeTS(propreply, p.Reply)                   # :1041 / :652
    if r.proto == CLASSIC:
        r.bcast.append((instance_no, inst.Ballot, inst.Cmds))      # :661


def execute_commands(r, instances, execute):
    """executeCommands' inner walk over the instances it reaches, in order (MIN :1071-1091,
    CLASSIC :680-699); execute(cmd) stands for Cmds[j].Execute(r.State)"""
    for inst in instances:
        if inst.Cmds is None:                                      # :1072 / :681
            break
        for j in range(len(inst.Cmds)):                            # :1074 / :683
            val = execute(inst.Cmds[j])                            # :1075 / :684
            if r.Dreply and inst.Lb is not None and inst.Lb.ClientProposals is not None:  # :1076 / :685
                p = inst.Lb.ClientProposals[j]
                if r.proto == MIN:
                    propreply = ProposeReplyTS(TRUE, p.CommandId, val, p.Timestamp, r.Leader)  # :1077-1082
                else:
                    propreply = ProposeReplyTS(TRUE, p.CommandId, val, p.Timestamp)            # :686-690
                r.ReplyProposeTS(propreply, p.Reply)               # :1083 / :691


# ---- the call's records onto those objects -------------------------------------------------------
def _slot_fault(kind, s, x, n_props, n_ret, ret_first, mask, inst_base):
    """the per-slot conditions of include/mpx.h for an eligible slot: (code, selected)"""
    first, n = int(x["first_cmd"]), int(x["n_cmds"])
    code = R.OK
    if first > n_props or n > n_props - first:
        code = R.E_INVAL
    selected = True
    if mask is not None:
        rel = int(x["instance"]) - inst_base
        if rel < 0 or rel >= len(mask):
            code = code or R.E_NIL_INSTANCE
            return code, False
        selected = bool(mask[rel])
    if kind == R.RB_EXECUTED and selected:   # only a selected slot reads results
        rf = first if ret_first is None else int(ret_first[s])
        if rf > n_ret or n > n_ret - rf:
            code = R.E_INVAL
    return code, selected


def build_replies(kind, sends, meta, mask=None, inst_base=0, ret=None, ret_first=None, cap=None,
                  pad_client=None, proto=MIN, dev=False):
    """The reference's answer to one mpx_build_replies call. Returns a dict: recs (REPLY_REC: the
    replies below cap, then with pad_client the pad records up to cap), commit_sends
    (COMMIT_SEND per slot), res (REPLY_RESULT scalar), code (R.OK or the first faulty slot's
    code), writers (client -> [(OK, CommandId, Value, Timestamp)] in call order) and bcast.
    dev=False: the host form, a faulty slot fails the call (only code is meaningful).
    dev=True: the device form, a faulty slot emits nothing and the others are exact; code is
    what the next synchronising call answers (E_NIL_INSTANCE before E_INVAL)."""
    sends = np.ascontiguousarray(sends, R.ACCEPT_SEND)
    meta = np.ascontiguousarray(meta, R.PROPOSAL)
    n_ret = 0 if ret is None else len(ret)
    refusals = kind == R.RB_FALSE
    eligible_flags = (R.PH_NOT_LEADER | R.PH_REFUSED) if refusals else (R.PH_ACCEPT | R.PH_PREPARE)
    r = Replica(proto, dreply=(kind == R.RB_EXECUTED))
    cs = np.zeros(len(sends), R.COMMIT_SEND)
    codes, n_slots, reached = [], 0, []
    for s, x in enumerate(sends):
        flags, first, n = int(x["flags"]), int(x["first_cmd"]), int(x["n_cmds"])
        cs[s] = (x["instance"], x["ballot"], first, n, 0, (0, 0))
        if not flags & eligible_flags:
            continue
        code, selected = _slot_fault(kind, s, x, len(meta), n_ret, ret_first, mask, inst_base)
        if code:
            codes.append(code)
            if not dev:
                return dict(code=code)
            continue
        if not selected:
            continue
        n_slots += 1
        proposals = [Propose(int(meta["command_id"][j]), int(meta["timestamp"][j]),
                             int(meta["client"][j])) for j in range(first, first + n)]
        if refusals:
            if flags & R.PH_NOT_LEADER:       # every proposal is its own handlePropose call
                for p in proposals:
                    handle_propose_refuse(r, p)
            elif proposals:                   # the batch is drained, `propose` is its first
                handle_propose_refuse(r, proposals[0])
            continue
        rf = first if ret_first is None else int(ret_first[s])
        cmds = list(range(rf, rf + n))        # a command is known by where its result lies
        inst = Instance(cmds, int(x["ballot"]), LeaderBookkeeping(proposals))
        cs[s]["flags"] = R.CS_SEND
        if kind == R.RB_DECIDED:
            handle_accept_reply_commit(r, int(x["instance"]), inst)
        else:
            reached.append(inst)
    if kind == R.RB_EXECUTED:
        execute_commands(r, reached, lambda c: int(ret[c]))
    total = len(r.calls)
    cap = total + (pad_client is not None) if cap is None else cap
    n_out = cap if pad_client is not None else min(total, cap)
    recs = np.zeros(n_out, R.REPLY_REC)
    for i, (w, p) in enumerate(r.calls[:n_out]):
        recs[i] = (p.Value, p.Timestamp, p.CommandId, w)
    if pad_client is not None:
        recs["client"][min(total, cap):] = pad_client
    res = np.zeros((), R.REPLY_RESULT)
    res["n_replies"], res["n_slots"] = total, n_slots
    code = R.OK
    if codes:
        code = R.E_NIL_INSTANCE if R.E_NIL_INSTANCE in codes else R.E_INVAL
    writers = {w: [(p.OK, p.CommandId, p.Value, p.Timestamp) for p in ps]
               for w, ps in r.writers.items()}
    return dict(recs=recs, commit_sends=cs, res=res, code=code, writers=writers, bcast=r.bcast)


# ---- inputs ---------------------------------------------------------------------------------------
def mk_sends(rows):
    """rows of (instance, ballot, flags, first_cmd, n_cmds[, last_committed])"""
    a = np.zeros(len(rows), R.ACCEPT_SEND)
    for i, row in enumerate(rows):
        a[i] = (row[0], row[1], row[5] if len(row) > 5 else -1, row[2], row[3], row[4], 0)
    return a


def mk_meta(rows):
    """rows of (timestamp, command_id, client)"""
    a = np.zeros(len(rows), R.PROPOSAL)
    for i, row in enumerate(rows):
        a[i] = row
    return a


SLOT_KINDS = ("not_leader", "refused", "accept_selected", "accept_unselected", "empty")


def fuzz_case(seed, census=None):
    """One call's arguments (a dict for build_replies / the engine wrappers). The kind goes round
    with the seed; the slots mix every MPX_PH_* flag, empty slots, small batches and now and then
    a full one, so the totals cross tile boundaries. census (optional dict): counts per SLOT_KINDS
    and "slots"."""
    rng = np.random.default_rng(9000 + seed)
    kind = (R.RB_FALSE, R.RB_DECIDED, R.RB_EXECUTED)[seed % 3]
    n_sends = int(rng.integers(1, 700))
    base = int(rng.integers(-50, 1000))
    n_inst = n_sends + int(rng.integers(0, 20))
    window = rng.permutation(n_inst)[:n_sends]
    big = int(rng.integers(0, n_sends)) if rng.random() < 0.5 else -1
    rows, at = [], 0
    mask = (rng.random(n_inst) < 0.6).astype(np.uint8) * rng.integers(1, 256, n_inst).astype(np.uint8)
    for s in range(n_sends):
        u = rng.random()
        if kind == R.RB_FALSE:
            flags = R.PH_NOT_LEADER if u < 0.4 else R.PH_REFUSED if u < 0.7 else R.PH_ACCEPT
        else:
            flags = (R.PH_ACCEPT if u < 0.7 else R.PH_PREPARE if u < 0.8 else
                     R.PH_REFUSED if u < 0.9 else R.PH_NOT_LEADER)
        n = 0 if rng.random() < 0.1 else int(rng.integers(1, 12))
        if s == big:
            n = R.PROPOSE_MAX_BATCH
        if rng.random() < 0.05:
            at += int(rng.integers(1, 9))  # proposals no slot names
        inst = -1 if flags == R.PH_NOT_LEADER else base + int(window[s])
        rows.append((inst, int(rng.integers(0, 99)), flags, at, n, int(rng.integers(-1, 50))))
        at += n
        if census is not None:
            census["slots"] = census.get("slots", 0) + 1
            sel = kind != R.RB_FALSE and flags & (R.PH_ACCEPT | R.PH_PREPARE)
            name = ("empty" if n == 0 else "not_leader" if flags == R.PH_NOT_LEADER else
                    "refused" if flags == R.PH_REFUSED else
                    None if not sel else
                    "accept_selected" if mask[inst - base] else "accept_unselected")
            if name:
                census[name] = census.get(name, 0) + 1
    n_props = at + int(rng.integers(0, 5))
    meta = np.zeros(n_props, R.PROPOSAL)
    meta["timestamp"] = rng.integers(-(1 << 62), 1 << 62, n_props)
    meta["command_id"] = rng.integers(-(1 << 31), 1 << 31, n_props)
    meta["client"] = rng.integers(0, 64, n_props)
    case = dict(kind=kind, sends=mk_sends(rows), meta=meta, inst_base=base)
    if kind != R.RB_FALSE:
        case["mask"] = mask
    if kind == R.RB_EXECUTED:
        if rng.random() < 0.5:  # an apply over gathered commands: the results lie elsewhere
            order = rng.permutation(n_sends)
            rf, nxt = np.zeros(n_sends, np.uint64), 0
            for s in order:
                rf[s] = nxt
                nxt += rows[s][4]
            case["ret_first"] = rf
            case["ret"] = rng.integers(-(1 << 62), 1 << 62, nxt + 3)
        else:
            case["ret"] = rng.integers(-(1 << 62), 1 << 62, n_props)
    total = int(build_replies(**case)["res"]["n_replies"])
    u = rng.random()
    if u < 0.3:
        case["cap"] = max(total - int(rng.integers(1, 40)), 0)
    elif u < 0.7:
        case["pad_client"] = 64
        case["cap"] = total + int(rng.integers(0, 1100))
    return case

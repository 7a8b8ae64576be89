"""Python transliteration of the reference's stable-store appends, over Go-shaped objects: a Replica
whose StableStore is a bytearray, Instances with the fields the Go reads, commands as
state.Command values, the record sites applied one by one in the batch's order.
  MIN      recordInstanceMetadata  bareminpaxos.go:164-174   recordCommands  :177-188
  CLASSIC  recordInstanceMetadata  paxos.go:107-116          recordCommands  :119-130
  sites    handlePropose       bareminpaxos.go:697-698 / paxos.go:436-437
           handleAccept        bareminpaxos.go:798-800
           handleCommit        bareminpaxos.go:881-882 / paxos.go:547-548
           handleCommitShort   bareminpaxos.go:909 / paxos.go:574
           handleAcceptReply   bareminpaxos.go:1045 / paxos.go:656 (the commit branch)

TEST INFRASTRUCTURE: the reference model of mpx_record_log for the CPU and GPU tests. Only
record_log() below knows the record layouts: it maps the call's records onto those objects and runs
the sites item by item in array order; what the StableStore holds afterwards is the answer.

Documented deviation: a faulty recording item (its value or its instance cannot be resolved) fails
the host form; in the device form the message is dropped before the site sees it, so it records
nothing, and the code arrives at the next synchronising call."""
import struct

import numpy as np

from minpaxos_amd import records as R

PREPARING, PREPARED, ACCEPTED, COMMITTED = 0, 1, 2, 3


class Command:
    """state.Command"""

    def __init__(self, op, k, v):
        self.Op, self.K, self.V = op, k, v

    def Marshal(self, w):                                   # statemarsh.go:8-19
        w += struct.pack("<B", self.Op)
        w += struct.pack("<q", self.K)
        w += struct.pack("<q", self.V)


class MinInstance:
    """minpaxosproto.Instance"""

    def __init__(self, cmds, ballot, status):
        self.Cmds, self.Ballot, self.Status = cmds, ballot, status


class ClassicInstance:
    """paxos.Instance"""

    def __init__(self, cmds, ballot, status):
        self.cmds, self.ballot, self.status = cmds, ballot, status


def u32(x):
    return x & 0xFFFFFFFF


class MinReplica:
    def __init__(self, durable=True):
        self.Durable, self.StableStore = durable, bytearray()

    def recordInstanceMetadata(self, inst, instNo):         # bareminpaxos.go:164
        if not self.Durable:                                # :165
            return                                          # :166
        b = bytearray(12)                                   # :169
        b[0:4] = struct.pack("<I", u32(inst.Ballot))        # :170
        b[4:8] = struct.pack("<I", u32(inst.Status))        # :171
        b[8:12] = struct.pack("<I", u32(instNo))            # :172
        self.StableStore += b                               # :173

    def recordCommands(self, cmds):                         # bareminpaxos.go:177
        if not self.Durable:                                # :178
            return                                          # :179
        if cmds is None:                                    # :182
            return                                          # :183
        for i in range(len(cmds)):                          # :185
            cmds[i].Marshal(self.StableStore)               # :186


class ClassicReplica:
    def __init__(self, durable=True):
        self.Durable, self.StableStore = durable, bytearray()

    def recordInstanceMetadata(self, inst):                 # paxos.go:107
        if not self.Durable:                                # :108
            return                                          # :109
        b = bytearray(5)                                    # :112
        b[0:4] = struct.pack("<I", u32(inst.ballot))        # :113
        b[4] = inst.status & 0xFF                           # :114
        self.StableStore += b                               # :115

    def recordCommands(self, cmds):                         # paxos.go:119
        if not self.Durable:                                # :120
            return                                          # :121
        if cmds is None:                                    # :124
            return                                          # :125
        for i in range(len(cmds)):                          # :127
            cmds[i].Marshal(self.StableStore)               # :128


# ---- the record sites ----------------------------------------------------------------------------
def site_min(r, ballot, status, inst_no, command, with_commands):
    """MIN: the instance as the handler left it, then its two record calls"""
    inst = MinInstance(command, ballot, status)
    r.recordInstanceMetadata(inst, inst_no)                 # :697 / :798 / :881 / :909 / :1045
    if with_commands:
        r.recordCommands(command)                           # :698 / :799 / :882


def site_classic(r, ballot, status, command, with_commands):
    inst = ClassicInstance(command, ballot, status)
    r.recordInstanceMetadata(inst)                          # paxos.go:436 / :547 / :574 / :656
    if with_commands:
        r.recordCommands(command)                           # :437 / :548


STATUS = {R.LR_ACCEPTS: ACCEPTED, R.LR_COMMITS: COMMITTED, R.LR_SENDS: PREPARED, R.LR_DECIDED: COMMITTED}
BRANCHES = {
    R.LR_ACCEPTS: ("records", "does_not_record"),
    R.LR_COMMITS: ("commit", "commit_short"),
    R.LR_SENDS: ("records", "prepare", "not_leader", "refused"),
    R.LR_DECIDED: ("records", "masked_out", "not_accepted"),
}


def new_census():
    return {k: dict({b: 0 for b in bs}, items=0) for k, bs in BRANCHES.items()}


def _result(n_recs=0, n_cmds=0, n_bytes=0, flags=0):
    r = np.zeros((), R.RECORD_RESULT)
    r["n_recs"], r["n_cmds"], r["n_bytes"], r["flags"] = n_recs, n_cmds, n_bytes, flags
    return r


def _resolve(x, i, sources, perm, rec_end):
    """the message's Command as Unmarshal left it: (source, lo, hi) or None when it cannot be resolved"""
    p = int(perm[i]) if perm is not None else i
    if p >= rec_end[-1]:
        return None
    s = int(np.searchsorted(rec_end, p, side="right"))
    src, v = sources[s], int(x["value_id"])
    n_frames = 0 if src.get("cmd_off") is None else len(src["cmd_off"]) - 1
    if v >= n_frames:
        return None
    lo, hi = int(src["cmd_off"][v]), int(src["cmd_off"][v + 1])
    if hi < lo or hi > len(src["op"]) or hi - lo >= 0xFFFFFFFF:
        return None
    return s, lo, hi


def _commands(sources, s, lo, hi):
    src = sources[s]
    return [Command(int(src["op"][j]), int(src["key"][j]), int(src["val"][j])) for j in range(lo, hi)]


def record_log(kind, fmt, items, sources=(), effect=None, perm=None, mask=None, inst_base=0,
               out_cap=None, dev=False, d_n=None, census=None):
    """The reference's answer to one mpx_record_log call. Returns a dict: out (the bytes, empty when
    they did not fit), item_off, res, code. dev=False: the host form, a faulty item fails the call
    (only code is meaningful). dev=True: the device form (see the module's deviation); code is what
    the next synchronising call answers."""
    if kind == R.LR_ACCEPTS and fmt == R.LOG_DURABLE_CLASSIC:
        return dict(code=R.E_UNSUPPORTED)
    n = len(items) if d_n is None else min(int(d_n), len(items))
    msgs = kind in (R.LR_ACCEPTS, R.LR_COMMITS)
    rec_end = np.cumsum([int(s["n_recs"]) for s in sources]) if len(sources) else np.array([0])
    if not dev and msgs and perm is not None and any(int(p) >= rec_end[-1] for p in perm[:len(items)]):
        return dict(code=R.E_INVAL)
    r = MinReplica() if fmt == R.LOG_DURABLE else ClassicReplica()
    status = STATUS[kind]
    item_off, n_recs, n_cmds, nil, inval = [], 0, 0, False, False
    cen = None if census is None else census[kind]

    def note(branch):
        if cen is not None:
            cen[branch] += 1
            cen["items"] += 1
    for i in range(len(items)):
        item_off.append(len(r.StableStore))
        if i >= n:
            continue
        x = items[i]
        ballot, inst_no = int(x["ballot"]), int(x["instance"])
        command, with_commands = None, False
        if msgs:
            if kind == R.LR_ACCEPTS:
                if not int(effect[i]) & R.AH_STORED:
                    note("does_not_record")
                    continue
                with_commands = True
                note("records")
            else:
                with_commands = bool(int(effect[i]) & R.CH_CMDS) and int(x["value_id"]) != R.VALUE_KEEP
                note("commit" if with_commands else "commit_short")
            if with_commands:
                at = _resolve(x, i, sources, perm, rec_end)
                if at is None:
                    inval = True
                    if not dev:
                        return dict(code=R.E_INVAL)
                    continue
                command = _commands(sources, *at)
        else:
            flags = int(x["flags"])
            if not flags & R.PH_ACCEPT:
                note("prepare" if flags & R.PH_PREPARE else "not_leader" if flags & R.PH_NOT_LEADER
                     else "refused") if kind == R.LR_SENDS else note("not_accepted")
                continue
            if kind == R.LR_SENDS:
                lo, k = int(x["first_cmd"]), int(x["n_cmds"])
                if lo + k > len(sources[0]["op"]) or k == 0xFFFFFFFF:
                    inval = True
                    if not dev:
                        return dict(code=R.E_INVAL)
                    continue
                command, with_commands = _commands(sources, 0, lo, lo + k), True
                note("records")
            else:
                rel = inst_no - inst_base
                if not 0 <= rel < (0 if mask is None else len(mask)):
                    nil = True
                    if not dev:
                        return dict(code=R.E_NIL_INSTANCE)
                    continue
                if not mask[rel]:
                    note("masked_out")
                    continue
                note("records")
        if fmt == R.LOG_DURABLE:
            site_min(r, ballot, status, inst_no, command, with_commands)
        else:
            site_classic(r, ballot, status, command, with_commands)
        n_recs += 1
        n_cmds += len(command) if command is not None else 0
    total = len(r.StableStore)
    item_off.append(total)
    if not dev and total >= 0xFFFFFFFF:
        return dict(code=R.E_UNSUPPORTED)
    if out_cap is None:
        out_cap = total
    full = total > out_cap
    code = R.E_NIL_INSTANCE if nil else R.E_INVAL if inval else R.OK
    out = np.frombuffer(bytes(r.StableStore), np.uint8) if not full else np.zeros(0, np.uint8)
    return dict(out=out, item_off=np.array(item_off, np.uint64), code=code,
                res=_result(n_recs, n_cmds, total, R.LR_FULL if full else 0))


# ---- inputs ---------------------------------------------------------------------------------------
def mk_msgs(rows):
    """rows of (instance, ballot, value_id)"""
    a = np.zeros(len(rows), R.ACCEPT_MSG)
    for i, (instance, ballot, value_id) in enumerate(rows):
        a[i] = (instance, ballot, 1, value_id)
    return a


def mk_sends(rows):
    """rows of (instance, ballot, flags, first_cmd, n_cmds)"""
    a = np.zeros(len(rows), R.ACCEPT_SEND)
    for i, (instance, ballot, flags, first, k) in enumerate(rows):
        a[i] = (instance, ballot, -1, flags, first, k, 0)
    return a


def mk_cmds(n, seed=0):
    """n commands with distinctive fields"""
    rng = np.random.default_rng(93000 + seed)
    return (rng.integers(0, 6, n).astype(np.uint8), rng.integers(-(1 << 62), 1 << 62, n),
            rng.integers(-(1 << 62), 1 << 62, n))


def mk_source(sizes, n_recs=None, seed=0, gap=0):
    """one connection's unmarshal output: frame v has sizes[v] commands (gap: commands no frame
    names after the last)"""
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.uint64)
    op, key, val = mk_cmds(int(off[-1]) + gap, seed)
    return dict(cmd_off=off, op=op, key=key, val=val, n_recs=len(sizes) if n_recs is None else n_recs)


def msgs_case(kind, fmt, sizes, records, n_src=1, seed=0, ballot=None):
    """n = len(sizes) messages of ascending instances; message i carries sizes[i] commands (None: a
    CommitShort) and records[i] says whether it is flagged (ACCEPTS: AH_STORED; COMMITS: CH_CMDS).
    The messages alternate over n_src sources and reach the batch through perm when n_src > 1."""
    n = len(sizes)
    frames = [[] for _ in range(n_src)]
    rows, eff, perm_src = [], [], []
    for i, k in enumerate(sizes):
        s = i % n_src
        frames[s].append(k)
        v = R.VALUE_KEEP if k is None else sum(f is not None for f in frames[s]) - 1
        rows.append((100 + i // 2, (7 + i) if ballot is None else ballot, v))
        flag = R.AH_STORED if kind == R.LR_ACCEPTS else R.CH_CMDS
        eff.append((flag | 1) if records[i] else 1)
        perm_src.append((s, len(frames[s]) - 1))
    sources = [mk_source([f for f in fr if f is not None], len(fr), seed * 16 + s, gap=s)
               for s, fr in enumerate(frames)]
    rec_base = np.concatenate([[0], np.cumsum([len(fr) for fr in frames])])
    perm = np.array([rec_base[s] + r for s, r in perm_src], np.uint32) if n_src > 1 else None
    return dict(kind=kind, fmt=fmt, items=mk_msgs(rows), sources=sources,
                effect=np.array(eff, np.uint8), perm=perm)


def sends_case(kind, fmt, sizes, flags, seed=0, n_inst=None, mask=None, inst_base=100):
    """slot i has flags[i] and sizes[i] commands, instances ascending from inst_base"""
    rows, at = [], 2
    for i, (k, f) in enumerate(zip(sizes, flags)):
        rows.append((-1 if f == R.PH_NOT_LEADER else inst_base + i, 11 + i % 5, f, at, k))
        at += k
    case = dict(kind=kind, fmt=fmt, items=mk_sends(rows))
    if kind == R.LR_SENDS:
        op, key, val = mk_cmds(at + 3, seed)
        case["sources"] = [dict(cmd_off=None, op=op, key=key, val=val, n_recs=len(rows))]
    else:
        case.update(mask=mask, inst_base=inst_base)
    return case


def fuzz_case(seed):
    """One call's arguments (a dict for record_log / the engine's record_log): the kind by seed % 4,
    MIN's format for even seed // 4 (and every ACCEPTS call), CLASSIC's for odd."""
    rng = np.random.default_rng(43000 + seed)
    kind = seed % 4
    fmt = R.LOG_DURABLE if kind == R.LR_ACCEPTS or (seed // 4) % 2 == 0 else R.LOG_DURABLE_CLASSIC
    n = int(rng.integers(1, 700))
    sizes_of = lambda: int(rng.choice([0, 1, 2, 3, 17, 600], p=[0.12, 0.4, 0.25, 0.17, 0.05, 0.01]))
    if kind in (R.LR_ACCEPTS, R.LR_COMMITS):
        n_src = int(rng.integers(1, 5))
        sizes, records = [], []
        for _ in range(n):
            short = kind == R.LR_COMMITS and rng.random() < 0.3
            sizes.append(None if short else sizes_of())
            records.append(bool(rng.random() < (0.6 if kind == R.LR_ACCEPTS else 0.85)))
        case = msgs_case(kind, fmt, sizes, records, n_src, seed)
        case["items"]["instance"] = int(rng.integers(-30, 900)) + np.sort(rng.integers(0, n, n))
        if n_src == 1 and rng.random() < 0.5:
            case["perm"] = np.arange(n, dtype=np.uint32)    # one source in arrival order: perm is optional
        return case
    flags = rng.choice([R.PH_ACCEPT, R.PH_PREPARE, R.PH_NOT_LEADER, R.PH_REFUSED], n,
                       p=[0.55, 0.15, 0.15, 0.15]).tolist()
    sizes = [sizes_of() if kind == R.LR_SENDS else int(rng.integers(0, 4)) for _ in range(n)]
    base = int(rng.integers(-30, 900))
    mask = (rng.random(n + 5) < 0.6).astype(np.uint8) if kind == R.LR_DECIDED else None
    return sends_case(kind, fmt, sizes, flags, seed, mask=mask, inst_base=base)


def gathered(case, got=None):
    """the recording items of a MIN-format case as mpx_encode_log takes them: (LOG_REC records,
    cmd_off, op, key, val) with the commands gathered, by plain array indexing (no Go-shaped objects:
    a second opinion for the cross-check)"""
    kind, items = case["kind"], case["items"]
    sources = case.get("sources", ())
    rec_end = np.cumsum([int(s["n_recs"]) for s in sources]) if len(sources) else None
    recs, off, op, key, val = [], [0], [], [], []
    for i, x in enumerate(items):
        sl = None
        if kind in (R.LR_ACCEPTS, R.LR_COMMITS):
            e = int(case["effect"][i])
            if kind == R.LR_ACCEPTS and not e & R.AH_STORED:
                continue
            if kind == R.LR_ACCEPTS or (e & R.CH_CMDS and int(x["value_id"]) != R.VALUE_KEEP):
                p = i if case.get("perm") is None else int(case["perm"][i])
                s = int(np.searchsorted(rec_end, p, side="right"))
                v = int(x["value_id"])
                sl = (s, int(sources[s]["cmd_off"][v]), int(sources[s]["cmd_off"][v + 1]))
        else:
            if not int(x["flags"]) & R.PH_ACCEPT:
                continue
            if kind == R.LR_SENDS:
                sl = (0, int(x["first_cmd"]), int(x["first_cmd"]) + int(x["n_cmds"]))
            elif not case["mask"][int(x["instance"]) - case["inst_base"]]:
                continue
        recs.append((int(x["ballot"]), STATUS[kind], int(x["instance"]), 0))
        if sl is not None:
            s, lo, hi = sl
            op.append(sources[s]["op"][lo:hi]), key.append(sources[s]["key"][lo:hi])
            val.append(sources[s]["val"][lo:hi])
            off.append(off[-1] + hi - lo)
        else:
            off.append(off[-1])
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)
    return (np.array(recs, R.LOG_REC) if recs else np.zeros(0, R.LOG_REC), np.array(off, np.uint64),
            cat(op, np.uint8), cat(key, np.int64), cat(val, np.int64))

"""Python transliteration of where the reference assigns an instance's commands, over Go-shaped
objects: an instanceSpace of *Instance (None = nil) whose Cmds may be nil, the messages applied one
by one in the batch's order.
  MIN handleAccept      bareminpaxos.go:786-793  r.instanceSpace[i] = &Instance{..., accept.Command}
  CLASSIC handleAccept  paxos.go:479-483, :491, :506  cmds = accept.Command
  handleCommit          bareminpaxos.go:861-868 / paxos.go:526-534
  handleCommitShort     bareminpaxos.go:890-898
  handlePropose         bareminpaxos.go:687-699 / paxos.go:410-437
  Unmarshal             make([]state.Command, alen1): minpaxosprotomarsh.go:492, :667;
                        paxosprotomarsh.go:263, :422 (a non-nil slice, also of zero commands)

TEST INFRASTRUCTURE: the reference model of mpx_store_commands and mpx_store_compact for the CPU and
GPU tests. Only store_commands() / store_compact() below know the record layouts: they map the
call's records onto those objects, run the assignments message by message and read the winner of a
slot purely as "what Cmds the slot holds after the loop", then lay the winners' commands out as the
engine's arena (include/mpx.h).

Documented deviation: a faulty storing item (its value or its instance cannot be resolved) fails
the host form; in the device form the message is dropped before the handlers see it, so it neither
stores nor supersedes, and the code arrives at the next synchronising call."""
import numpy as np

from minpaxos_amd import records as R


class Instance:
    def __init__(self, cmds):
        self.Cmds = cmds      # None = nil; a Cmds object otherwise (possibly of zero commands)


class Cmds:
    """a []state.Command: where its commands are (source, first, count) and which item made it
    (None: it was in the slot before the batch)"""

    def __init__(self, src, first, n, item=None):
        self.src, self.first, self.n, self.item = src, first, n, item


def handle_accept_stored(space, i, command):
    """the message was not ignored and its ballot equals defaultBallot (MPX_AH_STORED)"""
    space[i] = Instance(command)                  # bareminpaxos.go:786-793 / paxos.go:479-483, :491, :506


def handle_commit(space, i, command):
    if space[i] is None:                          # bareminpaxos.go:861 / paxos.go:526
        space[i] = Instance(command)              # :862-867 / :527-532
    else:
        space[i].Cmds = command                   # :868 / :534


def handle_commit_short(space, i):
    if space[i] is None:                          # bareminpaxos.go:890
        space[i] = Instance(None)                 # :891-896  Cmds == nil
    # else: the slot keeps its Cmds                 :897-898


def handle_propose_installed(space, i, command):
    space[i] = Instance(command)                  # bareminpaxos.go:687-699 / paxos.go:410-437


# ---- the call's records onto those objects -------------------------------------------------------
def _space_of(inst):
    return [Instance(Cmds("arena", int(x["first_cmd"]), int(x["n_cmds"]))) if x["flags"] & R.IC_HAS_CMDS
            else None for x in inst]


def _result(n_stored=0, n_cmds=0, n_superseded=0, flags=0):
    r = np.zeros((), R.STORE_RESULT)
    r["n_stored"], r["n_cmds"], r["n_superseded"], r["flags"] = n_stored, n_cmds, n_superseded, flags
    return r


def store_commands(kind, items, sources, arena, used, inst, inst_base=0, effect=None, perm=None,
                   store_mask=R.AH_STORED, handler="accept", dev=False, d_n=None, census=None):
    """The reference's answer to one mpx_store_commands call. sources: dicts cmd_off / op / key / val
    / n_recs. Returns a dict: op, key, val (the arena after the call), used, inst, res, code.
    dev=False: the host form, a faulty item fails the call (only code is meaningful). dev=True: the
    device form (see the module's deviation); code is what the next synchronising call answers.
    handler: which of handleAccept / handleCommit the MSGS items went through."""
    a_op, a_key, a_val = (np.array(x, copy=True) for x in arena)
    inst = np.array(inst, dtype=R.INST_CMDS, copy=True)
    cap, n_inst = len(a_op), len(inst)
    n = len(items) if d_n is None else min(int(d_n), len(items))
    rec_end = np.cumsum([int(s["n_recs"]) for s in sources])
    if not dev and (used > cap or (perm is not None and any(int(p) >= rec_end[-1] for p in perm[:len(items)]))):
        return dict(code=R.E_INVAL)
    space = _space_of(inst)
    before = [x.Cmds if x is not None else None for x in space]
    n_storing, nil, inval = 0, False, used > cap
    for i in range(n):
        x = items[i]
        keep = kind == R.SC_MSGS and int(x["value_id"]) == R.VALUE_KEEP
        if kind == R.SC_MSGS:
            stores = bool(int(effect[i]) & store_mask) and not keep
        else:
            stores = bool(int(x["flags"]) & (R.PH_ACCEPT | R.PH_PREPARE))
        rel = int(x["instance"]) - inst_base
        if not stores:
            if census is not None:
                census["keep" if keep else "does_not_store"] += 1
            # what the handlers do to the slot besides: a CommitShort installs a nil-Cmds instance
            if keep and 0 <= rel < n_inst:
                handle_commit_short(space, rel)
            continue
        # the message's Command, resolved as Unmarshal left it
        bad = False
        if kind == R.SC_MSGS:
            p = int(perm[i]) if perm is not None else i
            if p >= rec_end[-1]:
                bad = True
            else:
                s = int(np.searchsorted(rec_end, p, side="right"))
                src, v = sources[s], int(x["value_id"])
                n_frames = 0 if src.get("cmd_off") is None else len(src["cmd_off"]) - 1
                if v >= n_frames:
                    bad = True
                else:
                    lo, hi = int(src["cmd_off"][v]), int(src["cmd_off"][v + 1])
                    bad = hi < lo or hi > len(src["op"]) or hi - lo >= 0xFFFFFFFF
        else:
            s, lo, k = 0, int(x["first_cmd"]), int(x["n_cmds"])
            hi = lo + k
            bad = hi > len(sources[0]["op"]) or k == 0xFFFFFFFF
        if bad:
            inval = True
            if not dev:
                return dict(code=R.E_INVAL)
            continue
        if not 0 <= rel < n_inst:
            nil = True
            if not dev:
                return dict(code=R.E_NIL_INSTANCE)
            continue
        n_storing += 1
        command = Cmds(s, lo, hi - lo, item=i)
        if census is not None:
            census["empty_slice"] += hi == lo
            census["overwrites" if before[rel] is not None else "fills_nil"] += 1
        if kind == R.SC_SENDS:
            handle_propose_installed(space, rel, command)
        elif handler == "accept":
            handle_accept_stored(space, rel, command)
        else:
            handle_commit(space, rel, command)
    # the winners: what the slots hold now that this batch put there, in item order
    won = sorted((x.Cmds.item, rel) for rel, x in enumerate(space)
                 if x is not None and x.Cmds is not None and x.Cmds.item is not None)
    total = sum(space[rel].Cmds.n for _, rel in won)
    if census is not None:
        census["wins"] += len(won)
        census["superseded"] += n_storing - len(won)
        census["items"] += n
    if not dev and total >= 0xFFFFFFFF:
        return dict(code=R.E_UNSUPPORTED)
    code = R.E_NIL_INSTANCE if nil else R.E_INVAL if inval else R.OK
    full = used > cap or used + total > cap
    res = _result(len(won), total, n_storing - len(won), R.SC_FULL if full else 0)
    if not full:
        at = used
        for _, rel in won:
            c = space[rel].Cmds
            src = sources[c.src]
            a_op[at:at + c.n] = src["op"][c.first:c.first + c.n]
            a_key[at:at + c.n] = src["key"][c.first:c.first + c.n]
            a_val[at:at + c.n] = src["val"][c.first:c.first + c.n]
            inst[rel] = (at, c.n, R.IC_HAS_CMDS)
            at += c.n
        used = at
    return dict(op=a_op, key=a_key, val=a_val, used=used, inst=inst, res=res, code=code)


def store_compact(inst, arena, used, to_cap, dev=False, fill=None):
    """The reference's answer to one mpx_store_compact call: the instances that still have Cmds, in
    window order, keep them, laid out back to back in a new arena of to_cap commands (fill: what
    the target held before, default zeros). Returns a dict: op, key, val (the target), used, inst,
    res, code."""
    inst = np.array(inst, dtype=R.INST_CMDS, copy=True)
    f_op, f_key, f_val = arena
    t_op, t_key, t_val = (np.zeros(to_cap, t) for t in (np.uint8, np.int64, np.int64)) if fill is None \
        else (np.array(x, copy=True) for x in fill)
    if not dev and used > len(f_op):
        return dict(code=R.E_INVAL)
    bound = min(used, len(f_op))
    space = _space_of(inst)
    code, rows = R.OK, []
    for rel, x in enumerate(space):
        if x is None:
            continue
        c = x.Cmds
        if c.first > bound or c.n > bound - c.first or c.n == 0xFFFFFFFF:
            code = R.E_INVAL
            if not dev:
                return dict(code=code)
            c.first, c.n = 0, 0           # the device form: the slot contributes no commands
        rows.append((rel, c))
    total = sum(c.n for _, c in rows)
    if not dev and total >= 0xFFFFFFFF:
        return dict(code=R.E_UNSUPPORTED)
    full = total > to_cap
    res = _result(len(rows), total, 0, R.SC_FULL if full else 0)
    t_used = None
    if not full:
        at = 0
        for rel, c in rows:
            t_op[at:at + c.n] = f_op[c.first:c.first + c.n]
            t_key[at:at + c.n] = f_key[c.first:c.first + c.n]
            t_val[at:at + c.n] = f_val[c.first:c.first + c.n]
            inst[rel] = (at, c.n, R.IC_HAS_CMDS)
            at += c.n
        t_used = at
    return dict(op=t_op, key=t_key, val=t_val, used=t_used, inst=inst, res=res, code=code)


# ---- inputs ---------------------------------------------------------------------------------------
def mk_msgs(rows):
    """rows of (instance, value_id)"""
    a = np.zeros(len(rows), R.ACCEPT_MSG)
    for i, (instance, value_id) in enumerate(rows):
        a[i] = (instance, 7, 1, value_id)
    return a


def mk_sends(rows):
    """rows of (instance, flags, first_cmd, n_cmds)"""
    a = np.zeros(len(rows), R.ACCEPT_SEND)
    for i, (instance, flags, first, k) in enumerate(rows):
        a[i] = (instance, 7, -1, flags, first, k, 0)
    return a


def mk_cmds(n, seed=0):
    """n commands with distinctive fields"""
    rng = np.random.default_rng(91000 + seed)
    return (rng.integers(0, 6, n).astype(np.uint8), rng.integers(-(1 << 62), 1 << 62, n),
            rng.integers(-(1 << 62), 1 << 62, n))


def mk_source(sizes, n_recs=None, seed=0, gap=0):
    """one connection's unmarshal output: frame v has sizes[v] commands (gap: commands no frame
    names before each)"""
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.uint64)
    op, key, val = mk_cmds(int(off[-1]) + gap, seed)
    return dict(cmd_off=off, op=op, key=key, val=val, n_recs=len(sizes) if n_recs is None else n_recs)


def mk_arena(cap, seed=0):
    """an arena of cap commands whose unused part holds a recognisable pattern"""
    rng = np.random.default_rng(92000 + seed)
    return (rng.integers(100, 200, cap).astype(np.uint8), rng.integers(1, 1 << 40, cap),
            rng.integers(1, 1 << 40, cap))


def mk_window(n_inst, used, p_has, rng):
    """a window some of whose slots already have commands somewhere in [0, used)"""
    inst = np.zeros(n_inst, R.INST_CMDS)
    inst["first_cmd"] = 0xDEAD0000 + np.arange(n_inst)      # poison where the flag is clear
    inst["n_cmds"] = 0xBEEF
    for i in np.flatnonzero(rng.random(n_inst) < p_has):
        k = int(rng.integers(0, min(used, 4) + 1))
        inst[i] = (int(rng.integers(0, used - k + 1)), k, R.IC_HAS_CMDS)
    return inst


BRANCHES = ("wins", "superseded", "does_not_store", "keep", "empty_slice", "overwrites", "fills_nil")


def new_census():
    return dict({b: 0 for b in BRANCHES}, items=0)


def fuzz_case(seed, n_runs=None):
    """One call's arguments (a dict for store_commands / the engine's store_commands): odd seeds a
    proposer's sends, even seeds the merged messages of one to four connections through perm."""
    rng = np.random.default_rng(41000 + seed)
    n_inst = int(rng.integers(8, 400))
    base = int(rng.integers(-30, 900))
    n_runs = int(rng.integers(1, min(n_inst, 120))) if n_runs is None else n_runs
    where = np.sort(rng.choice(n_inst, n_runs, replace=False))
    used = int(rng.integers(0, 50))
    sizes_of = lambda k: rng.choice([0, 1, 2, 3, 17], k, p=[0.12, 0.4, 0.25, 0.18, 0.05])
    inst = mk_window(n_inst, used, 0.4, rng)
    big = int(rng.integers(0, n_runs)) if rng.random() < 0.25 else -1
    if seed % 2:
        rows, at = [], int(rng.integers(0, 5))
        for r, rel in enumerate(where):
            for _ in range(int(rng.choice([1, 1, 1, 2, 3]))):
                u = rng.random()
                flags = R.PH_ACCEPT if u < 0.5 else R.PH_PREPARE if u < 0.65 else \
                    R.PH_NOT_LEADER if u < 0.8 else R.PH_REFUSED
                k = 5000 if r == big else int(sizes_of(1)[0])
                instance = -1 if flags == R.PH_NOT_LEADER else base + int(rel)
                rows.append((instance, flags, at, k))
                at += k
        op, key, val = mk_cmds(at + 3, seed)
        case = dict(kind=R.SC_SENDS, items=mk_sends(rows),
                    sources=[dict(cmd_off=None, op=op, key=key, val=val, n_recs=len(rows))])
    else:
        n_src = int(rng.integers(1, 5))
        frames = [[] for _ in range(n_src)]
        msgs, eff, perm_src = [], [], []
        for r, rel in enumerate(where):
            for _ in range(int(rng.choice([1, 1, 2, 3, 4]))):
                s = int(rng.integers(0, n_src))
                u = rng.random()
                if u < 0.12:                       # a CommitShort
                    msgs.append((base + int(rel), R.VALUE_KEEP))
                    eff.append(int(rng.choice([0, R.CH_INSTALLED, R.CH_CMDS])))
                    frames[s].append(None)
                else:
                    frames[s].append(5000 if r == big and u > 0.6 else int(sizes_of(1)[0]))
                    msgs.append((base + int(rel), sum(f is not None for f in frames[s]) - 1))
                    eff.append(R.AH_STORED | R.AH_REPLIED if u > 0.42 else int(rng.choice([0, R.AH_REPLIED])))
                perm_src.append((s, len(frames[s]) - 1))
        sources = [mk_source([f for f in fr if f is not None], len(fr), seed * 8 + s, gap=s)
                   for s, fr in enumerate(frames)]
        rec_base = np.concatenate([[0], np.cumsum([len(fr) for fr in frames])])
        perm = np.array([rec_base[s] + r for s, r in perm_src], np.uint32)
        if n_src == 1 and rng.random() < 0.5:
            perm = None                            # one source in arrival order: perm is optional
        case = dict(kind=R.SC_MSGS, items=mk_msgs(msgs), sources=sources,
                    effect=np.array(eff, np.uint8), perm=perm,
                    handler="commit" if seed % 4 == 2 else "accept")
    case.update(inst=inst, inst_base=base, used=used)
    total = int(store_commands(arena=mk_arena(0), **dict(case, used=0))["res"]["n_cmds"])
    u = rng.random()
    cap = used + total + (0 if u < 0.3 else int(rng.integers(1, 300)))
    if u > 0.9 and total:
        cap = used + total - 1                     # the arena is short by one command
    case["arena"] = mk_arena(cap, seed)
    return case

"""Python transliteration of executeCommands' walk (bareminpaxos.go:1066-1098, paxos.go:675-706:
the same code) over Go-shaped objects: a Replica with an instanceSpace of *Instance whose Cmds may
be nil, committedUpTo and the walk's cursor i. Execute is recorded, not run: the call order of
Cmds[j].Execute is what the engine's gather must reproduce.

TEST INFRASTRUCTURE: the reference model of mpx_execute_gather for the CPU and GPU tests. Only
execute_gather() below knows the record layouts: it maps the call's records onto those objects
(one Replica per group: the sharded engine runs one replica's log per group), runs the Go loop
once per group in group order and reads the calls back as the engine's outputs, with the engine's
treatment of capacity, padding and faulty groups and instances (include/mpx.h).

Documented deviation: instanceSpace[i] == nil at or below committedUpTo, where
the Go dereferences nil, stops the walk like Cmds == nil; mpx_inst_cmds.flags == 0 stands for
both, so the adapter builds an Instance with Cmds nil for it."""
import numpy as np

from minpaxos_amd import records as R

NONE = 0  # state.NONE: Execute returns NIL and touches nothing (state.go:85-102)


class Instance:
    def __init__(self, cmds):
        self.Cmds = cmds             # None = nil; [] = an empty, non-nil slice


class Replica:
    """what executeCommands reads of a replica, and where its Execute calls land"""

    def __init__(self, instance_space, committed_upto):
        self.instanceSpace = instance_space   # dict: instance number -> *Instance
        self.committedUpTo = committed_upto
        self.calls = []                       # (instance, j, command) in Execute's call order
        self.ran = []                         # the instances the walk passed, in order


def execute_commands(r, i):
    """one turn of executeCommands' outer loop from cursor i (:1071-1091 / :680-699); returns the
    cursor it leaves (the Go keeps it in the local i)"""
    while i <= r.committedUpTo:                          # :1071 / :680
        if r.instanceSpace[i].Cmds is not None:          # :1072 / :681
            inst = r.instanceSpace[i]                    # :1073 / :682
            for j in range(len(inst.Cmds)):              # :1074 / :683
                r.calls.append((i, j, inst.Cmds[j]))     # :1075 / :684  val := Cmds[j].Execute(State)
            i += 1                                       # :1086 / :695
            r.ran.append(i - 1)
        else:
            break                                        # :1089 / :698
    return i


# ---- the call's records onto those objects -------------------------------------------------------
def execute_gather(inst, committed_upto, executed, cmds, inst_base=0, ipg=None, sends=None,
                   cap=None, pad=False, dev=False):
    """The reference's answer to one mpx_execute_gather call. Returns a dict: op, key, val (the
    commands below cap, then with pad the pad commands up to cap), mask, executed, inst_first,
    ret_first (None without sends), grp_cmd_off, res (EXECUTE_RESULT scalar), code, and order: the
    (instance, j) of every Execute call.
    dev=False: the host form, a faulty group or instance fails the call (only code is meaningful).
    dev=True: the device form: a faulty group does nothing, a faulty instance executes with no
    commands; code is what the next synchronising call answers."""
    inst = np.ascontiguousarray(inst, R.INST_CMDS)
    cu = np.atleast_1d(np.asarray(committed_upto, np.int64))
    ex = np.atleast_1d(np.asarray(executed, np.int64))
    op, key, val = (np.asarray(x) for x in cmds)
    n, G, n_src = len(inst), len(cu), len(op)
    ipg = (n // G if G else 0) if ipg is None else ipg
    assert n == G * ipg
    flags, firsts, counts = (inst[f].tolist() for f in ("flags", "first_cmd", "n_cmds"))
    faulty = []

    class Space:
        """instanceSpace, its *Instance made when the walk first reads it (so an instance whose
        command range leaves the source is judged only if the walk reaches it)"""

        def __getitem__(self, i):
            idx = i - inst_base
            if not flags[idx] & R.IC_HAS_CMDS:
                return Instance(None)
            first, k = firsts[idx], counts[idx]
            if first > n_src or k > n_src - first:
                faulty.append(i)
                return Instance([])     # the device form: it executes with no commands
            return Instance(range(first, first + k))

    code = R.OK
    mask = np.zeros(n, np.uint8)
    ex_out = ex.copy()
    lens = np.zeros(n, np.int64)
    order, src, grp_cmd_off, moved = [], [], [0], 0
    for g in range(G):
        first_g = inst_base + g * ipg
        if not all(first_g - 1 <= int(x) <= first_g + ipg - 1 for x in (cu[g], ex[g])):
            code = R.E_INVAL
            if not dev:
                return dict(code=code)
            grp_cmd_off.append(len(src))   # the device form: the group does nothing
            continue
        r = Replica(Space(), int(cu[g]))
        i = execute_commands(r, int(ex[g]) + 1)
        if faulty:
            code = R.E_INVAL
            if not dev:
                return dict(code=code)
        ex_out[g] = i - 1
        moved += ex_out[g] != ex[g]
        at = len(src)
        order += [(i, j) for i, j, _ in r.calls]
        src += [c for _, _, c in r.calls]
        if r.ran:
            lo, hi = r.ran[0] - inst_base, r.ran[-1] - inst_base + 1
            mask[lo:hi] = 1
            for i, _, _ in r.calls:
                lens[i - inst_base] += 1
        grp_cmd_off.append(len(src))
        assert len(src) - at == int(lens[g * ipg:(g + 1) * ipg].sum())
    total = len(src)
    if not dev and (n >= 0xFFFFFFFF or total >= 0xFFFFFFFF):
        return dict(code=R.E_UNSUPPORTED)
    cap = total if cap is None else cap
    n_real = min(total, cap)
    n_out = cap if pad else n_real
    take = np.asarray(src[:n_real], np.int64)
    o_op, o_key, o_val = np.zeros(n_out, np.uint8), np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
    o_op[:n_real], o_key[:n_real], o_val[:n_real] = op[take], key[take], val[take]
    o_op[n_real:], o_key[n_real:], o_val[n_real:] = NONE, np.arange(n_real, n_out), 0
    inst_first = np.concatenate([[0], np.cumsum(lens)])[:n].astype(np.uint64)
    ret_first = None
    if sends is not None:
        ret_first = np.zeros(len(sends), np.uint64)
        for s, x in enumerate(sends):
            rel = int(x["instance"]) - inst_base
            if 0 <= rel < n:
                ret_first[s] = inst_first[rel]
    res = np.zeros((), R.EXECUTE_RESULT)
    res["n_cmds"], res["n_inst"], res["n_groups"] = total, int(mask.sum()), moved
    return dict(op=o_op, key=o_key, val=o_val, mask=mask, executed=ex_out.astype(np.int32),
                inst_first=inst_first, ret_first=ret_first,
                grp_cmd_off=np.asarray(grp_cmd_off, np.uint64), res=res, code=code, order=order)


# ---- inputs ---------------------------------------------------------------------------------------
def mk_inst(rows):
    """rows of (first_cmd, n_cmds) for Cmds != nil, or None for Cmds == nil / a nil instance"""
    a = np.zeros(len(rows), R.INST_CMDS)
    for i, row in enumerate(rows):
        if row is not None:
            a[i] = (row[0], row[1], R.IC_HAS_CMDS)
    return a


def mk_cmds(n, seed=0):
    """n source commands with distinctive fields"""
    rng = np.random.default_rng(77000 + seed)
    return (rng.integers(0, 6, n).astype(np.uint8), rng.integers(-(1 << 62), 1 << 62, n),
            rng.integers(-(1 << 62), 1 << 62, n))


def mk_sends(instances):
    a = np.zeros(len(instances), R.ACCEPT_SEND)
    a["instance"] = instances
    a["flags"] = R.PH_ACCEPT
    return a


BRANCHES = ("stop_first", "stop_middle", "stop_last", "no_stop", "executed_is_committed",
            "executed_above_committed", "nothing_committed", "empty_slice")


def fuzz_case(seed, census=None, n_groups=None, ipg=None):
    """One call's arguments (a dict for execute_gather / Engine.execute_gather). Groups draw their
    cursors and their nil slots so that every branch of the walk comes up; census (optional dict):
    groups per BRANCHES and "groups"."""
    rng = np.random.default_rng(31000 + seed)
    G = int(rng.integers(1, 40)) if n_groups is None else n_groups
    ipg = int(rng.integers(1, 70)) if ipg is None else ipg
    base = int(rng.integers(-50, 1000))
    n = G * ipg
    sizes = rng.choice([0, 1, 2, 3, 16, 17], n, p=[0.1, 0.4, 0.2, 0.2, 0.05, 0.05])
    big = int(rng.integers(0, n)) if rng.random() < 0.3 else -1
    rows, at = [], int(rng.integers(0, 9))
    for i in range(n):
        k = 5000 if i == big else int(sizes[i])
        rows.append([at, k])
        at += k + (int(rng.integers(1, 4)) if rng.random() < 0.2 else 0)  # commands no slot names
    n_src = at + int(rng.integers(0, 5))
    cu, ex = np.zeros(G, np.int32), np.zeros(G, np.int32)
    for g in range(G):
        first = base + g * ipg
        u = rng.random()
        lo = first - 1 + int(rng.integers(0, ipg + 1))   # any legal cursor
        hi = first - 1 + int(rng.integers(0, ipg + 1))
        if u < 0.12:
            ex[g], cu[g], name = max(lo, hi), min(lo, hi), "executed_above_committed"
            if ex[g] == cu[g]:
                name = "executed_is_committed"
        elif u < 0.2:
            ex[g] = cu[g] = lo
            name = "executed_is_committed"
        elif u < 0.28:
            ex[g], cu[g], name = first - 1, first - 1, "nothing_committed"
        else:
            ex[g], cu[g] = min(lo, hi), max(lo, hi)
            span = int(cu[g] - ex[g])
            name = "no_stop"
            if span == 0:
                name = "executed_is_committed" if ex[g] >= first else "nothing_committed"
            elif rng.random() < 0.6:
                where = rng.random()
                k = 0 if where < 0.3 else span - 1 if where < 0.6 else int(rng.integers(0, span))
                rows[int(ex[g]) + 1 + k - base] = None
                name = "stop_first" if k == 0 else "stop_last" if k == span - 1 else "stop_middle"
        # nil slots outside the walk's range change nothing
        for _ in range(int(rng.integers(0, 3))):
            i = int(rng.integers(first, first + ipg))
            if not (ex[g] < i <= cu[g]):
                rows[i - base] = None
        if census is not None:
            census["groups"] = census.get("groups", 0) + 1
            census[name] = census.get(name, 0) + 1
            walked = [rows[i - base] for i in range(int(ex[g]) + 1, int(cu[g]) + 1)]
            if any(r is not None and r[1] == 0 for r in walked):
                census["empty_slice"] = census.get("empty_slice", 0) + 1
    case = dict(inst=mk_inst(rows), committed_upto=cu, executed=ex, cmds=mk_cmds(n_src, seed),
                inst_base=base, ipg=ipg)
    if seed % 2:
        inside = base + rng.integers(0, n, int(rng.integers(1, 30)))
        case["sends"] = mk_sends(np.concatenate([inside, [base - 1, base + n, -1]]).astype(np.int32))
    total = int(execute_gather(**case)["res"]["n_cmds"])
    u = rng.random()
    if u < 0.3:
        case["cap"] = max(total - int(rng.integers(1, 40)), 0)
    elif u < 0.7:
        case["pad"] = True
        case["cap"] = total + int(rng.integers(0, 1100))
    return case

"""mpx_encode_accepts_stored against the Go: an adapter, not a second transliteration.

bcastAccept and the Marshals stay where they are restated once, in tests/proposer_translit.py
(imported unchanged). This module only knows the store layout: from the acceptor window `st`, the
leader bookkeeping window `lb`, the slots' INST_CMDS and the command arena it builds the
Go-shaped log instance (ballot, status, cmds) that proposer_translit.bcast_accept_min asks for.

The status rule. The Go keeps one Status per instance; the engine keeps it in two windows:
mpx_propose_handle writes PREPARED into both st and lb, mpx_accept_tally moves only lb to
COMMITTED, the acceptor and commit handlers write only st. So an instance is nil exactly when st
says so, its Ballot is st's, and its Status is lb's wherever lb has one, else st's.
"""
import numpy as np

import proposer_translit as P
from go_translit import GoPanic
from minpaxos_amd import records as R


def log_instance(st, lb, inst, arena, k):
    """*r.instanceSpace[k] of the window (k a window index) as (ballot, status, cmds), or the nil
    dereference. An unflagged slot has Cmds == nil: no commands (V(0) on the wire)."""
    if int(st["status"][k]) == P.NIL:
        raise GoPanic(R.E_NIL_INSTANCE, f"*r.instanceSpace[{k}] is nil")
    status = int(st["status"][k])
    if lb is not None and int(lb["status"][k]) != P.NIL:
        status = int(lb["status"][k])
    cmds = []
    if int(inst["flags"][k]) & R.IC_HAS_CMDS:
        c0, nc = int(inst["first_cmd"][k]), int(inst["n_cmds"][k])
        if c0 > len(arena[0]) or nc > len(arena[0]) - c0:
            raise GoPanic(R.E_INVAL, f"slot {k}: commands [{c0}, {c0 + nc}) leave the arena")
        cmds = [(int(arena[0][j]), int(arena[1][j]), int(arena[2][j])) for j in range(c0, c0 + nc)]
    return int(st["ballot"][k]), status, cmds


def encode_accepts_stored(mode, N, sends, groups, cmds, inst_base=0, ipg=None, peer_commits=None,
                          st=None, lb=None, inst=None, arena=None, thrifty=False,
                          alive_mask=0xFFFF, note=None, want_frames=False):
    """proposer_translit.encode_accepts with the log taken from the store. note (optional list)
    receives per MIN frame (kind, [window indices of its log records])."""
    groups = np.atleast_1d(groups)
    G = len(groups)
    op, key, val = cmds
    if ipg is None:
        ipg = len(st) // G
    n_inst = G * ipg
    per = [[] for _ in range(N)]
    for s in sends:
        if not int(s["flags"]) & R.PH_ACCEPT:
            continue
        inst_no = int(s["instance"])
        idx = inst_no - inst_base
        if idx < 0 or idx >= n_inst:
            raise GoPanic(R.E_INVAL, "send outside the window")
        g = idx // ipg
        first = inst_base + g * ipg
        c0, nc = int(s["first_cmd"]), int(s["n_cmds"])
        command = [(int(op[j]), int(key[j]), int(val[j])) for j in range(c0, c0 + nc)]
        grp = groups[g]
        if not 0 <= int(grp["self_id"]) < N:
            raise GoPanic(R.E_INVAL, "self_id")
        r = P.Replica(N, grp, first, ipg, None, thrifty=thrifty, alive=alive_mask,
                      peer_commits=None if peer_commits is None else
                      [int(x) for x in np.asarray(peer_commits).reshape(G, N)[g]])
        r.crtInstance = inst_no + 1  # handlePropose has advanced it past instNo (:688)
        if mode == R.MODE_MIN:
            lc = int(s["last_committed"])
            if lc >= inst_no or lc < first - 1:
                raise GoPanic(R.E_INVAL, "last_committed")
            seen, kinds = [], []

            def log_inst(i):
                k = r.space(i) + g * ipg
                seen.append(k)
                return log_instance(st, lb, inst, arena, k)
            out = P.bcast_accept_min(r, inst_no, int(s["ballot"]), lc, command, log_inst, kinds)
            if note is not None:
                at = 0
                for kind, m in kinds:
                    note.append((kind, seen[at:at + m]))
                    at += m
        else:
            out = P.bcast_accept_classic(r, inst_no, int(s["ballot"]), command)
        for q, b in out:
            per[q].append(b)
    dest_off = np.zeros(N + 1, np.uint64)
    for q in range(N):
        dest_off[q + 1] = int(dest_off[q]) + sum(len(b) for b in per[q])
    by = np.frombuffer(b"".join(b"".join(x) for x in per), np.uint8)
    return (by, dest_off, per) if want_frames else (by, dest_off)


def dense_log(st, lb, inst, arena):
    """the window-ordered copy mpx_encode_accepts takes, built on the host from the same store:
    (LOG_REC[n_inst], cmd_off u64[n_inst + 1], op, key, val)"""
    n = len(st)
    rec = np.zeros(n, R.LOG_REC)
    rec["ballot"] = st["ballot"]
    rec["status"] = st["status"]
    if lb is not None:
        has = (lb["status"] != P.NIL) & (st["status"] != P.NIL)
        rec["status"][has] = lb["status"][has]
    k = np.where((inst["flags"] & R.IC_HAS_CMDS) != 0, inst["n_cmds"], 0).astype(np.int64)
    k[st["status"] == P.NIL] = 0
    coff = np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum(k)
    at = np.concatenate([np.arange(int(inst["first_cmd"][i]), int(inst["first_cmd"][i]) + int(k[i]))
                         for i in range(n)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rec, coff, arena[0][at], arena[1][at], arena[2][at]


def dense_args(a):
    """a stored case as proposer_translit.encode_accepts' / Engine.encode_accepts' arguments"""
    d = {k: v for k, v in a.items() if k not in ("st", "lb", "inst", "arena")}
    d["log"] = dense_log(a["st"], a["lb"], a["inst"], a["arena"])
    return d


def scatter(rng, log, lb_kind=0, p_unflag=0.5, p_share=0.3, dead=3, slack=0):
    """a dense log (proposer_translit.mk_log's tuple) as a store that marshals to the same bytes:
    the records' command ranges in a random order in the arena with up to `dead` dead commands
    between them; a record without commands unflagged with probability p_unflag; a record whose
    commands equal an earlier record's sharing that record's range with probability p_share (the
    dense log is changed to make them equal: the dense form of the result is dense_log's).
    lb_kind 0: no lb; 1: lb mirrors st, NIL at some slots and COMMITTED over others.
    Returns (st, lb, inst, arena)."""
    lrec, lcoff, lop, lkey, lval = log
    n = len(lrec)
    st = np.zeros(n, R.ACCEPTOR_STATE)
    st["status"], st["ballot"] = lrec["status"], lrec["ballot"]
    st["value_id"] = rng.integers(0, 1 << 20, n)
    inst = np.zeros(n, R.INST_CMDS)
    cnt = np.diff(lcoff.astype(np.int64))
    order = rng.permutation(n)
    op, key, val = [], [], []
    by_count = {}
    for i in order:
        c = int(cnt[i])
        if int(lrec["status"][i]) == P.NIL:
            inst[i] = (int(rng.integers(0, 1 << 40)), int(rng.integers(0, 9)), 0)
            continue
        if c == 0 and rng.random() < p_unflag:
            inst[i] = (int(rng.integers(0, 1 << 40)), int(rng.integers(0, 9)), 0)  # Cmds == nil
            continue
        if c and c in by_count and rng.random() < p_share:
            inst[i] = (by_count[c], c, R.IC_HAS_CMDS)
            continue
        for _ in range(int(rng.integers(0, dead + 1))):
            op.append(0xEE), key.append(-1), val.append(-1)
        inst[i] = (len(op), c, R.IC_HAS_CMDS)
        if c:
            by_count[c] = len(op)
        a = int(lcoff[i])
        op += lop[a:a + c].tolist()
        key += lkey[a:a + c].tolist()
        val += lval[a:a + c].tolist()
    for _ in range(slack):
        op.append(0xEE), key.append(-1), val.append(-1)
    lb = None
    if lb_kind:
        lb = np.zeros(n, R.INST_STATE)
        lb["status"] = st["status"]
        lb["accept_oks"] = rng.integers(0, 5, n)
        u = rng.random(n)
        lb["status"][u < 0.3] = P.NIL
        up = (u > 0.7) & (st["status"] != P.NIL)
        lb["status"][up] = P.COMMITTED
    return st, lb, inst, (np.array(op, np.uint8), np.array(key, np.int64), np.array(val, np.int64))


def fuzz_stored(seed, N, mode):
    """proposer_translit.fuzz_encode's case with its dense log scattered into a permuted arena.
    Returns encode_accepts_stored's arguments."""
    a = P.fuzz_encode(seed, N, mode)
    rng = np.random.default_rng(9000 + seed)
    st, lb, inst, arena = scatter(rng, a.pop("log"), lb_kind=seed % 3 != 0)
    return dict(a, st=st, lb=lb, inst=inst, arena=arena)


FRAME_KINDS = ("from_first", "from_pc", "empty", "no_cmds", "unflagged", "shared")


def frame_kinds(a, N):
    """of a MIN case's frames, the fraction that: take the log from first_g, from peer_commits +
    1, carry an empty log, a record without commands, an unflagged record, a record whose range
    another slot names too. Returns ({kind: count}, frames)."""
    note = []
    encode_accepts_stored(R.MODE_MIN, N, note=note, **a)
    inst = a["inst"]
    flagged = (inst["flags"] & R.IC_HAS_CMDS) != 0
    ranges = {}
    for i in np.flatnonzero(flagged & (inst["n_cmds"] > 0) & (a["st"]["status"] != P.NIL)):
        ranges.setdefault((int(inst["first_cmd"][i]), int(inst["n_cmds"][i])), []).append(int(i))
    shared = {i for v in ranges.values() if len(v) > 1 for i in v}
    c = dict.fromkeys(FRAME_KINDS, 0)
    for kind, ks in note:
        c["from_first"] += kind == "from_first" and len(ks) > 0
        c["from_pc"] += kind == "from_pc" and len(ks) > 0
        c["empty"] += len(ks) == 0
        c["no_cmds"] += any(not flagged[k] or int(inst["n_cmds"][k]) == 0 for k in ks)
        c["unflagged"] += any(not flagged[k] for k in ks)
        c["shared"] += any(k in shared for k in ks)
    return c, len(note)

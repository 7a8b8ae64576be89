"""GPU tests of the fused group step's edges, through mpx_group_step_dev and
mpx_group_step_totals_dev on guarded buffers.

Every input and every output of a call is its own devguard.Guard, the inputs sized exactly, so a
group without replies or without commands at an array's end really is the end of that array.
Results are bit-exact against oracle_lib.Oracle.group_step; afterwards every margin must still
hold the sentinel, and so must every output element the oracle does not write (ret / conf_prev of
commands that were not executed, st_out of instances without replies, table entries past a
group's count). All shapes run the 256-key, N = 5 fast-path variant: 1 to 67 groups of at most 256
instances, well under a second each. What they are chosen for:
  - the kernel's loads go out as one batch with clamped indices, and a group with no replies or no
    commands must not read those arrays at all: such groups first and last, one reply, one command
  - conf_prev and ret are written for the executed commands [x0, x1) of a group only, wherever
    the group's first command and that range fall: ragged command counts put them at every
    residue mod 16, the buffers run at shifts 0, 1, 8 and 15, and conf_prev may be NULL
  - the key lookup and the append of new keys in every table state: empty tables, no new key,
    exactly one, a full table with one more (MPX_E_KV_FULL), keys that share a home slot
  - a two-step sequence captured into a graph and replayed twice
No case provokes a fault: the error case is a table that is full, which the kernel reports.
"""

import numpy as np
import pytest

from devguard import Guard, sentinel_array
from oracle_lib import Oracle, OracleError
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import Arena
from minpaxos_amd.engine import MpxError

pytestmark = pytest.mark.gpu
N, K = 5, 256
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
MODES = [MIN, CLASSIC]
MODE_IDS = ["min", "classic"]
SHIFTS = (0, 1, 8, 15)
# the fast path's table: 512 slots, home = the top 9 bits of a 32-bit multiplicative hash scaled
# to the slot count (step.hip fhome)
SLOTS = 512


def fhome(key):
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    x = (k ^ (k >> 32)) & 0xFFFFFFFF
    return (((x * 0x9E3779B1) & 0xFFFFFFFF) * SLOTS) >> 32


def colliding_keys(n, home, start=1000):
    out, k = [], start
    while len(out) < n:
        if fhome(k) == home:
            out.append(k)
        k += 1
    return np.array(out, np.int64)


def same(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, \
        (name, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    k = max(got.size, 1)
    gb = got.reshape(-1).view(np.uint8).reshape(k, -1)
    wb = want.reshape(-1).view(np.uint8).reshape(k, -1)
    bad = np.flatnonzero((gb != wb).any(axis=1))
    i = bad[:4]
    raise AssertionError(f"{name}: {len(bad)} of {k} elements differ, first at {i.tolist()}: "
                         f"got {got.reshape(-1)[i]} want {want.reshape(-1)[i]}")


# ---- batches ---------------------------------------------------------------------------------------
def make_batch(seed, G, ipg, cmd_cnt, rec_cnt, keys, p_put=0.5, p_ok=0.8, executed_in=None,
               nil=None, has_cmds=None):
    """a group batch with `cmd_cnt[g, i]` commands and `rec_cnt[g, i]` replies (at most N - 1, from
    distinct replicas) of instance i of group g; group g's keys are drawn from keys[g]. executed_in:
    per group (committed_in = executed_in); nil: (g, i) pairs of nil instances (they get no replies);
    has_cmds: (g, i) pairs whose has_cmds byte is 0 (every other one 1), None = no array"""
    rng = np.random.default_rng(seed)
    cmd_cnt = np.array(cmd_cnt, np.int64).reshape(G, ipg)
    rec_cnt = np.array(rec_cnt, np.int64).reshape(G, ipg)
    st = np.zeros(G * ipg, R.INST_STATE)
    st["status"] = R.PREPARED
    for g, i in nil or ():
        st["status"][g * ipg + i] = R.STATUS_NIL
        rec_cnt[g, i] = 0
    n = int(rec_cnt.sum())
    assert n > 0 and rec_cnt.max() <= N - 1
    flat = rec_cnt.reshape(-1)
    rec = np.zeros(n, R.ACCEPT_REPLY)
    rec["instance"] = np.repeat(np.tile(np.arange(ipg, dtype=np.int32), G), flat)
    ids = np.argsort(rng.random((G * ipg, N - 1)), axis=1) + 1  # a permutation of 1..N-1 each
    rec["id"] = ids[np.repeat(np.arange(G * ipg), flat),
                    np.concatenate([np.arange(c) for c in flat]) if n else []]
    rec["ok"] = rng.random(n) < p_ok
    rec["ballot"] = 16 + 16 * rng.integers(0, 3, n)
    grp_rec_off = np.concatenate([[0], np.cumsum(rec_cnt.sum(axis=1))]).astype(np.uint64)
    cmd_off = np.concatenate([[0], np.cumsum(cmd_cnt.reshape(-1))]).astype(np.uint32)
    m = int(cmd_off[-1])
    assert m > 0
    per_group = cmd_cnt.sum(axis=1)
    assert per_group.max() <= 1024 and rec_cnt.sum(axis=1).max() <= 1024  # the fast path's image
    key = np.concatenate([np.asarray(keys[g], np.int64)[rng.integers(0, len(keys[g]), c)]
                          for g, c in enumerate(per_group)])
    op = np.where(rng.random(m) < p_put, R.OP_PUT, R.OP_GET).astype(np.uint8)
    val = (np.arange(m, dtype=np.int64) + 1) * 1000003 + seed
    ex = np.full(G, -1, np.int32) if executed_in is None else np.array(executed_in, np.int32)
    hc = None
    if has_cmds is not None:
        hc = np.ones(G * ipg, np.uint8)
        for g, i in has_cmds:
            hc[g * ipg + i] = 0
    return dict(n_groups=G, ipg=ipg, n_replicas=N, recs=rec, grp_rec_off=grp_rec_off, st_in=st,
                committed_in=ex.copy(), executed_in=ex, op=op, key=key, val=val, cmd_off=cmd_off,
                peer_in=rng.integers(-1, 40, G * N).astype(np.int32), has_cmds=hc)


def executed_mask(b, want):
    """the commands the step executed: those of instances executed_in + 1 .. executed_out"""
    G, ipg = b["n_groups"], b["ipg"]
    mask = np.zeros(len(b["op"]), bool)
    for g in range(G):
        lo = max(int(b["executed_in"][g]) + 1, 0)
        hi = int(want["executed_out"][g])
        if hi >= lo:
            mask[int(b["cmd_off"][g * ipg + lo]):int(b["cmd_off"][g * ipg + hi + 1])] = True
    return mask


def oracle_step(mode, b, kv):
    """the oracle's outputs for batch b on tables kv = (cnt, key, val); ret starts as the sentinel,
    so the commands the oracle does not execute keep it"""
    m = len(b["op"])
    return Oracle(N, mode, kv_per_group=K).group_step(
        b, kv_cnt=kv[0], kv_key=kv[1], kv_val=kv[2], ret=sentinel_array(m, np.int64))


def empty_tables(G):
    return np.zeros(G, np.uint32), np.zeros(G * K, np.int64), np.zeros(G * K, np.int64)


class StepDev:
    """one batch on the device: every array a Guard of its own"""
    IN = (("recs", R.ACCEPT_REPLY), ("grp_rec_off", np.uint64), ("st_in", R.INST_STATE),
          ("committed_in", np.int32), ("executed_in", np.int32), ("peer_in", np.int32),
          ("op", np.uint8), ("key", np.int64), ("val", np.int64), ("cmd_off", np.uint32))

    def __init__(self, e, ar, b, kv, shift=0, conf=True, totals=False, kv_out=None):
        self.e, self.b, self.totals = e, b, totals
        G, ipg, m = b["n_groups"], b["ipg"], len(b["op"])
        self.g_in = {name: Guard(ar, len(b[name]), dt, name=name).put(b[name])
                     for name, dt in self.IN}
        self.g_has = None if b.get("has_cmds") is None else \
            Guard(ar, G * ipg, np.uint8, name="has_cmds").put(b["has_cmds"])
        # tables: kv is host arrays (staged here) or the output Guards of an earlier step
        if isinstance(kv[0], Guard):
            self.g_kv_in = kv
        else:
            self.g_kv_in = tuple(Guard(ar, len(a), dt, name="kv_in_" + nm).put(a)
                                 for a, dt, nm in zip(kv, (np.uint32, np.int64, np.int64),
                                                      ("cnt", "key", "val")))
        self.g_kv_out = kv_out or (Guard(ar, G, np.uint32, name="kv_cnt_out"),
                                   Guard(ar, G * K, np.int64, name="kv_key_out"),
                                   Guard(ar, G * K, np.int64, name="kv_val_out"))
        self.out = dict(
            st_out=Guard(ar, G * ipg, R.INST_STATE, name="st_out"),
            committed_out=Guard(ar, G, np.int32, name="committed_out"),
            executed_out=Guard(ar, G, np.int32, name="executed_out"),
            peer_out=Guard(ar, G * N, np.int32, name="peer_out"),
            ret=Guard(ar, m, np.int64, shift=8 * (shift % 2), name="ret"),
            decided=Guard(ar, G * ipg, np.uint8, shift=shift, name="decided"),
            n_decided=Guard(ar, G, np.uint32, name="n_decided"))
        self.g_conf = Guard(ar, m, np.uint8, shift=shift, name="conf_prev") if conf else None
        self.g_tot = Guard(ar, 3, np.int64, name="totals") if totals else None
        i, o = self.g_in, self.out
        ptr = [i["recs"].ptr, i["grp_rec_off"].ptr, i["st_in"].ptr, o["st_out"].ptr,
               i["committed_in"].ptr, o["committed_out"].ptr, i["executed_in"].ptr,
               o["executed_out"].ptr, i["peer_in"].ptr, o["peer_out"].ptr, i["op"].ptr,
               i["key"].ptr, i["val"].ptr, i["cmd_off"].ptr,
               self.g_has.ptr if self.g_has else None, o["ret"].ptr,
               self.g_conf.ptr if conf else None, *[g.ptr for g in self.g_kv_in],
               *[g.ptr for g in self.g_kv_out], o["decided"].ptr, o["n_decided"].ptr]
        self.gb = _lib.MpxGroupBatch(G, ipg, *ptr)

    def outputs(self):
        return list(self.out.values()) + list(self.g_kv_out) + \
            [g for g in (self.g_conf, self.g_tot) if g is not None]

    def refill(self, s=None):
        for g in self.outputs():
            g.fill(s)

    def call(self, s=None):
        if self.totals:
            self.e.group_step_totals_dev(self.gb, self.g_tot.ptr, s)
        else:
            self.e.group_step_dev(self.gb, s)

    def check(self, want, what=""):
        """every output against the oracle's, every margin, every element that must be left alone;
        the inputs unchanged"""
        b, G, ipg = self.b, self.b["n_groups"], self.b["ipg"]
        for name, g in self.g_in.items():
            same(f"{what}input {name}", g.assert_margins(), np.ascontiguousarray(b[name], g.dtype))
        if self.g_has:
            same(what + "input has_cmds", self.g_has.assert_margins(), b["has_cmds"])
        got = {name: g.assert_margins() for name, g in self.out.items()}
        for name in ("committed_out", "executed_out", "peer_out", "decided", "n_decided"):
            same(what + name, got[name], want[name])
        # instance state: written for the instances that have replies, nothing else touched
        touched = np.zeros(G * ipg, bool)
        rec_group = np.repeat(np.arange(G), np.diff(b["grp_rec_off"]).astype(np.int64))
        touched[rec_group * ipg + b["recs"]["instance"]] = True
        same(what + "st_out[touched]", got["st_out"][touched], want["st_out"][touched])
        self.out["st_out"].assert_untouched(~touched)
        same(what + "st_out = st_in elsewhere", want["st_out"][~touched], b["st_in"][~touched])
        # results: the executed commands', the others still the sentinel
        ex = executed_mask(b, want)
        same(what + "ret", got["ret"], want["ret"])  # (the oracle's started as the sentinel)
        self.out["ret"].assert_untouched(~ex)
        assert not (want["ret"][ex] == sentinel_array(1, np.int64)[0]).any()
        if self.g_conf:
            conf = self.g_conf.assert_margins()
            same(what + "conf_prev[executed]", conf[ex], want["conf_prev"][ex])
            self.g_conf.assert_untouched(~ex)
        # tables: each group's entries up to its count, the rest of its row left alone
        cnt, kk, kv = (g.assert_margins() for g in self.g_kv_out)
        same(what + "kv_cnt", cnt, want["kv_cnt"])
        live = (np.arange(K)[None, :] < want["kv_cnt"][:, None]).reshape(-1)
        same(what + "kv_key", kk[live], want["kv_key"][live])
        same(what + "kv_val", kv[live], want["kv_val"][live])
        self.g_kv_out[1].assert_untouched(~live)
        self.g_kv_out[2].assert_untouched(~live)
        if self.totals:
            n_inst = sum(max(int(want["executed_out"][g]) - max(int(b["executed_in"][g]) + 1, 0) + 1, 0)
                         for g in range(G))
            same(what + "totals", self.g_tot.assert_margins(),
                 np.array([int(want["n_decided"].sum()), n_inst, int(ex.sum())], np.int64))
        return ex


def done(e, s=None):
    e.stream_synchronize(s)
    e.synchronize()


# ---- empty groups at an array's end, odd counts, every residue of the executed range ---------------
G_MIX, IPG_MIX = 67, 48
# seeds at which the asserts of mixed_want hold for both modes (found by trying 0, 1, 2, ...)
MIX_SEED = {"a": 1, "b": 1}
_mixed = {}


def mixed_batch(which):
    """67 groups of 48 instances with 0 to 5 commands and 0 to 4 replies per instance.
    "a": group 0 has no replies, the last group no commands (op / key / val end at the group
    before it); "b": group 0 has no commands, the last group no replies (recs ends at the group
    before it) and a has_cmds array stops some groups early. In both: group 1 has one reply,
    group 2 one command, every fifth group starts executing at instance 5, every seventh has a
    nil instance inside its committed range."""
    if which in _mixed:
        return _mixed[which]
    rng = np.random.default_rng(MIX_SEED[which])
    G, ipg = G_MIX, IPG_MIX
    cmd = rng.integers(0, 6, (G, ipg))
    rec = np.full((G, ipg), N - 1)
    rec[rng.random((G, ipg)) < 0.04] = 0
    rec[rng.random((G, ipg)) < 0.1] = 2
    norec, nocmd = (0, G - 1) if which == "a" else (G - 1, 0)
    rec[norec] = 0
    cmd[nocmd] = 0
    rec[1] = 0
    rec[1, 7] = 1
    cmd[2] = 0
    cmd[2, 0] = 1
    ex = np.full(G, -1, np.int32)
    ex[3::5] = 4
    nil = [(g, 20) for g in range(5, G, 7)]
    has = [(g, 30) for g in range(1, G, 6)] if which == "b" else None
    keys = [rng.integers(-(1 << 62), 1 << 62, 40) for _ in range(G)]
    b = make_batch(1000 + ord(which), G, ipg, cmd, rec, keys, p_ok=0.9, executed_in=ex, nil=nil,
                   has_cmds=has)
    assert b["grp_rec_off"][norec] == b["grp_rec_off"][norec + 1]
    assert b["cmd_off"][nocmd * ipg] == b["cmd_off"][(nocmd + 1) * ipg]
    _mixed[which] = b
    return b


_mixed_want = {}


def mixed_want(mode, which):
    k = (mode, which)
    if k not in _mixed_want:
        b = mixed_batch(which)
        want = oracle_step(mode, b, empty_tables(G_MIX))
        ex = executed_mask(b, want)
        # the shape does what it is for: the first command of a group, and the first and the last
        # executed command of a group, at every residue mod 16; ranges strictly inside a group;
        # groups that execute nothing
        G, ipg = G_MIX, IPG_MIX
        c_lo = b["cmd_off"][np.arange(G) * ipg].astype(np.int64)
        c_hi = b["cmd_off"][np.arange(1, G + 1) * ipg].astype(np.int64)
        first = np.array([np.flatnonzero(ex[a:z])[0] + a if ex[a:z].any() else -1
                          for a, z in zip(c_lo, c_hi)])
        last = np.array([np.flatnonzero(ex[a:z])[-1] + a if ex[a:z].any() else -1
                         for a, z in zip(c_lo, c_hi)])
        some = first >= 0
        assert set(c_lo % 16) == set(range(16))
        assert set(first[some] % 16) == set(range(16)) and set((last[some] + 1) % 16) == set(range(16))
        assert ((first > c_lo) & some).sum() >= 5 and ((last + 1 < c_hi) & some).sum() >= 5
        assert (~some).sum() >= 1 and ((last - first < 16) & some).sum() >= 1
        _mixed_want[k] = want
    return _mixed_want[k]


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ragged_groups_at_every_shift(mk_engine, mode, which, shift):
    """conf_prev / decided at an address that is 0, 1, 8 or 15 mod 16 (ret at 0 or 8), with the
    step totals on the odd shifts"""
    e = mk_engine(N, mode, kv_per_group=K)
    b, want = mixed_batch(which), mixed_want(mode, which)
    with Arena(e) as ar:
        d = StepDev(e, ar, b, empty_tables(G_MIX), shift=shift, totals=shift % 2 == 1)
        d.call()
        done(e)
        d.check(want)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_null_conf_prev_and_one_group(mk_engine, mode):
    """conf_prev = NULL: everything else as before; then the grid's smallest shape, one group"""
    e = mk_engine(N, mode, kv_per_group=K)
    b, want = mixed_batch("a"), mixed_want(mode, "a")
    with Arena(e) as ar:
        d = StepDev(e, ar, b, empty_tables(G_MIX), shift=1, conf=False)
        d.call()
        done(e)
        d.check(want)
        rng = np.random.default_rng(77)
        one = make_batch(78, 1, 256, rng.integers(0, 6, (1, 256)), np.full((1, 256), N - 1),
                         [np.arange(200) * 7919 - 5000], p_ok=1.0)
        d = StepDev(e, ar, one, empty_tables(1), shift=15, totals=True)
        d.call()
        done(e)
        ex = d.check(oracle_step(mode, one, empty_tables(1)))
        assert ex.sum() > 300


# ---- keys across table states ------------------------------------------------------------------------
def key_sets(G):
    """per group 100 keys; group 1's include 8 that share a home slot, and 8 in the slots after
    it, so the probes of the first run through the second"""
    rng = np.random.default_rng(31)
    keys = [rng.integers(-(1 << 40), 1 << 40, 100) for _ in range(G)]
    home = 137
    clash = np.concatenate([colliding_keys(8, home), colliding_keys(8, home + 3, start=50000)])
    assert len({fhome(k) for k in clash[:8]}) == 1
    keys[1] = np.concatenate([clash, keys[1][:84]])
    keys[G - 1] = colliding_keys(6, SLOTS - 1)  # ... and a run that wraps past the last slot
    return keys


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_keys_new_known_and_colliding(mk_engine, mode):
    """empty tables (every key new), then the same keys on the tables that step left (none new),
    then one new key in one group; the tables travel from step to step on the device"""
    e = mk_engine(N, mode, kv_per_group=K)
    G, ipg = 5, 64
    keys = key_sets(G)
    full = np.full((G, ipg), N - 1)
    b1 = make_batch(41, G, ipg, np.full((G, ipg), 4), full, keys, p_ok=1.0)
    w1 = oracle_step(mode, b1, empty_tables(G))
    assert (w1["executed_out"] == ipg - 1).all() and (w1["kv_cnt"] > 0).all()
    t1 = (w1["kv_cnt"], w1["kv_key"], w1["kv_val"])
    # every key of the second step is in the tables: it uses the keys step 1 PUT
    keys2 = [t1[1][g * K:g * K + int(t1[0][g])] for g in range(G)]
    b2 = make_batch(42, G, ipg, np.full((G, ipg), 4), full, keys2, p_ok=1.0)
    w2 = oracle_step(mode, b2, t1)
    same("no key new", w2["kv_cnt"], w1["kv_cnt"])
    t2 = (w2["kv_cnt"], w2["kv_key"], w2["kv_val"])
    # ... and the third step's too, but for one PUT of a new key in the middle of group 2
    b3 = make_batch(43, G, ipg, np.full((G, ipg), 4), full, keys2, p_ok=1.0)
    at = int(b3["cmd_off"][2 * ipg + 31]) + 2
    b3["key"][at], b3["op"][at] = 0x7777777777, R.OP_PUT
    assert 0x7777777777 not in keys2[2]
    w3 = oracle_step(mode, b3, t2)
    same("one key new", w3["kv_cnt"], w2["kv_cnt"] + (np.arange(G) == 2).astype(np.uint32))
    with Arena(e) as ar:
        d1 = StepDev(e, ar, b1, empty_tables(G), shift=1)
        d1.call()
        done(e)
        d1.check(w1, "step 1: ")
        d2 = StepDev(e, ar, b2, d1.g_kv_out, shift=8, totals=True)
        d2.call()
        done(e)
        d2.check(w2, "step 2: ")
        d3 = StepDev(e, ar, b3, d2.g_kv_out, shift=15)
        d3.call()
        done(e)
        d3.check(w3, "step 3: ")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_full_table_one_more_key(mk_engine, mode):
    """group 1's table holds kv_per_group keys: GETs and PUTs of those run as ever, one PUT of a
    new key is MPX_E_KV_FULL from the engine as from the oracle; nothing outside the outputs is
    written"""
    e = mk_engine(N, mode, kv_per_group=K)
    G, ipg = 3, 32
    keys = [np.arange(K, dtype=np.int64) * 3 + 11 + 1000 * g for g in range(G)]
    cnt = np.array([10, K, K - 1], np.uint32)
    kk, kv = np.zeros(G * K, np.int64), np.zeros(G * K, np.int64)
    for g in range(G):
        kk[g * K:g * K + cnt[g]] = keys[g][:cnt[g]]
        kv[g * K:g * K + cnt[g]] = keys[g][:cnt[g]] * 5
    b = make_batch(51, G, ipg, np.full((G, ipg), 4), np.full((G, ipg), N - 1), keys, p_ok=1.0)
    # every key is in its group's table, except the one group 2 lacks: its table fills exactly
    b["key"][int(b["cmd_off"][2 * ipg]) + 1], b["op"][int(b["cmd_off"][2 * ipg]) + 1] = \
        keys[2][K - 1], R.OP_PUT
    lack = b["key"][int(b["cmd_off"][2 * ipg]):] == keys[2][K - 1]
    b["op"][int(b["cmd_off"][2 * ipg]):][lack] = R.OP_PUT
    want = oracle_step(mode, b, (cnt, kk, kv))
    assert int(want["kv_cnt"][2]) == K and int(want["kv_cnt"][1]) == K
    with Arena(e) as ar:
        d = StepDev(e, ar, b, (cnt, kk, kv), shift=8)
        d.call()
        done(e)
        d.check(want, "full, no new key: ")
        # one more key for the full table of group 1
        at = int(b["cmd_off"][1 * ipg + 9])
        b2 = dict(b, key=b["key"].copy(), op=b["op"].copy())
        b2["key"][at], b2["op"][at] = -424242, R.OP_PUT
        with pytest.raises(OracleError) as oi:
            oracle_step(mode, b2, (cnt, kk, kv))
        assert oi.value.code == R.E_KV_FULL
        d = StepDev(e, ar, b2, (cnt, kk, kv), shift=8)
        d.call()
        with pytest.raises(MpxError) as ei:
            done(e)
        assert ei.value.code == R.E_KV_FULL
        for g in list(d.g_in.values()) + d.outputs():
            g.assert_margins()
        # the other groups' results are what they were, and the full group's table keeps its keys
        same("kv_cnt", d.g_kv_out[0].payload(), want["kv_cnt"])
        same("group 1 keys", d.g_kv_out[1].payload()[K:2 * K], kk[K:2 * K])
        lo, hi = int(b["cmd_off"][2 * ipg]), len(b["op"])
        same("group 2 ret", d.out["ret"].payload()[lo:hi], want["ret"][lo:hi])
        same("group 2 conf_prev", d.g_conf.payload()[lo:hi], want["conf_prev"][lo:hi])


# ---- graph replay --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_two_steps_captured_and_replayed(mk_engine, mode):
    """step 1 on empty tables and step 2 on its output tables, both with totals, captured on one
    stream into one graph and replayed twice over refilled outputs"""
    e = mk_engine(N, mode, kv_per_group=K)
    b1 = mixed_batch("a")
    w1 = mixed_want(mode, "a")
    b2 = mixed_batch("b")
    w2 = oracle_step(mode, b2, (w1["kv_cnt"], w1["kv_key"], w1["kv_val"]))
    s = e.stream_create()
    try:
        with Arena(e) as ar:
            d1 = StepDev(e, ar, b1, empty_tables(G_MIX), shift=1, totals=True)
            d2 = StepDev(e, ar, b2, d1.g_kv_out, shift=15, totals=True)
            d1.call(s)  # once eagerly on the stream that will capture them
            d2.call(s)
            done(e, s)
            d1.check(w1, "eager step 1: ")
            d2.check(w2, "eager step 2: ")
            e.graph_begin(s)
            d1.call(s)
            d2.call(s)
            graph = e.graph_end(s)
            try:
                for rep in range(2):
                    d1.refill(s)
                    d2.refill(s)
                    e.graph_launch(graph, s)
                    done(e, s)
                    d1.check(w1, f"replay {rep} step 1: ")
                    d2.check(w2, f"replay {rep} step 2: ")
            finally:
                e.graph_destroy(graph)
    finally:
        e.stream_destroy(s)

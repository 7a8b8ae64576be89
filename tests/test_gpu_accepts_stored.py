"""GPU tests of mpx_encode_accepts_stored (the Accept frames with the catch-up log read from the
instance store), host and device forms, byte-exact against tests/accepts_stored_translit.py and
identical with mpx_encode_accepts fed the dense log built on the host from the same store. Shapes
are the smallest that reach each path: the output window is 8192 bytes, the item chunk 256, a scan
tile 4096 slots. In the device form `out`, `dest_off` and the arena sit on guards exactly their
capacity long."""
import numpy as np
import pytest

import accepts_stored_kat as K
import accepts_stored_translit as S
import proposer_translit as P
import test_gpu_proposer as TP
from devguard import Guard
from go_translit import GoPanic
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError

pytestmark = pytest.mark.gpu
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
WINDOW = 8192
STORE = ("st", "lb", "inst", "arena")


def stored(a, seed=0, **kw):
    """a test_gpu_proposer / proposer_translit case (dense log) as a stored case"""
    a = dict(a)
    st, lb, inst, arena = S.scatter(np.random.default_rng(700 + seed), a.pop("log"), **kw)
    return dict(a, st=st, lb=lb, inst=inst, arena=arena)


def dev_batch(ar, a, op_shift=1, thrifty=None, alive_mask=None, null_store=False):
    """device copies of a stored case as an MpxAcceptStoreBatch; the arena on guards exactly its
    size, src_op (and cmd_op) at an odd address"""
    thrifty = a.get("thrifty", False) if thrifty is None else thrifty
    alive_mask = a.get("alive_mask", 0xFFFF) if alive_mask is None else alive_mask
    op, key, val = a["cmds"]
    keep = dict(sends=ar.put(a["sends"]), groups=ar.put(a["groups"]),
                op=Guard(ar, len(op), np.uint8, shift=op_shift).put(op), key=ar.put(key),
                val=ar.put(val))
    b = _lib.MpxAcceptStoreBatch()
    b.sends, b.n_sends, b.inst_base, b.ipg = keep["sends"].ptr, len(a["sends"]), a["inst_base"], a["ipg"]
    b.n_groups, b.groups = len(a["groups"]), keep["groups"].ptr
    b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = keep["op"].ptr, keep["key"].ptr, keep["val"].ptr, len(op)
    b.flags, b.alive_mask = (R.AB_THRIFTY if thrifty else 0), alive_mask
    if a.get("peer_commits") is not None and not null_store:
        keep["pc"] = ar.put(np.ascontiguousarray(a["peer_commits"], np.int32))
        b.peer_commits = keep["pc"].ptr
    if not null_store:
        sop, skey, sval = a["arena"]
        keep.update(st=ar.put(a["st"]), inst=ar.put(a["inst"]),
                    sop=Guard(ar, len(sop), np.uint8, shift=op_shift).put(sop),
                    skey=Guard(ar, len(sop), np.int64).put(skey),
                    sval=Guard(ar, len(sop), np.int64).put(sval))
        b.st, b.inst = keep["st"].ptr, keep["inst"].ptr
        b.src_op, b.src_key, b.src_val, b.n_src = keep["sop"].ptr, keep["skey"].ptr, keep["sval"].ptr, len(sop)
        if a["lb"] is not None:
            keep["lb"] = ar.put(a["lb"])
            b.lb = keep["lb"].ptr
    return b, keep


def run_dev(e, n, a, out_cap, out_shift=0, **kw):
    """the _dev form on guarded buffers; returns (out[:out_cap] as written, dest_off)"""
    with Arena(e) as ar:
        b, keep = dev_batch(ar, a, **kw)
        g_out, g_off = Guard(ar, out_cap, np.uint8, shift=out_shift), Guard(ar, n + 1, np.uint64)
        e.encode_accepts_stored_reserve(len(a["sends"]), len(a["groups"]) * a["ipg"])
        e.encode_accepts_stored_dev(b, g_out.ptr, out_cap, g_off.ptr)
        e.synchronize()
        for k in ("op", "sop", "skey", "sval"):
            if k in keep:
                keep[k].assert_margins()
        return g_out.assert_margins(), g_off.assert_margins()


def same_bytes(out, want, what):
    if out.tobytes() != want.tobytes():
        m = min(len(out), len(want))
        bad = np.flatnonzero(out[:m] != want[:m])
        raise AssertionError(f"{what}: lengths {len(out)} / {len(want)}, {len(bad)} bytes differ, "
                             f"first at {bad[:8]}")


def check(e, mode, n, a, dense=True, decode=False, forms=("host", "dev"), **kw):
    """both forms against the transliteration; the dense encoder on the host-built log gives the
    same bytes; optionally every destination's run decodes back to the stored instances"""
    note = []
    w_out, w_off, per = S.encode_accepts_stored(mode, n, want_frames=True, note=note, **a, **kw)
    if "host" in forms:
        out, off = e.encode_accepts_stored(**a, **kw)
        assert np.array_equal(off, w_off), (off, w_off)
        same_bytes(out, w_out, "host form")
    if "dev" in forms:
        out, off = run_dev(e, n, a, len(w_out), **kw)
        assert np.array_equal(off, w_off), (off, w_off)
        same_bytes(out, w_out, "device form")
    if dense:
        d = S.dense_args(a) if mode == MIN else {k: v for k, v in a.items() if k not in STORE}
        d_out, d_off = e.encode_accepts(**d, **kw)
        assert np.array_equal(d_off, w_off)
        same_bytes(d_out, w_out, "mpx_encode_accepts on the dense log")
    if decode:
        check_round_trip(e, mode, n, a, w_out, w_off, per, note, **kw)
    return w_out, w_off, per


def check_round_trip(e, mode, n, a, out, off, per, note, thrifty=None, alive_mask=None):
    """mpx_decode_stream -> mpx_unmarshal_frames of each destination's run: the frames' catch-up
    logs are the stored instances (ballot, status by the lb rule, commands from the arena)"""
    thrifty = a.get("thrifty", False) if thrifty is None else thrifty
    by_dest = {q: [] for q in range(n)}
    if mode == MIN:  # note is in send order, destination by ring order: regroup by destination
        at = 0
        for s in a["sends"]:
            if not int(s["flags"]) & R.PH_ACCEPT:
                continue
            g = (int(s["instance"]) - a["inst_base"]) // a["ipg"]
            self_id = int(np.atleast_1d(a["groups"])[g]["self_id"])
            want = n >> 1 if thrifty else n - 1
            for k in range(min(want, n - 1)):
                by_dest[(self_id + 1 + k) % n].append(note[at][1])
                at += 1
        assert at == len(note)
    for q in range(n):
        run = out[int(off[q]):int(off[q + 1])]
        TP.check_decode(e, mode, per[q], run)
        if mode != MIN or not len(run):
            continue
        var = e.decode_stream(run.tobytes())[2]
        arrays, res = e.unmarshal_frames(run.tobytes(), var)
        slots = [k for ks in by_dest[q] for k in ks]
        assert int(res["n_log_inst"]) == len(slots) and int(res["n_accepts"]) == len(per[q])
        inst = [S.log_instance(a["st"], a["lb"], a["inst"], a["arena"], k) for k in slots]
        assert arrays["log_recs"]["ballot"].tolist() == [x[0] for x in inst]
        assert arrays["log_recs"]["status"].tolist() == [x[1] for x in inst]
        assert np.diff(arrays["log_cmd_off"].astype(np.int64)).tolist() == [len(x[2]) for x in inst]
        cmds = [c for x in inst for c in x[2]]
        assert list(zip(arrays["log_op"].tolist(), arrays["log_key"].tolist(),
                        arrays["log_val"].tolist())) == cmds


# ---- the known answers -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_known_answers(mk_engine, name):
    a, want, want_off = K.CASES[name]
    e = mk_engine(K.N, MIN)
    out, off = e.encode_accepts_stored(**a)
    assert off.tolist() == want_off.tolist() and out.tobytes() == want.tobytes()
    out, off = run_dev(e, K.N, a, len(want))
    assert off.tolist() == want_off.tolist() and out.tobytes() == want.tobytes()
    check(e, MIN, K.N, a, decode=True)


def test_known_answer_classic_with_null_store(mk_engine):
    """CLASSIC frames carry no log: st / lb / inst / src_* are not read and may be null"""
    a = dict(K.CASES["self2_lb_null"][0], peer_commits=None)
    e = mk_engine(K.N, CLASSIC)
    want = bytes.fromhex("09 02000000 67000000 21000000 04" + K.NEW) * 2
    bare = dict(a, st=None, lb=None, inst=None, arena=None)
    for case in (a, bare):
        out, off = e.encode_accepts_stored(**case)
        assert out.tobytes() == want and off.tolist() == [0, 48, 96, 96]
    out, off = run_dev(e, K.N, a, len(want), null_store=True)
    assert out.tobytes() == want and off.tolist() == [0, 48, 96, 96]
    d_out, _ = e.encode_accepts(**{k: v for k, v in a.items() if k not in STORE})
    assert d_out.tobytes() == want


# ---- identity with the dense encoder ---------------------------------------------------------------
@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
def test_fuzz_identity_min(mk_engine, seed):
    check(mk_engine(5, MIN), MIN, 5, S.fuzz_stored(seed, 5, MIN), decode=seed < 3)


@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
def test_fuzz_identity_classic_null_store(mk_engine, seed):
    a = S.fuzz_stored(seed, 5, CLASSIC)
    e = mk_engine(5, CLASSIC)
    w_out, w_off, _ = check(e, CLASSIC, 5, a, forms=("host",))
    out, off = run_dev(e, 5, a, len(w_out), null_store=True)
    assert np.array_equal(off, w_off)
    same_bytes(out, w_out, "device form, null store")


@pytest.mark.parametrize("thrifty", [False, True], ids=["all", "thrifty"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_replica_counts(mk_engine, mode, n, thrifty):
    rng = np.random.default_rng(n)
    G = 24
    a = stored(TP.scenario(10 + n, mode, n, G, 6, rng.integers(0, 5, G).tolist(),
                           [rng.integers(0, 4, int(k)).tolist() for k in rng.integers(0, 5, G)]),
               seed=n, lb_kind=1)
    e = mk_engine(n, mode)
    check(e, mode, n, a, thrifty=thrifty, decode=True)
    check(e, mode, n, a, thrifty=thrifty, alive_mask=int(rng.integers(0, 1 << n)), forms=("dev",))
    check(e, mode, n, a, thrifty=thrifty, alive_mask=0, forms=("host",))


# ---- varint steps ----------------------------------------------------------------------------------
def test_varint_steps_of_a_records_command_count(mk_engine):
    """the steps test_gpu_proposer.py uses for n (0, 1, 63, 64, 5000, 8191, 8192), here as the
    command count of a catch-up record: V(k) of 1, 2 and 3 bytes; the new commands step too"""
    ks = [0, 1, 63, 64, 5000, 8191, 8192]
    a = stored(TP.scenario(1, MIN, 3, len(ks), 4, ks[::-1], [[k] for k in ks],
                           pc=lambda g, q, first, lc: first - 1), seed=1, p_unflag=0.0, dead=2)
    _, _, per = check(mk_engine(3, MIN), MIN, 3, a, decode=True)
    assert max(len(f) for q in per for f in q) > 2 * WINDOW + 100000


def test_varint_steps_of_m(mk_engine):
    """catch-up logs of 0, 1, 63 and 64 instances, instances without commands among them"""
    want_m = [0, 1, 63, 64]
    used = [[0, 2, 0, 1] * 16 for _ in want_m]
    a = stored(TP.scenario(3, MIN, 3, 4, 72, [1, 2, 0, 3], used,
                           pc=lambda g, q, first, lc: lc - want_m[g] if q != 1 else first - 1),
               seed=3, lb_kind=1)
    _, _, per = check(mk_engine(3, MIN), MIN, 3, a, decode=True)
    ms = sorted(TP.uvarint(f, 17 + 1 + 17 * TP.uvarint(f, 17)[0])[0] for q in per for f in q)
    assert set(want_m) <= set(ms) and ms[-1] == 64


# ---- the window boundary ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", range(-30, 3))
def test_record_header_and_command_at_every_byte_around_the_window_boundary(mk_engine, d):
    """one frame whose catch-up record header starts at byte 8192 + d: 17 + V(0) + V(m) + z records
    of 9 bytes + one of 10 + 17 k0, then the record under test (3 commands, the first at 8192 + d +
    9; the record before it ends with a command at 8192 + d - 17) and one more. Over d = -30 .. 2
    the command starts cover 8192 - 47 .. 8192 + 11."""
    T = WINDOW + d
    z = next(z for z in range(17) if (T - 29 - 9 * z) % 17 == 0)
    k0 = (T - 29 - 9 * z) // 17
    assert k0 >= 64 and z + 3 < 64
    used = [0] * z + [k0, 3, 2]
    a = stored(TP.scenario(d + 40, MIN, 2, 1, len(used) + 1, [0], [used], self_id=[0],
                           pc=lambda g, q, first, lc: first - 1), seed=d + 40, p_unflag=0.5, p_share=0)
    w_out, _, per = check(mk_engine(2, MIN), MIN, 2, a, dense=d % 8 == 0)
    frame = per[1][0]
    rec = S.log_instance(a["st"], a["lb"], a["inst"], a["arena"], z + 1)
    head = np.array([rec[0], rec[1]], "<i4").tobytes() + b"\x06"
    assert frame[T:T + 9] == head and len(frame) == T + 9 + 51 + 9 + 34
    assert frame[T + 9:T + 26] == P.command_marshal(*rec[2][0])


# ---- long and many ---------------------------------------------------------------------------------
def test_one_instance_of_5000_commands_ending_at_the_arenas_end(mk_engine):
    """85 KB of one log instance over eleven windows; its range ends exactly at n_src (the arena
    sits on guards, src_op at an odd address)"""
    a = stored(TP.scenario(8, MIN, 3, 1, 4, [2], [[1, 5000]], self_id=[0],
                           pc=lambda g, q, first, lc: first - 1 if q == 1 else lc - 1),
               seed=8, p_share=0, dead=3)
    # move the long instance's commands to the arena's end
    inst, (op, key, val) = a["inst"], a["arena"]
    c0 = int(inst["first_cmd"][1])
    order = np.concatenate([np.arange(c0), np.arange(c0 + 5000, len(op)), np.arange(c0, c0 + 5000)])
    a["arena"] = (op[order], key[order], val[order])
    if int(inst["first_cmd"][0]) > c0:
        inst["first_cmd"][0] -= 5000
    inst["first_cmd"][1] = len(op) - 5000
    assert int(inst["first_cmd"][1]) + int(inst["n_cmds"][1]) == len(a["arena"][0])
    w_out, w_off, _ = check(mk_engine(3, MIN), MIN, 3, a, decode=True)
    assert int(w_off[2]) - int(w_off[1]) > 10 * WINDOW and int(w_off[-1]) > 20 * WINDOW


def test_lagging_peer_300_instances_to_four_peers(mk_engine):
    """a 300-instance range whose first_cmds are a random permutation, the same range sent to 4
    peers"""
    rng = np.random.default_rng(9)
    used = rng.integers(0, 4, 300).tolist()
    a = stored(TP.scenario(9, MIN, 5, 1, 304, [3], [used], self_id=[2],
                           pc=lambda g, q, first, lc: first - 1 - q), seed=9, lb_kind=1, p_share=0)
    first = a["inst"]["first_cmd"][:300][np.array(used) > 0]
    assert (np.diff(first.astype(np.int64)) < 0).sum() > 50  # not in window order
    _, w_off, per = check(mk_engine(5, MIN), MIN, 5, a, decode=True)
    runs = np.diff(w_off.astype(np.int64)).tolist()
    assert runs[2] == 0 and len({x for q, x in enumerate(runs) if q != 2}) == 1 and runs[0] > WINDOW


@pytest.mark.parametrize("n_sends", [0, 1, 255, 256, 257, 1025])
def test_send_counts_with_one_record_logs(mk_engine, n_sends):
    rng = np.random.default_rng(n_sends)
    G = max(n_sends, 1)
    a = stored(TP.scenario(n_sends, MIN, 3, G, 2, rng.integers(0, 3, G).tolist(),
                           [[int(k)] for k in rng.integers(0, 3, G)],
                           pc=lambda g, q, first, lc: first - 1), seed=n_sends, lb_kind=n_sends & 1)
    if n_sends == 0:
        a["sends"] = a["sends"][:0]
    _, w_off, _ = check(mk_engine(3, MIN), MIN, 3, a, decode=n_sends == 257)
    assert (int(w_off[-1]) == 0) == (n_sends == 0)


def test_skipped_slots_between_accept_slots(mk_engine):
    rng = np.random.default_rng(6)
    G = 300
    flags = [R.PH_ACCEPT] * G
    for g in list(range(0, 5)) + list(range(140, 150)) + list(range(295, 300)):
        flags[g] = [R.PH_NOT_LEADER, R.PH_REFUSED, R.PH_PREPARE, 0][g % 4]  # start, middle, end
    a = stored(TP.scenario(6, MIN, 5, G, 4, rng.integers(0, 2, G).tolist(),
                           [[int(x) for x in rng.integers(0, 2, int(k))] for k in rng.integers(0, 3, G)],
                           flags=flags), seed=6, lb_kind=1)
    e = mk_engine(5, MIN)
    _, w_off, _ = check(e, MIN, 5, a, decode=True)
    assert int(w_off[-1]) > WINDOW
    out, off = e.encode_accepts_stored(**dict(a, sends=a["sends"][:5]))
    assert len(out) == 0 and not off.any()


# ---- capacity, errors, alignment, the reserve --------------------------------------------------------
def test_out_cap_short_by_one_byte_and_more(mk_engine):
    """nothing at or past out_cap, dest_off complete; the host form names the short buffer"""
    e = mk_engine(3, MIN)
    ns = [70, 3, 0, 500, 9, 1]
    a = stored(TP.scenario(7, MIN, 3, len(ns), 8, ns, [[1, 0, 2]] * len(ns)), seed=7, lb_kind=1)
    w_out, w_off = S.encode_accepts_stored(MIN, 3, **a)
    total = len(w_out)
    assert total > 2 * WINDOW
    for short, shift in ((1, 0), (1, 5), (WINDOW + 5, 16), (total, 1)):
        out, off = run_dev(e, 3, a, total - short, out_shift=shift)
        assert np.array_equal(off, w_off)
        same_bytes(out, w_out[:total - short], f"short by {short}")
    with pytest.raises(MpxError) as ei:
        e.encode_accepts_stored(out_cap=total - 1, **a)
    assert ei.value.code == R.E_INVAL
    out, _ = e.encode_accepts_stored(out_cap=total, **a)
    same_bytes(out, w_out, "exact out_cap")


def _dev_code(e, n, a, out_cap):
    """the code the device form's error word gives at the next synchronising call; guards checked"""
    with Arena(e) as ar:
        b, keep = dev_batch(ar, a)
        g_out, g_off = Guard(ar, out_cap, np.uint8), Guard(ar, n + 1, np.uint64)
        e.encode_accepts_stored_reserve(len(a["sends"]), len(a["groups"]) * a["ipg"])
        e.encode_accepts_stored_dev(b, g_out.ptr, out_cap, g_off.ptr)
        with pytest.raises(MpxError) as ei:
            e.synchronize()
        for k in ("sop", "skey", "sval"):
            keep[k].assert_margins()
        return ei.value.code, g_off.assert_margins(), g_out.assert_margins()


def test_nil_in_a_range_and_range_leaving_the_arena(mk_engine):
    e = mk_engine(3, MIN)
    a = stored(TP.scenario(8, MIN, 3, 3, 6, [2, 1, 4], [[1, 2, 3]] * 3,
                           pc=lambda g, q, first, lc: first), seed=8, p_share=0)
    w_out, w_off = S.encode_accepts_stored(MIN, 3, **a)
    n_src = len(a["arena"][0])
    # group 1's instance first + 2 is in every peer's range
    nil = dict(a, st=a["st"].copy())
    nil["st"]["status"][6 + 2] = P.NIL
    with pytest.raises(GoPanic) as gp:
        S.encode_accepts_stored(MIN, 3, **nil)
    assert gp.value.code == R.E_NIL_INSTANCE
    with pytest.raises(MpxError) as ei:
        e.encode_accepts_stored(**nil)
    assert ei.value.code == R.E_NIL_INSTANCE
    code, off, _ = _dev_code(e, 3, nil, len(w_out))
    assert code == R.E_NIL_INSTANCE
    # sized and encoded as having no commands: three commands fewer in each of the two frames
    assert int(off[-1]) == len(w_out) - 2 * 3 * 17
    for first, n in ((n_src - 2, 3), (n_src + 1, 0), (1 << 40, 3), (0, n_src + 1)):
        bad = dict(a, inst=a["inst"].copy())
        k = int(bad["inst"]["n_cmds"][6 + 2])
        bad["inst"][6 + 2] = (first, n, R.IC_HAS_CMDS)
        with pytest.raises(MpxError) as ei:
            e.encode_accepts_stored(**bad)
        assert ei.value.code == R.E_INVAL, (first, n)
        code, off, out = _dev_code(e, 3, bad, len(w_out))
        assert code == R.E_INVAL, (first, n)
        assert int(off[-1]) == len(w_out) - 2 * k * 17
        # ... which is what the slot gives without its flag: V(0)
        bare = dict(a, inst=a["inst"].copy())
        bare["inst"]["flags"][6 + 2] = 0
        b_out, b_off = S.encode_accepts_stored(MIN, 3, **bare)
        assert np.array_equal(off, b_off)
        same_bytes(out[:len(b_out)], b_out, "a range leaving the arena")
    # slots outside every range are not judged: a nil slot with a flagged range far outside the
    # arena, and group 0's first instance (every peer has it), non-nil, with such a range
    ok = dict(a, inst=a["inst"].copy())
    assert int(ok["st"]["status"][6 + 5]) == P.NIL and int(ok["st"]["status"][0]) != P.NIL
    ok["inst"][6 + 5] = (1 << 40, 7, R.IC_HAS_CMDS)
    ok["inst"][0] = (n_src - 1, 3, R.IC_HAS_CMDS)
    check(e, MIN, 3, ok, dense=False)
    check(e, MIN, 3, a)  # the engine is usable afterwards


def test_every_misalignment_is_rejected(mk_engine):
    e = mk_engine(3, MIN)
    a = K.CASES["self2_lb"][0]
    with Arena(e) as ar:
        b, keep = dev_batch(ar, a, op_shift=0)
        g_out, g_off = Guard(ar, 512, np.uint8), Guard(ar, 4, np.uint64)
        e.encode_accepts_stored_reserve(1, 8)
        for field, by in (("sends", 8), ("groups", 8), ("st", 8), ("lb", 8), ("inst", 8),
                          ("cmd_key", 4), ("cmd_val", 4), ("src_key", 4), ("src_val", 4),
                          ("peer_commits", 2)):
            x = _lib.MpxAcceptStoreBatch.from_buffer_copy(b)
            setattr(x, field, getattr(b, field) + by)
            with pytest.raises(MpxError, match="aligned") as ei:
                e.encode_accepts_stored_dev(x, g_out.ptr, 512, g_off.ptr)
            assert ei.value.code == R.E_INVAL, field
        with pytest.raises(MpxError, match="aligned"):
            e.encode_accepts_stored_dev(b, g_out.ptr, 512, g_off.ptr + 4)
        x = _lib.MpxAcceptStoreBatch.from_buffer_copy(b)
        x.reserved = 1
        with pytest.raises(MpxError, match="reserved"):
            e.encode_accepts_stored_dev(x, g_out.ptr, 512, g_off.ptr)
        # cmd_op, src_op and d_out at any address
        x = _lib.MpxAcceptStoreBatch.from_buffer_copy(b)
        e.encode_accepts_stored_dev(x, g_out.ptr + 3, 300, g_off.ptr)
        e.synchronize()
        assert g_off.assert_margins().tolist() == K.LENGTHS["self2_lb"]
        g_out.assert_margins()
        del keep


def test_reserve_contract(mk_engine):
    """the device form never allocates: it needs its own reserve (the dense form's, one array
    smaller, is not enough), an empty call needs none, and a reserve covers smaller calls"""
    e = mk_engine(3, MIN)
    a, want, want_off = K.CASES["self2_lb"]
    with Arena(e) as ar:
        b, keep = dev_batch(ar, a)
        g_out, g_off = Guard(ar, len(want), np.uint8), Guard(ar, 4, np.uint64)
        with pytest.raises(MpxError, match="mpx_encode_accepts_stored_reserve"):
            e.encode_accepts_stored_dev(b, g_out.ptr, len(want), g_off.ptr)
        none = _lib.MpxAcceptStoreBatch.from_buffer_copy(b)
        none.n_sends = 0
        e.encode_accepts_stored_dev(none, g_out.ptr, len(want), g_off.ptr)
        e.synchronize()
        assert not g_off.assert_margins().any()
        g_out.assert_untouched([(0, len(want))])
        e.encode_accepts_reserve(1, 8, 0)
        with pytest.raises(MpxError, match="mpx_encode_accepts_stored_reserve"):
            e.encode_accepts_stored_dev(b, g_out.ptr, len(want), g_off.ptr)
        e.encode_accepts_stored_reserve(64, 4096)
        e.encode_accepts_stored_dev(b, g_out.ptr, len(want), g_off.ptr)
        e.synchronize()
        assert g_out.assert_margins().tobytes() == want.tobytes()
        assert g_off.assert_margins().tolist() == want_off.tolist()
        del keep
    with pytest.raises(MpxError) as ei:
        e.encode_accepts_stored_reserve(1 << 32, 8)
    assert ei.value.code == R.E_UNSUPPORTED


# ---- the chain ---------------------------------------------------------------------------------------
def test_graph_of_a_leaders_turn_replayed_for_two_turns(mk_engine):
    """mpx_decode_client_streams_dev -> mpx_propose_handle_dev -> mpx_store_commands_dev(SENDS) ->
    mpx_encode_accepts_stored_dev on 8 groups, captured once and replayed for two consecutive
    turns on the state the first leaves. Between the replays only committed_upto, peer_commits and
    lb's status move, as the tally would leave them. Turn 2's frames carry turn 1's instance: its
    commands read from the arena, its status COMMITTED."""
    import client_translit as CL
    import store_translit as T
    import test_gpu_client as TC
    NR = 5
    e = mk_engine(NR, MIN)
    G, per_group, slot, ipg, base, D = 8, 3, 1024, 8, 50, 32
    n_inst, n_conns = G * ipg, G * per_group
    cap = n_conns * slot // 30
    # the transliterated turns
    grp = P.mk_groups([(D, g % NR, g % NR, 3, base + g * ipg, base + g * ipg - 1) for g in range(G)])
    st, lb = P.nil_state(n_inst), np.zeros(n_inst, R.INST_STATE)
    lb["status"] = P.NIL
    inst = np.zeros(n_inst, R.INST_CMDS)
    pc = np.array([[base + g * ipg - 1] * NR for g in range(G)], np.int32)
    turns, used = [], 0
    a_cap = 2 * cap
    arena = T.mk_arena(a_cap, 4)
    state0 = dict(grp=grp.copy(), st=st.copy(), lb=lb.copy(), inst=inst.copy(), pc=pc.copy())
    for turn, seed in enumerate((21, 22)):
        bufs, groups = TC._chain_input(seed, G, per_group, slot)
        wc = CL.decode_client_streams(bufs, groups, G)
        grp, st, lb, sends, _, _ = P.propose_handle(MIN, NR, grp, wc["prop_off"], st, base, ipg, lb)
        assert len(sends) == G and (sends["flags"] == R.PH_ACCEPT).all()
        ws = T.store_commands(R.SC_SENDS, sends, [dict(cmd_off=None, op=wc["op"], key=wc["key"],
                                                       val=wc["val"], n_recs=G)],
                              arena, used, inst, base)
        assert ws["code"] == R.OK and int(ws["res"]["n_stored"]) == G
        arena, used, inst = (ws["op"], ws["key"], ws["val"]), ws["used"], ws["inst"]
        note = []
        out, off = S.encode_accepts_stored(MIN, NR, sends, grp, (wc["op"], wc["key"], wc["val"]), base,
                                           ipg, pc, st=st, lb=lb, inst=inst, arena=arena, note=note)
        buf = np.zeros(n_conns * slot, np.uint8)
        conns = np.zeros(n_conns, R.CLIENT_CONN)
        for k, b in enumerate(bufs):
            conns[k] = (k * slot, len(b), groups[k])
            buf[k * slot:k * slot + len(b)] = np.frombuffer(b, np.uint8)
        turns.append(dict(buf=buf, conns=conns, wc=wc, sends=sends, st=st.copy(), out=out, off=off,
                          note=note, inst=inst.copy(), used=used))
        # what the tally leaves: the instance committed, the peers one behind or up to date
        for g in range(G):
            i = base + g * ipg + turn
            grp["committed_upto"][g] = i
            lb["status"][i - base] = P.COMMITTED
            pc[g] = [i - 1 if (g + q) % 3 else i for q in range(NR)]
        turns[-1]["after"] = dict(committed=grp["committed_upto"].copy(), lb=lb.copy(), pc=pc.copy())
    # turn 1: empty logs; turn 2: every lagging peer's frame carries turn 1's instance, COMMITTED
    assert all(ks == [] for _, ks in turns[0]["note"])
    carried = [ks for _, ks in turns[1]["note"] if ks]
    assert len(carried) > G and all(ks == [k for k in ks if k % ipg == 0] and len(ks) == 1 for ks in carried)
    assert all(S.log_instance(st, lb, inst, arena, ks[0])[1] == P.COMMITTED for ks in carried)
    assert any(len(S.log_instance(st, lb, inst, arena, ks[0])[2]) > 0 for ks in carried)
    out_cap = max(len(t["out"]) for t in turns)
    with Arena(e) as ar:
        g, g_buf, d_conns, out = TC.dev_buffers(ar, turns[0]["buf"], turns[0]["conns"], G, cap)
        g_grp, g_st = Guard(ar, G, R.PROPOSER_GROUP), Guard(ar, n_inst, R.ACCEPTOR_STATE)
        g_lb, g_snd = Guard(ar, n_inst, R.INST_STATE), Guard(ar, G, R.ACCEPT_SEND)
        g_pc = Guard(ar, G * NR, np.int32)
        s_g = dict(op=Guard(ar, a_cap, np.uint8, shift=1), key=Guard(ar, a_cap, np.int64, shift=8),
                   val=Guard(ar, a_cap, np.int64), used=Guard(ar, 1, np.uint64),
                   inst=Guard(ar, n_inst, R.INST_CMDS), res=Guard(ar, 1, R.STORE_RESULT))
        g_out, g_off = Guard(ar, out_cap, np.uint8), Guard(ar, NR + 1, np.uint64)
        sb = e.store_batch_dev(R.SC_SENDS, g_snd, G, [dict(cmd_off=None, n_frames=0, op=g["op"], key=g["key"],
                                                           val=g["val"], n_cmds=cap, n_recs=G)],
                               n_inst, base)
        sa = e.store_arena_dev(s_g["op"], s_g["key"], s_g["val"], a_cap, s_g["used"])
        ab = _lib.MpxAcceptStoreBatch()
        ab.sends, ab.n_sends, ab.inst_base, ab.ipg, ab.n_groups = g_snd.ptr, G, base, ipg, G
        ab.groups, ab.peer_commits = g_grp.ptr, g_pc.ptr
        ab.cmd_op, ab.cmd_key, ab.cmd_val, ab.n_cmds = g["op"].ptr, g["key"].ptr, g["val"].ptr, cap
        ab.st, ab.lb, ab.inst = g_st.ptr, g_lb.ptr, s_g["inst"].ptr
        ab.src_op, ab.src_key, ab.src_val, ab.n_src = s_g["op"].ptr, s_g["key"].ptr, s_g["val"].ptr, a_cap
        ab.alive_mask = 0xFFFF
        e.decode_client_streams_reserve(len(turns[0]["buf"]), n_conns, G)
        e.store_commands_reserve(G)
        e.encode_accepts_stored_reserve(G, n_inst)
        g_grp.put(state0["grp"])
        g_st.put(state0["st"])
        g_lb.put(state0["lb"])
        g_pc.put(state0["pc"])
        s_g["inst"].put(state0["inst"])
        s_g["used"].put(np.zeros(1, np.uint64))
        for name, x in zip(("op", "key", "val"), T.mk_arena(a_cap, 4)):
            s_g[name].put(x)
        s = e.stream_create()
        e.graph_begin(s)
        e.decode_client_streams_dev(g_buf.ptr, n_conns * slot, d_conns.ptr, n_conns, G, out,
                                    g["conn_res"].ptr, g["res"].ptr, s)
        e.propose_handle_dev(g_grp.ptr, G, g["prop_off"].ptr, g["send_off"].ptr, g_st.ptr, g_lb.ptr,
                             n_inst, base, ipg, g_snd.ptr, s)
        e.store_commands_dev(sb, sa, s_g["inst"], s_g["res"], s)
        e.encode_accepts_stored_dev(ab, g_out.ptr, out_cap, g_off.ptr, s)
        gr = e.graph_end(s)
        try:
            for t in turns:
                g_buf.put(t["buf"], s)
                d_conns_new = ar.put(t["conns"], s)
                e.memcpy(d_conns.ptr, d_conns_new.ptr, d_conns_new.nbytes, D2D, s)
                g_out.fill(s)
                g_off.fill(s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                assert g_snd.assert_margins().tobytes() == t["sends"].tobytes()
                assert g_st.assert_margins().tobytes() == t["st"].tobytes()
                assert s_g["inst"].assert_margins().tobytes() == t["inst"].tobytes()
                assert int(s_g["used"].assert_margins()[0]) == t["used"]
                assert np.array_equal(g_off.assert_margins(), t["off"])
                got = g_out.assert_margins()
                same_bytes(got[:len(t["out"])], t["out"], "the turn's Accept bytes")
                g_out.assert_untouched([(len(t["out"]), out_cap)])
                # the tally's step, on the device state
                grp_d = g_grp.assert_margins().copy()
                grp_d["committed_upto"] = t["after"]["committed"]
                g_grp.put(grp_d, s)
                lb_d = g_lb.assert_margins().copy()
                lb_d["status"] = t["after"]["lb"]["status"]
                g_lb.put(lb_d, s)
                g_pc.put(t["after"]["pc"], s)
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()

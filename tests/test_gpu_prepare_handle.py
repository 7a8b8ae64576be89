"""GPU tests of the prepare side (mpx_gather_prepares, mpx_prepare_handle,
mpx_encode_prepare_replies), host and device forms, exact against
tests/prepare_handle_translit.py: records, effects, group state and bytes. Shapes are the smallest
that reach each path: the handler's workgroup is 256 messages, the encoder's output window 8192
bytes, its item chunk 256, a scan tile 4096 items. In the device forms every output (and the
command arena) sits on guards exactly its capacity long."""
import ctypes as C

import numpy as np
import pytest

import prepare_handle_kat as K
import prepare_handle_translit as T
import unmarshal_translit as U
from devguard import Guard
from go_translit import GoBackend, GoPanic
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import Arena
from minpaxos_amd.engine import MpxError

pytestmark = pytest.mark.gpu
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
MODES = pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
WINDOW = 8192


def rdt(mode):
    return R.PREPARE_REPLY_MIN if mode == MIN else R.PREPARE_REPLY


def same_bytes(out, want, what):
    if out.tobytes() != want.tobytes():
        m = min(len(out), len(want))
        bad = np.flatnonzero(out[:m] != want[:m])
        raise AssertionError(f"{what}: lengths {len(out)} / {len(want)}, {len(bad)} bytes differ, "
                             f"first at {bad[:8]}")


def same_recs(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, got[:4], want[:4],
                                             np.flatnonzero(got != want)[:8])


# ---- the device forms on guards ----------------------------------------------------------------------
def store_dev(ar, a):
    """device copies of a case's store; the arena on guards exactly its size, src_op at an odd
    address"""
    sop, skey, sval = a["arena"]
    d = dict(st=ar.put(a["st"]), inst=ar.put(a["inst"]),
             sop=Guard(ar, len(sop), np.uint8, shift=1).put(sop),
             skey=Guard(ar, len(sop), np.int64).put(skey),
             sval=Guard(ar, len(sop), np.int64).put(sval))
    if a.get("lb") is not None:
        d["lb"] = ar.put(a["lb"])
    return d


def handle_dev(e, ar, mode, N, a, d=None):
    """mpx_prepare_handle_dev on guarded outputs; returns (results as host arrays, guards)"""
    msgs, groups = a["msgs"], np.atleast_1d(a["groups"])
    n, G = len(msgs), len(groups)
    d = d or store_dev(ar, a)
    g = dict(msgs=ar.put(msgs), grp=Guard(ar, G, R.PROPOSER_GROUP).put(groups),
             rep=Guard(ar, n, rdt(mode)), to=Guard(ar, n, np.int32),
             eff=Guard(ar, n, np.uint8, shift=3))
    if mode == MIN:
        g["lf"] = Guard(ar, n, np.int32)
        if a.get("gps") is not None:
            g["gps"] = Guard(ar, G, R.GROUP_PREP_STATE).put(a["gps"])
        if a.get("peer_commits") is not None:
            g["pc"] = Guard(ar, G * N, np.int32).put(a["peer_commits"])
    e.prepare_handle_dev(g["msgs"].ptr, n, d["st"].ptr, len(a["st"]), a["inst_base"], g["grp"].ptr, G,
                         a["ipg"], g["rep"].ptr, g["to"].ptr, g["eff"].ptr,
                         g["lf"].ptr if "lf" in g else None, g["gps"].ptr if "gps" in g else None,
                         g["pc"].ptr if "pc" in g else None)
    return g, d


def read_handle(g):
    out = dict(groups=g["grp"].assert_margins(), replies=g["rep"].assert_margins(),
               reply_to=g["to"].assert_margins(), effect=g["eff"].assert_margins())
    out["log_from"] = g["lf"].assert_margins() if "lf" in g else None
    out["gps"] = g["gps"].assert_margins() if "gps" in g else None
    out["peer_commits"] = g["pc"].assert_margins() if "pc" in g else None
    return out


def encode_batch(mode, a, d, rep_ptr, to_ptr, lf_ptr, n, n_dest):
    b = _lib.MpxPrepareReplyBatch()
    b.replies, b.reply_to, b.log_from, b.n, b.n_dest = rep_ptr, to_ptr, lf_ptr, n, n_dest
    b.inst_base, b.n_inst = a["inst_base"], len(a["st"])
    b.st, b.inst = d["st"].ptr, d["inst"].ptr
    if "lb" in d:
        b.lb = d["lb"].ptr
    b.src_op, b.src_key, b.src_val, b.n_src = d["sop"].ptr, d["skey"].ptr, d["sval"].ptr, \
        len(a["arena"][0])
    return b


def encode_dev(e, ar, mode, a, d, rep_ptr, to_ptr, lf_ptr, n, n_dest, out_cap, out_shift=0,
               sync=True):
    """mpx_encode_prepare_replies_dev on guarded out / dest_off; returns (out, dest_off) or, with
    sync=False, the guards"""
    b = encode_batch(mode, a, d, rep_ptr, to_ptr, lf_ptr, n, n_dest)
    g_out, g_off = Guard(ar, out_cap, np.uint8, shift=out_shift), Guard(ar, n_dest + 1, np.uint64)
    e.encode_prepare_replies_reserve(n, len(a["st"]), n_dest)
    e.encode_prepare_replies_dev(b, g_out.ptr, out_cap, g_off.ptr)
    if not sync:
        return g_out, g_off
    e.synchronize()
    for k in ("sop", "skey", "sval"):
        d[k].assert_margins()
    return g_out.assert_margins(), g_off.assert_margins()


STATE = ("groups", "replies", "reply_to", "effect", "log_from", "gps", "peer_commits")


def compare(got, want, what):
    for k in STATE:
        if want[k] is None:
            continue
        same_recs(np.asarray(got[k]), np.asarray(want[k]), f"{what}: {k}")


def check(e, mode, N, a, forms=("host", "dev"), out_shift=0):
    """handler and encoder, both forms, against the transliteration"""
    want = T.run_batch(mode, N, **a)
    store = {k: a.get(k) for k in ("st", "lb", "inst", "arena")}
    if "host" in forms:
        got = e.prepare_handle(a["msgs"], a["st"], a["groups"], a["inst_base"], a["ipg"],
                               a.get("gps"), a.get("peer_commits"))
        compare(got, want, "host form")
        out, off = e.encode_prepare_replies(got["replies"], got["reply_to"], got["log_from"], N,
                                            a["inst_base"], **store)
        assert np.array_equal(off, want["dest_off"]), (off, want["dest_off"])
        same_bytes(out, want["bytes"], "host form")
    if "dev" in forms:
        with Arena(e) as ar:
            g, d = handle_dev(e, ar, mode, N, a)
            e.synchronize()
            compare(read_handle(g), want, "device form")
            out, off = encode_dev(e, ar, mode, a, d, g["rep"].ptr, g["to"].ptr,
                                  g["lf"].ptr if "lf" in g else None, len(a["msgs"]), N,
                                  len(want["bytes"]), out_shift)
            assert np.array_equal(off, want["dest_off"]), (off, want["dest_off"])
            same_bytes(out, want["bytes"], "device form")
    return want


# ---- known answers and fuzz ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_known_answers(mk_engine, name):
    mode, kw, want = K.CASES[name]()
    N = kw.pop("N")
    e = mk_engine(N, mode)
    got = check(e, mode, N, kw)
    assert bytes(got["bytes"]) == want["frame"]
    out, off = e.encode_prepare_replies(got["replies"], got["reply_to"], got["log_from"], N,
                                        kw["inst_base"], st=kw["st"], inst=kw["inst"],
                                        arena=kw["arena"])
    assert out.tobytes() == want["frame"]


@MODES
@pytest.mark.parametrize("seed", T.FUZZ_SEEDS)
def test_fuzz(mk_engine, mode, seed):
    N = 3 if seed % 2 == 0 else 5
    check(mk_engine(N, mode), mode, N, T.fuzz_case(seed, mode, N=N), out_shift=seed % 16)


@MODES
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_message_counts(mk_engine, mode, n):
    """the handler's 256-message workgroups and the encoder's 256-item chunks, over 1, 3 and 65
    groups of 8 slots; with one group a run crosses every tile boundary"""
    for G in (1, 3, 65):
        N = 5 if G == 3 else 3
        a = T.fuzz_case(1000 + n + G, mode, N=N, G=G, ipg=8, n=n)
        check(mk_engine(N, mode), mode, N, a, forms=("dev",) if G != 3 else ("host", "dev"))


def big_case(mode, counts=(0, 1, 63, 64, 500), log=1, ipg=8, N=3, seed=5):
    """group g's reply carries counts[g] commands (MIN: the Cmds of slot committedUpTo + 1;
    CLASSIC: the prepared instance's) and, in MIN, a log of `log` instances"""
    rng = np.random.default_rng(seed)
    G = len(counts)
    fill = [log + 2] * G
    big = {g * ipg + (log if mode == MIN else 1): c for g, c in enumerate(counts)}
    st, lb, inst, arena = T.make_store(rng, G, ipg, 0, fill, lb_kind=1, big=big)
    groups = np.zeros(G, R.PROPOSER_GROUP)
    msgs = np.zeros(G, R.PREPARE_MSG)
    for g in range(G):
        first = g * ipg
        groups[g] = (7, g % N, 0, 2, first, first + log - 1, (0, 0))
        msgs[g] = (g, 9, (g + 1) % N, first - 1) if mode == MIN else (first + 1, 9, (g + 1) % N, 1)
    return dict(msgs=msgs, groups=groups, st=st, inst_base=0, ipg=ipg, lb=lb, inst=inst,
                arena=arena)


@MODES
def test_command_counts_and_a_frame_longer_than_a_window(mk_engine, mode):
    a = big_case(mode)
    want = check(mk_engine(3, mode), mode, 3, a)
    assert max(len(f) for f in want["frames"]) > WINDOW
    n_cmds = [int(a["inst"]["n_cmds"][int(v)]) for v in want["replies"]["value_id"]]
    assert n_cmds == [0, 1, 63, 64, 500]


# ---- the window boundary -----------------------------------------------------------------------------
@pytest.mark.parametrize("d", range(-30, 3))
def test_record_header_and_command_at_every_byte_around_the_window_boundary(mk_engine, d):
    """test_gpu_accepts_stored.py's sweep for a MIN PrepareReply frame: an 18-byte head and the
    frame's own Command slice (2 commands) ahead of the log, the header of log record k at byte
    8192 + d, its first command at 8192 + d + 9, the record before it ending with a command at
    8192 + d - 17 (T.boundary_case; test_prepare_handle_translit.py checks where its inputs put the
    headers and the commands)"""
    a, k = T.boundary_case(d)
    want = check(mk_engine(2, MIN), MIN, 2, a)
    frame, at = want["frames"][0], WINDOW + d
    status = int(a["lb"]["status"][k]) if int(a["lb"]["status"][k]) != T.NIL else int(a["st"]["status"][k])
    head = np.array([a["st"]["ballot"][k], status], "<i4").tobytes() + b"\x06"
    assert frame[at:at + 9] == head and len(frame) == at + 9 + 51 + 9 + 34
    c = int(a["inst"]["first_cmd"][k])
    assert frame[at + 9:at + 26] == T.command_marshal(tuple(int(x[c]) for x in a["arena"]))


def test_command_slice_across_the_window_boundary(mk_engine):
    """the frame's own Command slice (482 commands from the arena) lies across byte 8192, a log of
    three records behind it; both forms"""
    a = T.command_straddle_case()
    want = check(mk_engine(2, MIN), MIN, 2, a)
    frame = want["frames"][0]
    c = int(a["inst"]["first_cmd"][3]) + 480
    assert 18 + 2 + 17 * 480 < WINDOW < 18 + 2 + 17 * 481 < len(frame)
    assert frame[8180:8197] == T.command_marshal(tuple(int(x[c]) for x in a["arena"]))


@pytest.mark.parametrize("log", [0, 1, 64])
def test_log_lengths_min(mk_engine, log):
    a = big_case(MIN, counts=(2, 0, 3), log=log, ipg=72, seed=log)
    if log == 64:
        assert ((a["inst"]["flags"][:64] & R.IC_HAS_CMDS) == 0).any()  # a CommitShort's slot inside
    want = check(mk_engine(3, MIN), MIN, 3, a)
    lens = (want["replies"]["last_committed"] - want["log_from"] + 1).tolist()
    assert lens == [log] * 3
    assert (((want["effect"] & R.PRH_LOG) != 0) == (log > 0)).all()


def test_classic_strict_compares_and_to_infinity(mk_engine):
    """ballots equal to D and to inst.ballot (both compares are strict), ToInfinity 0, 1 and 2"""
    st = np.zeros(8, R.ACCEPTOR_STATE)
    st["status"], st["ballot"], st["value_id"] = R.STATUS_NIL, -1, R.VALUE_KEEP
    st["status"][2:5], st["ballot"][2:5] = R.ACCEPTED, 20
    inst = np.zeros(8, R.INST_CMDS)
    inst[3] = (0, 2, R.IC_HAS_CMDS)
    arena = (np.array([1, 2], np.uint8), np.array([3, 4], np.int64), np.array([5, 6], np.int64))
    groups = np.array([(20, 0, 0, 0, 0, -1, (0, 0))], R.PROPOSER_GROUP)
    #        key ballot leader arg
    msgs = np.array([(0, 20, 1, 2),    # nil, == D: ok; a byte of 2 raises nothing
                     (0, 30, 1, 2),    # > D, not TRUE: D stays 20
                     (0, 19, 2, 1),    # nil, < D: refused
                     (1, 25, 1, 0),    # ToInfinity 0: nothing raised
                     (1, 25, 1, 1),    # raises D to 25
                     (1, 25, 2, 1),    # == D now: ok, not raised again
                     (2, 20, 0, 1),    # inst, == inst.ballot: ok
                     (3, 19, 0, 1),    # inst, below: refused, the commands go out
                     (4, 21, 0, 1)],   # inst, above: ok; 21 < D = 25: nothing raised
                    R.PREPARE_MSG)
    a = dict(msgs=msgs, groups=groups, st=st, inst_base=0, ipg=8, inst=inst, arena=arena)
    want = check(mk_engine(3, CLASSIC), CLASSIC, 3, a)
    assert want["replies"]["ok"].tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1]
    assert want["replies"]["ballot"].tolist() == [20, 20, 20, 20, 20, 25, 20, 20, 20]
    assert (want["effect"] & R.PRH_RAISED).tolist() == [0, 0, 0, 0, 2, 0, 0, 0, 0]
    assert int(want["groups"]["default_ballot"][0]) == 25


# ---- the encoder's out rule -----------------------------------------------------------------------------
@MODES
def test_destinations_alignments_and_out_cap(mk_engine, mode):
    """all replies to one destination, reply_to = -1 mixed in, n_dest of 1 and 16, out at every
    offset from a 16-byte boundary, out_cap exactly the total and one byte short"""
    N = 5
    e = mk_engine(N, mode)
    a = T.fuzz_case(3, mode, N=N, G=6, n=70)
    h = T.run_batch(mode, N, **a)
    store = {k: a.get(k) for k in ("st", "lb", "inst", "arena")}
    n = len(a["msgs"])
    rng = np.random.default_rng(1)
    variants = [(np.full(n, 2, np.int32), N), (np.zeros(n, np.int32), 1),
                (np.where(rng.random(n) < 0.4, -1, h["reply_to"]).astype(np.int32), N),
                (rng.integers(-1, 16, n).astype(np.int32), 16), (np.full(n, -1, np.int32), N)]
    with Arena(e) as ar:
        d = store_dev(ar, a)
        d_rep = ar.put(h["replies"])
        d_lf = ar.put(h["log_from"]) if mode == MIN else None
        for v, (to, n_dest) in enumerate(variants):
            w_out, w_off = T.partition(h["frames"], to, n_dest)
            out, off = e.encode_prepare_replies(h["replies"], to, h["log_from"], n_dest,
                                                a["inst_base"], **store)
            assert np.array_equal(off, w_off)
            same_bytes(out, w_out, f"host form, variant {v}")
            d_to = ar.put(to)
            for shift in (range(16) if v == 2 else (v,)):
                out, off = encode_dev(e, ar, mode, a, d, d_rep.ptr, d_to.ptr,
                                      d_lf.ptr if d_lf else None, n, n_dest, len(w_out), shift)
                assert np.array_equal(off, w_off)
                same_bytes(out, w_out, f"device form, variant {v}, shift {shift}")
        # one byte short: the device form writes the prefix and the complete dest_off, the host
        # form answers MPX_E_INVAL
        to = h["reply_to"]
        w_out, w_off = T.partition(h["frames"], to, N)
        d_to = ar.put(to)
        for short, shift in ((1, 0), (1, 7), (len(w_out), 1)):
            out, off = encode_dev(e, ar, mode, a, d, d_rep.ptr, d_to.ptr, d_lf.ptr if d_lf else None,
                                  n, N, len(w_out) - short, shift)
            assert np.array_equal(off, w_off)
            same_bytes(out, w_out[:len(w_out) - short], f"short by {short}")
        with pytest.raises(MpxError) as ei:
            e.encode_prepare_replies(h["replies"], to, h["log_from"], N, a["inst_base"],
                                     out_cap=len(w_out) - 1, **store)
        assert ei.value.code == R.E_INVAL
        out, _ = e.encode_prepare_replies(h["replies"], to, h["log_from"], N, a["inst_base"],
                                          out_cap=len(w_out), **store)
        same_bytes(out, w_out, "exact out_cap")


def test_short_out_cap_inside_a_long_frame(mk_engine):
    a = big_case(MIN)
    e = mk_engine(3, MIN)
    h = T.run_batch(MIN, 3, **a)
    total = len(h["bytes"])
    assert total > WINDOW + 100
    with Arena(e) as ar:
        d = store_dev(ar, a)
        d_rep, d_to, d_lf = ar.put(h["replies"]), ar.put(h["reply_to"]), ar.put(h["log_from"])
        for cap, shift in ((total - 1, 5), (WINDOW + 3, 0), (WINDOW - 1, 9), (0, 0)):
            out, off = encode_dev(e, ar, MIN, a, d, d_rep.ptr, d_to.ptr, d_lf.ptr, len(a["msgs"]), 3,
                                  cap, shift)
            assert np.array_equal(off, h["dest_off"])
            same_bytes(out, h["bytes"][:cap], f"out_cap {cap}")


# ---- errors through the device error word, and the safe encoding -------------------------------------
def dev_code(e, mode, N, a, n_dest=None):
    """the handler's code from the error word, then the encoder run on what it left: whatever the
    fault, the bytes written equal dest_off's total and every guard is intact. Returns (handler
    code, encoder code, handler results)."""
    n_dest = N if n_dest is None else n_dest
    with Arena(e) as ar:
        g, d = handle_dev(e, ar, mode, N, a)
        hc = 0
        try:
            e.synchronize()
        except MpxError as x:
            hc = x.code
        got = read_handle(g)
        n = len(a["msgs"])
        cap = 1 << 16
        g_out, g_off = encode_dev(e, ar, mode, a, d, g["rep"].ptr, g["to"].ptr,
                                  g["lf"].ptr if "lf" in g else None, n, n_dest, cap, 3, sync=False)
        ec = 0
        try:
            e.synchronize()
        except MpxError as x:
            ec = x.code
        off = g_off.assert_margins()
        out = g_out.assert_margins()
        total = int(off[-1])
        assert total <= cap and (np.diff(off.astype(np.int64)) >= 0).all()
        g_out.assert_untouched([(total, cap)])
        # the run parses as whole PrepareReply frames: sizes and bytes agree
        pos, buf = 0, out[:total].tobytes()
        while pos < total:
            code, _, pos = U.unmarshal(mode, buf, pos)
            assert code == R.PEER_PREPARE_REPLY
        assert pos == total
        for k in ("sop", "skey", "sval"):
            d[k].assert_margins()
        return hc, ec, got


def kat(name):
    mode, kw, _ = K.CASES[name]()
    N = kw.pop("N")
    return mode, N, kw


def test_handler_errors_min(mk_engine):
    mode, N, a = kat("min_command_and_log")
    e = mk_engine(N, mode)

    def both(bad, code):
        with pytest.raises(GoPanic) as gp:
            T.run_batch(mode, N, **bad)
        assert gp.value.code == code
        with pytest.raises(MpxError) as ei:
            e.prepare_handle(bad["msgs"], bad["st"], bad["groups"], bad["inst_base"], bad["ipg"])
        assert ei.value.code == code
        hc, _, got = dev_code(e, mode, N, bad)
        assert hc == code
        return got

    def msg(*m):
        return np.array(list(m), R.PREPARE_MSG)
    both(dict(a, msgs=msg((0, 0x20, 0, 7))), R.E_NIL_INSTANCE)       # the log starts below first
    nil = dict(a, st=a["st"].copy())
    nil["st"]["status"][1] = R.STATUS_NIL                               # a nil slot in the range
    grp = a["groups"].copy()
    grp["crt_instance"] = 12
    got = both(dict(nil, groups=grp), R.E_NIL_INSTANCE)
    assert int(got["replies"]["value_id"][0]) == R.VALUE_KEEP
    assert int(got["log_from"][0]) == int(got["replies"]["last_committed"][0]) + 1
    full = dict(a, st=a["st"].copy())
    full["st"]["status"][:], full["st"]["ballot"][:] = R.ACCEPTED, 1   # crtInstance leaves the window
    both(full, R.E_NIL_INSTANCE)
    cu = a["groups"].copy()
    cu["committed_upto"] = 12                                           # slot committedUpTo + 1 is nil
    both(dict(a, groups=cu), R.E_NIL_INSTANCE)
    both(dict(a, msgs=msg((0, 0x20, 3, 9))), R.E_BAD_ID)
    both(dict(a, msgs=msg((0, 0x20, -1, 9))), R.E_BAD_ID)
    both(dict(a, msgs=msg((1, 0x20, 0, 9))), R.E_INVAL)                 # no such group
    two = dict(a, st=np.concatenate([a["st"], a["st"]]), inst=np.concatenate([a["inst"], a["inst"]]),
               groups=np.concatenate([a["groups"], a["groups"]]))
    two["groups"]["crt_instance"][1], two["groups"]["committed_upto"][1] = 20, 19
    both(dict(two, msgs=msg((1, 0x20, 0, 25), (0, 0x20, 0, 9))), R.E_INVAL)   # out of order


def test_handler_errors_classic(mk_engine):
    mode, N, a = kat("classic_inst")
    e = mk_engine(N, mode)
    for m, code in (([(12, 8, 2, 1)], R.E_NIL_INSTANCE), ([(3, 8, 2, 1)], R.E_NIL_INSTANCE),
                    ([(8, 8, 3, 1)], R.E_BAD_ID), ([(8, 8, 2, 1), (7, 8, 2, 1)], R.E_INVAL)):
        bad = dict(a, msgs=np.array(m, R.PREPARE_MSG))
        with pytest.raises(GoPanic) as gp:
            T.run_batch(mode, N, **bad)
        assert gp.value.code == code
        with pytest.raises(MpxError) as ei:
            e.prepare_handle(bad["msgs"], bad["st"], bad["groups"], bad["inst_base"], bad["ipg"])
        assert ei.value.code == code
        assert dev_code(e, mode, N, bad)[0] == code


@MODES
def test_encoder_errors(mk_engine, mode):
    """a reply_to past n_dest, a value_id outside the window, a Command range and a log instance's
    range that leave the arena, a log range that leaves the window, a nil instance inside one"""
    name = "min_command_and_log" if mode == MIN else "classic_inst"
    _, N, a = kat(name)
    e = mk_engine(N, mode)
    h = T.run_batch(mode, N, **a)
    n_src = len(a["arena"][0])
    vid = int(h["replies"]["value_id"][0])

    def run(code, replies=None, to=None, lf=None, **store):
        s = {k: store.get(k, a.get(k)) for k in ("st", "lb", "inst", "arena")}
        rep = h["replies"] if replies is None else replies
        to = h["reply_to"] if to is None else to
        lf = h["log_from"] if lf is None else lf
        with pytest.raises(MpxError) as ei:
            e.encode_prepare_replies(rep, to, lf, N, a["inst_base"], **s)
        assert ei.value.code == code
        case = dict(a, **s)
        with Arena(e) as ar:
            d = store_dev(ar, case)
            g_out, g_off = encode_dev(e, ar, mode, case, d, ar.put(rep).ptr, ar.put(to).ptr,
                                      ar.put(lf).ptr if mode == MIN else None, 1, N, 4096, 1,
                                      sync=False)
            with pytest.raises(MpxError) as ei:
                e.synchronize()
            assert ei.value.code == code
            off, out = g_off.assert_margins(), g_out.assert_margins()
            total = int(off[-1])
            g_out.assert_untouched([(total, 4096)])
            pos, buf = 0, out[:total].tobytes()
            while pos < total:
                _, _, pos = U.unmarshal(mode, buf, pos)
            assert pos == total
            for k in ("sop", "skey", "sval"):
                d[k].assert_margins()
        return total

    assert run(R.E_INVAL, to=np.array([N], np.int32)) == 0
    rep = h["replies"].copy()
    rep["value_id"][0] = len(a["st"])
    run(R.E_INVAL, replies=rep)
    for first, k in ((n_src - 1, 2), (n_src + 1, 0), (1 << 40, 1), (0, n_src + 1)):
        inst = a["inst"].copy()
        inst[vid] = (first, k, R.IC_HAS_CMDS)
        total = run(R.E_INVAL, inst=inst)
        assert total == len(h["bytes"]) - 17 * int(a["inst"]["n_cmds"][vid])   # encoded as V(0)
    if mode == MIN:
        run(R.E_INVAL, lf=np.array([9], np.int32))
        rep = h["replies"].copy()
        rep["last_committed"][0] = 18
        run(R.E_INVAL, replies=rep)
        st = a["st"].copy()
        st["status"][1] = R.STATUS_NIL
        run(R.E_NIL_INSTANCE, st=st)
        inst = a["inst"].copy()
        inst[0] = (n_src, 1, R.IC_HAS_CMDS)
        run(R.E_INVAL, inst=inst)


def test_dev_forms_need_their_reserve(mk_engine):
    mode, N, a = kat("min_command_and_log")
    e = mk_engine(N, mode)
    h = T.run_batch(mode, N, **a)
    with Arena(e) as ar:
        d = store_dev(ar, a)
        b = encode_batch(mode, a, d, ar.put(h["replies"]).ptr, ar.put(h["reply_to"]).ptr,
                         ar.put(h["log_from"]).ptr, 1, N)
        g_out, g_off = Guard(ar, 256, np.uint8), Guard(ar, N + 1, np.uint64)
        with pytest.raises(MpxError, match="mpx_encode_prepare_replies_reserve"):
            e.encode_prepare_replies_dev(b, g_out.ptr, 256, g_off.ptr)
        none = _lib.MpxPrepareReplyBatch.from_buffer_copy(b)
        none.n = 0
        e.encode_prepare_replies_dev(none, g_out.ptr, 256, g_off.ptr)
        e.synchronize()
        assert not g_off.assert_margins().any()
        g_out.assert_untouched([(0, 256)])
        e.encode_prepare_replies_reserve(64, 4096, N)
        e.encode_prepare_replies_dev(b, g_out.ptr, 256, g_off.ptr)
        e.synchronize()
        assert g_out.assert_margins()[:int(g_off.assert_margins()[-1])].tobytes() == \
            bytes(h["bytes"])


# ---- the round trip: handler -> encoder -> decode -> unmarshal -> select ------------------------------
def leader_side(e, mode, N, followers, leader):
    """each follower's run for `leader` through mpx_decode_stream and mpx_unmarshal_frames;
    returns per follower (decoded prepare records, the transliteration's results, kept indices)"""
    out = []
    for a in followers:
        got = e.prepare_handle(a["msgs"], a["st"], a["groups"], a["inst_base"], a["ipg"])
        want = T.run_batch(mode, N, **{k: v for k, v in a.items() if k not in ("gps", "peer_commits")})
        same_recs(got["replies"], want["replies"], "replies")
        by, off = e.encode_prepare_replies(got["replies"], got["reply_to"], got["log_from"], N,
                                           a["inst_base"], st=a["st"], lb=a["lb"], inst=a["inst"],
                                           arena=a["arena"])
        run = by[int(off[leader]):int(off[leader + 1])].tobytes()
        keep = np.flatnonzero(got["reply_to"] == leader)
        _, pr, var, _, res = e.decode_stream(run, caps=(1, len(keep) + 1, len(keep) + 1, 1))
        assert int(res["stop_reason"]) == R.DECODE_END and len(pr) == len(keep) == len(var)
        rep = got["replies"][keep]
        for f in rep.dtype.names:
            if f != "value_id":
                assert np.array_equal(pr[f], rep[f]), f
        arrays, ures = e.unmarshal_frames(run, var)
        # the commands and the log are the store's content
        cmds, log = [], []
        for i in keep:
            r = got["replies"][i]
            v = int(r["value_id"])
            if v != R.VALUE_KEEP and int(a["inst"]["flags"][v]) & R.IC_HAS_CMDS:
                c0, nc = int(a["inst"]["first_cmd"][v]), int(a["inst"]["n_cmds"][v])
                cmds += [(int(a["arena"][0][j]), int(a["arena"][1][j]), int(a["arena"][2][j]))
                         for j in range(c0, c0 + nc)]
            if mode == MIN:
                for inst_no in range(int(got["log_from"][i]), int(r["last_committed"]) + 1):
                    k = inst_no - a["inst_base"]
                    status = int(a["st"]["status"][k])
                    if a["lb"] is not None and int(a["lb"]["status"][k]) != R.STATUS_NIL:
                        status = int(a["lb"]["status"][k])
                    log.append((int(a["st"]["ballot"][k]), status, inst_no))
        assert list(zip(arrays["op"].tolist(), arrays["key"].tolist(), arrays["val"].tolist())) == cmds
        assert [(int(x["ballot"]), int(x["status"]), int(x["inst_no"]))
                for x in arrays["log_recs"]] == log
        out.append((pr, want, keep))
    return out


def test_round_trip_and_select_classic(mk_engine):
    N, G, ipg, leader = 5, 6, 8, 2
    e = mk_engine(N, CLASSIC)
    followers = []
    for f in range(4):
        a = T.fuzz_case(40 + f, CLASSIC, N=N, G=G, ipg=ipg, n=60)
        a["inst_base"] = 0
        a["msgs"]["key"] = np.sort(np.random.default_rng(f).integers(0, G * ipg, 60))
        a["msgs"]["leader_id"] = np.where(np.arange(60) % 3 == 0, (leader + 1) % N, leader)
        followers.append(a)
    sides = leader_side(e, CLASSIC, N, followers, leader)
    recs, _, _ = e.order_records([pr for pr, _, _ in sides], G * ipg, 0)
    ref = [w["replies"][keep].copy() for _, w, keep in sides]
    for r, (pr, _, _) in zip(ref, sides):
        r["value_id"] = pr["value_id"]        # (a handle the leader's decode assigns)
    allref = np.concatenate(ref)
    allref = allref[np.argsort(allref["instance"], kind="stable")]
    same_recs(recs, allref, "ordered replies")
    st = np.zeros(G * ipg, R.PREP_STATE)
    st["status"], st["ballot"], st["max_recv_ballot"], st["value_id"] = R.PREPARING, 40, -1, 7
    got = e.prepare_select(recs, st, 0, 3)
    want = GoBackend(N, CLASSIC).prepare_select(allref, st, 0, 3)
    same_recs(got[0], want[0], "prep state")
    assert got[1] == want[1] and np.array_equal(got[2], want[2])


def test_round_trip_and_select_min(mk_engine):
    N, G, ipg, leader = 5, 6, 8, 2
    e = mk_engine(N, MIN)
    followers = []
    for f in range(4):
        a = T.fuzz_case(60 + f, MIN, N=N, G=G, ipg=ipg, n=40)
        a["msgs"]["leader_id"] = np.where(np.arange(40) % 3 == 0, (leader + 1) % N, leader)
        a["msgs"]["ballot"] = np.where(np.arange(40) % 4 == 0, a["msgs"]["ballot"], 90)
        a["groups"]["self_id"] = f if f < leader else f + 1
        followers.append(a)
    sides = leader_side(e, MIN, N, followers, leader)
    # the contract order through mpx_order_records: 16-byte keys (the group of each reply's
    # connection slot), its permutation applied to the 24-byte records
    keys = []
    for (pr, _, keep), a in zip(sides, followers):
        k = np.zeros(len(pr), R.ACCEPT_MSG)
        k["instance"] = a["msgs"]["key"][keep]
        keys.append(k)
    _, perm, _ = e.order_records(keys, G, 0)
    cat = np.concatenate([pr for pr, _, _ in sides])
    recs = cat[perm]
    grp = np.concatenate(keys)["instance"][perm]
    off = np.searchsorted(grp, np.arange(G + 1)).astype(np.uint64)
    ref = np.concatenate([w["replies"][keep] for _, w, keep in sides])
    ref["value_id"] = cat["value_id"]
    ref = ref[np.argsort(np.concatenate(keys)["instance"], kind="stable")]
    same_recs(recs, ref, "ordered replies")
    gst = np.zeros(G, R.GROUP_PREP_STATE)
    gst["default_ballot"], gst["max_recv_ballot"], gst["value_id"] = 90, 90, R.VALUE_KEEP
    gst["highest_instance"] = [followers[0]["inst_base"] + g * ipg for g in range(G)]
    gst["committed_upto"] = gst["highest_instance"] - 1
    pc = np.repeat(gst["highest_instance"], N).astype(np.int32)
    got = e.prepare_select_min(recs, off, gst, pc)
    want = GoBackend(N, MIN).prepare_select_min(ref, off, gst, pc)
    same_recs(got[0], want[0], "group prep state")
    assert np.array_equal(got[1], want[1])
    same_recs(got[2], want[2], "effects")


# ---- the gather ----------------------------------------------------------------------------------------
def prepare_stream(mode, rng, n):
    """Prepares between Beacons and CommitShorts; returns (bytes, the Prepare records for group 4)"""
    parts, msgs = [], []
    for _ in range(n):
        u = rng.random()
        if u < 0.2:
            parts.append(bytes([R.PEER_BEACON]) + bytes(rng.integers(0, 256, 8).astype(np.uint8)))
        elif u < 0.4:
            parts.append(bytes([R.PEER_COMMIT_SHORT]) + bytes(rng.integers(0, 256, 16).astype(np.uint8)))
        else:
            leader, ballot = int(rng.integers(0, 5)), int(rng.integers(-(1 << 31), 1 << 31))
            x = int(rng.integers(-(1 << 31), 1 << 31))
            y = int(rng.integers(0, 256))
            parts.append(T.prepare_frame(mode, leader, ballot, x, y))
            msgs.append((4, ballot, leader, x) if mode == MIN else (x, ballot, leader, y))
    return b"".join(parts), np.array(msgs, R.PREPARE_MSG) if msgs else np.zeros(0, R.PREPARE_MSG)


@MODES
def test_gather_behind_decode_stream_dev(mk_engine, mode):
    e = mk_engine(5, mode)
    for n in (1, 40, 5000):
        buf, want = prepare_stream(mode, np.random.default_rng(n), n)
        ln = len(buf)
        _, _, _, oth, res = e.decode_stream(buf)
        msgs, idx, cnt = e.gather_prepares(buf, oth, group=4)
        assert cnt == len(want)
        same_recs(msgs, want, "host form")
        assert (oth["code"][idx] == R.PEER_PREPARE).all() and (np.diff(idx.astype(np.int64)) > 0).all()
        with Arena(e) as ar:
            pad = np.zeros((ln + 15) // 16 * 16, np.uint8)
            pad[:ln] = np.frombuffer(buf, np.uint8)
            d_buf = ar.put(pad)
            caps = (8, 8, 8, n + 7)
            g_ar, g_pr = Guard(ar, caps[0], R.ACCEPT_REPLY), Guard(ar, caps[1], rdt(mode))
            g_var, g_oth = Guard(ar, caps[2], R.VAR_FRAME), Guard(ar, caps[3], R.PEER_FRAME)
            g_res = Guard(ar, 1, R.STREAM_RESULT)
            out = _lib.MpxDecodeOut(g_ar.ptr, caps[0], g_pr.ptr, caps[1], g_var.ptr, caps[2],
                                    g_oth.ptr, caps[3])
            e.decode_stream_reserve(ln)
            e.encode_prepare_replies_reserve(caps[3], 0, 1)
            for cap in (len(want), max(len(want) - 3, 0)):
                g_msg, g_idx = Guard(ar, cap, R.PREPARE_MSG), Guard(ar, cap, np.uint32)
                g_cnt = Guard(ar, 1, np.uint64)
                g_res.put(np.zeros(1, R.STREAM_RESULT))      # (in/out: zero for a new stream)
                e.decode_stream_dev(d_buf.ptr, ln, 0, out, g_res.ptr)
                e.gather_prepares_dev(d_buf.ptr, ln, g_oth.ptr, caps[3],
                                      g_res.ptr + R.STREAM_RESULT.fields["n_other"][1], 4,
                                      g_msg.ptr, g_idx.ptr, cap, g_cnt.ptr)
                e.synchronize()
                assert int(g_cnt.assert_margins()[0]) == len(want)
                same_recs(g_msg.assert_margins(), want[:cap], "device form")
                assert np.array_equal(g_idx.assert_margins(), idx[:cap])
    # a frame whose body runs past len: the host form refuses, the device form skips it
    buf, want = prepare_stream(mode, np.random.default_rng(3), 12)
    _, _, _, oth, _ = e.decode_stream(buf)
    last = int(np.flatnonzero(oth["code"] == R.PEER_PREPARE)[-1])
    cut = int(oth["offset"][last]) + 5
    with pytest.raises(MpxError) as ei:
        e.gather_prepares(buf[:cut], oth, group=4)
    assert ei.value.code == R.E_INVAL


# ---- the chain in a graph ---------------------------------------------------------------------------------
@MODES
def test_graph_gather_handle_encode_replayed_twice(mk_engine, mode):
    """mpx_gather_prepares_dev -> mpx_prepare_handle_dev -> mpx_encode_prepare_replies_dev captured
    as one linear chain and replayed twice, the input bytes and the groups changed in between"""
    N, G, ipg = 3, 1 if mode == MIN else 4, 8
    e = mk_engine(N, mode)
    turns = []
    for t in range(2):
        a = T.fuzz_case(80 + t, mode, N=N, G=G, ipg=ipg, n=24)
        if t:  # one store for both turns: the first turn's
            for k in ("st", "lb", "inst", "arena", "inst_base"):
                a[k] = turns[0]["a"][k]
            b = T.fuzz_case(80, mode, N=N, G=G, ipg=ipg, n=24)
            a["groups"] = b["groups"]
            a["groups"]["default_ballot"] += 3
            a["msgs"] = b["msgs"][::-1].copy()
            a["msgs"]["ballot"] += 1
            a["msgs"] = a["msgs"][np.argsort(a["msgs"]["key"], kind="stable")]
        m = a["msgs"]
        frames = [T.prepare_frame(mode, int(x["leader_id"]), int(x["ballot"]),
                                  int(x["arg"]) if mode == MIN else int(x["key"]), int(x["arg"]))
                  for x in m]
        beacon = bytes([R.PEER_BEACON]) + b"\x07" * 8
        buf = beacon + b"".join(f + (beacon if i % 5 == 0 else b"") for i, f in enumerate(frames))
        if mode == MIN:
            m["key"] = 0
        turns.append(dict(a=a, buf=buf, want=T.run_batch(mode, N, **a)))
    cap_len = max(len(t["buf"]) for t in turns)
    cap_len = (cap_len + 15) // 16 * 16
    n_max, oth_cap, out_cap = 24, 64, 1 << 14
    a0 = turns[0]["a"]
    with Arena(e) as ar:
        d = store_dev(ar, a0)
        d_buf = ar.full(cap_len, np.uint8, 0)
        g_oth, g_res = Guard(ar, oth_cap, R.PEER_FRAME), Guard(ar, 1, R.STREAM_RESULT)
        g_ar, g_pr, g_var = Guard(ar, 4, R.ACCEPT_REPLY), Guard(ar, 4, rdt(mode)), Guard(ar, 4, R.VAR_FRAME)
        g_msg, g_idx, g_cnt = Guard(ar, n_max, R.PREPARE_MSG), Guard(ar, n_max, np.uint32), \
            Guard(ar, 1, np.uint64)
        g_grp = Guard(ar, G, R.PROPOSER_GROUP)
        g_rep, g_to, g_eff = Guard(ar, n_max, rdt(mode)), Guard(ar, n_max, np.int32), \
            Guard(ar, n_max, np.uint8)
        g_lf = Guard(ar, n_max, np.int32) if mode == MIN else None
        g_out, g_off = Guard(ar, out_cap, np.uint8, shift=5), Guard(ar, N + 1, np.uint64)
        dec = _lib.MpxDecodeOut(g_ar.ptr, 4, g_pr.ptr, 4, g_var.ptr, 4, g_oth.ptr, oth_cap)
        eb = encode_batch(mode, a0, d, g_rep.ptr, g_to.ptr, g_lf.ptr if g_lf else None, n_max, N)
        e.decode_stream_reserve(cap_len)
        e.encode_prepare_replies_reserve(max(n_max, oth_cap), len(a0["st"]), N)
        s = e.stream_create()
        try:
            for t in turns:  # the decode runs outside the graph: its byte count changes per turn
                pad = np.zeros(cap_len, np.uint8)
                pad[:len(t["buf"])] = np.frombuffer(t["buf"], np.uint8)
                t["pad"] = pad
            e.graph_begin(s)
            e.gather_prepares_dev(d_buf.ptr, cap_len, g_oth.ptr, oth_cap,
                                  g_res.ptr + R.STREAM_RESULT.fields["n_other"][1], 0, g_msg.ptr,
                                  g_idx.ptr, n_max, g_cnt.ptr, s)
            e.prepare_handle_dev(g_msg.ptr, n_max, d["st"].ptr, len(a0["st"]), a0["inst_base"],
                                 g_grp.ptr, G, ipg, g_rep.ptr, g_to.ptr, g_eff.ptr,
                                 g_lf.ptr if g_lf else None, None, None, s)
            e.encode_prepare_replies_dev(eb, g_out.ptr, out_cap, g_off.ptr, s)
            gr = e.graph_end(s)
            try:
                for t in turns:
                    a, want = t["a"], t["want"]
                    assert len(a["msgs"]) == n_max
                    e.memcpy(d_buf.ptr, t["pad"].ctypes.data_as(C.c_void_p), cap_len, 1, s)
                    e.stream_synchronize(s)
                    g_res.put(np.zeros(1, R.STREAM_RESULT), s)  # (in/out: zero for a new stream)
                    e.decode_stream_dev(d_buf.ptr, len(t["buf"]), 0, dec, g_res.ptr, s)
                    g_grp.put(a["groups"], s)
                    g_out.fill(s)
                    e.graph_launch(gr, s)
                    e.stream_synchronize(s)
                    e.synchronize()
                    assert int(g_cnt.assert_margins()[0]) == n_max
                    same_recs(g_msg.assert_margins(), a["msgs"], "gathered")
                    same_recs(g_rep.assert_margins(), want["replies"], "replies")
                    same_recs(g_grp.assert_margins(), want["groups"], "groups")
                    assert np.array_equal(g_eff.assert_margins(), want["effect"])
                    off = g_off.assert_margins()
                    assert np.array_equal(off, want["dest_off"])
                    same_bytes(g_out.assert_margins()[:int(off[-1])], want["bytes"], "graph replay")
            finally:
                e.graph_destroy(gr)
        finally:
            e.stream_destroy(s)

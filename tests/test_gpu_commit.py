"""GPU tests of the commit side: mpx_commit_handle (batched handleCommit / handleCommitShort with
committedUpTo), mpx_encode_commits (the CommitShort / Commit frames bcastCommit writes per peer
connection) and mpx_gather_commit_shorts, host and device forms, bit- and byte-exact against
tests/commit_translit.py. Shapes are the smallest that reach each path: the handler walks tiles of
1024 records with a lane per instance, the prefix kernel runs a wave per group over chunks of 64
statuses, the encoder's output window is 8192 bytes and its item chunk 256."""
import numpy as np
import pytest

import commit_translit as T
from devguard import Guard
from go_translit import GoBackend
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError
from proposer_translit import mk_cmds, mk_state, nil_state

pytestmark = pytest.mark.gpu
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
MODES = [MIN, CLASSIC]
MODE_IDS = ["min", "classic"]
WINDOW = 8192
TILE = 1024
NIL, KEEP, C = T.NIL, T.KEEP, T.COMMITTED
CH_NAMES = ("st", "committed_upto", "effect", "log_recs")


def same_arrays(names, got, want):
    for name, g, w in zip(names, got, want):
        if w is None:
            assert g is None, name
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            diff = [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()][:5]
            raise AssertionError(f"{name} differs at {diff}: got {g[diff]} want {w[diff]}")


# ---- commit_handle ---------------------------------------------------------------------------------
def ch_dev(e, ar, msgs, st, committed_upto, inst_base, ipg, want_log=True, eff_shift=0,
           want_call=False):
    """the _dev form in place on guarded buffers; returns what the host form returns"""
    n, G = len(msgs), len(committed_upto)
    d_msgs = ar.put(msgs)
    g_st = Guard(ar, len(st), R.ACCEPTOR_STATE).put(st)
    g_cu = Guard(ar, G, np.int32).put(committed_upto)
    g_eff = Guard(ar, n, np.uint8, shift=eff_shift)
    g_log = Guard(ar, n, R.LOG_REC) if want_log else None

    def call(s=None):
        e.commit_handle_dev(d_msgs.ptr, n, g_st.ptr, len(st), inst_base, g_cu.ptr, G, ipg,
                            g_eff.ptr, g_log.ptr if g_log else None, s)

    def results():
        return (g_st.assert_margins(), g_cu.assert_margins(), g_eff.assert_margins(),
                g_log.assert_margins() if g_log else None)
    if want_call:
        return call, results, (d_msgs, g_st, g_cu, g_eff, g_log)
    call()
    e.synchronize()
    return results()


def check_ch(e, a, want_log=True, eff_shift=0):
    want = T.commit_handle(**a)
    if not want_log:
        want = want[:3] + (None,)
    got = e.commit_handle(a["msgs"], a["st"], a["committed_upto"], a["inst_base"], a["ipg"],
                          want_log=want_log)
    same_arrays(CH_NAMES, got, want)
    with Arena(e) as ar:
        same_arrays(CH_NAMES, ch_dev(e, ar, **a, want_log=want_log, eff_shift=eff_shift), want)
    return want


def random_state(rng, n_inst):
    st = np.zeros(n_inst, R.ACCEPTOR_STATE)
    st["status"] = np.where(rng.random(n_inst) < 0.4, NIL, rng.integers(0, 4, n_inst))
    live = st["status"] != NIL
    st["ballot"] = np.where(live, rng.integers(0, 1 << 10, n_inst), 0)
    st["value_id"] = np.where(live, rng.integers(0, 1 << 20, n_inst), 0)
    st["flags"] = np.where(live & (rng.random(n_inst) < 0.4), R.PF_HAS_PROPOSALS, 0)
    return st


def batch(seed, counts, ipg, base=-37, touch_every=1, n_inst=None):
    """instance k of the touched ones carries counts[k] messages; every touch_every-th instance of
    the window is touched; the window is as many groups of ipg as that takes"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    k = len(counts)
    if n_inst is None:
        n_inst = max(-(-(k * touch_every) // ipg), 1) * ipg
    G = n_inst // ipg
    st = random_state(rng, n_inst)
    cu = np.array([base + g * ipg - 1 for g in range(G)], np.int32)
    for g in range(G):  # a committed prefix and a watermark somewhere inside it
        p = int(rng.integers(0, ipg + 1))
        st["status"][g * ipg:g * ipg + p] = C
        cu[g] += int(rng.integers(0, p + 1))
    n = int(counts.sum())
    msgs = np.zeros(n, R.ACCEPT_MSG)
    msgs["instance"] = np.repeat(base + np.arange(k) * touch_every, counts)
    msgs["ballot"] = rng.integers(0, 1 << 10, n)
    msgs["leader_id"] = rng.integers(0, 5, n)
    msgs["value_id"] = np.where(rng.random(n) < 0.5, KEEP, rng.integers(0, 1 << 20, n))
    return dict(msgs=msgs, st=st, committed_upto=cu, inst_base=base, ipg=ipg)


def test_ch_known_answers(mk_engine):
    """the hand-traced answers of test_commit_translit.py, through the engine"""
    e = mk_engine(5, MIN)
    H = R.PF_HAS_PROPOSALS

    def run(rows, msgs, cu, ipg=None):
        st = mk_state(rows)
        a = dict(msgs=T.mk_msgs(msgs), st=st, committed_upto=np.array(cu, np.int32),
                 inst_base=100, ipg=len(st) // len(cu) if ipg is None else ipg)
        w = check_ch(e, a)
        return [tuple(int(x) for x in r) for r in w[0].tolist()], w[1].tolist(), w[2].tolist()
    N4 = (NIL, 0, 0, 0)
    assert run([N4, N4], [(100, 17, 2, 55)], [99]) == \
        ([(C, 17, 55, 0), N4], [100], [R.CH_INSTALLED | R.CH_CMDS])
    assert run([N4], [(100, 9, 0, KEEP)], [99]) == ([(C, 9, KEEP, 0)], [100], [R.CH_INSTALLED])
    assert run([(T.PREPARED, 17, 44, H)], [(100, 18, 0, 55), (100, 18, 0, KEEP)], [99]) == \
        ([(C, 18, 55, R.PF_REQUEUED)], [100], [R.CH_CMDS | R.CH_REQUEUE, 0])
    assert run([N4] * 4, [(100, 1, 0, 5), (101, 1, 0, KEEP), (103, 1, 0, 6)], [99])[1] == [101]
    rows = [N4, N4, (C, 1, 1, 0), (C, 1, 1, 0)]
    assert run(rows, [(100, 1, 0, 5)], [99, 101], ipg=2)[1] == [100, 101]  # group 1 untouched
    rows = [(C, 1, 1, 0), N4, (C, 1, 1, 0), (C, 1, 1, 0)]
    assert run(rows, [(101, 1, 0, 5)], [99, 101], ipg=2)[1] == [101, 101]  # the window's end


@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ch_message_counts(mk_engine, mode, n):
    """one message per instance around the tile size; the mode changes nothing"""
    e = mk_engine(5, mode)
    a = batch(n, [1] * n, 64)
    w = check_ch(e, a, eff_shift=n % 4)
    if n == 0:  # nothing is touched, the watermarks included
        assert np.array_equal(w[1], a["committed_upto"]) and w[0].tobytes() == a["st"].tobytes()


def test_ch_one_instance_spanning_three_tiles(mk_engine):
    check_ch(mk_engine(5, MIN), batch(1, [3, 1, 2500, 2, 1], 8), eff_shift=1)


def test_ch_run_starting_on_a_tiles_last_record(mk_engine):
    a = batch(2, [1] * (TILE - 1) + [5, 1, 1], 256)
    assert int(a["msgs"]["instance"][TILE - 1]) != int(a["msgs"]["instance"][TILE - 2])
    assert int(a["msgs"]["instance"][TILE - 1]) == int(a["msgs"]["instance"][TILE + 3])
    check_ch(mk_engine(5, MIN), a)


@pytest.mark.parametrize("ipg,G", [(1, 1), (1, 300), (3, 1), (3, 77), (64, 5), (256, 2), (256, 9)])
def test_ch_window_shapes(mk_engine, ipg, G):
    """group sizes below, at and above a wave's 64 statuses, 1 to 300 groups, every other instance
    touched and ragged fan-in"""
    rng = np.random.default_rng(ipg * 1000 + G)
    k = -(-(G * ipg) // 2)
    a = batch(ipg + G, rng.choice([1, 1, 2, 4], k).tolist(), ipg, touch_every=2, n_inst=G * ipg)
    assert len(a["committed_upto"]) == G
    check_ch(mk_engine(5, MIN), a, want_log=bool(G & 1))


ADVANCES = [0, 1, 63, 64, 65, 128, 255, 256]


@pytest.mark.parametrize("start", [-1, 10])
def test_ch_prefix_advances(mk_engine, start):
    """a group per advance: the watermark starts at first_g - 1 (or 10 slots in) with `adv` slots
    behind it COMMITTED or committed by this batch's last message, then a nil slot; 256 slots
    from first_g - 1 reach the window's end"""
    ipg, base = 256, 1000
    G = len(ADVANCES)
    st = nil_state(G * ipg)
    cu = np.zeros(G, np.int32)
    rows = []
    for g, adv in enumerate(ADVANCES):
        first = base + g * ipg
        c0 = first + start
        adv = min(adv, first + ipg - 1 - c0)
        cu[g] = c0
        st[g * ipg:g * ipg + start + 1] = (C, 1, 1, 0)
        lo = g * ipg + start + 1
        st[lo:lo + adv] = (C, 2, 2, 0)
        if adv:  # the run's last slot is committed by the batch
            st[lo + adv - 1] = (R.ACCEPTED, 2, 2, 0)
            rows.append((c0 + adv, 3, 0, KEEP if g & 1 else 9))
        else:    # a message that does not touch the watermark's neighbour
            rows.append((c0 + 5, 3, 0, 9))
    a = dict(msgs=T.mk_msgs(rows), st=st, committed_upto=cu, inst_base=base, ipg=ipg)
    w = check_ch(mk_engine(5, CLASSIC), a)
    want = [min(adv, ipg - 1 - start) for adv in ADVANCES]
    assert (w[1] - cu).tolist() == want
    assert int(w[1][-1]) == base + G * ipg - 1  # the window's end


def test_ch_errors(mk_engine):
    e = mk_engine(5, MIN)
    good = batch(3, [1, 2, 1], 4, base=100)
    for inst in (99, 104):  # outside the window: the reference's index panic
        a = dict(good, msgs=good["msgs"].copy())
        a["msgs"]["instance"][-1 if inst > 100 else 0] = inst
        with pytest.raises(MpxError) as ei:
            e.commit_handle(a["msgs"], a["st"], a["committed_upto"], 100, 4)
        assert ei.value.code == R.E_NIL_INSTANCE
        with Arena(e) as ar, pytest.raises(MpxError) as ei:
            ch_dev(e, ar, **a)
        assert ei.value.code == R.E_NIL_INSTANCE
    a = dict(good, msgs=good["msgs"][::-1].copy())  # descending
    with pytest.raises(MpxError) as ei:
        e.commit_handle(a["msgs"], a["st"], a["committed_upto"], 100, 4)
    assert ei.value.code == R.E_INVAL
    for bad in (98, 104):  # committed_upto outside [first_g - 1, first_g + ipg - 1]
        a = dict(good, committed_upto=np.array([bad], np.int32))
        with pytest.raises(MpxError) as ei:
            e.commit_handle(a["msgs"], a["st"], a["committed_upto"], 100, 4)
        assert ei.value.code == R.E_INVAL
        with Arena(e) as ar, pytest.raises(MpxError) as ei:  # the _dev form: the error word
            ch_dev(e, ar, **a)
        assert ei.value.code == R.E_INVAL
    with pytest.raises(MpxError) as ei:  # n_inst != n_groups * ipg
        e.commit_handle(good["msgs"], good["st"], good["committed_upto"], 100, 3)
    assert ei.value.code == R.E_INVAL
    check_ch(e, good)  # the engine is usable afterwards


@pytest.mark.parametrize("seed", T.FUZZ_SEEDS)
def test_ch_fuzz(mk_engine, seed):
    check_ch(mk_engine(5, MIN if seed & 1 else CLASSIC), T.fuzz_commit(seed), want_log=seed % 3 != 0)


def test_ch_graph_replay(mk_engine):
    """the two-kernel chain captured into a graph and replayed twice on fresh inputs"""
    e = mk_engine(5, MIN)
    a = batch(9, [1, 3, 1, 1, 2] * 300, 64)
    want = T.commit_handle(**a)
    with Arena(e) as ar:
        call, results, (d_msgs, g_st, g_cu, g_eff, g_log) = ch_dev(e, ar, **a, want_call=True)
        fresh = [ar.put(a["st"]), ar.put(a["committed_upto"])]
        s = e.stream_create()
        e.graph_begin(s)
        call(s)
        g = e.graph_end(s)
        try:
            for _ in range(2):
                for dst, src in zip((g_st, g_cu), fresh):
                    e.memcpy(dst.ptr, src.ptr, src.nbytes, D2D, s)
                g_eff.fill(s)
                g_log.fill(s)
                e.graph_launch(g, s)
                e.stream_synchronize(s)
                same_arrays(CH_NAMES, results(), want)
        finally:
            e.graph_destroy(g)
            e.stream_destroy(s)
        e.synchronize()


# ---- encode_commits --------------------------------------------------------------------------------
def scenario(seed, n, G, ipg, n_cmds, self_id=None, flags=None, base=50):
    """one send per entry of n_cmds, on consecutive instances of a window of G groups"""
    rng = np.random.default_rng(seed)
    ids = [g % n for g in range(G)] if self_id is None else self_id
    rows, c0 = [], 0
    for i, nc in enumerate(n_cmds):
        rows.append((base + i, int(rng.integers(0, 1 << 20)), c0, nc,
                     R.CS_SEND if flags is None else flags[i]))
        c0 += nc
    assert len(n_cmds) <= G * ipg
    return dict(sends=T.mk_commit_sends(rows), groups=T.mk_self(ids), cmds=mk_cmds(rng, c0),
                inst_base=base, ipg=ipg)


def commits_of(e, run, var):
    """the run's Commit frames through unmarshal_frames (a run without one has nothing to do)"""
    if len(var) == 0:
        return {"commits": np.zeros(0, R.ACCEPT_MSG)}
    arrs, r = e.unmarshal_frames(run, var)
    assert int(r["n_commits"]) == len(var) and int(r["n_accepts"]) == 0
    return arrs


def check_round_trip(e, a, q, run, frames):
    """destination q's run through the stream decoder of the engine's wire mode, its Commits
    through unmarshal_frames and its CommitShorts through the gather: they equal the sends"""
    if len(run) == 0:
        assert not frames
        return
    ar_, pr, var, oth, res = e.decode_stream(run.tobytes())
    assert int(res["stop_reason"]) == R.DECODE_END and len(ar_) == len(pr) == 0
    full = [f for f in frames if f[0] == T.COMMIT_RPC]
    assert len(var) == len(full) and len(oth) == len(frames) - len(full)
    assert (var["code"] == R.PEER_COMMIT).all() and (oth["code"] == R.PEER_COMMIT_SHORT).all()
    # which sends reached q, and how
    N = e.n_replicas
    op, key, val = a["cmds"]
    want_full, want_short = [], []
    for s in a["sends"]:
        if not int(s["flags"]) & R.CS_SEND:
            continue
        Id = int(a["groups"][(int(s["instance"]) - a["inst_base"]) // a["ipg"]]["self_id"])
        alive = [(a.get("alive_mask", 0xFFFF) >> x) & 1 == 1 for x in range(N)]
        for dq, b in T.bcast_commit(N, Id, a.get("thrifty", False), alive, 0, 0, []):
            if dq == q:
                (want_full if b[0] == T.COMMIT_RPC else want_short).append((s, Id))
    arrs = commits_of(e, run, var)
    assert len(arrs["commits"]) == len(want_full)
    for i, (s, Id) in enumerate(want_full):
        assert tuple(arrs["commits"][i].tolist()) == (int(s["instance"]), int(s["ballot"]), Id, i)
        lo, hi = int(arrs["cmd_off"][i]), int(arrs["cmd_off"][i + 1])
        c0, nc = int(s["first_cmd"]), int(s["n_cmds"])
        assert hi - lo == nc
        assert np.array_equal(arrs["op"][lo:hi], op[c0:c0 + nc])
        assert np.array_equal(arrs["key"][lo:hi], key[c0:c0 + nc])
        assert np.array_equal(arrs["val"][lo:hi], val[c0:c0 + nc])
    msgs, cnt, idx, ns = e.gather_commit_shorts(run, oth)
    assert ns == len(want_short) == len(msgs)
    assert idx.tolist() == list(range(ns))
    for i, (s, Id) in enumerate(want_short):
        assert tuple(msgs[i].tolist()) == (int(s["instance"]), int(s["ballot"]), Id, KEEP)
        assert int(cnt[i]) == int(s["n_cmds"])


def check_enc(e, a, decode=True):
    N = e.n_replicas
    w_out, w_off, per = T.encode_commits(N, **a, want_frames=True)
    out, off = e.encode_commits(**a)
    assert np.array_equal(off, w_off), (off, w_off)
    if out.tobytes() != w_out.tobytes():
        bad = np.flatnonzero(out != w_out)
        raise AssertionError(f"{len(bad)} bytes differ, first at {bad[:8]} of {len(out)}")
    if decode:
        for q in range(N):
            check_round_trip(e, a, q, out[int(off[q]):int(off[q + 1])], per[q])
    return w_out, w_off, per


@pytest.mark.parametrize("thrifty", [False, True], ids=["all", "thrifty"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 16])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_enc_replica_counts(mk_engine, mode, n, thrifty):
    """every N, both loops, alive masks from all to none, each run back through the decoders"""
    rng = np.random.default_rng(n)
    G = 12
    a = scenario(10 + n, n, G, 3, rng.integers(0, 5, 30).tolist())
    e = mk_engine(n, mode)
    check_enc(e, dict(a, thrifty=thrifty))
    check_enc(e, dict(a, thrifty=thrifty, alive_mask=int(rng.integers(0, 1 << n))))
    check_enc(e, dict(a, thrifty=thrifty, alive_mask=0), decode=False)
    check_enc(e, dict(a, thrifty=thrifty, alive_mask=1 << (n // 2)), decode=False)


@pytest.mark.parametrize("thrifty", [False, True], ids=["all", "thrifty"])
def test_enc_command_counts_across_windows(mk_engine, thrifty):
    """n_cmds at the varint steps, one frame of exactly a window (481 commands: 13 + 2 + 8177
    bytes) and one of ten windows (5000); the 17-byte and odd-sized frames around them put the
    window boundaries at every byte phase of a header and of a command"""
    ns = [0, 1, 63, 64, 481, 2, 5000, 481, 1, 481, 0, 64, 63, 481, 3]
    a = dict(scenario(1, 3, len(ns), 1, ns, self_id=[0] * len(ns)), thrifty=thrifty)
    w_out, _, per = check_enc(mk_engine(3, MIN), a)
    if thrifty:
        assert len(w_out) > 10 * WINDOW and max(len(f) for f in per[2]) == 13 + 2 + 17 * 5000
    else:
        assert len(w_out) == 2 * 17 * len(ns)


def test_enc_many_small_frames_and_skipped_slots(mk_engine):
    """3000 sends over 300 groups led by differing replicas: windows hold several hundred frames,
    item chunks hold frames, skipped slots and non-destinations, and a destination that receives
    nothing is a run of empty items between two others"""
    rng = np.random.default_rng(6)
    G, ipg = 300, 10
    flags = [R.CS_SEND] * 3000
    for i in list(range(0, 300)) + list(range(1400, 1700)) + list(range(2990, 3000)):
        flags[i] = 0
    a = scenario(6, 5, G, ipg, rng.integers(0, 3, 3000).tolist(), flags=flags)
    e = mk_engine(5, CLASSIC)
    _, w_off, _ = check_enc(e, dict(a, thrifty=True))
    assert int(w_off[-1]) > 8 * WINDOW
    # not thrifty: the send-major path over three tiles of 1024 sends, the last one partial
    _, w_off, _ = check_enc(e, a)
    assert int(w_off[-1]) > 8 * WINDOW
    check_enc(e, dict(a, alive_mask=0b01101), decode=False)
    one = dict(a, groups=T.mk_self([2] * G))  # destination 2 receives nothing, dead 3 neither
    check_enc(e, dict(one, alive_mask=0b10111), decode=False)
    check_enc(e, dict(one, alive_mask=0b10111, thrifty=True), decode=False)
    only_skipped = dict(a, sends=a["sends"][:300])
    out, off = e.encode_commits(**only_skipped)
    assert len(out) == 0 and not off.any()
    out, off = e.encode_commits(**dict(a, sends=a["sends"][:0]))
    assert len(out) == 0 and not off.any()


def dev_batch(ar, a, op_shift=0):
    """device copies of a scenario as an MpxCommitBatch (cmd_op on a guarded, shifted buffer)"""
    op, key, val = a["cmds"]
    keep = [ar.put(a["sends"]), ar.put(a["groups"]),
            Guard(ar, len(op), np.uint8, shift=op_shift).put(op), ar.put(key), ar.put(val)]
    p = [x.ptr for x in keep]
    b = _lib.MpxCommitBatch()
    b.sends, b.n_sends, b.inst_base, b.ipg = p[0], len(a["sends"]), a["inst_base"], a["ipg"]
    b.n_groups, b.groups = len(a["groups"]), p[1]
    b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = p[2], p[3], p[4], len(op)
    b.flags = R.AB_THRIFTY if a.get("thrifty") else 0
    b.alive_mask = a.get("alive_mask", 0xFFFF)
    return b, keep


@pytest.mark.parametrize("thrifty", [False, True], ids=["all", "thrifty"])
def test_enc_dev_alignment_capacity_and_graph_replay(mk_engine, thrifty):
    """the _dev form: needs its reserve; misaligned cmd_op and out at every 16-byte phase class;
    out_cap exact and short (dest_off complete, guard bytes untouched); a captured graph replayed
    twice"""
    e = mk_engine(3, CLASSIC)
    ns = [70, 3, 0, 500, 9, 1, 481, 0, 2] * (1 if thrifty else 130)  # (not thrifty: two tiles)
    a = dict(scenario(7, 3, len(ns), 2, ns), thrifty=thrifty)
    w_out, w_off = T.encode_commits(3, **a)
    total = len(w_out)
    assert total > 2 * WINDOW
    with Arena(e) as ar:
        b, keep = dev_batch(ar, a, op_shift=3)
        g_off = Guard(ar, 4, np.uint64)
        g_out = Guard(ar, total, np.uint8)
        with pytest.raises(MpxError, match="mpx_encode_commits_reserve"):
            e.encode_commits_dev(b, g_out.ptr, total, g_off.ptr)
        e.encode_commits_reserve(len(ns))
        for shift in (0, 1, 7, 15, 16, 33):
            g = Guard(ar, total, np.uint8, shift=shift)
            e.encode_commits_dev(b, g.ptr, total, g_off.ptr)
            e.synchronize()
            assert g.assert_margins().tobytes() == w_out.tobytes(), shift
            assert np.array_equal(g_off.assert_margins(), w_off)
        for short in (1, 15, 16, 17, WINDOW + 5, total - 1, total):
            g = Guard(ar, total - short, np.uint8, shift=5)
            g_off.fill()
            e.encode_commits_dev(b, g.ptr, total - short, g_off.ptr)
            e.synchronize()
            assert g.assert_margins().tobytes() == w_out[:total - short].tobytes(), short
            assert np.array_equal(g_off.assert_margins(), w_off)
        s = e.stream_create()
        e.graph_begin(s)
        e.encode_commits_dev(b, g_out.ptr, total, g_off.ptr, s)
        gr = e.graph_end(s)
        try:
            for _ in range(2):
                g_out.fill(s)
                g_off.fill(s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                assert g_out.assert_margins().tobytes() == w_out.tobytes()
                assert np.array_equal(g_off.assert_margins(), w_off)
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()
        del keep
    with pytest.raises(MpxError) as ei:  # the host form names a buffer one byte short
        e.encode_commits(out_cap=total - 1, **a)
    assert ei.value.code == R.E_INVAL
    out, off = e.encode_commits(out_cap=total, **a)  # ... and takes one exactly met
    assert out.tobytes() == w_out.tobytes() and np.array_equal(off, w_off)


def test_enc_errors(mk_engine):
    e = mk_engine(3, MIN)
    a = scenario(8, 3, 3, 2, [2, 1, 4, 0])
    for field, value in (("instance", 50 + 6), ("instance", 49), ("first_cmd", 7), ("n_cmds", 6)):
        bad = dict(a, sends=a["sends"].copy())
        bad["sends"][field][1] = value
        with pytest.raises(MpxError) as ei:
            e.encode_commits(**bad)
        assert ei.value.code == R.E_INVAL, (field, value)
        with Arena(e) as ar:  # the _dev form reports it through the error word, no frame for it
            b, keep = dev_batch(ar, bad)
            e.encode_commits_reserve(4)
            g_out, g_off = Guard(ar, 4096, np.uint8), Guard(ar, 4, np.uint64)
            e.encode_commits_dev(b, g_out.ptr, 4096, g_off.ptr)
            with pytest.raises(MpxError) as ei:
                e.synchronize()
            assert ei.value.code == R.E_INVAL
            ok = dict(a, sends=a["sends"].copy())
            ok["sends"]["flags"][1] = 0
            w_out, w_off = T.encode_commits(3, **ok)
            assert np.array_equal(g_off.assert_margins(), w_off)
            assert g_out.assert_margins()[:len(w_out)].tobytes() == w_out.tobytes()
            del keep
    bad = dict(a, groups=T.mk_self([0, 3, 1]))
    with pytest.raises(MpxError) as ei:
        e.encode_commits(**bad)
    assert ei.value.code == R.E_INVAL
    check_enc(e, a)  # the engine is usable afterwards


@pytest.mark.parametrize("seed", T.FUZZ_SEEDS)
def test_enc_fuzz(mk_engine, seed):
    N = (3, 5)[seed & 1]
    check_enc(mk_engine(N, MODES[(seed >> 1) & 1]), T.fuzz_bcast(seed, N), decode=seed < 8)


# ---- gather_commit_shorts --------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [0, 1, 300, 9000])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_gather(mk_engine, mode, n_frames):
    """CommitShorts among other frames at every byte phase of the two enclosing vectors; the host
    form, the _dev form on guarded buffers with a short capacity, and a device frame count"""
    e = mk_engine(5, mode)
    buf, ns = T.mixed_stream(n_frames, mode, n_frames)
    buf = buf + b"\x0b" + b"\x01" * 16 if n_frames else buf  # a CommitShort ending the buffer
    ns += 1 if n_frames else 0
    oth = e.decode_stream(buf)[3] if buf else np.zeros(0, R.PEER_FRAME)
    want = T.gather_commit_shorts(buf, oth)
    assert len(want[0]) == ns
    if n_frames >= 9000:  # every byte phase of the two enclosing vectors
        assert len(set(int(o) & 15 for o in oth["offset"][oth["code"] == 11])) == 16
    got = e.gather_commit_shorts(buf, oth)
    same_arrays(("msgs", "count", "frame_index"), got[:3], want)
    assert got[3] == ns
    got = e.gather_commit_shorts(buf, oth, cap=ns // 2)  # n_shorts stays complete
    same_arrays(("msgs", "count", "frame_index"), got[:3], [x[:ns // 2] for x in want])
    assert got[3] == ns
    with Arena(e) as ar:
        e.encode_commits_reserve(0, len(oth))
        d_buf = Guard(ar, len(buf), np.uint8).put(np.frombuffer(buf, np.uint8))
        d_oth = ar.put(oth) if len(oth) else ar.empty(1, R.PEER_FRAME)
        for cap, k in ((ns, None), (ns + 3, None), (max(ns - 2, 0), None), (ns, len(oth) // 2)):
            g_m, g_c = Guard(ar, cap, R.ACCEPT_MSG), Guard(ar, cap, np.int32)
            g_i, g_n = Guard(ar, cap, np.uint32), Guard(ar, 1, np.uint64)
            d_k = ar.put(np.array([k], np.uint64)) if k is not None else None
            e.gather_commit_shorts_dev(d_buf.ptr, len(buf), d_oth.ptr, len(oth),
                                       d_k.ptr if d_k else None, g_m.ptr, g_c.ptr, g_i.ptr, cap,
                                       g_n.ptr)
            e.synchronize()
            w = want if k is None else T.gather_commit_shorts(buf, oth[:k])
            m = len(w[0])
            assert int(g_n.assert_margins()[0]) == m
            fill = min(m, cap)
            same_arrays(("msgs", "count", "frame_index"),
                        [g_m.assert_margins()[:fill], g_c.assert_margins()[:fill],
                         g_i.assert_margins()[:fill]], [x[:fill] for x in w])
            for g in (g_m, g_c, g_i):
                g.assert_untouched([(fill, cap)])
        d_buf.assert_margins()


def test_gather_errors(mk_engine):
    e = mk_engine(5, MIN)
    buf = b"\x0b" + bytes(range(16)) + b"\x0b" + bytes(range(16))
    oth = np.zeros(2, R.PEER_FRAME)
    oth["offset"], oth["code"] = [0, 17], 11
    assert e.gather_commit_shorts(buf, oth)[3] == 2
    with pytest.raises(MpxError) as ei:
        e.gather_commit_shorts(buf[:-1], oth)
    assert ei.value.code == R.E_INVAL
    with Arena(e) as ar:  # the _dev form skips the frame and raises the error word
        e.encode_commits_reserve(0, 2)
        d_buf = ar.put(np.frombuffer(buf, np.uint8))
        g_m, g_c = Guard(ar, 2, R.ACCEPT_MSG), Guard(ar, 2, np.int32)
        g_i, g_n = Guard(ar, 2, np.uint32), Guard(ar, 1, np.uint64)
        with pytest.raises(MpxError) as ei:  # the stream's alignment
            e.gather_commit_shorts_dev(d_buf.ptr + 1, 33, ar.put(oth).ptr, 2, None, g_m.ptr,
                                       g_c.ptr, g_i.ptr, 2, g_n.ptr)
        assert ei.value.code == R.E_INVAL
        e.gather_commit_shorts_dev(d_buf.ptr, 33, ar.put(oth).ptr, 2, None, g_m.ptr, g_c.ptr,
                                   g_i.ptr, 2, g_n.ptr)
        with pytest.raises(MpxError) as ei:
            e.synchronize()
        assert ei.value.code == R.E_INVAL
        g_m.assert_margins()
        g_m.assert_untouched([(1, 2)])
    assert e.gather_commit_shorts(buf, oth)[3] == 2  # the engine is usable afterwards


# ---- the leader's decisions to the followers' watermarks -------------------------------------------
def test_classic_commit_loop(mk_engine):
    """CLASSIC, N = 5: the tally's decided mask -> mpx_encode_commits_dev -> every follower's run
    through decode_stream, unmarshal_frames and the gather, merged and stably sorted by instance
    -> mpx_commit_handle_dev. The followers' committed_upto equals the transliteration's."""
    N, ipg, base, D = 5, 48, 300, 33
    e = mk_engine(N, CLASSIC)
    rng = np.random.default_rng(5)
    # replies: two OKs decide an instance (the leader's own vote makes three of five)
    decide = sorted(set(rng.choice(ipg, 30, replace=False).tolist() + [0, 1, 2]))
    rows = []
    for k in range(ipg):
        for _ in range(2 if k in decide else int(rng.integers(0, 2))):
            rows.append((base + k, D, -1, 1, (0, 0, 0)))
    recs = np.array(rows, R.ACCEPT_REPLY)
    lb = np.zeros(ipg, R.INST_STATE)
    lb["status"] = R.PREPARED
    g_st, g_cu, _, dec = e.accept_tally(recs, lb, base, base - 1)
    w_st, w_cu, _, w_dec = GoBackend(N, CLASSIC).accept_tally(recs, lb, base, base - 1,
                                                             np.zeros(N, np.int32))
    assert np.array_equal(dec, w_dec) and g_cu == w_cu
    assert np.flatnonzero(dec).tolist() == decide and w_cu >= base + 2
    # the leader's bcastCommit, thrifty: two followers get CommitShorts, two get Commits
    n_cmds = rng.integers(0, 4, ipg)
    first = np.concatenate([[0], np.cumsum(n_cmds)[:-1]])
    sends = T.mk_commit_sends([(base + k, D, int(first[k]), int(n_cmds[k]),
                                R.CS_SEND if dec[k] else 0) for k in range(ipg)])
    a = dict(sends=sends, groups=T.mk_self([0]), cmds=mk_cmds(rng, int(n_cmds.sum())),
             inst_base=base, ipg=ipg, thrifty=True)
    w_out, w_off, per = T.encode_commits(N, **a, want_frames=True)
    with Arena(e) as ar:
        b, keep = dev_batch(ar, a)
        e.encode_commits_reserve(ipg)
        g_out, g_off = Guard(ar, len(w_out), np.uint8, shift=9), Guard(ar, N + 1, np.uint64)
        e.encode_commits_dev(b, g_out.ptr, len(w_out), g_off.ptr)
        e.synchronize()
        out, off = g_out.assert_margins(), g_off.assert_margins()
        assert out.tobytes() == w_out.tobytes() and np.array_equal(off, w_off)
        kinds = set()
        for q in range(1, N):
            run = out[int(off[q]):int(off[q + 1])].tobytes()
            _, _, var, oth, res = e.decode_stream(run)
            assert int(res["stop_reason"]) == R.DECODE_END
            arrs = commits_of(e, run, var)
            shorts, cnt, idx, ns = e.gather_commit_shorts(run, oth)
            kinds.add((len(arrs["commits"]) > 0, ns > 0))
            # the shim's merge: by stream offset, then a stable sort by instance
            offs = np.concatenate([var["offset"][var["code"] == R.PEER_COMMIT],
                                   oth["offset"][idx]])
            msgs = np.concatenate([arrs["commits"], shorts])[np.argsort(offs, kind="stable")]
            msgs = msgs[np.argsort(msgs["instance"], kind="stable")]
            assert msgs["instance"].tolist() == [base + k for k in decide]
            # a follower that accepted some of the instances and knows nothing of the others
            fst = nil_state(ipg)
            acc = rng.random(ipg) < 0.6
            fst["status"][acc] = R.ACCEPTED
            fst["ballot"][acc] = D
            fst["value_id"][acc] = 7
            cu = np.array([base - 1], np.int32)
            want = T.commit_handle(msgs, fst, cu, base, ipg)
            same_arrays(CH_NAMES, ch_dev(e, ar, msgs, fst, cu, base, ipg), want)
            assert int(want[1][0]) == w_cu  # the follower's watermark is the leader's
        assert kinds == {(True, False), (False, True)}
        del keep

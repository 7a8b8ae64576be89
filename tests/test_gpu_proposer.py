"""GPU tests of the proposer side: mpx_propose_handle (batched handlePropose) and
mpx_encode_accepts (the Accept frames bcastAccept writes per peer connection), host and device
forms, MIN and CLASSIC, bit- and byte-exact against tests/proposer_translit.py. Shapes are the
smallest that reach each path: the handler runs a lane per group in workgroups of 256, a slot
holds at most 5000 proposals, the encoder's output window is 8192 bytes and its item chunk 256."""
import struct

import numpy as np
import pytest

import proposer_translit as P
from devguard import Guard
from go_translit import GoBackend, GoPanic
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError

pytestmark = pytest.mark.gpu
N = 5
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
MODES = [MIN, CLASSIC]
MODE_IDS = ["min", "classic"]
WINDOW = 8192
HAS = R.PF_HAS_PROPOSALS


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


PH_NAMES = ("groups", "st", "lb", "sends", "send_off")


# ---- propose_handle --------------------------------------------------------------------------------
def ph_dev(e, ar, groups, prop_off, st, base, ipg, lb, stream=None, want_call=False):
    """the _dev form in place on guarded buffers; returns what the host form returns"""
    G = len(groups)
    n = np.diff(np.asarray(prop_off, np.int64))
    send_off = np.zeros(G + 1, np.uint64)
    send_off[1:] = np.cumsum(-(-n // R.PROPOSE_MAX_BATCH))
    ns = int(send_off[-1])
    g_grp = Guard(ar, G, R.PROPOSER_GROUP).put(groups)
    g_st = Guard(ar, len(st), R.ACCEPTOR_STATE).put(st)
    g_lb = Guard(ar, len(st), R.INST_STATE).put(lb) if lb is not None else None
    g_snd = Guard(ar, ns, R.ACCEPT_SEND)
    d_poff, d_soff = ar.put(np.asarray(prop_off, np.uint64)), ar.put(send_off)

    def call(s=None):
        e.propose_handle_dev(g_grp.ptr, G, d_poff.ptr, d_soff.ptr, g_st.ptr,
                             g_lb.ptr if g_lb else None, len(st), base, ipg, g_snd.ptr, s)

    def results():
        return (g_grp.assert_margins(), g_st.assert_margins(),
                g_lb.assert_margins() if g_lb else None, g_snd.assert_margins(), send_off)
    if want_call:
        return call, results, (g_grp, g_st, g_lb, g_snd)
    call(stream)
    e.stream_synchronize(stream)
    e.synchronize()
    return results()


def check_ph(e, mode, groups, prop_off, st, base, ipg, with_lb=True, n=N):
    lb = np.zeros(len(st), R.INST_STATE) if with_lb else None
    if lb is not None:
        lb["nacks"] = 7  # what an uninstalled instance keeps
    want = P.propose_handle(mode, n, groups, prop_off, st, base, ipg, lb)[:5]
    got = e.propose_handle(groups, np.asarray(prop_off, np.uint64), st, base, ipg, lb)
    same_arrays(PH_NAMES, got, want)
    with Arena(e) as ar:
        same_arrays(PH_NAMES, ph_dev(e, ar, groups, prop_off, st, base, ipg, lb), want)
    return want


USED = (R.COMMITTED, 17, 7, 0)
NILROW = (P.NIL, 0, 0, 0)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ph_known_answers(mk_engine, mode):
    """the hand-traced answers of test_proposer_translit.py, through the engine"""
    e = mk_engine(N, mode)

    def run(grp, n_props, rows):
        st = P.mk_state(rows)
        w = check_ph(e, mode, P.mk_groups([grp]), [0, n_props], st, 100, len(st))
        return [tuple(int(x) for x in r)[:6] for r in w[3].tolist()], w
    if mode == MIN:
        assert run((17, 1, 2, 5, 100, 99), 3, [NILROW] * 4)[0] == [(-1, 0, 0, R.PH_NOT_LEADER, 0, 3)]
        assert run((17, 1, 1, 2, 100, 99), 2, [NILROW] * 4)[0] == [(-1, 0, 0, R.PH_NOT_LEADER, 0, 2)]
        s, w = run((17, 1, 1, 3, 100, 102), 2, [USED] * 3 + [NILROW] * 2)
        assert s == [(103, 17, 102, R.PH_ACCEPT, 0, 2)] and w[0]["crt_instance"][0] == 104
        assert w[1].tolist()[3] == (R.PREPARED, 17, 0, HAS) and w[2].tolist()[3] == (R.PREPARED, 0, 0, 0)
        s, w = run((17, 1, 1, 3, 100, 100), 4, [USED] * 3 + [NILROW] * 2)
        assert s == [(103, 17, 100, R.PH_REFUSED, 0, 4)] and w[0]["crt_instance"][0] == 103
        s, w = run((17, 1, 1, 3, 100, 99), 5001, [NILROW] * 4)
        assert s == [(100, 17, 99, R.PH_ACCEPT, 0, 5000), (101, 17, 99, R.PH_REFUSED, 5000, 1)]
    else:
        s, w = run((17, 1, 1, 0, 100, 99), 10001, [NILROW] * 4)
        assert s == [(100, 17, 99, R.PH_ACCEPT, 0, 5000), (101, 17, 99, R.PH_ACCEPT, 5000, 5000),
                     (102, 17, 99, R.PH_ACCEPT, 10000, 1)] and w[0]["crt_instance"][0] == 103
        s, w = run((-1, 3, 3, 0, 100, 99), 2, [NILROW] * 2)
        assert s == [(100, 3, 99, R.PH_PREPARE, 0, 2)]
        assert w[1].tolist()[0] == (R.PREPARING, 3, 0, HAS) and w[2].tolist()[0] == (R.PREPARING, 0, 0, 0)
        assert run((17, 1, 0, 0, 100, 99), 2, [NILROW] * 2)[0] == [(-1, 0, 0, R.PH_NOT_LEADER, 0, 2)]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ph_no_groups_and_no_proposals(mk_engine, mode):
    e = mk_engine(N, mode)
    got = e.propose_handle(np.zeros(0, R.PROPOSER_GROUP), np.zeros(1, np.uint64),
                           np.zeros(0, R.ACCEPTOR_STATE), 0, 4)
    assert len(got[0]) == len(got[1]) == len(got[3]) == 0 and list(got[4]) == [0]
    e.propose_handle_dev(None, 0, None, None, None, None, 0, 0, 4, None)  # launches nothing
    e.synchronize()
    # groups without proposals: nothing changes, crt_instance included (it is not advanced)
    groups = P.mk_groups([(17, 1, 1, 3, 10, 10), (17, 1, 1, 3, 14, 13), (17, 1, 1, 3, 18, 17)])
    st = P.mk_state([USED] * 5 + [NILROW] * 3 + [USED] * 4)
    want = check_ph(e, mode, groups, [0, 0, 2, 2], st, 10, 4)
    assert want[0]["crt_instance"][[0, 2]].tolist() == [10, 18] and len(want[3]) == 1


@pytest.mark.parametrize("G", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ph_group_counts(mk_engine, mode, G):
    """wave and workgroup edges of the lane-per-group launch; every fifth group not the leader"""
    rng = np.random.default_rng(G)
    ipg, base = 4, -7
    rows = [(16 + 16 * (g % 3) + g % N, g % N, (g + (g % 5 == 4)) % N, 3, base + g * ipg + 1,
             base + g * ipg) for g in range(G)]
    st = P.nil_state(G * ipg)
    st[::ipg] = USED
    prop_off = np.zeros(G + 1, np.uint64)
    prop_off[1:] = np.cumsum(rng.integers(0, 4, G))
    check_ph(mk_engine(N, mode), mode, P.mk_groups(rows), prop_off, st, base, ipg)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ph_batch_counts_and_advances(mk_engine, mode):
    """per-group proposal counts around MAX_BATCH, and crt advancing over 0, 1 and 300 slots"""
    counts = [1, 4999, 5000, 5001, 10001, 3, 3, 3]
    adv = [0, 0, 0, 0, 0, 0, 1, 300]
    ipg, base = 304, 1000
    G = len(counts)
    st = P.nil_state(G * ipg)
    rows = []
    for g in range(G):
        st[g * ipg:g * ipg + adv[g]] = USED
        rows.append((33, 1, 1, 4, base + g * ipg, base + g * ipg + adv[g] - 1))
    prop_off = np.zeros(G + 1, np.uint64)
    prop_off[1:] = np.cumsum(counts)
    want = check_ph(mk_engine(N, mode), mode, P.mk_groups(rows), prop_off, st, base, ipg,
                    with_lb=False)
    assert list(want[4]) == [0, 1, 2, 3, 5, 8, 9, 10, 11]
    assert want[0]["crt_instance"][7] == base + 7 * ipg + 301


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ph_window_overflow(mk_engine, mode):
    e = mk_engine(N, mode)
    groups = P.mk_groups([(17, 1, 1, 3, 100, 101), (17, 1, 1, 3, 102, 103)])
    st = P.mk_state([NILROW] * 2 + [USED] * 2)  # group 1 advances out of its window
    with pytest.raises(GoPanic):
        P.propose_handle(mode, N, groups, [0, 1, 2], st, 100, 2)
    with pytest.raises(MpxError) as ei:
        e.propose_handle(groups, np.array([0, 1, 2], np.uint64), st, 100, 2)
    assert ei.value.code == R.E_NIL_INSTANCE
    with Arena(e) as ar, pytest.raises(MpxError) as ei:
        ph_dev(e, ar, groups, [0, 1, 2], st, 100, 2, None)
    assert ei.value.code == R.E_NIL_INSTANCE
    groups["crt_instance"][1] = 104  # already outside: the host form sees it before any launch
    with pytest.raises(MpxError) as ei:
        e.propose_handle(groups, np.array([0, 1, 2], np.uint64), st, 100, 2)
    assert ei.value.code == R.E_NIL_INSTANCE
    with pytest.raises(MpxError) as ei:  # n_inst != n_groups * ipg
        e.propose_handle(groups, np.array([0, 1, 2], np.uint64), st, 100, 3)
    assert ei.value.code == R.E_INVAL
    # the engine is usable afterwards
    check_ph(e, mode, P.mk_groups([(17, 1, 1, 3, 100, 99)]), [0, 2], P.nil_state(2), 100, 2)


@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ph_fuzz(mk_engine, mode, seed):
    groups, prop_off, st, base, ipg = P.fuzz_propose(seed, N, mode)
    check_ph(mk_engine(N, mode), mode, groups, prop_off, st, base, ipg, with_lb=bool(seed & 1))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ph_graph_replay(mk_engine, mode):
    """the _dev call captured into a graph and replayed three times on fresh copies"""
    e = mk_engine(N, mode)
    groups, prop_off, st, base, ipg = P.fuzz_propose(5, N, mode)
    lb = np.zeros(len(st), R.INST_STATE)
    want = P.propose_handle(mode, N, groups, prop_off, st, base, ipg, lb)[:5]
    with Arena(e) as ar:
        call, results, (g_grp, g_st, g_lb, g_snd) = ph_dev(e, ar, groups, prop_off, st, base, ipg,
                                                          lb, want_call=True)
        fresh = [ar.put(groups), ar.put(st), ar.put(lb)]
        s = e.stream_create()
        e.graph_begin(s)
        call(s)
        g = e.graph_end(s)
        try:
            for _ in range(3):
                for dst, src in zip((g_grp, g_st, g_lb), fresh):
                    e.memcpy(dst.ptr, src.ptr, src.nbytes, D2D, s)
                g_snd.fill(s)
                e.graph_launch(g, s)
                e.stream_synchronize(s)
                same_arrays(PH_NAMES, results(), want)
        finally:
            e.graph_destroy(g)
            e.stream_destroy(s)
        e.synchronize()


# ---- encode_accepts --------------------------------------------------------------------------------
def scenario(seed, mode, n, G, ipg, n_cmds, used, self_id=None, pc=None, flags=None, base=50):
    """one send per group: group g has used[g] logged instances (a list of command counts), its
    next instance carries n_cmds[g] new commands; pc(g, q, first, lc) gives peerCommits"""
    rng = np.random.default_rng(seed)
    rows, sends, counts = [], [], []
    c0 = 0
    pcs = np.zeros((G, n), np.int32)
    for g in range(G):
        first = base + g * ipg
        u = used[g]
        inst, lc = first + len(u), first + len(u) - 1
        sid = (g % n) if self_id is None else self_id[g]
        rows.append((16 * (1 + g % 7) + sid, sid, sid, n, inst + 1, lc))
        f = R.PH_ACCEPT if flags is None else flags[g]
        sends.append((inst, rows[-1][0], lc, f, c0, n_cmds[g]))
        c0 += n_cmds[g]
        counts += list(u) + [None] * (ipg - len(u))
        for q in range(n):
            pcs[g, q] = int(rng.integers(first - 2, lc + 2)) if pc is None else pc(g, q, first, lc)
    return dict(sends=P.mk_sends(sends), groups=P.mk_groups(rows), cmds=P.mk_cmds(rng, c0),
                inst_base=base, ipg=ipg, peer_commits=pcs, log=P.mk_log(rng, counts))


def uvarint(b, pos):
    u, k = 0, 0
    while True:
        x = b[pos + k]
        u |= (x & 0x7F) << (7 * k)
        k += 1
        if x < 0x80:
            return u >> 1, k


def check_decode(e, mode, frames, run):
    """a destination's run through the stream decoder: END, and one mpx_var_frame per Accept"""
    if len(run) == 0:
        assert not frames
        return
    ar, pr, var, oth, res = e.decode_stream(run.tobytes())
    assert int(res["stop_reason"]) == R.DECODE_END and len(ar) == len(pr) == len(oth) == 0
    assert len(var) == len(frames)
    off = 0
    for v, f in zip(var, frames):
        pos = 17 if mode == MIN else 13
        nc, k = uvarint(f, pos)
        cmds_off = pos + k
        end = cmds_off + 17 * nc
        m, k2 = uvarint(f, end) if mode == MIN else (0, 0)
        assert (int(v["offset"]), int(v["length"]), int(v["code"]), int(v["n_cmds"]),
                int(v["cmds_off"]), int(v["n_log"]), int(v["log_off"])) == \
            (off, len(f), R.PEER_ACCEPT, nc, off + cmds_off, m, off + end + k2)
        off += len(f)


def check_enc(e, mode, n, a, decode=True, **kw):
    w_out, w_off, per = P.encode_accepts(mode, n, want_frames=True, **a, **kw)
    out, off = e.encode_accepts(**a, **kw)
    assert np.array_equal(off, w_off), (off, w_off)
    if out.tobytes() != w_out.tobytes():
        bad = np.flatnonzero(out != w_out)
        raise AssertionError(f"{len(bad)} bytes differ, first at {bad[:8]} of {len(out)}")
    if decode:
        for q in range(n):
            check_decode(e, mode, per[q], out[int(off[q]):int(off[q + 1])])
    return w_out, w_off, per


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_enc_varint_steps_and_long_frames(mk_engine, mode):
    """n_cmds at every varint length step; 5000 commands are 85 KB, 8192 are 139 KB: frames that
    span more than two output windows"""
    ns = [0, 1, 63, 64, 5000, 8191, 8192]
    a = scenario(1, mode, 3, len(ns), 4, ns, [[2], [0], [1, 1], [], [3], [0, 0], [1]])
    w_out, _, per = check_enc(mk_engine(3, mode), mode, 3, a)
    assert max(len(f) for q in per for f in q) > 2 * WINDOW + 100000


@pytest.mark.parametrize("thrifty", [False, True], ids=["all", "thrifty"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_enc_replica_counts(mk_engine, mode, n, thrifty):
    rng = np.random.default_rng(n)
    G = 24
    a = scenario(10 + n, mode, n, G, 6, rng.integers(0, 5, G).tolist(),
                 [rng.integers(0, 4, int(k)).tolist() for k in rng.integers(0, 5, G)])
    e = mk_engine(n, mode)
    check_enc(e, mode, n, a, thrifty=thrifty)
    check_enc(e, mode, n, a, thrifty=thrifty, alive_mask=int(rng.integers(0, 1 << n)))
    check_enc(e, mode, n, a, thrifty=thrifty, alive_mask=0)


def test_enc_catch_up_counts(mk_engine):
    """catch-up logs of 0, 1, 63 and 64 instances, instances without commands among them"""
    want_m = [0, 1, 63, 64]
    used = [[0, 2, 0, 1] * 16 for _ in want_m]
    a = scenario(3, MIN, 3, 4, 72, [1, 2, 0, 3], used,
                 pc=lambda g, q, first, lc: lc - want_m[g] if q != 1 else first - 1)
    _, _, per = check_enc(mk_engine(3, MIN), MIN, 3, a)
    ms = sorted(uvarint(f, 17 + 1 + 17 * uvarint(f, 17)[0])[0] for q in per for f in q)
    assert set(want_m) <= set(ms) and ms[-1] == 64


def split(total, fixed):
    """command counts (each < 64) of frames of fixed + 17 n bytes that add up to `total`"""
    k = next(k for k in range(1, 200) if (total - fixed * k) % 17 == 0 and
             0 <= (total - fixed * k) // 17 <= 63 * k)
    c = (total - fixed * k) // 17
    return [c // k + (1 if i < c % k else 0) for i in range(k)]


@pytest.mark.parametrize("end", [WINDOW - 1, WINDOW, WINDOW + 1])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_enc_frames_ending_around_a_window_boundary(mk_engine, mode, end):
    fixed = 19 if mode == MIN else 14  # no catch-up log: peers are up to date
    ns = split(end, fixed) + [3, 0, 2]
    G = len(ns)
    a = scenario(4, mode, 2, G, 2, ns, [[1]] * G, self_id=[0] * G,
                 pc=lambda g, q, first, lc: lc)
    w_out, w_off, per = check_enc(mk_engine(2, mode), mode, 2, a)
    ends = np.cumsum([len(f) for f in per[1]])
    assert end in ends and len(w_out) > WINDOW + 1


@pytest.mark.parametrize("d", P.SWEEP)
def test_enc_record_header_and_command_at_every_byte_around_the_window_boundary(mk_engine, d):
    """the dense MIN encoder on one frame whose catch-up record header starts at byte 8192 + d, the
    log in log_recs / log_cmd_off / log_op..: test_gpu_accepts_stored.py's sweep (P.boundary_case;
    test_proposer_translit.py checks where its inputs put the headers and the commands)"""
    a, k = P.boundary_case(d)
    _, _, per = check_enc(mk_engine(2, MIN), MIN, 2, a, decode=d % 8 == 0)
    frame, T = per[1][0], WINDOW + d
    lrec, lcoff, lop, lkey, lval = a["log"]
    c = int(lcoff[k])
    head = np.array([lrec["ballot"][k], lrec["status"][k]], "<i4").tobytes() + b"\x06"
    assert frame[T:T + 9] == head and len(frame) == T + 9 + 51 + 9 + 34
    assert frame[T + 9:T + 26] == P.command_marshal(int(lop[c]), int(lkey[c]), int(lval[c]))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_enc_300_groups_many_frames_per_window(mk_engine, mode):
    """300 groups led by differing replicas; small frames, so a window holds over 100 of them and
    an item chunk of 256 holds frames, skipped slots and non-destinations"""
    rng = np.random.default_rng(6)
    G = 300
    flags = [R.PH_ACCEPT] * G
    for g in list(range(0, 5)) + list(range(140, 150)) + list(range(295, 300)):
        flags[g] = [R.PH_NOT_LEADER, R.PH_REFUSED, R.PH_PREPARE, 0][g % 4]  # start, middle, end
    a = scenario(6, mode, N, G, 4, rng.integers(0, 2, G).tolist(),
                 [[int(x) for x in rng.integers(0, 2, int(k))] for k in rng.integers(0, 3, G)],
                 flags=flags)
    _, w_off, per = check_enc(mk_engine(N, mode), mode, N, a)
    assert int(w_off[-1]) > WINDOW
    assert int(w_off[-1]) / sum(len(q) for q in per) < WINDOW / 100
    only_skipped = dict(a, sends=a["sends"][:5])
    out, off = mk_engine(N, mode).encode_accepts(**only_skipped)
    assert len(out) == 0 and not off.any()


def dev_batch(ar, a, n, op_shift=0, thrifty=False, alive_mask=0xFFFF):
    """device copies of a scenario as an MpxAcceptBatch (cmd_op on a guarded, shifted buffer)"""
    op, key, val = a["cmds"]
    lrec, lcoff, lop, lkey, lval = a["log"]
    keep = [ar.put(a["sends"]), ar.put(a["groups"]), ar.put(a["peer_commits"]),
            Guard(ar, len(op), np.uint8, shift=op_shift).put(op), ar.put(key), ar.put(val),
            ar.put(lrec), ar.put(lcoff), Guard(ar, len(lop), np.uint8, shift=op_shift).put(lop),
            ar.put(lkey), ar.put(lval)]
    p = [x.ptr for x in keep]
    b = _lib.MpxAcceptBatch()
    b.sends, b.n_sends, b.inst_base, b.ipg = p[0], len(a["sends"]), a["inst_base"], a["ipg"]
    b.n_groups, b.groups, b.peer_commits = len(a["groups"]), p[1], p[2]
    b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = p[3], p[4], p[5], len(op)
    b.log_recs, b.log_cmd_off, b.log_op, b.log_key, b.log_val = p[6], p[7], p[8], p[9], p[10]
    b.n_log_cmds = len(lop)
    b.flags, b.alive_mask = (R.AB_THRIFTY if thrifty else 0), alive_mask
    return b, keep


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_enc_dev_alignment_capacity_and_graph_replay(mk_engine, mode):
    """the _dev form: needs its reserve; misaligned cmd_op and out; out_cap exact and one byte
    short (dest_off complete, guard bytes untouched); a captured graph replayed three times"""
    e = mk_engine(3, mode)
    ns = [70, 3, 0, 500, 9, 1]
    a = scenario(7, mode, 3, len(ns), 8, ns, [[1, 0, 2]] * len(ns))
    w_out, w_off = P.encode_accepts(mode, 3, **a)
    total = len(w_out)
    assert total > 2 * WINDOW
    with Arena(e) as ar:
        b, keep = dev_batch(ar, a, 3, op_shift=3)
        g_off = Guard(ar, 4, np.uint64)
        g_out = Guard(ar, total, np.uint8)
        with pytest.raises(MpxError, match="mpx_encode_accepts_reserve"):
            e.encode_accepts_dev(b, g_out.ptr, total, g_off.ptr)
        e.encode_accepts_reserve(len(ns), len(ns) * 8, len(a["log"][2]))
        for shift in (0, 1, 7, 16):
            g = Guard(ar, total, np.uint8, shift=shift)
            e.encode_accepts_dev(b, g.ptr, total, g_off.ptr)
            e.synchronize()
            assert g.assert_margins().tobytes() == w_out.tobytes(), shift
            assert np.array_equal(g_off.assert_margins(), w_off)
        for short in (1, WINDOW + 5, total):
            g = Guard(ar, total - short, np.uint8, shift=5)
            g_off.fill()
            e.encode_accepts_dev(b, g.ptr, total - short, g_off.ptr)
            e.synchronize()
            assert g.assert_margins().tobytes() == w_out[:total - short].tobytes(), short
            assert np.array_equal(g_off.assert_margins(), w_off)
        s = e.stream_create()
        e.graph_begin(s)
        e.encode_accepts_dev(b, g_out.ptr, total, g_off.ptr, s)
        gr = e.graph_end(s)
        try:
            for _ in range(3):
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
    with pytest.raises(MpxError) as ei:  # the host form names a short buffer
        e.encode_accepts(out_cap=total - 1, **a)
    assert ei.value.code == R.E_INVAL
    out, off = e.encode_accepts(out_cap=total, **a)
    assert out.tobytes() == w_out.tobytes()


def test_enc_errors(mk_engine):
    e = mk_engine(3, MIN)
    a = scenario(8, MIN, 3, 3, 6, [2, 1, 4], [[1, 2, 0]] * 3, pc=lambda g, q, first, lc: first)
    a["log"][0]["status"][6 + 2] = P.NIL  # group 1's instance first + 2 is in every peer's range
    with pytest.raises(GoPanic) as gp:
        P.encode_accepts(MIN, 3, **a)
    assert gp.value.code == R.E_NIL_INSTANCE
    with pytest.raises(MpxError) as ei:
        e.encode_accepts(**a)
    assert ei.value.code == R.E_NIL_INSTANCE
    with Arena(e) as ar:  # the _dev form reports it through the error word
        b, keep = dev_batch(ar, a, 3)
        e.encode_accepts_reserve(3, 18, 16)
        g_out, g_off = Guard(ar, 4096, np.uint8), Guard(ar, 4, np.uint64)
        e.encode_accepts_dev(b, g_out.ptr, 4096, g_off.ptr)
        with pytest.raises(MpxError) as ei:
            e.synchronize()
        assert ei.value.code == R.E_NIL_INSTANCE
        g_out.assert_margins()
        del keep
    a["log"][0]["status"][6 + 2] = R.COMMITTED
    for field, value in (("last_committed", int(a["sends"]["instance"][1])),
                         ("last_committed", 50 + 6 - 2), ("instance", 50 + 18), ("instance", 49)):
        bad = dict(a, sends=a["sends"].copy())
        bad["sends"][field][1] = value
        with pytest.raises(MpxError) as ei:
            e.encode_accepts(**bad)
        assert ei.value.code == R.E_INVAL, (field, value)
    check_enc(e, MIN, 3, a)  # the engine is usable afterwards


@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_enc_fuzz(mk_engine, mode, seed):
    check_enc(mk_engine(N, mode), mode, N, P.fuzz_encode(seed, N, mode), decode=seed < 4)


# ---- the whole Phase-2 round trip through the engine -----------------------------------------------
def test_phase2_round_trip(mk_engine):
    """N = 5, MIN: propose_handle -> encode_accepts; four followers decode_stream -> accept_handle
    -> encode_accept_replies; the leader decode_stream -> accept_tally on the lb propose_handle
    wrote. Three rounds of one log: each round's instance comes out decided, states and scalars
    equal go_translit's tally, and the next round carries it in the catch-up logs."""
    e = mk_engine(N, MIN)
    rng = np.random.default_rng(77)
    ipg, base, D = 16, 200, 32
    grp = P.mk_groups([(D, 0, 0, 3, base, base - 1)])
    st = P.nil_state(ipg)
    lb = np.zeros(ipg, R.INST_STATE)
    fst = [P.nil_state(ipg) for _ in range(N)]
    counts = [None] * ipg
    log_cmds = [np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64)]
    cu, pcs = base - 1, np.full(N, base - 1, np.int32)
    for rnd in range(3):
        k = int(rng.integers(1, 6))
        cmds = P.mk_cmds(rng, k)
        grp["committed_upto"] = cu
        want = P.propose_handle(MIN, N, grp, [0, k], st, base, ipg, lb)
        got = e.propose_handle(grp, np.array([0, k], np.uint64), st, base, ipg, lb)
        same_arrays(PH_NAMES, got, want[:5])
        grp, st, lb, sends, _ = got
        inst = base + rnd
        assert int(sends["flags"][0]) == R.PH_ACCEPT and int(sends["instance"][0]) == inst
        lrec = np.zeros(ipg, R.LOG_REC)
        lrec["status"] = [P.NIL if c is None else R.COMMITTED for c in counts]
        lrec["ballot"] = D
        lcoff = np.zeros(ipg + 1, np.uint64)
        lcoff[1:] = np.cumsum([0 if c is None else c for c in counts])
        a = dict(sends=sends, groups=grp, cmds=cmds, inst_base=base, ipg=ipg,
                 peer_commits=pcs.reshape(1, N), log=(lrec, lcoff, *log_cmds))
        out, off, per = check_enc(e, MIN, N, a)
        to_leader = []
        for q in range(1, N):
            run = out[int(off[q]):int(off[q + 1])].tobytes()
            _, _, var, _, res = e.decode_stream(run)
            assert int(res["stop_reason"]) == R.DECODE_END and len(var) == 1
            msgs = np.zeros(len(var), R.ACCEPT_MSG)
            for i, v in enumerate(var):
                o = int(v["offset"])
                msgs[i] = struct.unpack_from("<iii", run, o + 1)[1:] + (
                    struct.unpack_from("<i", run, o + 1)[0], i)
                assert int(v["n_cmds"]) == k and int(v["n_log"]) == inst - max(int(pcs[q]) + 1, base)
            fg = np.zeros(1, R.ACCEPTOR_GROUP)
            fg[0] = (D, q)
            fst[q], rep, to, eff = e.accept_handle(msgs, fst[q], fg, base, ipg)
            assert (eff & R.AH_REPLIED).all() and (to == 0).all()
            rbytes, roff = e.encode_accept_replies(rep, to)
            assert int(roff[1]) == len(rbytes) == R.ACCEPT_REPLY_FRAME[MIN]
            to_leader.append(rbytes.tobytes())
        recs = []
        for bts in to_leader:
            ar_, _, _, _, res = e.decode_stream(bts)
            assert int(res["stop_reason"]) == R.DECODE_END
            recs.append(ar_)
        recs = np.concatenate(recs)
        recs = recs[np.argsort(recs["instance"], kind="stable")]
        g_st, g_cu, g_pc, g_dec = e.accept_tally(recs, lb, base, cu, pcs)
        w_st, w_cu, w_pc, w_dec = GoBackend(N, MIN).accept_tally(recs, lb, base, cu, pcs)
        assert g_st.tobytes() == w_st.tobytes() and np.array_equal(g_dec, w_dec)
        assert g_cu == w_cu and np.array_equal(g_pc, w_pc)
        assert g_dec[rnd] and int(g_st["status"][rnd]) == R.COMMITTED and g_cu == inst
        lb, cu = g_st, int(g_cu)
        counts[rnd] = k
        log_cmds = [np.concatenate([x, y]) for x, y in zip(log_cmds, cmds)]
        pcs = np.array([cu, cu, cu - 1, base - 1, cu], np.int32)  # 2 lags one, 3 knows nothing

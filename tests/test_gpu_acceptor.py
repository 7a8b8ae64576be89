"""GPU tests of the acceptor side: mpx_accept_handle (batched handleAccept) and
mpx_encode_accept_replies (the AcceptReply frames per leader connection), host and device forms,
MIN and CLASSIC, bit-exact against tests/acceptor_translit.py. Shapes are the smallest that reach
each path of the kernels: the tile is 1024 records, the workgroup 256 lanes."""
import numpy as np
import pytest

import acceptor_translit as A
from go_translit import GoBackend
from minpaxos_amd import records as R
from minpaxos_amd.engine import MpxError

pytestmark = pytest.mark.gpu
N = 5
MODES = [R.MODE_MIN, R.MODE_CLASSIC]
MODE_IDS = ["min", "classic"]
NAMES = ("st", "replies", "reply_to", "effect")


def assert_same(got, want):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            diff = [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()][:5]
            raise AssertionError(f"{name} differs at {diff}: got {g[diff]} want {w[diff]}")


def check(e, mode, case):
    msgs, st, groups, base, ipg = case
    want = A.accept_handle(mode, N, msgs, st, groups, base, ipg)
    got = e.accept_handle(msgs, st, groups, base, ipg)
    assert_same(got, want)


def shape_case(seed, runs, stride=1, ipg=1 << 20, base=0):
    """one message run per instance, instance k at window index k * stride"""
    rng = np.random.default_rng(seed)
    idx = np.arange(len(runs)) * stride
    n_inst = int(idx[-1]) + 1 if len(runs) else 1
    return A.case_from_runs(rng, idx, runs, n_inst, ipg, base, N)


# ---- the acceptor step ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_known_answers(mk_engine, mode):
    e = mk_engine(N, mode)
    for case in (A.KAT_MIN if mode == R.MODE_MIN else A.KAT_CLASSIC):
        msgs, st, groups, base = A.kat_inputs(case)
        assert_same(e.accept_handle(msgs, st, groups, base), A.kat_expected(mode, case))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_no_messages(mk_engine, mode):
    e = mk_engine(N, mode)
    st = A.mk_state([(R.PREPARED, 16, 5, 1), (A.NIL, 0, 0, 0)])
    got = e.accept_handle(np.zeros(0, R.ACCEPT_MSG), st, A.mk_groups([(16, 1)]))
    assert got[0].tobytes() == st.tobytes() and all(len(x) == 0 for x in got[1:])


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_tile_edge(mk_engine, mode, n):
    """single-message instances up to, at and past one tile: four rounds of 256 owned instances"""
    check(mk_engine(N, mode), mode, shape_case(n, [1] * n, base=11))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_overhang(mk_engine, mode):
    """a run that starts at record 1020 and is 10 long: 6 records past the tile, from LDS"""
    check(mk_engine(N, mode), mode, shape_case(5, [1] * 1020 + [10] + [1] * 50))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_long_overhang(mk_engine, mode):
    """a run that starts at record 1000 and is 1200 long: past the 64 overhang records kept in
    LDS, over a whole tile without heads and into the next one"""
    check(mk_engine(N, mode), mode, shape_case(6, [1] * 1000 + [1200] + [2] * 100))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_groups(mk_engine, mode):
    """ipg = 8, 300 groups with their own default_ballot and self_id; runs cross group
    boundaries inside a tile"""
    rng = np.random.default_rng(8)
    G, ipg = 300, 8
    runs = rng.integers(1, 3, G * ipg).tolist()
    case = list(A.case_from_runs(rng, np.arange(G * ipg), runs, G * ipg, ipg, 0, N))
    case[2] = A.mk_groups([(16 * (1 + g), g % N) for g in range(G)])
    D = case[2]["default_ballot"][(case[0]["instance"]) // ipg]
    case[0]["ballot"] = D + 16 * rng.integers(-1, 2, len(D))
    case[1]["ballot"] = case[2]["default_ballot"][np.arange(G * ipg) // ipg] + \
        16 * rng.integers(-1, 2, G * ipg)
    check(mk_engine(N, mode), mode, tuple(case))


class Dev:
    """device copies of one case for the _dev form"""

    def __init__(self, e, ar, case, st_out_separate):
        self.e, self.ar = e, ar
        self.msgs, self.st, self.groups, self.base, self.ipg = case
        self.n, self.n_inst = len(self.msgs), len(self.st)
        self.d_msgs, self.d_groups = ar.put(self.msgs), ar.put(self.groups)
        self.d_st = ar.put(self.st)
        self.d_out = ar.full(self.n_inst, R.ACCEPTOR_STATE, 0x55) if st_out_separate else self.d_st
        self.d_rep = ar.full(self.n, R.ACCEPT_REPLY, 0x55)
        self.d_to = ar.full(self.n, np.int32, 0x55)
        self.d_eff = ar.full(self.n, np.uint8, 0x55)

    def call(self, stream=None):
        self.e.accept_handle_dev(self.d_msgs.ptr, self.n, self.d_st.ptr, self.d_out.ptr,
                                 self.n_inst, self.base, self.d_groups.ptr, len(self.groups),
                                 self.ipg, self.d_rep.ptr, self.d_to.ptr, self.d_eff.ptr, stream)

    def results(self):
        g = self.ar.get
        return g(self.d_out), g(self.d_rep), g(self.d_to), g(self.d_eff)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_sparse_window_dev_separate_st_out(mk_engine, mode):
    """every 7th instance has messages; st_out apart from st_in: only those entries are written"""
    from minpaxos_amd.devbuf import Arena
    e = mk_engine(N, mode)
    rng = np.random.default_rng(7)
    case = shape_case(7, rng.integers(1, 4, 400).tolist(), stride=7, base=3)
    want = A.accept_handle(mode, N, *case)
    with Arena(e) as ar:
        d = Dev(e, ar, case, st_out_separate=True)
        d.call()
        e.synchronize()
        st_out, rep, to, eff = d.results()
        assert ar.get(d.d_st).tobytes() == case[1].tobytes()  # st_in is read only
    touched = np.zeros(len(st_out), bool)
    touched[case[0]["instance"] - case[3]] = True
    assert touched.sum() == 400
    assert np.all(st_out[~touched].view(np.uint8) == 0x55)
    assert st_out[touched].tobytes() == want[0][touched].tobytes()
    assert_same((want[0], rep, to, eff), want)
    # and the host form leaves instances without messages as they were
    got = e.accept_handle(*[case[i] for i in (0, 1, 2, 3, 4)])
    assert got[0][~touched].tobytes() == case[1][~touched].tobytes()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_dev_aliased_and_graph_replay(mk_engine, mode):
    """st_out aliasing st_in; then the call captured into a graph and replayed twice, each time
    on a fresh copy of the states"""
    from minpaxos_amd.devbuf import Arena, D2D
    e = mk_engine(N, mode)
    case = shape_case(9, [1] * 700 + [400] + [3] * 300, base=5)
    want = A.accept_handle(mode, N, *case)
    with Arena(e) as ar:
        d = Dev(e, ar, case, st_out_separate=False)
        fresh = ar.put(case[1])
        d.call()
        e.synchronize()
        assert_same(d.results(), want)
        s = e.stream_create()
        e.graph_begin(s)
        d.call(s)
        g = e.graph_end(s)
        try:
            for _ in range(2):
                e.memcpy(d.d_st.ptr, fresh.ptr, fresh.nbytes, D2D, s)
                for buf in (d.d_rep, d.d_to, d.d_eff):
                    e.memset(buf.ptr, 0x55, buf.nbytes, s)
                e.graph_launch(g, s)
                e.stream_synchronize(s)
                assert_same(d.results(), want)
        finally:
            e.graph_destroy(g)
            e.stream_destroy(s)
        e.synchronize()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_errors(mk_engine, mode):
    e = mk_engine(N, mode)
    g = A.mk_groups([(16, 1)])
    st = A.mk_state([(A.NIL, 0, 0, 0)] * 4)
    for msgs, code in (([(10 + 4, 16, 0, 1)], R.E_NIL_INSTANCE),   # past the window
                       ([(10 - 1, 16, 0, 1)], R.E_NIL_INSTANCE),   # before it
                       ([(12, 16, 0, 1), (11, 16, 0, 1)], R.E_INVAL),  # descending
                       ([(11, 16, N, 1)], R.E_BAD_ID),             # replies to PeerWriters[N]
                       ([(11, 16, -1, 1)], R.E_BAD_ID)):
        with pytest.raises(MpxError) as ei:
            e.accept_handle(A.mk_msgs(msgs), st, g, 10)
        assert ei.value.code == code, msgs
    # the engine is usable afterwards; n_inst must be n_groups * ipg
    check(e, mode, shape_case(1, [2, 1, 3]))
    with pytest.raises(MpxError) as ei:
        e.accept_handle(A.mk_msgs([(0, 16, 0, 1)]), st, g, 0, ipg=3)
    assert ei.value.code == R.E_INVAL
    if mode == R.MODE_MIN:  # a message that does not reply never indexes PeerWriters
        got = e.accept_handle(A.mk_msgs([(11, 32, N, 1)]), st, g, 10)
        assert got[2][0] == -1 and got[3][0] == 0


@pytest.mark.parametrize("seed", list(A.FUZZ_SEEDS))
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_fuzz(mk_engine, mode, seed):
    check(mk_engine(N, mode), mode, A.fuzz_case(seed, N))


# ---- the reply bytes -----------------------------------------------------------------------------
def some_replies(rng, n, mode):
    rep = np.zeros(n, R.ACCEPT_REPLY)
    rep["instance"] = rng.integers(-(1 << 31), 1 << 31, n)
    rep["ballot"] = rng.integers(-(1 << 31), 1 << 31, n)
    rep["ok"] = rng.integers(0, 2, n)
    rep["id"] = rng.integers(0, N, n) if mode == R.MODE_MIN else -1
    return rep


def check_encode(e, mode, rep, to, n_dest=N):
    out, off = e.encode_accept_replies(rep, to, n_dest)
    w_out, w_off = A.encode_accept_replies(mode, rep, to, n_dest)
    assert np.array_equal(off, w_off)
    assert out.tobytes() == w_out.tobytes()
    # every destination's run decodes back to the records sent to it, in order
    for d in range(n_dest):
        run = out[int(off[d]):int(off[d + 1])]
        sent = rep[np.asarray(to) == d]
        if len(sent) == 0:
            assert len(run) == 0
            continue
        ar, pr, var, oth, res = e.decode_stream(run.tobytes())
        assert int(res["stop_reason"]) == R.DECODE_END and len(pr) == len(var) == len(oth) == 0
        assert ar.tobytes() == sent.tobytes(), d


@pytest.mark.parametrize("n", [0, 1, 1025])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_encode_sizes(mk_engine, mode, n):
    rng = np.random.default_rng(20 + n)
    check_encode(mk_engine(N, mode), mode, some_replies(rng, n, mode), rng.integers(0, N, n))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_encode_one_destination(mk_engine, mode):
    rng = np.random.default_rng(31)
    check_encode(mk_engine(N, mode), mode, some_replies(rng, 1500, mode), np.full(1500, 3))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_encode_spread_with_skipped_slots(mk_engine, mode):
    rng = np.random.default_rng(32)
    n = 3000
    e = mk_engine(N, mode)
    check_encode(e, mode, some_replies(rng, n, mode), rng.integers(-1, N, n))
    check_encode(e, mode, some_replies(rng, n, mode), rng.integers(-1, 16, n), n_dest=16)
    check_encode(e, mode, some_replies(rng, 70, mode), np.full(70, -1))  # nothing to send
    with pytest.raises(MpxError) as ei:
        e.encode_accept_replies(some_replies(rng, 10, mode), np.full(10, N), N)
    assert ei.value.code == R.E_INVAL


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_encode_dev_needs_reserve_and_takes_any_alignment(mk_engine, mode):
    from minpaxos_amd.devbuf import Arena
    e = mk_engine(N, mode)
    rng = np.random.default_rng(33)
    n, F = 2500, R.ACCEPT_REPLY_FRAME[mode]
    rep, to = some_replies(rng, n, mode), rng.integers(-1, N, n).astype(np.int32)
    w_out, w_off = A.encode_accept_replies(mode, rep, to, N)
    with Arena(e) as ar:
        d_rep, d_to = ar.put(rep), ar.put(to)
        d_out, d_off = ar.full(n * F + 16, np.uint8, 0x55), ar.full(N + 1, np.uint64, 0x55)
        with pytest.raises(MpxError):
            e.encode_accept_replies_dev(d_rep.ptr, d_to.ptr, n, N, d_out.ptr, d_off.ptr)
        e.encode_accept_replies_reserve(n)
        for shift in (0, 1, 6):
            e.memset(d_out.ptr, 0x55, d_out.nbytes)
            e.encode_accept_replies_dev(d_rep.ptr, d_to.ptr, n, N, d_out.ptr + shift, d_off.ptr)
            e.synchronize()
            got = ar.get(d_out)
            assert np.array_equal(ar.get(d_off), w_off)
            assert got[shift:shift + len(w_out)].tobytes() == w_out.tobytes(), shift
            assert np.all(got[:shift] == 0x55) and np.all(got[shift + len(w_out):] == 0x55)


# ---- closing the loop: what the acceptors emit is what the leader's tally consumes --------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_followers_feed_the_leaders_tally(mk_engine, mode):
    e = mk_engine(N, mode)
    rng = np.random.default_rng(40)
    n_inst, D = 600, 16
    got_rep, want_rep = [], []
    for f in range(1, N):
        runs = rng.integers(1, 3, n_inst).tolist()  # some Accepts arrive twice
        case = list(A.case_from_runs(rng, np.arange(n_inst), runs, n_inst, n_inst, 0, N))
        case[2] = A.mk_groups([(D if f < 4 else 2 * D, f)])  # follower 4 has moved on
        case[0]["ballot"], case[0]["leader_id"] = D, 0
        case[1]["ballot"] = D + 16 * rng.integers(-1, 2, n_inst)
        want = A.accept_handle(mode, N, *case)
        got = e.accept_handle(*case)
        assert_same(got, want)
        got_rep.append(got[1][(got[3] & R.AH_REPLIED) != 0])
        want_rep.append(want[1][(want[3] & R.AH_REPLIED) != 0])

    def merged(parts):  # one arrival order for both sides, then the shim's stable sort
        allr = np.concatenate(parts)
        allr = allr[np.random.default_rng(41).permutation(len(allr))]
        return allr[np.argsort(allr["instance"], kind="stable")]
    lst = np.zeros(n_inst, R.INST_STATE)
    lst["status"] = rng.choice([R.PREPARED, R.ACCEPTED, R.COMMITTED], n_inst, p=[.45, .45, .1])
    g_st, g_cu, g_pc, g_dec = e.accept_tally(merged(got_rep), lst, 0, -1)
    w_st, w_cu, w_pc, w_dec = GoBackend(N, mode).accept_tally(merged(want_rep), lst, 0, -1)
    assert len(merged(got_rep)) > n_inst and g_dec.any()
    assert g_st.tobytes() == w_st.tobytes()
    assert np.array_equal(g_dec, w_dec) and g_cu == w_cu and np.array_equal(g_pc, w_pc)

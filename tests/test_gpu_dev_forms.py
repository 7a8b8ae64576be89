"""GPU tests of the device-pointer (_dev) entry points, called directly on guarded buffers.

Every host form stages its arguments into one 256-byte aligned arena and calls its _dev form with
st_out == st_in on the engine's stream, then copies back the valid prefix only. What that hides -
writes past a capacity or next to an output, entries that must stay untouched, unaligned byte
outputs, other streams, graph replays and the control words a call must leave zero - is checked
here: mpx_accept_tally_dev, mpx_prepare_select_dev, mpx_prepare_select_min_dev,
mpx_decode_peer_stream_dev (mpx_decode_reserve), mpx_decode_stream_dev (mpx_decode_stream_reserve)
and mpx_encode_log_dev (mpx_encode_log_reserve). Every output is a devguard.Guard whose margins
are read back after every call; everything is bit-exact against the oracle (log bytes: against the
struct.pack restatement of test_logenc.py). Shapes are the smallest that reach the edges: the
record tile is 1024 records and 256 lanes, the decode tile 16 KB of 128-byte chunks, the log
window 8 KB. No case provokes a fault: the error cases are argument checks that return before
any launch.
"""
import numpy as np
import pytest

import test_logenc as LE
from devguard import Guard
from oracle_lib import Oracle
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd import synth
from minpaxos_amd import wire as W
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError

pytestmark = pytest.mark.gpu
N = 5
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
MODES = [MIN, CLASSIC]
MODE_IDS = ["min", "classic"]
TILE = 1024  # tile.hpp kTileRecs


def same(name, got, want):
    """bit-exact equality of two arrays of one dtype, naming the first elements that differ"""
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


def same_rec(name, got, want, fields=None):
    """two records of one structured dtype, field by field"""
    assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
    for f in fields or got.dtype.names:
        assert int(got[f]) == int(want[f]), (name, f, int(got[f]), int(want[f]))


def restore(e, g, d_fresh, s):
    """a guard back to the sentinel and, for an in/out buffer, its payload back to the input, in
    stream order on s"""
    g.fill(s)
    if d_fresh is not None and g.nbytes:
        e.memcpy(g.ptr, d_fresh.ptr, g.nbytes, D2D, s)


def done(e, s=None):
    """wait for the call and surface what its kernels reported"""
    e.stream_synchronize(s)
    e.synchronize()


# ---- accept tally and CLASSIC prepare: one lane per instance over tiles of 1024 records ------------
def sparse_counts(seed, n_inst=1500, lead=37, trail=41):
    """records per window index: a leading and a trailing gap, every fifth instance inside
    without records, 1 to 3 records otherwise"""
    rng = np.random.default_rng(seed)
    cnt = np.zeros(n_inst, np.int64)
    inner = np.arange(lead, n_inst - trail)
    cnt[inner] = rng.integers(1, 4, len(inner))
    cnt[inner[(inner - lead) % 5 == 4]] = 0
    return cnt


def assert_sparse_geometry(cnt):
    off = np.concatenate([[0], np.cumsum(cnt)])
    n = int(off[-1])
    assert cnt[0] == 0 and cnt[-1] == 0 and (cnt[1:-1] == 0).sum() > 200
    assert 2 <= -(-n // TILE) <= 3, n
    crossing = [(int(off[i]), int(off[i + 1])) for i in range(len(cnt))
                if any(off[i] < b < off[i + 1] for b in range(TILE, n, TILE))]
    assert crossing, "no run crosses a tile boundary"


class TallyFam:
    """mpx_accept_tally[_dev]: scalars = [committedUpTo, peerCommits[N]], flags = decided"""
    rec_dtype, st_dtype, n_scalars = R.ACCEPT_REPLY, R.INST_STATE, 1 + N

    @staticmethod
    def case(cnt, seed, base):
        rng = np.random.default_rng(seed)
        n_inst, n = len(cnt), int(cnt.sum())
        idx = np.repeat(np.arange(n_inst), cnt)
        recs = np.zeros(n, R.ACCEPT_REPLY)
        recs["instance"] = base + idx
        recs["ballot"] = 16 + 16 * rng.integers(0, 3, n)
        recs["id"] = rng.integers(0, N, n)
        recs["ok"] = rng.random(n) < 0.7
        st = np.zeros(n_inst, R.INST_STATE)
        st["status"] = rng.choice([R.PREPARED, R.ACCEPTED, R.COMMITTED], n_inst, p=[.45, .45, .1])
        st["accept_oks"] = rng.integers(0, 2, n_inst)
        st["nacks"] = rng.integers(0, 2, n_inst)
        st["max_recv_ballot"] = 16 * rng.integers(0, 4, n_inst)
        st["status"][(cnt == 0) & (rng.random(n_inst) < 0.2)] = R.STATUS_NIL
        # a committed stretch from the window's start, so that CLASSIC's updateCommittedUpTo
        # walks from the leading gap over instances with and without records
        head = np.arange(n_inst) < min(n_inst, 70)
        st["status"][head & (cnt == 0)] = R.COMMITTED
        st["status"][head & (cnt > 0)] = R.ACCEPTED
        st["accept_oks"][head & (cnt > 0)] = 1
        recs["ok"][head[idx]] = 1
        sc = np.concatenate([[base + min(10, n_inst) - 1], 1000 + np.arange(N)]).astype(np.int32)
        return recs, st, base, sc

    @staticmethod
    def oracle(mode, case):
        recs, st, base, sc = case
        w_st, cu, pc, dec = Oracle(N, mode).accept_tally(recs, st, base, int(sc[0]), sc[1:])
        return w_st, np.concatenate([[cu], pc]).astype(np.int32), dec

    @staticmethod
    def host(e, case):
        recs, st, base, sc = case
        g_st, cu, pc, dec = e.accept_tally(recs, st, base, int(sc[0]), sc[1:])
        return g_st, np.concatenate([[cu], pc]).astype(np.int32), dec

    @staticmethod
    def dev(e, *a):
        e.accept_tally_dev(*a)


class PrepareFam:
    """mpx_prepare_select[_dev]: scalars = [defaultBallot], flags = prepared"""
    rec_dtype, st_dtype, n_scalars = R.PREPARE_REPLY, R.PREP_STATE, 1

    @staticmethod
    def case(cnt, seed, base):
        rng = np.random.default_rng(seed)
        n_inst, n = len(cnt), int(cnt.sum())
        recs = np.zeros(n, R.PREPARE_REPLY)
        recs["instance"] = base + np.repeat(np.arange(n_inst), cnt)
        recs["ballot"] = (rng.integers(0, 16, n) << 4) | rng.integers(0, N, n)
        recs["ballot"][rng.random(n) < 1 / 16] = -1
        recs["ok"] = rng.random(n) < 0.8
        recs["value_id"] = np.arange(1, n + 1)
        st = np.zeros(n_inst, R.PREP_STATE)
        st["ballot"] = 256 + 16 * rng.integers(0, 3, n_inst)
        st["status"] = rng.choice([R.PREPARING, R.PREPARED, R.ACCEPTED], n_inst, p=[.8, .1, .1])
        st["prepare_oks"] = rng.integers(0, 2, n_inst)
        st["nacks"] = rng.integers(0, 2, n_inst)
        st["max_recv_ballot"] = rng.integers(0, 128, n_inst)
        st["value_id"] = np.uint32(0x80000000) | np.arange(n_inst, dtype=np.uint32)
        st["flags"] = rng.integers(0, 2, n_inst) * R.PF_HAS_PROPOSALS
        st["status"][(cnt == 0) & (rng.random(n_inst) < 0.2)] = R.STATUS_NIL
        return recs, st, base, np.array([100], np.int32)

    @staticmethod
    def oracle(mode, case):
        recs, st, base, sc = case
        w_st, db, prep = Oracle(N, mode).prepare_select(recs, st, base, int(sc[0]))
        return w_st, np.array([db], np.int32), prep

    @staticmethod
    def host(e, case):
        recs, st, base, sc = case
        g_st, db, prep = e.prepare_select(recs, st, base, int(sc[0]))
        return g_st, np.array([db], np.int32), prep

    @staticmethod
    def dev(e, *a):
        e.prepare_select_dev(*a)


# (family, engine mode): the tally has both protocols, the per-instance prepare is CLASSIC's
WINDOW_FAMS = [(TallyFam, MIN), (TallyFam, CLASSIC), (PrepareFam, CLASSIC)]
WINDOW_IDS = ["tally-min", "tally-classic", "prepare-classic"]
BASE = 7001
_window_cache = {}


def window_case(fam, mode, key):
    """(case, counts, the oracle's result) of one shape, computed once"""
    k = (fam, mode, key)
    if k not in _window_cache:
        if key == "sparse":
            cnt = sparse_counts(11)
            assert_sparse_geometry(cnt)
        else:  # single-record instances between two small gaps
            cnt = np.concatenate([[0] * 3, [1] * key, [0] * 3]).astype(np.int64)
        case = fam.case(cnt, 50 + len(cnt), BASE)
        want = fam.oracle(mode, case)
        if key == "sparse":  # the shape does something: scalars move, flags of both kinds
            assert want[1][0] != case[3][0] and 0 < want[2].sum() < (cnt > 0).sum()
        _window_cache[k] = (case, cnt, want)
    return _window_cache[k]


class WindowDev:
    """device copies of one case: inputs plain, every output guarded"""

    def __init__(self, fam, e, ar, case, separate, flags):
        self.fam, self.e, self.ar = fam, e, ar
        self.recs, self.st, self.base, self.sc = case
        self.n, self.n_inst = len(self.recs), len(self.st)
        self.d_recs = ar.put(self.recs)
        self.d_st_fresh, self.d_sc_fresh = ar.put(self.st), ar.put(self.sc)
        self.g_sc = Guard(ar, len(self.sc), np.int32, name="scalars").put(self.sc)
        if separate:
            self.d_in = ar.put(self.st)
            self.g_out = Guard(ar, self.n_inst, fam.st_dtype, name="st_out")
            self.p_in = self.d_in.ptr
        else:
            self.d_in = None
            self.g_out = Guard(ar, self.n_inst, fam.st_dtype, name="st").put(self.st)
            self.p_in = self.g_out.ptr
        self.g_fl = Guard(ar, self.n_inst, np.uint8, name="flags") if flags else None

    def guards(self):
        return [g for g in (self.g_sc, self.g_out, self.g_fl) if g is not None]

    def restore(self, s):
        restore(self.e, self.g_sc, self.d_sc_fresh, s)
        restore(self.e, self.g_out, None if self.d_in is not None else self.d_st_fresh, s)
        if self.g_fl is not None:
            restore(self.e, self.g_fl, None, s)

    def call(self, s=None):
        self.fam.dev(self.e, self.d_recs.ptr if self.n else None, self.n, self.p_in,
                     self.g_out.ptr, self.n_inst, self.base, self.g_sc.ptr,
                     self.g_fl.ptr if self.g_fl is not None else None, s)

    def results(self):
        """(st_out, scalars, flags) with every margin checked"""
        out = [g.assert_margins() for g in self.guards()]
        return out[1], out[0], out[2] if self.g_fl is not None else None


def check_separate(fam, e, ar, case, cnt, want, flags=True, stream=None):
    """cases (a) and (b): st_out apart from st_in"""
    d = WindowDev(fam, e, ar, case, separate=True, flags=flags)
    d.call(stream)
    done(e, stream)
    st_out, sc, fl = d.results()
    touched = cnt > 0
    d.g_out.assert_untouched(~touched)
    same("st_out[touched]", st_out[touched], want[0][touched])
    same("st_in", ar.get(d.d_in), case[1])
    same("scalars", sc, want[1])
    if flags:
        same("flags", fl, want[2])  # all n_inst of them: no sentinel in any gap
    return st_out, sc


@pytest.mark.parametrize("fam,mode", WINDOW_FAMS, ids=WINDOW_IDS)
def test_window_separate_outputs_and_null_flags(mk_engine, fam, mode):
    """(a) st_out apart from st_in, on a stream of the caller's; (b) the same without flags"""
    e = mk_engine(N, mode)
    case, cnt, want = window_case(fam, mode, "sparse")
    s = e.stream_create()
    try:
        with Arena(e) as ar:
            st_a, sc_a = check_separate(fam, e, ar, case, cnt, want, flags=True, stream=s)
            if fam is TallyFam and mode == CLASSIC:  # peerCommits belong to MIN
                same("peerCommits", sc_a[1:], case[3][1:])
            st_b, sc_b = check_separate(fam, e, ar, case, cnt, want, flags=False, stream=s)
            same("st_out without flags", st_b, st_a)
            same("scalars without flags", sc_b, sc_a)
    finally:
        e.stream_destroy(s)
    for g, w, name in zip(fam.host(e, case), want, ("st", "scalars", "flags")):
        same("host form after: " + name, g, w)


@pytest.mark.parametrize("fam,mode", WINDOW_FAMS, ids=WINDOW_IDS)
def test_window_aliased_and_graph_replay(mk_engine, fam, mode):
    """(c) st_out aliasing st_in equals the host form; (d) that call captured and replayed twice
    on restored inputs, then a host-form call on the engine the replays left behind"""
    e = mk_engine(N, mode)
    case, cnt, want = window_case(fam, mode, "sparse")
    names = ("st", "scalars", "flags")
    host = fam.host(e, case)
    for g, w, name in zip(host, want, names):
        same("host form: " + name, g, w)
    with Arena(e) as ar:
        d = WindowDev(fam, e, ar, case, separate=False, flags=True)
        d.call()
        done(e)
        for g, w, name in zip(d.results(), host, names):
            same("aliased: " + name, g, w)
        s = e.stream_create()
        d.restore(s)
        d.call(s)  # once eagerly on the stream that will capture it
        done(e, s)
        e.graph_begin(s)
        d.call(s)
        graph = e.graph_end(s)
        try:
            for rep in range(2):
                d.restore(s)
                e.graph_launch(graph, s)
                done(e, s)
                for g, w, name in zip(d.results(), want, names):
                    same(f"replay {rep}: {name}", g, w)
        finally:
            e.graph_destroy(graph)
            e.stream_destroy(s)
    for g, w, name in zip(fam.host(e, case), want, names):
        same("host form after the replays: " + name, g, w)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025])
@pytest.mark.parametrize("fam,mode", WINDOW_FAMS, ids=WINDOW_IDS)
def test_window_tile_edges(mk_engine, fam, mode, n):
    """single-record instances up to, at and past one tile, twice in a row on one engine"""
    e = mk_engine(N, mode)
    case, cnt, want = window_case(fam, mode, n)
    with Arena(e) as ar:
        for _ in range(2):
            check_separate(fam, e, ar, case, cnt, want)


@pytest.mark.parametrize("fam,mode", WINDOW_FAMS, ids=WINDOW_IDS)
def test_window_no_records(mk_engine, fam, mode):
    """n = 0: the flags are all zero, states and scalars are not touched"""
    e = mk_engine(N, mode)
    case, cnt, _ = window_case(fam, mode, 1)
    case = (case[0][:0],) + case[1:]
    with Arena(e) as ar:
        d = WindowDev(fam, e, ar, case, separate=True, flags=True)
        d.call()
        done(e)
        st_out, sc, fl = d.results()
        d.g_out.assert_untouched([(0, d.n_inst)])
        same("scalars", sc, case[3])
        same("flags", fl, np.zeros(d.n_inst, np.uint8))


# ---- MIN prepare: one lane per group ----------------------------------------------------------------
def prepare_min_case():
    G = 300
    rec9, _, gst = synth.prepare_replies_min(G, N, seed=46, replies_per_group=9)
    rng = np.random.default_rng(47)
    cnt = rng.integers(0, 10, G)
    cnt[::11] = 0
    keep = (np.arange(9)[None, :] < cnt[:, None]).reshape(-1)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    pc = rng.integers(-1, 50, G * N).astype(np.int32)
    assert (cnt == 0).sum() >= 27 and cnt.max() == 9 and int(off[-1]) > TILE
    return np.ascontiguousarray(rec9[keep]), off, gst, pc


@pytest.mark.parametrize("with_eff", [True, False], ids=["eff", "null-eff"])
def test_prepare_min_dev(mk_engine, with_eff):
    e = mk_engine(N, MIN)
    recs, off, gst, pc = prepare_min_case()
    want = Oracle(N, MIN).prepare_select_min(recs, off, gst, pc)
    assert (want[2]["flags"] & R.EF_TRIGGER).any() and (want[2]["flags"] == 0).any()
    names = ("gst", "peer_commits", "eff")
    n, G = len(recs), len(gst)
    with Arena(e) as ar:
        d_recs, d_off = ar.put(recs), ar.put(off)
        d_gst, d_pc = ar.put(gst), ar.put(pc)
        g_gst = Guard(ar, G, R.GROUP_PREP_STATE, name="gst").put(gst)
        g_pc = Guard(ar, G * N, np.int32, name="peer_commits").put(pc)
        g_eff = Guard(ar, n, R.PREPARE_EFFECT, name="eff") if with_eff else None

        def call(s=None):
            e.prepare_select_min_dev(d_recs.ptr, n, d_off.ptr, g_gst.ptr, G, g_pc.ptr,
                                     g_eff.ptr if with_eff else None, s)

        def check(what):
            same(f"{what}: gst", g_gst.assert_margins(), want[0])
            same(f"{what}: peer_commits", g_pc.assert_margins(), want[1])
            if with_eff:
                same(f"{what}: eff", g_eff.assert_margins(), want[2])

        def put_back(s):
            restore(e, g_gst, d_gst, s)
            restore(e, g_pc, d_pc, s)
            if with_eff:
                restore(e, g_eff, None, s)

        s = e.stream_create()
        call(s)  # eagerly, on a stream of the caller's
        done(e, s)
        check("eager")
        e.graph_begin(s)
        call(s)
        graph = e.graph_end(s)
        try:
            for rep in range(2):
                put_back(s)
                e.graph_launch(graph, s)
                done(e, s)
                check(f"replay {rep}")
        finally:
            e.graph_destroy(graph)
            e.stream_destroy(s)
    for g, w, name in zip(e.prepare_select_min(recs, off, gst, pc), want, names):
        same("host form after the replays: " + name, g, w)


# ---- fixed-frame peer stream decode: 16 KB tiles of 128-byte chunks --------------------------------
def peer_streams():
    """about 40 KB (three tiles) of AcceptReplies with other fixed frames between them, ending at
    a frame boundary, inside a frame, and at a variable-length frame"""
    recs, _ = synth.accept_replies(620, N, 0.7, seed=42, inst_base=0x0D0D00)
    body = synth.peer_stream(recs, seed=47, p_beacon=0.08, p_prepare=0.08, p_commit_short=0.08,
                             p_unknown=0.05)
    assert 2 * 16384 < len(body) < 3 * 16384
    return {"end": (body, R.DECODE_END), "partial": (body[:-5], R.DECODE_PARTIAL),
            "variable": (np.concatenate([body, np.frombuffer(
                W.accept(MIN, 0, 5, 16, [(1, 2, 3)], 4), np.uint8)]), R.DECODE_VARIABLE)}


class PeerDev:
    def __init__(self, e, ar, buf, n_ar, n_oth):
        self.e = e
        self.n = len(buf)
        self.d_buf = ar.put(buf) if self.n else None
        self.g_ar = Guard(ar, n_ar + 1, R.ACCEPT_REPLY, name="ar")
        self.g_oth = Guard(ar, n_oth + 1, R.PEER_FRAME, name="other")
        self.g_res = Guard(ar, 1, R.DECODE_RESULT, name="res")

    def call(self, ar_cap, oth_cap, s=None, null_ar=False, null_oth=False):
        for g in (self.g_ar, self.g_oth, self.g_res):
            g.fill(s)
        self.e.decode_peer_stream_dev(self.d_buf.ptr if self.d_buf is not None else None, self.n,
                                      None if null_ar else self.g_ar.ptr, ar_cap,
                                      None if null_oth else self.g_oth.ptr, oth_cap,
                                      self.g_res.ptr, s)
        done(self.e, s)
        return self.g_ar.assert_margins(), self.g_oth.assert_margins(), \
            self.g_res.assert_margins()[0]


def check_peer(d, want, ar_cap, oth_cap, **kw):
    w_ar, w_oth, w_res = want
    ar, oth, res = d.call(ar_cap, oth_cap, **kw)
    ka, ko = min(len(w_ar), ar_cap), min(len(w_oth), oth_cap)
    same("ar prefix", ar[:ka], w_ar[:ka])
    same("other prefix", oth[:ko], w_oth[:ko])
    d.g_ar.assert_untouched([(ka, d.g_ar.count)])  # the element at index cap and all after it
    d.g_oth.assert_untouched([(ko, d.g_oth.count)])
    same_rec("res", res, w_res)  # the counts are complete


@pytest.mark.parametrize("cut", ["end", "partial", "variable"])
def test_decode_peer_stream_dev(mk_engine, cut):
    e = mk_engine(N, MIN)
    buf, why = peer_streams()[cut]
    want = Oracle(N, MIN).decode_peer_stream(buf)
    n_ar, n_oth = len(want[0]), len(want[1])
    assert int(want[2]["stop_reason"]) == why and n_ar > 600 and n_oth > 100
    assert int(want[2]["n_accept_replies"]) == n_ar and int(want[2]["n_other"]) == n_oth
    s = e.stream_create()
    try:
        with Arena(e) as ar:
            d = PeerDev(e, ar, buf, n_ar, n_oth)
            with pytest.raises(MpxError, match="mpx_decode_reserve"):  # no launch without scratch
                d.call(n_ar, n_oth)
            e.decode_reserve(len(buf))
            with pytest.raises(MpxError, match="16-byte aligned") as ei:  # no launch either
                e.decode_peer_stream_dev(d.d_buf.ptr + 4, len(buf) - 4, d.g_ar.ptr, n_ar,
                                         d.g_oth.ptr, n_oth, d.g_res.ptr)
            assert ei.value.code == R.E_INVAL
            check_peer(d, want, n_ar, n_oth)
            check_peer(d, want, n_ar, n_oth, s=s)  # on a stream of the caller's
            for cap in (0, 1, n_ar // 2):
                check_peer(d, want, cap, n_oth)
            for cap in (0, 1, n_oth // 2):
                check_peer(d, want, n_ar, cap)
            check_peer(d, want, 0, 0, null_ar=True, null_oth=True)
            # len = 0, with and without a buffer
            empty = Oracle(N, MIN).decode_peer_stream(b"")
            assert int(empty[2]["stop_reason"]) == R.DECODE_END
            check_peer(PeerDev(e, ar, buf[:0], 3, 3), empty, 3, 3)
            d.n = 0
            check_peer(d, empty, n_ar, n_oth)
    finally:
        e.stream_destroy(s)
    got = e.decode_peer_stream(buf)
    for g, w, name in zip(got[:2], want[:2], ("ar", "other")):
        same("host form after: " + name, g, w)
    same_rec("host form after: res", got[2], want[2])


# ---- full stream decode: MPX_DECODE_LONG chaining, capacities, argument errors -------------------
RES_FIELDS = ("consumed", "n_accept_replies", "n_prepare_replies", "n_var", "n_other",
              "stop_reason", "stop_code")
OUT_NAMES = ("ar", "prep", "var", "other")


def prep_dtype(proto):
    return R.PREPARE_REPLY_MIN if proto == MIN else R.PREPARE_REPLY


def stream_cuts(proto):
    """about 40 KB of every kind of frame, ending at a frame boundary, inside a fixed frame and
    inside a variable-length frame"""
    rng = np.random.default_rng(120 + proto)
    frames = 1700 if proto == MIN else 2500  # (CLASSIC's frames are shorter)
    body = W.random_stream(proto, rng, frames, p_var=0.12, max_cmds=5, p_big=0.0)
    assert 2 * 16384 < len(body) < 4 * 16384, len(body)
    cmds = [(1, i, -i) for i in range(4)]
    return {"end": (body, R.DECODE_END),
            "partial": (body + W.accept_reply(proto, 1, 1, 16, 2)[:6], R.DECODE_PARTIAL),
            "variable": (body + W.prepare_reply(proto, 9, 1, 16, cmds, 1, 8)[:-9],
                         R.DECODE_PARTIAL)}


def long_stream(proto, malformed):
    """frames far beyond MPX_DECODE_WINDOW between short ones: a 60-command and a 5000-command
    Accept / PrepareReply, in MIN one with a CatchUpLog; optionally a malformed varint last"""
    rng = np.random.default_rng(130 + proto)
    short = lambda k: W.random_stream(proto, rng, k, p_var=0.0)  # noqa: E731
    c60 = [(2, i, i * i) for i in range(60)]
    c5000 = [(1, -i, i) for i in range(5000)]
    log = [(16, 3, c60[:7]), (32, 2, []), (16, 3, c60[:2])]
    parts = [short(40), W.accept(proto, 0, 7, 16, c60, 6), short(3),
             W.prepare_reply(proto, 8, 1, 16, c5000, 1, 7), short(25),
             W.prepare_reply(proto, 9, 0, 32, c60[:9], 2, 7, log), short(1),
             W.accept(proto, 0, 9, 16, c5000[:70], 8, log[:1]), W.commit(0, 9, 16, c60), short(30)]
    if malformed:
        parts += [W.prepare_reply(proto, 1, 1, 16, [])[:1 + (17 if proto == MIN else 9)] +
                  bytes([0xFF] * 9 + [0x03]), short(5)]
    return b"".join(parts), R.DECODE_MALFORMED if malformed else R.DECODE_END


class StreamDev:
    """one buffer on the device with guarded outputs sized for all of its records"""

    def __init__(self, e, ar, buf, want):
        self.e, self.n = e, len(buf)
        self.d_buf = ar.put(np.frombuffer(buf, np.uint8))
        dts = (R.ACCEPT_REPLY, prep_dtype(e.mode), R.VAR_FRAME, R.PEER_FRAME)
        self.g = [Guard(ar, len(w) + 1, dt, name=nm) for w, dt, nm in zip(want[:4], dts, OUT_NAMES)]
        self.g_res = Guard(ar, 1, R.STREAM_RESULT, name="res")
        self.frames = sum(len(w) for w in (want[0], want[2], want[3])) + 1

    def chain(self, caps, s=None, null=False):
        """zero d_res, call from start = 0 and again from `next` while the result is
        MPX_DECODE_LONG, at most once per frame; every margin checked after every call.
        Returns (the four outputs, the final result, the number of calls)"""
        for g in self.g:
            g.fill(s)
        self.g_res.put(np.zeros(1, R.STREAM_RESULT), s)
        ptr = [None if null else g.ptr for g in self.g]
        out = _lib.MpxDecodeOut(ptr[0], caps[0], ptr[1], caps[1], ptr[2], caps[2], ptr[3], caps[3])
        start = 0
        for calls in range(1, self.frames + 2):
            self.e.decode_stream_dev(self.d_buf.ptr, self.n, start, out, self.g_res.ptr, s)
            done(self.e, s)
            outs = [g.assert_margins() for g in self.g]
            r = self.g_res.assert_margins()[0]
            if int(r["stop_reason"]) != R.DECODE_LONG:
                return outs, r, calls
            assert start <= int(r["consumed"]) < int(r["next"]) <= self.n, (start, r)
            start = int(r["next"])
        raise AssertionError(f"the chain did not end within {self.frames + 1} calls")


def check_stream(d, want, caps=None, **kw):
    full = tuple(len(w) for w in want[:4])
    caps = full if caps is None else caps
    outs, r, calls = d.chain(caps, **kw)
    for g, got, w, cap, name in zip(d.g, outs, want[:4], caps, OUT_NAMES):
        k = min(len(w), cap)
        same(name + " prefix", got[:k], w[:k])
        g.assert_untouched([(k, g.count)])  # nothing at or past the capacity
    same_rec("res", r, want[4], RES_FIELDS)  # the counts are complete whatever the capacities
    return outs, calls


@pytest.mark.parametrize("cut", ["end", "partial", "variable"])
@pytest.mark.parametrize("proto", MODES, ids=MODE_IDS)
def test_decode_stream_dev_cuts_and_capacities(mk_engine, proto, cut):
    e = mk_engine(N, proto)
    buf, why = stream_cuts(proto)[cut]
    want = Oracle(N, proto).decode_stream(buf)
    full = tuple(len(w) for w in want[:4])
    assert int(want[4]["stop_reason"]) == why and min(full) >= 40, full
    e.decode_stream_reserve(len(buf))
    s = e.stream_create()
    try:
        with Arena(e) as ar:
            d = StreamDev(e, ar, buf, want)
            check_stream(d, want)
            check_stream(d, want, s=s)  # on a stream of the caller's
            for k in range(4):  # each capacity short in turn
                for cap in (0, 1, full[k] // 2):
                    caps = full[:k] + (cap,) + full[k + 1:]
                    outs, _ = check_stream(d, want, caps)
                    # value_id of the stored PrepareReplies indexes the FULL var sequence
                    vid = outs[1][:min(full[1], caps[1])]["value_id"]
                    assert (want[2]["code"][vid] == R.PEER_PREPARE_REPLY).all()
                    assert (np.diff(vid.astype(np.int64)) > 0).all()
            check_stream(d, want, (0, 0, 0, 0), null=True)
    finally:
        e.stream_destroy(s)
    # ... and the host form with short capacities: the prefixes and the complete counts
    caps = tuple(x // 2 for x in full)
    got = e.decode_stream(buf, caps=caps)
    for g, w, cap, name in zip(got[:4], want[:4], caps, OUT_NAMES):
        assert len(g) == cap
        same("host form, short capacities: " + name, g, w[:cap])
    same_rec("host form, short capacities: res", got[4], want[4], RES_FIELDS)
    got = e.decode_stream(buf, caps=(0, 1, 0, 1))
    assert [len(x) for x in got[:4]] == [0, 1, 0, 1]
    same("host form, capacity 1: prep", got[1], want[1][:1])
    same("host form, capacity 1: other", got[3], want[3][:1])
    same_rec("host form, capacity 1: res", got[4], want[4], RES_FIELDS)


@pytest.mark.parametrize("malformed", [False, True], ids=["end", "malformed"])
@pytest.mark.parametrize("proto", MODES, ids=MODE_IDS)
def test_decode_stream_dev_long_chain(mk_engine, proto, malformed):
    """every frame beyond the window is one MPX_DECODE_LONG stop that the caller resumes"""
    e = mk_engine(N, proto)
    buf, why = long_stream(proto, malformed)
    want = Oracle(N, proto).decode_stream(buf)
    assert int(want[4]["stop_reason"]) == why and int(want[2]["n_cmds"].max()) == 5000
    if proto == MIN:
        assert int(want[2]["n_log"].max()) == 3
    e.decode_stream_reserve(len(buf))
    with Arena(e) as ar:
        d = StreamDev(e, ar, buf, want)
        _, calls = check_stream(d, want)
        # a frame of more than two chunks and a window is LONG wherever it starts: one call each,
        # and one for what follows the last of them; only variable-length frames can be LONG
        sure = int((want[2]["length"] > 2 * 128 + R.DECODE_WINDOW).sum())
        assert sure >= 4 and sure + 1 <= calls <= len(want[2]) + 1, (sure, calls)
        half = tuple(len(w) // 2 for w in want[:4])
        check_stream(d, want, half)
    got = e.decode_stream(buf)
    for g, w, name in zip(got[:4], want[:4], OUT_NAMES):
        same("host form after: " + name, g, w)
    same_rec("host form after: res", got[4], want[4], RES_FIELDS)


@pytest.mark.parametrize("proto", MODES, ids=MODE_IDS)
def test_decode_stream_dev_argument_errors(mk_engine, proto):
    """none of these launches anything"""
    e = mk_engine(N, proto)
    buf, _ = stream_cuts(proto)["end"]
    want = Oracle(N, proto).decode_stream(buf)
    with Arena(e) as ar:
        d = StreamDev(e, ar, buf, want)
        ptr = [g.ptr for g in d.g]
        out = _lib.MpxDecodeOut(ptr[0], 1, ptr[1], 1, ptr[2], 1, ptr[3], 1)
        with pytest.raises(MpxError, match="mpx_decode_stream_reserve") as ei:
            e.decode_stream_dev(d.d_buf.ptr, d.n, 0, out, d.g_res.ptr)
        assert ei.value.code == R.E_INVAL
        e.decode_stream_reserve(len(buf))
        with pytest.raises(MpxError, match="start is past") as ei:
            e.decode_stream_dev(d.d_buf.ptr, d.n, d.n + 1, out, d.g_res.ptr)
        assert ei.value.code == R.E_INVAL
        for mis in (1, 8):
            with pytest.raises(MpxError, match="16-byte aligned") as ei:
                e.decode_stream_dev(d.d_buf.ptr + mis, d.n - mis, 0, out, d.g_res.ptr)
            assert ei.value.code == R.E_INVAL
        done(e)
        for g in d.g + [d.g_res]:
            g.assert_margins()
            g.assert_untouched([(0, g.count)])
        check_stream(d, want)  # the handle is as good as new


# ---- log encoding: unaligned outputs, exact extents ---------------------------------------------------
SHIFTS = (0, 1, 4, 8, 15)


class LogDev:
    def __init__(self, e, ar, case, out_shift=0, op_shift=0, null_cmds=False):
        self.e = e
        recs, off, op, key, val = case
        self.n, self.m = len(recs), len(op)
        self.bound = e.lib.mpx_encode_log_bound(self.n, self.m)
        self.d_recs = ar.put(recs) if self.n else None
        self.d_off = ar.put(off)
        shifted = np.concatenate([np.zeros(op_shift, np.uint8), op])
        self.d_op, self.d_key, self.d_val = ar.put(shifted), ar.put(key), ar.put(val)
        self.p_op = None if null_cmds else self.d_op.ptr + op_shift
        self.p_key = None if null_cmds else self.d_key.ptr
        self.p_val = None if null_cmds else self.d_val.ptr
        self.g_out = Guard(ar, self.bound, np.uint8, shift=out_shift, name="out")
        self.g_ro = Guard(ar, self.n + 1, np.uint64, name="rec_off")

    def call(self, fmt, s=None):
        self.e.encode_log_dev(fmt, self.d_recs.ptr if self.n else None, self.n, self.d_off.ptr,
                              self.p_op, self.p_key, self.p_val, self.m, self.g_out.ptr,
                              self.g_ro.ptr, s)

    def check(self, want, ro, what):
        out, gro = self.g_out.assert_margins(), self.g_ro.assert_margins()
        assert [int(x) for x in gro] == list(ro), what
        assert out[:len(want)].tobytes() == want, what
        # every byte from rec_off[n] to the bound still holds the sentinel
        self.g_out.assert_untouched([(len(want), self.bound)])


def reserve_log(e, cases):
    e.encode_log_reserve(max(len(c[1][0]) for c in cases), max(len(c[1][2]) for c in cases))


@pytest.mark.parametrize("fmt", LE.FMTS, ids=LE.FMT_IDS)
@pytest.mark.parametrize("family", list(LE.FAMILIES))
def test_encode_log_dev_edges_at_every_shift(mk_engine, family, fmt):
    """every edge case through the _dev form with d_out at an address that is 0, 1, 4, 8 or 15
    mod 16: the first case at all five, the others at one each in turn"""
    e = mk_engine(N, MIN)
    cases = LE.edge_cases(family, fmt)
    with Arena(e) as ar:
        with pytest.raises(MpxError, match="mpx_encode_log_reserve"):  # no launch without scratch
            LogDev(e, ar, cases[0][1]).call(fmt)
    reserve_log(e, cases)
    for i, (label, case, want, ro) in enumerate(cases):
        for shift in (SHIFTS if i == 0 else SHIFTS[i % 5:i % 5 + 1]):
            with Arena(e) as ar:
                d = LogDev(e, ar, case, out_shift=shift)
                d.call(fmt)
                done(e)
                d.check(want, ro, (label, shift))


@pytest.mark.parametrize("fmt", LE.FMTS, ids=LE.FMT_IDS)
def test_encode_log_dev_unaligned_op_empty_and_graph(mk_engine, fmt):
    e = mk_engine(N, MIN)
    cases = [LE.edge_cases(f, fmt)[0] for f in ("varint", "full_range", "sweep")]
    reserve_log(e, cases + LE.edge_cases("dense", fmt)[:1])
    s = e.stream_create()
    try:
        with Arena(e) as ar:
            # d_op at an odd address, on a stream of the caller's
            for op_shift, (label, case, want, ro) in zip((1, 3, 3), cases):
                d = LogDev(e, ar, case, out_shift=op_shift, op_shift=op_shift)
                d.call(fmt, s)
                done(e, s)
                d.check(want, ro, (label, "op", op_shift))
            # m = 0: all records empty, no command arrays at all
            empties = LE.mk_case([0] * 2000, 9)
            want, ro = LE.expected(fmt, *empties)
            assert len(want) == 2000 * LE.rec_len(fmt, 0) > 2 * LE.WINDOW
            d = LogDev(e, ar, empties, out_shift=4, null_cmds=True)
            d.call(fmt)
            done(e)
            d.check(want, ro, "m = 0")
            # n = 0: rec_off[0] = 0 and nothing else
            none = tuple(x[:0] for x in empties[:1]) + (np.zeros(1, np.uint64),) + \
                tuple(x[:0] for x in empties[2:])
            d = LogDev(e, ar, none, null_cmds=True)
            assert d.bound == 0
            d.call(fmt)
            done(e)
            d.check(b"", [0], "n = 0")
            # a graph replay into a refilled, unaligned output
            label, case, want, ro = cases[1]
            d = LogDev(e, ar, case, out_shift=8)
            d.call(fmt, s)
            done(e, s)
            d.check(want, ro, "eager")
            e.graph_begin(s)
            d.call(fmt, s)
            graph = e.graph_end(s)
            try:
                for rep in range(2):
                    d.g_out.fill(s)
                    d.g_ro.fill(s)
                    e.graph_launch(graph, s)
                    done(e, s)
                    d.check(want, ro, ("replay", rep))
            finally:
                e.graph_destroy(graph)
    finally:
        e.stream_destroy(s)
    out, gro = e.encode_log(fmt, *case)
    same("host form after the replays: out", out, np.frombuffer(want, np.uint8))
    same("host form after the replays: rec_off", gro, np.array(ro, np.uint64))

"""GPU tests of the client side (mpx_decode_client_streams, mpx_decode_client_streams_dev): many
connections' bytes framed at once, bit-exact against tests/client_translit.py (clientListener and
its Unmarshals, one connection and one byte at a time). Every case runs the host form and the
_dev form, the latter with its outputs on devguard.Guard buffers exactly their capacity long and
its input in a Guard that ends at the buffer's last byte. Shapes are the smallest that reach the
edges: a chunk is 128 bytes (MPX_CLIENT_ALIGN), a tile 128 chunks (16 KB), a group of tile maps 128
tiles (2 MB), the per-connection kernels' blocks 256 and 1024 connections. The error cases are
reported through the error word or refused before any launch: no case provokes a fault."""
import numpy as np
import pytest

import client_kat
import client_translit as T
from devguard import Guard
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd import wire
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError

N = 5
CHUNK, TILE, GROUP = 128, 128 * 128, 128 * 128 * 128
NAMES = ("op", "key", "val", "meta", "prop_off", "send_off", "conn_res", "res")
P = wire.propose(7, 1, 10, 20, 1000)
Z = bytes(30)


def layout(bufs, groups=None, gaps=()):
    """the connections at 128-byte offsets; gaps: after these connections, one more 128-byte
    chunk of 0x00 that belongs to nobody"""
    conns = np.zeros(len(bufs), R.CLIENT_CONN)
    at = 0
    for k, b in enumerate(bufs):
        conns[k] = (at, len(b), 0 if groups is None else groups[k])
        at += -(-len(b) // CHUNK) * CHUNK + (CHUNK if k in gaps else 0)
    if bufs and len(bufs[-1]) and (len(bufs) - 1) not in gaps:
        at = int(conns["offset"][-1]) + len(bufs[-1])  # the buffer ends with the last byte
    buf = np.zeros(at, np.uint8)
    for k, b in enumerate(bufs):
        o = int(conns["offset"][k])
        buf[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
    return buf, conns


def same(got, want, cap, what=""):
    n = min(int(want["res"]["n_proposals"]), cap)
    for name in NAMES:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if name in ("op", "key", "val", "meta"):
            g, w = g[:n], w[:n]
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            if g.shape == ():
                raise AssertionError(f"{what} {name}: got {g} want {w}")
            diff = [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()][:5]
            raise AssertionError(f"{what} {name} differs at {diff}: got {g[diff]} want {w[diff]}")


def dev_buffers(ar, buf, conns, n_groups, cap):
    g = dict(op=Guard(ar, cap, np.uint8), key=Guard(ar, cap, np.int64),
             val=Guard(ar, cap, np.int64), meta=Guard(ar, cap, R.PROPOSAL),
             prop_off=Guard(ar, n_groups + 1, np.uint64), send_off=Guard(ar, n_groups + 1, np.uint64),
             conn_res=Guard(ar, len(conns), R.CLIENT_CONN_RESULT), res=Guard(ar, 1, R.CLIENT_RESULT))
    g_buf = Guard(ar, len(buf), np.uint8).put(buf)  # ends at the buffer's last byte
    d_conns = ar.put(conns) if len(conns) else None
    out = _lib.MpxClientOut(g["op"].ptr if cap else None, g["key"].ptr if cap else None,
                            g["val"].ptr if cap else None, g["meta"].ptr if cap else None, cap,
                            g["prop_off"].ptr, g["send_off"].ptr)
    return g, g_buf, d_conns, out


def read_dev(g, n_written):
    """every guard's payload with its margins checked; proposals past n_written left alone"""
    got = {}
    for name in NAMES:
        got[name] = g[name].assert_margins()
        if name in ("op", "key", "val", "meta"):
            g[name].assert_untouched([(n_written, g[name].count)])
    got["res"] = got["res"][0]
    return got


def run_dev(e, buf, conns, n_groups, cap, stream=None):
    with Arena(e) as ar:
        g, g_buf, d_conns, out = dev_buffers(ar, buf, conns, n_groups, cap)
        e.decode_client_streams_reserve(len(buf), len(conns), n_groups)
        e.decode_client_streams_dev(g_buf.ptr, len(buf), d_conns.ptr if d_conns else None,
                                    len(conns), n_groups, out, g["conn_res"].ptr, g["res"].ptr,
                                    stream)
        e.synchronize()
        g_buf.assert_margins()
        n = min(int(g["res"].payload()[0]["n_proposals"]), cap)
        return read_dev(g, n)


def check(e, bufs, groups=None, n_groups=1, cap=None, gaps=(), want=None, forms=("host", "dev")):
    buf, conns = layout(bufs, groups, gaps)
    if want is None:
        want = T.decode_client_streams(bufs, groups, n_groups)
    total = int(want["res"]["n_proposals"])
    cap = total if cap is None else cap
    if "host" in forms:
        got = e.decode_client_streams(None, n_groups=n_groups, prop_cap=cap, buf=buf, conns=conns)
        same(got, want, cap, "host")
    if "dev" in forms:
        same(run_dev(e, buf, conns, n_groups, cap), want, cap, "dev")
    return want


@pytest.fixture
def eng(mk_engine):
    return mk_engine(N, R.MODE_MIN)


@pytest.mark.gpu
@pytest.mark.parametrize("case", client_kat.KAT_CLIENT, ids=lambda c: c["name"])
def test_known_answers(eng, case):
    want = check(eng, client_kat.kat_bytes(case), case["groups"], case["n_groups"])
    assert want["prop_off"].tolist() == case["prop_off"]


@pytest.mark.gpu
def test_no_connection_and_empty_connections(eng):
    check(eng, [], n_groups=1)
    check(eng, [], n_groups=3)
    check(eng, [b""] * 5, [0, 0, 1, 1, 2], 3)
    check(eng, [b"", b"", P, b"", b""], [0, 0, 1, 1, 2], 3)


@pytest.mark.gpu
def test_every_truncation_of_a_trailing_frame(eng):
    """PROPOSE cut to 1..29 bytes and READ to 1..12: PARTIAL, consumed and stop_code"""
    bufs = [P * 2 + P[:k] for k in range(1, 30)] + \
           [P + wire.read(3, 4)[:k] for k in range(1, 13)] + \
           [wire.propose_and_read(1, 2, 3, 4, 5)[:k] for k in (1, 17, 29)]
    want = check(eng, bufs)
    cr = want["conn_res"]
    assert (cr["stop_reason"] == R.DECODE_PARTIAL).all()
    assert cr["consumed"][:29].tolist() == [60] * 29 and cr["stop_code"][:29].tolist() == [0] * 29
    assert cr["consumed"][29:41].tolist() == [30] * 12 and cr["stop_code"][29:41].tolist() == [2] * 12
    assert cr["stop_code"][41:].tolist() == [4] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("at", [0, TILE, GROUP], ids=["chunk", "tile", "group"])
def test_frames_straddle_the_boundaries_at_every_phase(eng, at):
    """k unknown bytes (k = 0..29) before a run of Proposes: at = 0 moves the frames over every
    chunk boundary at every phase; at = TILE / GROUP puts the shifted run across the end of a
    tile / of a group of tile maps"""
    rng = np.random.default_rng(at + 1)
    run = wire.random_client_stream(rng, 12, p_read=0, p_par=0, p_unknown=0)
    bufs = []
    for k in range(30):
        lead = (at - 45 - k) // 30 if at else 0  # Proposes up to just before the boundary
        bufs.append(Z * lead + bytes([7] * k) + run)
        if at:
            assert len(Z * lead) + k < at < len(bufs[-1])
    if at == GROUP:  # one 2 MB connection is enough per phase class: three phases
        bufs = bufs[0:30:13]
    want = check(eng, bufs, forms=("dev",) if at else ("host", "dev"))
    assert (want["conn_res"]["stop_reason"] == R.DECODE_END).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [127, 128, 129, TILE - 1, TILE, TILE + 1])
def test_stream_lengths_around_chunk_and_tile(eng, n):
    """streams of exactly n bytes (every len mod 16 among them), alone and followed by a
    connection, ending in whatever frame the length cuts"""
    rng = np.random.default_rng(n)
    s = wire.random_client_stream(rng, n // 10)
    assert len(s) >= n
    check(eng, [s[:n]])
    check(eng, [s[:n], P])
    check(eng, [Z * (n // 30) + bytes([9] * (n % 30))])  # ends exactly at a frame boundary


@pytest.mark.gpu
@pytest.mark.parametrize("rem", range(16))
def test_every_len_mod_16(eng, rem):
    s = (P * 6)[:128 + rem]
    buf, _ = layout([P, s])
    assert len(buf) % 16 == rem
    check(eng, [P, s])


@pytest.mark.gpu
@pytest.mark.parametrize("n_conns", [1, 2, 255, 256, 257, 1024, 1025])
def test_connection_counts_with_empty_connections(eng, n_conns):
    """empty connections first, in the middle, last and in runs"""
    rng = np.random.default_rng(n_conns)
    bufs = [wire.random_client_stream(rng, int(rng.integers(1, 6))) for _ in range(n_conns)]
    for k in range(n_conns):
        if k in (0, n_conns // 2, n_conns - 1) and n_conns > 2 or 10 <= k < 14 or rng.random() < 0.1:
            bufs[k] = b""
    groups = np.sort(rng.integers(0, 7, n_conns)).tolist()
    check(eng, bufs, groups, 7)


@pytest.mark.gpu
def test_65536_connections_of_one_frame(eng):
    n = 65536
    frames = [wire.propose(k, k & 255, -k, k * 3, k + (1 << 40)) for k in range(n)]
    want = dict(op=(np.arange(n) & 255).astype(np.uint8), key=-np.arange(n, dtype=np.int64),
                val=3 * np.arange(n, dtype=np.int64), meta=np.zeros(n, R.PROPOSAL),
                prop_off=np.array([0, n], np.uint64), send_off=np.array([0, 14], np.uint64),
                conn_res=np.zeros(n, R.CLIENT_CONN_RESULT), res=np.zeros((), R.CLIENT_RESULT))
    want["meta"]["timestamp"] = np.arange(n) + (1 << 40)
    want["meta"]["command_id"] = want["meta"]["client"] = np.arange(n)
    cr = want["conn_res"]
    cr["first"], cr["consumed"], cr["n_proposals"], cr["stop_code"] = np.arange(n), 30, 1, -1
    want["res"]["n_proposals"], want["res"]["n_sends"] = n, 14
    for k in (0, 1, 4097, n - 1):  # the closed form is what the transliteration says
        assert T.client_listener(frames[k]) == ([(k, k & 255, -k, 3 * k, k + (1 << 40))], 0, 30,
                                                R.DECODE_END, -1)
    check(eng, frames, want=want)


@pytest.mark.gpu
def test_three_tiles_between_one_frame_connections(eng):
    rng = np.random.default_rng(5)
    big = wire.random_client_stream(rng, 2600)
    big = big[:3 * TILE + 7]
    bufs = [P, wire.read(1, 2), big, P, Z]
    want = check(eng, bufs, [0, 0, 1, 2, 2], 3)
    assert int(want["conn_res"]["consumed"][2]) <= len(big)


@pytest.mark.gpu
def test_partial_connection_then_full_one_and_unframed_gaps(eng):
    """a stop in connection k has no effect on connection k + 1; 128-byte gaps of 0x00 between
    connections are nobody's: not framed (four Proposes would fit each)"""
    bufs = [P + P[:11], P * 3, P[:1], Z * 5 + b"\x02", P]
    want = check(eng, bufs, gaps={0, 1, 3, 4})
    assert want["conn_res"]["n_proposals"].tolist() == [1, 3, 0, 5, 1]
    assert int(want["res"]["n_partial"]) == 3
    check(eng, [Z * 4 + bytes(8), P], gaps={0})  # a full chunk of zeroes, then a gap of zeroes


@pytest.mark.gpu
def test_prop_cap_one_short_and_zero(eng):
    rng = np.random.default_rng(8)
    bufs = [wire.random_client_stream(rng, 40) for _ in range(9)]
    want = T.decode_client_streams(bufs)
    total = int(want["res"]["n_proposals"])
    for cap in (total - 1, 0, 1, total + 3):
        check(eng, bufs, cap=cap, want=want)


@pytest.mark.gpu
@pytest.mark.parametrize("n_g", [0, 1, 4999, 5000, 5001, 10000])
def test_sends_per_group_follow_ceil(eng, n_g):
    """groups with no connection at the start, in the middle and at the end"""
    bufs = [Z * 3, Z * n_g, b"", Z * 5001]
    want = check(eng, bufs, [1, 3, 3, 4], 7)
    sends = -(-n_g // R.PROPOSE_MAX_BATCH)
    assert want["prop_off"].tolist() == [0, 0, 3, 3, 3 + n_g, n_g + 5004, n_g + 5004, n_g + 5004]
    assert want["send_off"].tolist() == [0, 0, 1, 1, 1 + sends, 3 + sends, 3 + sends, 3 + sends]


@pytest.mark.gpu
@pytest.mark.parametrize("n_groups", [1, 2, 65536])
def test_group_counts(eng, n_groups):
    rng = np.random.default_rng(n_groups)
    bufs = [wire.random_client_stream(rng, 20) for _ in range(40)]
    groups = np.sort(rng.integers(0, n_groups, 40)).tolist()
    check(eng, bufs, groups, n_groups)


def _code(fn, *a, **kw):
    with pytest.raises(MpxError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _faults():
    """(name, edit of conns, the connections it makes faulty)"""
    def misaligned(c, n):
        c["offset"][2] += 64

    def out_of_range(c, n):
        c["length"][2] = n - int(c["offset"][2]) + 1

    def past_the_end(c, n):
        c["offset"][2] = (n + 127) // 128 * 128 + 128

    def overlap(c, n):
        c["offset"][2] = c["offset"][1]

    def group_order(c, n):
        c["group"][2] = 0

    def group_range(c, n):
        c["group"][2] = 9
    return [misaligned, out_of_range, past_the_end, overlap, group_order, group_range]


@pytest.mark.gpu
@pytest.mark.parametrize("fault", _faults(), ids=lambda f: f.__name__)
def test_faulty_connection_frames_nothing_and_its_neighbours_are_exact(eng, fault):
    """host form: MPX_E_INVAL before anything is staged; _dev form: the error word, the faulty
    connection frames nothing, its neighbours are exact and the margins are intact"""
    e = eng
    rng = np.random.default_rng(3)
    bufs = [wire.random_client_stream(rng, 9) for _ in range(5)]
    groups, n_groups = [0, 1, 1, 2, 3], 4
    buf, conns = layout(bufs, groups)
    fault(conns, len(buf))
    assert _code(e.decode_client_streams, None, n_groups=n_groups, buf=buf, conns=conns) == R.E_INVAL
    # what is left: connection 2 as an empty one, in the largest group before it
    want = T.decode_client_streams([b"" if k == 2 else b for k, b in enumerate(bufs)], groups,
                                   n_groups)
    cap = int(want["res"]["n_proposals"])
    with Arena(e) as ar:
        g, g_buf, d_conns, out = dev_buffers(ar, buf, conns, n_groups, cap)
        e.decode_client_streams_reserve(len(buf), len(conns), n_groups)
        e.decode_client_streams_dev(g_buf.ptr, len(buf), d_conns.ptr, len(conns), n_groups, out,
                                    g["conn_res"].ptr, g["res"].ptr)
        assert _code(e.synchronize) == R.E_INVAL
        same(read_dev(g, cap), want, cap, fault.__name__)
    check(e, bufs, groups, n_groups)  # the engine is usable afterwards


@pytest.mark.gpu
def test_argument_errors_alignment_and_limits(eng):
    e = eng
    buf, conns = layout([P, P])
    out = _lib.MpxClientOut(None, None, None, None, 0, None, None)
    res = _lib.MpxClientResult()
    lib, h = e.lib, e.h
    off = np.zeros(1, np.uint64)  # prop_off / send_off with n_groups == 0
    for o in (_lib.MpxClientOut(None, None, None, None, 0, off.ctypes.data, None),
              _lib.MpxClientOut(None, None, None, None, 0, None, off.ctypes.data)):
        assert lib.mpx_decode_client_streams(h, None, 0, None, 0, 0, o, None, res) == R.E_INVAL
    assert lib.mpx_decode_client_streams(h, None, 0, None, 0, 0, out, None, res) == R.OK
    assert lib.mpx_decode_client_streams(h, None, 0, None, 0, 0, None, None, res) == R.E_INVAL
    assert lib.mpx_decode_client_streams(h, None, 0, None, 0, 0, out, None, None) == R.E_INVAL
    assert lib.mpx_decode_client_streams(h, None, 0, None, 1, 1, out, None, res) == R.E_INVAL
    assert lib.mpx_decode_client_streams(h, None, 0, None, 0, R.CLIENT_MAX_GROUPS + 1, out, None,
                                         res) == R.E_UNSUPPORTED
    assert lib.mpx_decode_client_streams(h, None, 0, None, R.CLIENT_MAX_CONNS + 1, 1, out, None,
                                         res) == R.E_INVAL  # (null conns answers first)
    assert lib.mpx_decode_client_streams_reserve(h, R.DECODE_MAX_BYTES + 1, 1, 1) == R.E_UNSUPPORTED
    assert lib.mpx_decode_client_streams_reserve(h, 1, R.CLIENT_MAX_CONNS + 1, 1) == R.E_UNSUPPORTED
    with Arena(e) as ar:
        g, g_buf, d_conns, out = dev_buffers(ar, buf, conns, 1, 2)
        e.decode_client_streams_reserve(len(buf), 2, 1)

        def call(d_buf=g_buf.ptr, d_c=d_conns.ptr, o=out, d_cr=g["conn_res"].ptr, d_res=g["res"].ptr):
            return _code(e.decode_client_streams_dev, d_buf, len(buf), d_c, 2, 1, o, d_cr, d_res)

        def outs(**kw):
            f = dict(op=g["op"].ptr, key=g["key"].ptr, val=g["val"].ptr, meta=g["meta"].ptr,
                     prop_cap=2, prop_off=g["prop_off"].ptr, send_off=g["send_off"].ptr)
            f.update(kw)
            return _lib.MpxClientOut(*[f[k] for k in ("op", "key", "val", "meta", "prop_cap",
                                                      "prop_off", "send_off")])
        assert call(d_buf=g_buf.ptr + 8) == R.E_INVAL
        assert call(d_c=d_conns.ptr + 8) == R.E_INVAL
        assert call(d_cr=g["conn_res"].ptr + 8) == R.E_INVAL
        assert call(d_res=g["res"].ptr + 4) == R.E_INVAL
        assert call(o=outs(meta=g["meta"].ptr + 8)) == R.E_INVAL
        assert call(o=outs(key=g["key"].ptr + 4)) == R.E_INVAL
        assert call(o=outs(val=g["val"].ptr + 4)) == R.E_INVAL
        assert call(o=outs(prop_off=g["prop_off"].ptr + 4)) == R.E_INVAL
        assert call(o=outs(send_off=g["send_off"].ptr + 4)) == R.E_INVAL
        assert call(o=outs(op=None)) == R.E_INVAL  # a capacity with a null array
        e.synchronize()
        for name in NAMES:
            g[name].assert_untouched([(0, g[name].count)])
        # op takes any address
        g_op = Guard(ar, 2, np.uint8, shift=3)
        e.decode_client_streams_dev(g_buf.ptr, len(buf), d_conns.ptr, 2, 1, outs(op=g_op.ptr),
                                    g["conn_res"].ptr, g["res"].ptr)
        e.synchronize()
        assert g_op.assert_margins().tolist() == [1, 1]
    check(e, [P, P])


@pytest.mark.gpu
def test_dev_form_needs_its_reserve_and_never_grows(mk_engine):
    e = mk_engine(N, R.MODE_CLASSIC)
    bufs = [Z * 700, P]
    buf, conns = layout(bufs)
    with Arena(e) as ar:
        g, g_buf, d_conns, out = dev_buffers(ar, buf, conns, 1, 701)
        args = (g_buf.ptr, len(buf), d_conns.ptr, 2, 1, out, g["conn_res"].ptr, g["res"].ptr)
        with pytest.raises(MpxError) as ei:
            e.decode_client_streams_dev(*args)
        assert ei.value.code == R.E_INVAL and "mpx_decode_client_streams_reserve" in str(ei.value)
        e.decode_client_streams_reserve(1000, 2, 1)
        assert _code(e.decode_client_streams_dev, *args) == R.E_INVAL
        # no connection: no scratch
        e.decode_client_streams_dev(g_buf.ptr, len(buf), None, 0, 1, out, None, g["res"].ptr)
        e.synchronize()
        assert int(g["res"].assert_margins()[0]["n_proposals"]) == 0
        assert g["prop_off"].assert_margins().tolist() == [0, 0]
        g["op"].assert_untouched([(0, 701)])
    check(e, bufs)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_fuzz(eng, seed):
    rng = np.random.default_rng(5000 + seed)
    n_conns = int(rng.integers(1, 40))
    n_groups = int(rng.integers(1, 6))
    bufs = []
    for _ in range(n_conns):
        s = wire.random_client_stream(rng, int(rng.integers(0, 120)))
        if rng.random() < 0.4 and len(s):
            s = s[:int(rng.integers(0, len(s)))]
        bufs.append(s)
    groups = np.sort(rng.integers(0, n_groups, n_conns)).tolist()
    gaps = set(np.flatnonzero(rng.random(n_conns) < 0.2).tolist())
    total = int(T.decode_client_streams(bufs, groups, n_groups)["res"]["n_proposals"])
    check(eng, bufs, groups, n_groups, gaps=gaps, cap=total if seed % 3 else max(total - 2, 0))


# ---- chains: what the client decode leaves is what the proposer side takes -----------------------
def _chain_input(seed, G, per_group, slot):
    """per_group connections per group, each in a fixed receive slot of `slot` bytes: some
    Proposes among dropped frames, a cut-off tail here and there. Returns (bufs, groups)."""
    rng = np.random.default_rng(seed)
    bufs, groups = [], []
    for g in range(G):
        for c in range(per_group):
            s = wire.random_client_stream(rng, int(rng.integers(1, slot // 40)))
            if rng.random() < 0.3:
                s = s[:len(s) - int(rng.integers(1, 12))]
            if c == 0:
                s = P + s  # every group proposes something: one send per group in every replay
            assert len(s) <= slot
            bufs.append(s)
            groups.append(g)
    return bufs, groups


@pytest.mark.gpu
def test_graph_of_decode_propose_handle_and_encode_accepts(mk_engine):
    """decode_client_streams_dev -> propose_handle_dev -> encode_accepts_dev captured into one
    graph and replayed on two inputs (new d_conns lengths and bytes, same pointers), against
    client_translit and proposer_translit for states, sends and Accept bytes"""
    import proposer_translit as PT
    e = mk_engine(N, R.MODE_MIN)
    G, per_group, slot, ipg, base, D = 3, 4, 1024, 8, 50, 32
    n_inst, n_conns = G * ipg, G * per_group
    inputs = []
    for seed in (11, 12):
        bufs, groups = _chain_input(seed, G, per_group, slot)
        wc = T.decode_client_streams(bufs, groups, G)
        grp = PT.mk_groups([(D, 0, 0, 3, base + g * ipg, base + g * ipg - 1) for g in range(G)])
        st, lb = PT.nil_state(n_inst), np.zeros(n_inst, R.INST_STATE)
        wp = PT.propose_handle(R.MODE_MIN, N, grp, wc["prop_off"], st, base, ipg, lb)
        lrec = np.zeros(n_inst, R.LOG_REC)
        lrec["status"] = PT.NIL
        log = (lrec, np.zeros(n_inst + 1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.int64),
               np.zeros(0, np.int64))
        pcs = np.repeat(base + np.arange(G) * ipg - 1, N).astype(np.int32).reshape(G, N)
        w_out, w_off = PT.encode_accepts(R.MODE_MIN, N, wp[3], wp[0], (wc["op"], wc["key"], wc["val"]),
                                         base, ipg, pcs, log)
        assert len(wp[3]) == G and (wp[3]["flags"] == R.PH_ACCEPT).all() and len(w_out)
        buf = np.zeros(n_conns * slot, np.uint8)
        conns = np.zeros(n_conns, R.CLIENT_CONN)
        for k, b in enumerate(bufs):
            conns[k] = (k * slot, len(b), groups[k])
            buf[k * slot:k * slot + len(b)] = np.frombuffer(b, np.uint8)
        inputs.append((buf, conns, grp, st, lb, lrec, log, pcs, wc, wp, w_out, w_off))
    cap = n_conns * slot // 30
    out_cap = max(len(x[10]) for x in inputs) + 64
    with Arena(e) as ar:
        g, g_buf, d_conns, out = dev_buffers(ar, inputs[0][0], inputs[0][1], G, cap)
        g_grp, g_st = Guard(ar, G, R.PROPOSER_GROUP), Guard(ar, n_inst, R.ACCEPTOR_STATE)
        g_lb, g_snd = Guard(ar, n_inst, R.INST_STATE), Guard(ar, G, R.ACCEPT_SEND)
        g_out, g_off = Guard(ar, out_cap, np.uint8), Guard(ar, N + 1, np.uint64)
        lrec, log, pcs = inputs[0][5], inputs[0][6], inputs[0][7]
        keep = [ar.put(pcs), ar.put(lrec), ar.put(log[1]), Guard(ar, 0, np.uint8),
                Guard(ar, 0, np.int64), Guard(ar, 0, np.int64)]
        b = _lib.MpxAcceptBatch()
        b.sends, b.n_sends, b.inst_base, b.ipg = g_snd.ptr, G, base, ipg
        b.n_groups, b.groups, b.peer_commits = G, g_grp.ptr, keep[0].ptr
        b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = g["op"].ptr, g["key"].ptr, g["val"].ptr, cap
        b.log_recs, b.log_cmd_off = keep[1].ptr, keep[2].ptr
        b.log_op, b.log_key, b.log_val, b.n_log_cmds = keep[3].ptr, keep[4].ptr, keep[5].ptr, 0
        b.flags, b.alive_mask = 0, 0xFFFF
        e.decode_client_streams_reserve(len(inputs[0][0]), n_conns, G)
        e.encode_accepts_reserve(G, n_inst, 0)
        s = e.stream_create()
        e.graph_begin(s)
        e.decode_client_streams_dev(g_buf.ptr, n_conns * slot, d_conns.ptr, n_conns, G, out,
                                    g["conn_res"].ptr, g["res"].ptr, s)
        e.propose_handle_dev(g_grp.ptr, G, g["prop_off"].ptr, g["send_off"].ptr, g_st.ptr, g_lb.ptr,
                             n_inst, base, ipg, g_snd.ptr, s)
        e.encode_accepts_dev(b, g_out.ptr, out_cap, g_off.ptr, s)
        gr = e.graph_end(s)
        try:
            for buf, conns, grp, st, lb, _, _, _, wc, wp, w_out, w_off in inputs + inputs[:1]:
                for x in list(g.values()) + [g_snd, g_out, g_off]:
                    x.fill(s)
                g_buf.put(buf, s)
                g_grp.put(grp, s)
                g_st.put(st, s)
                g_lb.put(lb, s)
                src = ar.put(conns, s)
                e.memcpy(d_conns.ptr, src.ptr, src.nbytes, D2D, s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                same(read_dev(g, int(wc["res"]["n_proposals"])), wc, cap, "replay")
                assert g_grp.assert_margins().tobytes() == wp[0].tobytes()
                assert g_st.assert_margins().tobytes() == wp[1].tobytes()
                assert g_lb.assert_margins().tobytes() == wp[2].tobytes()
                assert g_snd.assert_margins().tobytes() == wp[3].tobytes()
                assert np.array_equal(g_off.assert_margins(), w_off)
                assert g_out.assert_margins()[:len(w_out)].tobytes() == w_out.tobytes()
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()
        del keep


@pytest.mark.gpu
def test_closed_loop_from_client_bytes_to_reply_bytes(mk_engine):
    """client bytes in; the Accept frames go through decode -> unmarshal -> accept_handle on two
    followers; their replies are ordered into the leader's tally; mpx_reply_recs are built on the
    host from meta and the decided mask; then mpx_encode_replies: every connection's reply run
    carries exactly its own CommandIds and Timestamps in its own order"""
    import struct

    import proposer_translit as PT
    NR = 3
    e = mk_engine(NR, R.MODE_MIN)
    G, per_group, slot, ipg, base, D = 3, 5, 1024, 8, 300, 48
    n_inst, n_conns = G * ipg, G * per_group
    bufs, groups = _chain_input(21, G, per_group, slot)
    got = check(e, bufs, groups, G, forms=("host",))
    want_ids = [[(p[0], p[4]) for p in T.client_listener(b)[0]] for b in bufs]
    grp = PT.mk_groups([(D, 0, 0, 2, base + g * ipg, base + g * ipg - 1) for g in range(G)])
    lb = np.zeros(n_inst, R.INST_STATE)
    grp, st, lb, sends, send_off = e.propose_handle(grp, got["prop_off"], PT.nil_state(n_inst), base,
                                                    ipg, lb)
    assert np.array_equal(send_off, got["send_off"]) and len(sends) == G
    lrec = np.zeros(n_inst, R.LOG_REC)
    lrec["status"] = PT.NIL
    log = (lrec, np.zeros(n_inst + 1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.int64),
           np.zeros(0, np.int64))
    pcs = np.repeat(base + np.arange(G) * ipg - 1, NR).astype(np.int32).reshape(G, NR)
    out, off = e.encode_accepts(sends, grp, (got["op"], got["key"], got["val"]), base, ipg, pcs, log)
    replies = []
    for q in (1, 2):
        run = out[int(off[q]):int(off[q + 1])].tobytes()
        _, _, var, _, res = e.decode_stream(run)
        assert int(res["stop_reason"]) == R.DECODE_END and len(var) == G
        um, _ = e.unmarshal_frames(run, var)
        assert np.array_equal(um["key"], got["key"]) and np.array_equal(um["op"], got["op"])
        fg = np.zeros(G, R.ACCEPTOR_GROUP)
        fg["default_ballot"], fg["self_id"] = D, q
        _, rep, to, eff = e.accept_handle(um["accepts"], PT.nil_state(n_inst), fg, base, ipg)
        assert (eff & R.AH_REPLIED).all() and (to == 0).all()
        replies.append(rep[::-1].copy())  # each connection in its own arrival order
    batch, _, _ = e.order_records(replies, n_inst, base)
    _, _, _, decided = e.accept_tally(batch, lb, base, base - 1, np.full(NR, base - 1, np.int32))
    assert int(decided.sum()) == G
    # the replies of the decided instances' commands, in instance order
    recs = []
    for s_ in sends:
        assert decided[int(s_["instance"]) - base]
        for j in range(int(s_["first_cmd"]), int(s_["first_cmd"]) + int(s_["n_cmds"])):
            m = got["meta"][j]
            recs.append((0, int(m["timestamp"]), int(m["command_id"]), int(m["client"])))
    recs = np.array(recs, R.REPLY_REC)
    assert len(recs) == int(got["res"]["n_proposals"])
    rbytes, roff = e.encode_replies(recs, n_conns)
    for k in range(n_conns):
        run = rbytes[int(roff[k]):int(roff[k + 1])].tobytes()
        assert len(run) == R.PROPOSE_REPLY_BYTES * len(want_ids[k])
        ids = [(struct.unpack_from("<i", run, 25 * i + 1)[0], struct.unpack_from("<q", run, 25 * i + 13)[0])
               for i in range(len(want_ids[k]))]
        assert ids == want_ids[k], k

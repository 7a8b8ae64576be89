"""GPU tests of batch assembly (mpx_order_records, mpx_order_records_dev): several sources'
records as one batch in the handlers' contract order, bit-exact against tests/order_translit.py
(the shim's stable sort). Every case runs the host form and the _dev form, the latter with its
outputs on devguard.Guard buffers exactly their capacity long, and, at or below
R.ORDER_ONE_LAUNCH_MAX records, both the one-launch kernel and the radix path (general=True, the
documented MPX_ORDER_GENERAL flag). Shapes are the smallest that reach the edges: a wave's run of
the radix tile is 1024 records, the tile (and the one-launch boundary) 4096, a radix pass 8 key
bits, the key type switches above 32 key bits. The error cases are reported through the error
word or refused before any launch: no case provokes a fault."""
import numpy as np
import pytest

import acceptor_translit as A
import order_translit as O
from devguard import Guard
from go_translit import GoBackend
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError

N = 5
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
ONE = R.ORDER_ONE_LAUNCH_MAX
NAMES = ("records", "perm", "result")


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            if g.shape == ():
                raise AssertionError(f"{what} {name}: got {g} want {w}")
            diff = [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()][:5]
            raise AssertionError(f"{what} {name} differs at {diff}: got {g[diff]} want {w[diff]}")


def dev_buffers(e, ar, case, want_perm=True, src_shift=False, out_misalign=0):
    """the case's sources on the device and guarded outputs; returns (srcs, guards)"""
    srcs = []
    arrivals = case["arrivals"] or [None] * len(case["sources"])
    for s, a in zip(case["sources"], arrivals):
        if src_shift and len(s):  # the records start 16 bytes into their buffer
            d = ar.put(np.concatenate([np.zeros(1, s.dtype), s]))
            d_recs = d.at(1)
        else:
            d_recs = ar.put(s).ptr if len(s) else None
        d_arr = ar.put(a).ptr if a is not None and len(s) else None
        srcs.append((d_recs, d_arr, len(s)))
    n = sum(len(s) for s in case["sources"])
    dt = case["sources"][0].dtype if case["sources"] else R.ACCEPT_REPLY
    g_out = Guard(ar, n, dt, shift=out_misalign)
    g_perm = Guard(ar, n, np.uint32) if want_perm else None
    g_res = Guard(ar, 1, R.ORDER_RESULT)
    return srcs, (g_out, g_perm, g_res)


def run_dev(e, ar, case, general=False, want_perm=True, src_shift=False, stream=None):
    srcs, (g_out, g_perm, g_res) = dev_buffers(e, ar, case, want_perm, src_shift)
    n = sum(x[2] for x in srcs)
    e.order_records_reserve(n, case["n_inst"])
    e.order_records_dev(srcs, case["n_inst"], case["inst_base"], case["arrival_bits"], g_out.ptr,
                        g_perm.ptr if g_perm else None, g_res.ptr, general=general, stream=stream)
    e.synchronize()
    return (g_out.assert_margins(), g_perm.assert_margins() if g_perm else None,
            g_res.assert_margins()[0])


def check(e, case, want_perm=True, src_shift=False, paths=None):
    """host and _dev form on every path the size allows, against the transliteration"""
    want = O.order_records(**case)
    n = len(want[0])
    if paths is None:
        paths = (False, True) if n <= ONE else (True,)
    for general in paths:
        what = f"n={n} general={general}"
        got = e.order_records(case["sources"], case["n_inst"], case["inst_base"], case["arrivals"],
                              case["arrival_bits"], want_perm=want_perm, general=general)
        same(got, want if want_perm else (want[0], None, want[2]), "host " + what)
        with Arena(e) as ar:
            got = run_dev(e, ar, case, general, want_perm, src_shift)
            same(got, want if want_perm else (want[0], None, want[2]), "dev " + what)
    return want


def mk_case(seed, n, n_inst, n_src=3, base=0, bits=0, dtype=R.ACCEPT_REPLY, inst=None):
    """n records over the window, split at random into n_src sources (some may be empty)"""
    rng = np.random.default_rng(seed)
    if inst is None:
        inst = base + rng.integers(0, n_inst, n)
        if n >= 2:  # both ends of the window
            inst[rng.integers(0, n)] = base
            inst[rng.integers(0, n)] = base + n_inst - 1
    cuts = np.sort(rng.integers(0, n + 1, n_src - 1))
    b = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    srcs = [O.records(dtype, inst[b[s]:b[s + 1]], rng=rng) for s in range(n_src)]
    arr = None
    if bits:
        arr = [rng.integers(0, 1 << bits, len(s), dtype=np.uint64).astype(np.uint32) for s in srcs]
    return dict(sources=srcs, n_inst=n_inst, inst_base=base, arrivals=arr, arrival_bits=bits)


@pytest.fixture
def eng(mk_engine):
    return mk_engine(N, MIN)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(O.KAT))
def test_known_answers(eng, name):
    for dtype in (R.ACCEPT_REPLY, R.ACCEPT_MSG):
        case, (perm, n_runs, lo, hi, ordered) = O.kat_case(name, dtype)
        _, got_perm, res = check(eng, case)
        assert got_perm.tolist() == perm and int(res["flags"]) == ordered


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                               8193, 12289])
def test_record_counts(eng, n):
    """a wave's run (1024), the tile and the one-launch boundary (4096), more than one tile"""
    check(eng, mk_case(n, n, max(1, n // 3), dtype=R.ACCEPT_REPLY if n & 1 else R.ACCEPT_MSG))
    check(eng, mk_case(n + 1, n, 300, bits=9), want_perm=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst", [1, 2, 255, 256, 257, 65536, 65537])
def test_window_sizes_step_the_pass_count(eng, n_inst):
    check(eng, mk_case(n_inst, 3000, n_inst))
    check(eng, mk_case(n_inst, 5000, n_inst, dtype=R.ACCEPT_MSG))


@pytest.mark.gpu
@pytest.mark.parametrize("n_inst,bits", [(2, 31), (3, 31), (1 << 31, 1), ((1 << 31) + 1, 1),
                                         (1 << 32, 0), (1 << 32, 1), (1, 0), (1, 1), (1, 31),
                                         (1, 32), (1 << 20, 12), (1 << 20, 13)])
def test_key_widths(eng, n_inst, bits):
    """ceil(log2(n_inst)) + arrival_bits of 32 and 33 is where the key type switches"""
    base = -(1 << 31) if n_inst > 1 << 30 else -5
    wide = O.key_bits(n_inst, bits) > 32
    assert wide == ((n_inst, bits) in [(3, 31), ((1 << 31) + 1, 1), (1 << 32, 1), (1 << 20, 13)])
    for n in (700, 5000):
        check(eng, mk_case(n + bits, n, n_inst, base=base, bits=bits))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3000, 6000])
def test_instance_distributions(eng, n):
    one = mk_case(1, n, 50, inst=np.full(n, 17))
    assert int(check(eng, one)[2]["n_runs"]) == 1
    desc = mk_case(2, n, n, inst=np.arange(n)[::-1].copy())
    res = check(eng, desc)[2]
    assert int(res["n_runs"]) == n and not int(res["flags"])
    up = np.sort(np.random.default_rng(3).integers(0, n // 2, n))
    assert int(check(eng, mk_case(3, n, n // 2, inst=up))[2]["flags"]) == R.ORD_WAS_ORDERED
    k = int(np.flatnonzero(np.diff(up) > 0)[len(up) // 3])  # one swap across a group boundary
    up[k], up[k + 1] = up[k + 1], up[k]
    assert int(check(eng, mk_case(3, n, n // 2, inst=up))[2]["flags"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [1, 2, 15, 16])
def test_source_counts_and_empty_sources(eng, n_src):
    for n in (900, 4500):
        case = mk_case(n_src, n, 211, n_src=n_src, bits=7)
        check(eng, case)
        if n_src == 1:
            continue
        for empty in ({0}, {n_src - 1}, {n_src // 2}, {0, n_src // 2, n_src - 1}):
            keep = [s for i, s in enumerate(case["sources"]) if i not in empty]
            karr = [a for i, a in enumerate(case["arrivals"]) if i not in empty]
            srcs, arrs = [], []
            for i in range(n_src):  # the kept sources around empty ones at the named places
                if i in empty or not keep:
                    srcs.append(np.zeros(0, R.ACCEPT_REPLY))
                    arrs.append(np.zeros(0, np.uint32))
                else:
                    srcs.append(keep.pop(0))
                    arrs.append(karr.pop(0))
            check(eng, dict(case, sources=srcs, arrivals=arrs), paths=(n > ONE,))


@pytest.mark.gpu
def test_source_that_starts_16_bytes_into_its_buffer(eng):
    for n in (1500, 5000):
        check(eng, mk_case(8, n, 97, n_src=4, dtype=R.ACCEPT_MSG), src_shift=True)


@pytest.mark.gpu
@pytest.mark.parametrize("base,n_inst", [(-1000, 600), (-(1 << 31), 77), (0x7FFFFFFF - 999, 1000),
                                         (0x7FFFFFFF, 1)])
def test_window_positions(eng, base, n_inst):
    for n in (800, 4200):
        want = check(eng, mk_case(n, n, n_inst, base=base))
        assert (int(want[2]["lo"]), int(want[2]["hi"])) == (base, base + n_inst - 1)


@pytest.mark.gpu
def test_reply_padding_bytes_are_copied(eng):
    case = mk_case(5, 2000, 64, dtype=R.ACCEPT_REPLY)
    assert all(s["pad"].any() for s in case["sources"] if len(s))
    out, _, _ = check(eng, case)
    assert out["pad"].any()


def _code(fn, *a, **kw):
    with pytest.raises(MpxError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1200, 5000])
def test_out_of_window_records_are_reported_not_followed(eng, n):
    """one record just below and one just above the window: MPX_E_NIL_INSTANCE from the host
    form's check and, in the _dev form, through the error word; the kernels' indices stay in
    bounds (the guards' margins are read back)"""
    e = eng
    base, n_inst = 100, 500
    good = mk_case(9, n, n_inst, base=base, bits=3)
    for bad in (base - 1, base + n_inst, -(1 << 31), 0x7FFFFFFF):
        case = dict(good, sources=[s.copy() for s in good["sources"]])
        big = max(case["sources"], key=len)
        big["instance"][len(big) // 2] = bad
        for general in (False, True):
            assert _code(e.order_records, case["sources"], n_inst, base, case["arrivals"], 3,
                         general=general) == R.E_NIL_INSTANCE
            with Arena(e) as ar:
                srcs, (g_out, g_perm, g_res) = dev_buffers(e, ar, case)
                e.order_records_reserve(n, n_inst)
                e.order_records_dev(srcs, n_inst, base, 3, g_out.ptr, g_perm.ptr, g_res.ptr,
                                    general=general)
                assert _code(e.synchronize) == R.E_NIL_INSTANCE
                for g in (g_out, g_perm, g_res):
                    g.assert_margins()
    check(e, good)  # the engine is usable afterwards


@pytest.mark.gpu
def test_argument_errors(eng):
    e = eng
    r = O.records(R.ACCEPT_REPLY, [4, 5, 6])
    a = np.array([1, 2, 3], np.uint32)
    assert _code(e.order_records, [r] * 17, 8) == R.E_INVAL
    assert _code(e.order_records, [r, r], 8, 0, [a, None], 2) == R.E_INVAL
    assert _code(e.order_records, [r], 8, 0, [a], 1) == R.E_INVAL      # key 2, 3 >= 2^1
    assert _code(e.order_records, [r], 8, 0, None, 3) == R.E_INVAL     # bits without keys
    assert _code(e.order_records, [r], 8, 0, [a], 0) == R.E_INVAL      # keys without bits
    assert _code(e.order_records, [r], 8, 0, [a], 33) == R.E_INVAL
    assert _code(e.order_records, [r], 0) == R.E_INVAL
    assert _code(e.order_records, [r], 8, 0x7FFFFFFF - 6) == R.E_INVAL
    res = _lib.MpxOrderResult()
    src = (_lib.MpxOrderSrc * 1)()
    assert e.lib.mpx_order_records(e.h, src, 0, 8, 0, 0, 2, None, None, res) == R.E_INVAL  # flags
    assert e.lib.mpx_order_records(e.h, src, 0, 8, 0, 0, 0, None, None, None) == R.E_INVAL
    with Arena(e) as ar:
        d = ar.put(np.concatenate([r, r]))
        g_out, g_res = Guard(ar, 4, R.ACCEPT_REPLY), Guard(ar, 1, R.ORDER_RESULT)
        d_arr = ar.put(np.arange(4, dtype=np.uint32))
        e.order_records_reserve(16, 8)
        ok = [(d.ptr, None, 3)]
        assert _code(e.order_records_dev, [(d.ptr + 4, None, 3)], 8, 0, 0, g_out.ptr, None,
                     g_res.ptr) == R.E_INVAL
        assert _code(e.order_records_dev, ok, 8, 0, 0, g_out.ptr + 4, None, g_res.ptr) == R.E_INVAL
        assert _code(e.order_records_dev, ok, 8, 0, 0, g_out.ptr, g_out.ptr + 2,
                     g_res.ptr) == R.E_INVAL
        assert _code(e.order_records_dev, ok, 8, 0, 0, g_out.ptr, None, g_res.ptr + 4) == R.E_INVAL
        assert _code(e.order_records_dev, [(d.ptr, d_arr.ptr + 2, 3)], 8, 0, 4, g_out.ptr, None,
                     g_res.ptr) == R.E_INVAL
        assert _code(e.order_records_dev, ok * 17, 8, 0, 0, g_out.ptr, None,
                     g_res.ptr) == R.E_INVAL
        assert _code(e.order_records_dev, ok, 8, 0, 0, g_out.ptr, None, None) == R.E_INVAL
        e.synchronize()
        g_out.assert_untouched([(0, 4)])
        g_res.assert_untouched([(0, 1)])
    check(e, mk_case(1, 100, 8))


@pytest.mark.gpu
def test_dev_form_needs_its_reserve_and_never_grows(mk_engine):
    e = mk_engine(N, CLASSIC)
    case = mk_case(4, 6000, 100)
    with Arena(e) as ar:
        srcs, (g_out, g_perm, g_res) = dev_buffers(e, ar, case)
        args = (srcs, 100, 0, 0, g_out.ptr, g_perm.ptr, g_res.ptr)
        with pytest.raises(MpxError) as ei:
            e.order_records_dev(*args)
        assert ei.value.code == R.E_INVAL and "mpx_order_records_reserve" in str(ei.value)
        e.order_records_reserve(100, 100)
        assert _code(e.order_records_dev, *args) == R.E_INVAL
        e.order_records_dev([], 100, 0, 0, None, None, g_res.ptr)  # no record: no scratch
        e.synchronize()
        assert int(g_res.assert_margins()[0]["hi"]) == -1
        g_out.assert_untouched([(0, 6000)])
    check(e, case)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", O.FUZZ_SEEDS)
def test_fuzz(eng, seed):
    check(eng, O.fuzz_order(seed), want_perm=seed % 5 != 4)


# ---- closed loops: what the stations before emit, ordered on the device, is what the handlers
# take -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_followers_replies_ordered_on_device_feed_the_tally(mk_engine, mode):
    """the loop of test_followers_feed_the_leaders_tally without a host sort: four followers'
    mpx_accept_handle replies as four sources, ordered, then mpx_accept_tally_dev"""
    e = mk_engine(N, mode)
    rng = np.random.default_rng(40)
    n_inst, D = 600, 16
    got_rep, want_rep = [], []
    for f in range(1, N):
        runs = rng.integers(1, 3, n_inst).tolist()
        case = list(A.case_from_runs(rng, np.arange(n_inst), runs, n_inst, n_inst, 0, N))
        case[2] = A.mk_groups([(D if f < 4 else 2 * D, f)])
        case[0]["ballot"], case[0]["leader_id"] = D, 0
        case[1]["ballot"] = D + 16 * rng.integers(-1, 2, n_inst)
        want = A.accept_handle(mode, N, *case)
        got = e.accept_handle(*case)
        # each connection delivers its replies in its own arrival order
        order = np.random.default_rng(41 + f).permutation(len(got[1]))
        got_rep.append(got[1][order][(got[3][order] & R.AH_REPLIED) != 0])
        want_rep.append(want[1][order][(want[3][order] & R.AH_REPLIED) != 0])
    lst = np.zeros(n_inst, R.INST_STATE)
    lst["status"] = rng.choice([R.PREPARED, R.ACCEPTED, R.COMMITTED], n_inst, p=[.45, .45, .1])
    batch, _, w_res = O.order_records(want_rep, n_inst)
    w_st, w_cu, w_pc, w_dec = GoBackend(N, mode).accept_tally(batch, lst, 0, -1)
    n = len(batch)
    assert n > n_inst and w_dec.any() and not int(w_res["flags"])
    with Arena(e) as ar:
        srcs = [(ar.put(r).ptr, None, len(r)) for r in got_rep]
        g_out, g_res = Guard(ar, n, R.ACCEPT_REPLY), Guard(ar, 1, R.ORDER_RESULT)
        d_st = ar.put(lst)
        g_st, g_dec = Guard(ar, n_inst, R.INST_STATE), Guard(ar, n_inst, np.uint8)
        g_sc = Guard(ar, 1 + N, np.int32).put(np.concatenate([[-1], np.zeros(N)]).astype(np.int32))
        e.order_records_reserve(n, n_inst)
        e.order_records_dev(srcs, n_inst, 0, 0, g_out.ptr, None, g_res.ptr)
        e.accept_tally_dev(g_out.ptr, n, d_st.ptr, g_st.ptr, n_inst, 0, g_sc.ptr, g_dec.ptr)
        e.synchronize()
        assert g_out.assert_margins().tobytes() == batch.tobytes()
        assert g_res.assert_margins()[0].tobytes() == w_res.tobytes()
        sc = g_sc.assert_margins()
        assert g_st.assert_margins().tobytes() == w_st.tobytes()
        assert np.array_equal(g_dec.assert_margins(), w_dec)
        assert int(sc[0]) == w_cu and np.array_equal(sc[1:], w_pc)


@pytest.mark.gpu
def test_graph_capture_of_order_then_tally(mk_engine):
    """order -> tally captured with mpx_graph_begin / mpx_graph_end and replayed on two inputs
    (one per path size: the captured call keeps its sizes, so two graphs of two replays each)"""
    e = mk_engine(N, MIN)
    n_inst = 500
    for n in (3000, 7000):
        rng = np.random.default_rng(n)
        inputs = []
        for k in range(2):
            inst = rng.integers(0, n_inst, n)
            recs = O.records(R.ACCEPT_REPLY, inst)
            recs["ballot"], recs["ok"], recs["id"] = 16, rng.integers(0, 2, n), rng.integers(1, N, n)
            parts = [recs[:n // 3], recs[n // 3:n // 2], recs[n // 2:]]
            st = np.zeros(n_inst, R.INST_STATE)
            st["status"] = rng.choice([R.PREPARED, R.ACCEPTED], n_inst)
            st["max_recv_ballot"] = 16
            batch, perm, res = O.order_records(parts, n_inst)
            inputs.append((parts, st, batch, perm, res,
                           GoBackend(N, MIN).accept_tally(batch, st, 0, -1)))
        sizes = [len(p) for p in inputs[0][0]]
        with Arena(e) as ar:
            d_parts = [ar.empty(k, R.ACCEPT_REPLY) for k in sizes]
            d_st = ar.empty(n_inst, R.INST_STATE)
            g_out, g_perm = Guard(ar, n, R.ACCEPT_REPLY), Guard(ar, n, np.uint32)
            g_res = Guard(ar, 1, R.ORDER_RESULT)
            g_st, g_dec = Guard(ar, n_inst, R.INST_STATE), Guard(ar, n_inst, np.uint8)
            g_sc = Guard(ar, 1 + N, np.int32)
            sc0 = ar.put(np.concatenate([[-1], np.zeros(N)]).astype(np.int32))
            e.order_records_reserve(n, n_inst)
            s = e.stream_create()
            e.graph_begin(s)
            e.order_records_dev([(d.ptr, None, k) for d, k in zip(d_parts, sizes)], n_inst, 0, 0,
                                g_out.ptr, g_perm.ptr, g_res.ptr, stream=s)
            e.accept_tally_dev(g_out.ptr, n, d_st.ptr, g_st.ptr, n_inst, 0, g_sc.ptr, g_dec.ptr, s)
            g = e.graph_end(s)
            try:
                for parts, st, batch, perm, res, (w_st, w_cu, w_pc, w_dec) in inputs + inputs[:1]:
                    for d, p in zip(d_parts, parts):
                        src = ar.put(p, s)
                        e.memcpy(d.ptr, src.ptr, src.nbytes, D2D, s)
                    src = ar.put(st, s)
                    e.memcpy(d_st.ptr, src.ptr, src.nbytes, D2D, s)
                    e.memcpy(g_sc.ptr, sc0.ptr, sc0.nbytes, D2D, s)
                    for x in (g_out, g_perm, g_res, g_st, g_dec):
                        x.fill(s)
                    # (the tally stores st_out only for instances that have records)
                    e.memcpy(g_st.ptr, src.ptr, src.nbytes, D2D, s)
                    e.graph_launch(g, s)
                    e.stream_synchronize(s)
                    same((g_out.assert_margins(), g_perm.assert_margins(),
                          g_res.assert_margins()[0]), (batch, perm, res), f"replay n={n}")
                    sc = g_sc.assert_margins()
                    assert g_st.assert_margins().tobytes() == w_st.tobytes()
                    assert np.array_equal(g_dec.assert_margins(), w_dec)
                    assert int(sc[0]) == w_cu and np.array_equal(sc[1:], w_pc)
            finally:
                e.graph_destroy(g)
                e.stream_destroy(s)
            e.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_two_leaders_accepts_ordered_on_device_feed_the_acceptor(mk_engine, mode):
    """two leaders' Accept runs: decode_stream -> unmarshal_frames per connection, the two record
    lists ordered on the device, then mpx_accept_handle_dev and mpx_encode_accept_replies_dev on
    the ordered batch, against acceptor_translit on the transliteration's batch"""
    import unmarshal_translit as U
    from minpaxos_amd import wire as W
    e = mk_engine(N, mode)
    rng = np.random.default_rng(90)
    base, n_inst, D = 1000, 400, 32
    runs, w_msgs, g_msgs = [], [], []
    for leader in (0, 1):  # each leader's Accepts arrive in its own (not ascending) order
        insts = base + rng.permutation(n_inst)[:300]
        frames = [W.accept(mode, leader, int(i), D + leader, [(1, int(i), 7)] * int(rng.integers(0, 3)),
                           base - 1, []) for i in insts]
        run = b"".join(frames)
        _, _, var, _, res = e.decode_stream(run)
        assert int(res["stop_reason"]) == R.DECODE_END and len(var) == len(insts)
        um, _ = e.unmarshal_frames(run, var)
        want, _ = U.expected(mode, run, U.walk(mode, run)[0])
        g_msgs.append(um["accepts"])
        w_msgs.append(want["accepts"])
        assert g_msgs[-1]["instance"].tolist() == insts.tolist()
    st = A.mk_state([(A.NIL, 0, 0, 0)] * n_inst)
    acc = rng.random(n_inst) < 0.4
    st["status"][acc], st["ballot"][acc], st["value_id"][acc] = R.ACCEPTED, D, 5
    groups = A.mk_groups([(D, 3)])
    batch, _, w_res = O.order_records(w_msgs, n_inst, base)
    w_st, w_rep, w_to, w_eff = A.accept_handle(mode, N, batch, st, groups, base, n_inst)
    w_out, w_off = A.encode_accept_replies(mode, w_rep, w_to, N)
    n = len(batch)
    assert int(w_res["n_runs"]) < n  # some instances hear from both leaders
    with Arena(e) as ar:
        srcs = [(ar.put(m).ptr, None, len(m)) for m in g_msgs]
        g_bat, g_res = Guard(ar, n, R.ACCEPT_MSG), Guard(ar, 1, R.ORDER_RESULT)
        d_st, d_grp = ar.put(st), ar.put(groups)
        g_st = Guard(ar, n_inst, R.ACCEPTOR_STATE).put(st)
        g_rep, g_to = Guard(ar, n, R.ACCEPT_REPLY), Guard(ar, n, np.int32)
        g_eff = Guard(ar, n, np.uint8)
        g_out, g_off = Guard(ar, len(w_out), np.uint8), Guard(ar, N + 1, np.uint64)
        e.order_records_reserve(n, n_inst)
        e.encode_accept_replies_reserve(n)
        e.order_records_dev(srcs, n_inst, base, 0, g_bat.ptr, None, g_res.ptr)
        e.accept_handle_dev(g_bat.ptr, n, d_st.ptr, g_st.ptr, n_inst, base, d_grp.ptr, 1, n_inst,
                            g_rep.ptr, g_to.ptr, g_eff.ptr)
        e.encode_accept_replies_dev(g_rep.ptr, g_to.ptr, n, N, g_out.ptr, g_off.ptr)
        e.synchronize()
        assert g_bat.assert_margins().tobytes() == batch.tobytes()
        assert g_res.assert_margins()[0].tobytes() == w_res.tobytes()
        assert g_st.assert_margins().tobytes() == w_st.tobytes()
        assert g_rep.assert_margins().tobytes() == w_rep.tobytes()
        assert np.array_equal(g_to.assert_margins(), w_to)
        assert np.array_equal(g_eff.assert_margins(), w_eff)
        assert np.array_equal(g_off.assert_margins(), np.asarray(w_off, np.uint64))
        assert g_out.assert_margins().tobytes() == bytes(w_out)


@pytest.mark.gpu
def test_commits_and_commit_shorts_merged_by_stream_offset_feed_the_commit_handler(mk_engine):
    """one stream of Commits and CommitShorts: mpx_unmarshal_frames' Commits and
    mpx_gather_commit_shorts' records as two sources with their frames' stream offsets as
    arrival keys, ordered, then mpx_commit_handle, against commit_translit on the batch merged by
    offset and stably sorted by instance"""
    import struct

    import commit_translit as CT
    from minpaxos_amd import wire as W
    from proposer_translit import nil_state
    e = mk_engine(N, MIN)
    rng = np.random.default_rng(91)
    base, ipg, G, D = 500, 64, 5, 48
    n_inst = ipg * G
    frames = []
    for k in range(700):  # an instance may see a CommitShort and a Commit, in either order
        i = base + int(rng.integers(0, n_inst))
        if rng.random() < 0.5:
            frames.append(W.commit(1, i, D, [(1, i, k)] * int(rng.integers(0, 3))))
        else:
            frames.append(bytes([R.PEER_COMMIT_SHORT]) + struct.pack("<iiii", 1, i, 1, D))
        if k % 9 == 0:
            frames.append(W.accept_reply(MIN, i, 1, D, 2))
    run = b"".join(frames)
    _, _, var, oth, res = e.decode_stream(run)
    assert int(res["stop_reason"]) == R.DECODE_END
    um, _ = e.unmarshal_frames(run, var)
    commits = um["commits"]
    shorts, cnt, idx, ns = e.gather_commit_shorts(run, oth)
    assert len(commits) > 200 and ns == len(shorts) > 200
    # the shim fills arrival: var[k].offset for the k-th Commit, other[frame_index].offset for
    # a CommitShort
    arr_c = var["offset"][var["code"] == R.PEER_COMMIT].astype(np.uint32)
    arr_s = oth["offset"][idx].astype(np.uint32)
    bits = len(run).bit_length()
    offs = np.concatenate([arr_c, arr_s])
    merged = np.concatenate([commits, shorts])[np.argsort(offs, kind="stable")]
    merged = merged[np.argsort(merged["instance"], kind="stable")]
    for general in (False, True):
        batch, perm, r = e.order_records([commits, shorts], n_inst, base, [arr_c, arr_s], bits,
                                         general=general)
        same((batch, perm, r), O.order_records([commits, shorts], n_inst, base, [arr_c, arr_s],
                                               bits), "commit merge")
        assert batch.tobytes() == merged.tobytes()
        st = nil_state(n_inst)
        cu = (base + np.arange(G) * ipg - 1).astype(np.int32)
        got = e.commit_handle(batch, st, cu, base, ipg)
        want = CT.commit_handle(merged, st, cu, base, ipg)
        for g, w in zip(got, want):
            assert np.asarray(g).tobytes() == np.asarray(w).tobytes()

"""GPU tests of reply assembly (mpx_build_replies, mpx_build_replies_dev): the client reply records
of a batch of handlePropose slots, bit-exact against tests/reply_translit.py (the three Go reply
loops over Go-shaped objects). Every case runs the host form and the _dev form, the latter with its
outputs on devguard.Guard buffers exactly their capacity long, and, whenever the call is within
the one-launch bounds, both the one-launch kernel and the general path (general=True, the
documented MPX_RB_GENERAL flag) against the same bytes. Shapes are the smallest that reach the
edges: pass 1 takes 256 slots per workgroup, the scan 4096 items per tile (over n_sends + 1 items),
the emit pass 1024 records per tile. The error cases are reported through the error word or refused
before any launch: no case provokes a fault."""
import ctypes as C
import struct

import numpy as np
import pytest

import reply_kat
import reply_translit as T
from devguard import Guard
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError

N = 3
TILE = 1024
A, NL, RF, PR = R.PH_ACCEPT, R.PH_NOT_LEADER, R.PH_REFUSED, R.PH_PREPARE


def _code(f, *a, **k):
    try:
        f(*a, **k)
    except MpxError as ex:
        return ex.code
    return R.OK


def mk_case(kind, counts, flags=None, sel=None, base=100, ret_first=None, **extra):
    """slots of counts[s] proposals, laid out back to back; instance base + s; proposal j is
    (timestamp 10^12 + j, id j - 7, client j % 61); EXECUTED: ret[i] = 3 i + 1"""
    n = len(counts)
    flags = [NL if kind == R.RB_FALSE else A] * n if flags is None else flags
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    sends = T.mk_sends([(-1 if flags[s] == NL else base + s, 4, flags[s], int(first[s]), int(counts[s]))
                        for s in range(n)])
    m = int(first[-1])
    meta = np.zeros(m, R.PROPOSAL)
    meta["timestamp"] = 10 ** 12 + np.arange(m)
    meta["command_id"] = np.arange(m) - 7
    meta["client"] = np.arange(m) % 61
    case = dict(kind=kind, sends=sends, meta=meta, inst_base=base, **extra)
    if kind != R.RB_FALSE:
        case["mask"] = np.ones(n, np.uint8) if sel is None else np.asarray(sel, np.uint8)
    if kind == R.RB_EXECUTED:
        n_ret = m if ret_first is None else int(max(int(r) + int(c) for r, c in zip(ret_first, counts))) \
            if n else 0
        case["ret"] = 3 * np.arange(n_ret, dtype=np.int64) + 1
        if ret_first is not None:
            case["ret_first"] = np.asarray(ret_first, np.uint64)
    return case


def run_host(e, case, cap, general, want_cs, with_recs=True):
    return e.build_replies(case["kind"], case["sends"], case["meta"], case.get("mask"),
                           case.get("inst_base", 0), case.get("ret"), case.get("ret_first"),
                           cap=cap, pad_client=case.get("pad_client"), want_commit_sends=want_cs,
                           general=general)


def dev_call(e, ar, case, cap, general, want_cs, shift=0):
    """the call's inputs on the device and its outputs on guards; returns (batch, guards)"""
    sends, meta = case["sends"], case["meta"]
    n = len(sends)
    mask, ret, rf = case.get("mask"), case.get("ret"), case.get("ret_first")
    d = dict(sends=ar.put(sends) if n else None, meta=ar.put(meta) if len(meta) else None,
             mask=None if mask is None else Guard(ar, len(mask), np.uint8, shift=3).put(mask),
             ret=None if ret is None else ar.put(ret),
             rf=None if rf is None else ar.put(rf))
    g = dict(recs=Guard(ar, cap, R.REPLY_REC, shift=shift), cs=Guard(ar, n, R.COMMIT_SEND),
             res=Guard(ar, 1, R.REPLY_RESULT))
    b = e.reply_batch_dev(case["kind"], d["sends"], n, d["meta"], len(meta), d["mask"],
                          0 if mask is None else len(mask), case.get("inst_base", 0), d["ret"],
                          0 if ret is None else len(ret), d["rf"], case.get("pad_client"), general)
    return b, g, d


def read_dev(g, cap, padded, want_cs):
    res = g["res"].assert_margins()[0]
    recs = g["recs"].assert_margins()
    k = cap if padded else min(int(res["n_replies"]), cap)
    g["recs"].assert_untouched([(k, cap)])
    cs = g["cs"].assert_margins()
    if not want_cs:
        g["cs"].assert_untouched([(0, g["cs"].count)])
    return recs[:k], (cs if want_cs else None), res


def run_dev(e, case, cap, general, want_cs, shift=0):
    """returns (recs, commit_sends, res, code of the next synchronising call)"""
    with Arena(e) as ar:
        b, g, d = dev_call(e, ar, case, cap, general, want_cs, shift)
        e.build_replies_reserve(len(case["sends"]))
        e.build_replies_dev(b, g["recs"].ptr if cap else None, cap,
                            g["cs"].ptr if want_cs else None, g["res"].ptr)
        code = _code(e.synchronize)
        if d["mask"] is not None:
            d["mask"].assert_margins()
        return read_dev(g, cap, case.get("pad_client") is not None, want_cs) + (code,)


def same(got, want, want_cs, what):
    recs, cs, res = got[:3]
    assert res.tobytes() == want["res"].tobytes(), (what, res, want["res"])
    if recs.tobytes() != want["recs"].tobytes():
        assert len(recs) == len(want["recs"]), (what, len(recs), len(want["recs"]))
        diff = [i for i in range(len(recs)) if recs[i].tobytes() != want["recs"][i].tobytes()][:5]
        raise AssertionError(f"{what} recs differ at {diff}: got {recs[diff]} want {want['recs'][diff]}")
    if want_cs:
        assert cs.tobytes() == want["commit_sends"].tobytes(), what


def paths_of(case, cap):
    """general = False always; True as well when the default would take the one-launch kernel"""
    one = len(case["sends"]) <= R.RB_ONE_LAUNCH_SLOTS and cap <= R.RB_ONE_LAUNCH_REPLIES
    return (False, True) if one else (False,)


def check(e, case, want_cs=None, forms=("host", "dev"), shifts=(0,)):
    want_cs = case["kind"] != R.RB_FALSE if want_cs is None else want_cs
    total = int(T.build_replies(**{k: v for k, v in case.items() if k not in ("cap", "pad_client")})
                ["res"]["n_replies"])
    cap = case.get("cap", total)
    want = T.build_replies(**dict(case, cap=cap))
    assert want["code"] == R.OK
    for general in paths_of(case, cap):
        if "host" in forms:
            same(run_host(e, case, cap, general, want_cs), want, want_cs, f"host general={general}")
        if "dev" in forms:
            for shift in shifts:
                got = run_dev(e, case, cap, general, want_cs, shift)
                assert got[3] == R.OK
                same(got, want, want_cs, f"dev general={general} shift={shift}")
    return want


@pytest.fixture
def eng(mk_engine):
    return mk_engine(N, R.MODE_MIN)


# ---- the known answers ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", reply_kat.KAT_REPLY, ids=lambda c: c["name"])
def test_known_answers(eng, case):
    want = check(eng, reply_kat.kat_args(case), shifts=(0, 8))
    assert [tuple(int(x) for x in r) for r in want["recs"].tolist()] == case["want"]


# ---- shapes --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_sends", [0, 1, 255, 256, 257, 4094, 4095, 4096, 4097])
def test_slot_counts_around_the_pass_one_workgroup_and_the_scan_tile(eng, n_sends):
    """slots of 0, 1 and 2 commands, two in three selected"""
    s = np.arange(n_sends)
    check(eng, mk_case(R.RB_DECIDED, s % 3, sel=(s % 5 != 1) * (1 + s % 200)))


@pytest.mark.gpu
@pytest.mark.parametrize("total", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_totals_and_slot_boundaries_around_the_emit_tile(eng, total):
    """a slot boundary at every position from 2 before to 2 after a tile boundary, in an output
    that starts on a 16-byte line and in one that starts in the middle of one"""
    edge = TILE if total <= TILE + 1 else 2 * TILE
    for d in (-2, -1, 0, 1, 2):
        k = min(edge + d, total)
        counts = [k - 7, 7, total - k] if k > 7 else [total]
        assert sum(counts) == total
        check(eng, mk_case(R.RB_EXECUTED, counts), shifts=(0, 8))
    check(eng, mk_case(R.RB_FALSE, [1] * total), forms=("dev",))


@pytest.mark.gpu
def test_65536_one_command_slots(eng):
    check(eng, mk_case(R.RB_EXECUTED, [1] * 65536))


@pytest.mark.gpu
@pytest.mark.parametrize("empties", [100, 1500])
def test_one_full_slot_among_empty_ones(eng, empties):
    counts = [0] * empties + [R.PROPOSE_MAX_BATCH] + [0] * empties
    check(eng, mk_case(R.RB_DECIDED, counts), shifts=(0, 8))
    check(eng, mk_case(R.RB_FALSE, counts, flags=[RF] * empties + [NL] + [RF] * empties))


@pytest.mark.gpu
def test_refused_slot_of_5000_answers_once(eng):
    want = check(eng, mk_case(R.RB_FALSE, [5000, 3, 5000], flags=[RF, NL, RF]))
    assert want["recs"]["client"].tolist() == [0, 5000 % 61, 5001 % 61, 5002 % 61, 5003 % 61]


@pytest.mark.gpu
def test_all_slots_unselected(eng):
    counts = [3, 0, 5000, 1] * 3
    want = check(eng, mk_case(R.RB_DECIDED, counts, sel=[0] * 12))
    assert int(want["res"]["n_replies"]) == 0 and not want["commit_sends"]["flags"].any()
    check(eng, mk_case(R.RB_EXECUTED, counts, sel=[0] * 12, cap=TILE + 1, pad_client=61))
    check(eng, mk_case(R.RB_FALSE, counts, flags=[A, PR, A, A] * 3))


# ---- capacity and padding ------------------------------------------------------------------------
@pytest.mark.gpu
def test_capacity_short_and_zero(eng):
    counts = [700, 0, 1, 323, 41, 1300]
    total = sum(counts)
    for cap in (total - 1, TILE, 1, 0):
        check(eng, mk_case(R.RB_EXECUTED, counts, cap=cap), shifts=(0, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 1, TILE + 1])
def test_pad_tail(eng, tail):
    counts = [700, 0, 1, 323, 41, 1300]
    for kind in (R.RB_FALSE, R.RB_DECIDED):
        check(eng, mk_case(kind, counts, sel=[1, 1, 0, 1, 1, 1], cap=sum(counts) - (kind != R.RB_FALSE)
                           + tail, pad_client=61), shifts=(0, 8))
    # a capacity that is already short gets no pad record
    check(eng, mk_case(R.RB_DECIDED, counts, cap=TILE - 3, pad_client=61))


# ---- the other outputs ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_ret_first(eng):
    counts = [5, 0, 1200, 3, 17]
    order = [3, 0, 4, 2, 1]
    rf, at = [0] * 5, 2
    for s in order:
        rf[s] = at
        at += counts[s] + 1
    check(eng, mk_case(R.RB_EXECUTED, counts, sel=[1, 1, 1, 0, 1], ret_first=rf))


@pytest.mark.gpu
def test_a_slot_the_mask_passes_over_reads_no_result(eng):
    """execute_gather -> build_replies(EXECUTED) over slots kept from earlier turns: ret_first puts
    an instance that did not execute where the executed ones before it end, for the last slots
    n_ret itself, so their result range leaves ret. The mask passes over them and they read no
    result: no fault, host and _dev form (the closed-loop test found the two contracts at odds,
    DESIGN §25). Selected, the same slot is the fault it was."""
    counts, base = [3, 2, 4], 100
    inst = np.zeros(3, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"], inst["flags"] = [0, 3, 5], counts, R.IC_HAS_CMDS
    case = mk_case(R.RB_EXECUTED, counts, base=base)
    cmds = (np.ones(9, np.uint8), np.arange(9, dtype=np.int64), np.arange(9, dtype=np.int64))
    x = eng.execute_gather(inst, [base], [base - 1], cmds, base, 3, sends=case["sends"])
    assert x["mask"].tolist() == [1, 0, 0] and x["ret_first"].tolist() == [0, 3, 3] and len(x["op"]) == 3
    case.update(mask=x["mask"], ret_first=x["ret_first"], ret=case["ret"][:3])
    want = check(eng, case)
    assert want["recs"]["value"].tolist() == [1, 4, 7] and int(want["res"]["n_slots"]) == 1
    bad = dict(case, mask=np.array([1, 0, 1], np.uint8))
    assert T.build_replies(**bad)["code"] == R.E_INVAL
    assert _code(run_host, eng, bad, 7, False, True) == R.E_INVAL
    got = run_dev(eng, bad, 7, False, True)
    assert got[3] == R.E_INVAL and got[0]["value"].tolist() == [1, 4, 7]
    check(eng, mk_case(R.RB_DECIDED, [2, 3]))


@pytest.mark.gpu
def test_commit_sends_with_and_without_recs(eng):
    counts = [5, 0, 1200, 3, 17]
    for kind in (R.RB_DECIDED, R.RB_EXECUTED):
        case = mk_case(kind, counts, flags=[A, A, PR, NL, RF], sel=[1, 0, 1, 1, 1])
        check(eng, case, want_cs=True)
        check(eng, case, want_cs=False)
        want = check(eng, dict(case, cap=0), want_cs=True)  # no recs at all
        assert want["commit_sends"]["flags"].tolist() == [1, 0, 1, 0, 0]


# ---- rejections ----------------------------------------------------------------------------------
def _faulty(fault):
    counts = [4, 2, 6, 0, 3, 1200]
    if fault == "commands":
        case = mk_case(R.RB_DECIDED, counts)
        case["sends"]["n_cmds"][2] = 2000            # past n_props
        return case, R.E_INVAL
    if fault == "first_cmd":
        case = mk_case(R.RB_FALSE, counts)
        case["sends"]["first_cmd"][4] = 1 << 40
        return case, R.E_INVAL
    if fault == "results":
        rf = [0, 4, 6, 12, 12, 15]
        case = mk_case(R.RB_EXECUTED, counts, ret_first=rf)
        case["ret_first"][1] = len(case["ret"]) - 1   # two results wanted, one left
        return case, R.E_INVAL
    case = mk_case(R.RB_DECIDED, counts, sel=[1, 1, 1, 1, 0, 1])
    if fault == "below_window":
        case["sends"]["instance"][0] = case["inst_base"] - 1
    else:
        case["sends"]["instance"][4] = case["inst_base"] + len(counts)
    return case, R.E_NIL_INSTANCE


@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["commands", "first_cmd", "results", "below_window", "above_window"])
def test_faulty_slot_by_error_word_and_by_code(eng, fault):
    """the host form answers before any launch; the _dev form raises the error word, the slot emits
    nothing, its commit_sends flags are 0 and the neighbouring slots are exact"""
    case, code = _faulty(fault)
    want_cs = case["kind"] != R.RB_FALSE
    assert T.build_replies(**case)["code"] == code
    want = T.build_replies(dev=True, **case)
    assert want["code"] == code and int(want["res"]["n_slots"]) >= 4
    cap = int(want["res"]["n_replies"])
    for general in (False, True):
        assert _code(run_host, eng, case, cap, general, want_cs) == code
        got = run_dev(eng, case, cap, general, want_cs)
        assert got[3] == code
        same(got, want, want_cs, f"dev general={general}")
    # the handle is clean again
    check(eng, mk_case(R.RB_DECIDED, [2, 3]))


@pytest.mark.gpu
def test_argument_rejections(eng):
    e = eng
    case = mk_case(R.RB_EXECUTED, [2, 3])
    res = _lib.MpxReplyResult()
    recs = np.zeros(8, R.REPLY_REC)
    cs = np.zeros(2, R.COMMIT_SEND)
    keep = [case["sends"], case["meta"], case["mask"], case["ret"], np.zeros(2, np.uint64)]
    ptr = [x.ctypes.data_as(C.c_void_p) for x in keep]

    def host(kind=R.RB_EXECUTED, flags=0, reserved=0, mask=True, ret=True, rf=False, with_cs=True,
             n_sends=2, sends=True, meta=True, with_res=True, with_recs=True):
        b = _lib.MpxReplyBatch(ptr[0] if sends else None, n_sends, 100, 2, ptr[1] if meta else None,
                               5, ptr[2] if mask else None, ptr[3] if ret else None, 5,
                               ptr[4] if rf else None, kind, flags, R.RB_NO_PAD, reserved)
        return e.lib.mpx_build_replies(e.h, C.byref(b), recs.ctypes.data_as(C.c_void_p) if with_recs
                                       else None, 8, cs.ctypes.data_as(C.c_void_p) if with_cs else
                                       None, C.byref(res) if with_res else None)
    assert host() == R.OK and res.n_replies == 5
    assert host(sends=False) == R.E_INVAL and host(meta=False) == R.E_INVAL
    assert host(with_res=False) == R.E_INVAL and host(with_recs=False) == R.E_INVAL
    assert e.lib.mpx_build_replies(e.h, None, None, 0, None, C.byref(res)) == R.E_INVAL
    assert host(kind=0) == R.E_INVAL and host(kind=4) == R.E_INVAL
    assert host(flags=2) == R.E_INVAL and host(reserved=1) == R.E_INVAL
    assert host(ret=False) == R.E_INVAL                                   # EXECUTED needs ret
    assert host(kind=R.RB_DECIDED) == R.E_INVAL                           # ... DECIDED forbids it
    assert host(kind=R.RB_DECIDED, ret=False, rf=True) == R.E_INVAL
    assert host(kind=R.RB_DECIDED, ret=False) == R.OK
    for bad in (dict(), dict(mask=False), dict(mask=False, ret=False),
                dict(mask=False, ret=False, rf=True, with_cs=False),
                dict(ret=False, with_cs=False), dict(mask=False, with_cs=False)):
        assert host(kind=R.RB_FALSE, **bad) == R.E_INVAL, bad
    assert host(kind=R.RB_FALSE, mask=False, ret=False, with_cs=False) == R.OK
    assert host(n_sends=0xFFFFFFFF) == R.E_UNSUPPORTED
    assert _code(e.build_replies_reserve, 0xFFFFFFFF) == R.E_UNSUPPORTED
    # the device form's alignment rules
    with Arena(e) as ar:
        b, g, d = dev_call(e, ar, dict(case, ret_first=np.array([0, 2], np.uint64)), 8, False, True)
        e.build_replies_reserve(2)

        def dev(field=None, by=0, recs=0, cs=0, res=0):
            x = _lib.MpxReplyBatch.from_buffer_copy(b)
            if field:
                setattr(x, field, getattr(x, field) + by)
            return _code(e.build_replies_dev, x, g["recs"].ptr + recs, 8, g["cs"].ptr + cs,
                         g["res"].ptr + res)
        assert dev("sends", 8) == R.E_INVAL and dev("meta", 8) == R.E_INVAL
        assert dev("ret", 4) == R.E_INVAL and dev("ret_first", 4) == R.E_INVAL
        assert dev(recs=4) == R.E_INVAL and dev(cs=8) == R.E_INVAL and dev(res=4) == R.E_INVAL
        e.synchronize()
        for x in g.values():
            x.assert_margins()
            x.assert_untouched([(0, x.count)])
        assert dev("mask", 1) == R.OK and dev(recs=0) == R.OK  # the mask may sit anywhere
        e.synchronize()
    del keep


@pytest.mark.gpu
def test_dev_form_needs_its_reserve_and_never_grows(mk_engine):
    e = mk_engine(N, R.MODE_CLASSIC)
    small, big = mk_case(R.RB_DECIDED, [2, 3]), mk_case(R.RB_DECIDED, [1] * 3000)
    with Arena(e) as ar:
        b, g, _ = dev_call(e, ar, small, 5, False, True)
        args = (b, g["recs"].ptr, 5, g["cs"].ptr, g["res"].ptr)
        with pytest.raises(MpxError) as ei:
            e.build_replies_dev(*args)
        assert ei.value.code == R.E_INVAL and "mpx_build_replies_reserve" in str(ei.value)
        # no slot: no scratch; the pad tail is still written
        none = e.reply_batch_dev(R.RB_DECIDED, None, 0, None, 0, pad_client=7)
        e.build_replies_dev(none, g["recs"].ptr, 5, None, g["res"].ptr)
        e.synchronize()
        assert g["res"].assert_margins()[0].tolist() == (0, 0)
        assert g["recs"].assert_margins()["client"].tolist() == [7] * 5
        g["cs"].assert_untouched([(0, 2)])
        e.build_replies_reserve(2)
        e.build_replies_dev(*args)
        e.synchronize()
        b2, g2, _ = dev_call(e, ar, big, 3000, False, True)
        assert _code(e.build_replies_dev, b2, g2["recs"].ptr, 3000, g2["cs"].ptr, g2["res"].ptr) == \
            R.E_INVAL
        e.synchronize()
        g2["recs"].assert_untouched([(0, 3000)])
    check(e, big)


# ---- fuzz ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_fuzz(eng, seed):
    check(eng, T.fuzz_case(seed), shifts=(8 * (seed & 1),))


# ---- chains --------------------------------------------------------------------------------------
def _reply_bytes(recs, n_clients):
    """per client, ProposeReplyTS.Marshal of its records in order (OK = 1, Leader = 0)"""
    runs = [b""] * n_clients
    for r in recs:
        runs[int(r["client"])] += struct.pack("<Biqqi", 1, int(r["command_id"]), int(r["value"]),
                                              int(r["timestamp"]), 0)
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True])
def test_graph_from_client_bytes_to_reply_and_commit_bytes(mk_engine, general):
    """decode_client_streams_dev -> propose_handle_dev -> accept_tally_dev on given replies ->
    build_replies_dev (DECIDED, padded, with commit_sends) -> encode_replies_dev(n = cap,
    n_clients + 1) -> encode_commits_dev, captured into one graph and replayed on two inputs that
    decide different instances (so different reply counts), against the transliterations"""
    import client_translit as CL
    import commit_translit as CT
    import proposer_translit as PT
    from go_translit import GoBackend
    from test_gpu_client import _chain_input, dev_buffers
    e = mk_engine(N, R.MODE_MIN)
    G, per_group, slot, ipg, base, D = 3, 4, 1024, 8, 50, 32
    n_inst, n_conns = G * ipg, G * per_group
    cap = n_conns * slot // 30
    inputs = []
    for seed, decided_groups in ((11, (0, 2)), (12, (1,))):
        bufs, groups = _chain_input(seed, G, per_group, slot)
        wc = CL.decode_client_streams(bufs, groups, G)
        grp = PT.mk_groups([(D, 0, 0, 2, base + g * ipg, base + g * ipg - 1) for g in range(G)])
        st, lb = PT.nil_state(n_inst), np.zeros(n_inst, R.INST_STATE)
        wp = PT.propose_handle(R.MODE_MIN, N, grp, wc["prop_off"], st, base, ipg, lb)
        sends = wp[3]
        assert len(sends) == G and (sends["flags"] == A).all()
        rep = np.zeros(G, R.ACCEPT_REPLY)  # one reply per instance, ascending
        for g in range(G):
            rep[g] = (sends["instance"][g], D, 1, 1 if g in decided_groups else 0, (0, 0, 0))
        sc = np.full(1 + N, base - 1, np.int32)
        w_lb, w_cu, w_pc, w_dec = GoBackend(N, R.MODE_MIN).accept_tally(rep, wp[2], base, base - 1,
                                                                        sc[1:])
        assert int(w_dec.sum()) == len(decided_groups)
        wr = T.build_replies(R.RB_DECIDED, sends, wc["meta"], w_dec, base, cap=cap, pad_client=n_conns)
        assert 0 < int(wr["res"]["n_replies"]) < int(wc["res"]["n_proposals"])
        w_cb, w_coff = CT.encode_commits(N, wr["commit_sends"], wp[0], (wc["op"], wc["key"], wc["val"]),
                                         base, ipg)
        buf = np.zeros(n_conns * slot, np.uint8)
        conns = np.zeros(n_conns, R.CLIENT_CONN)
        for k, b in enumerate(bufs):
            conns[k] = (k * slot, len(b), groups[k])
            buf[k * slot:k * slot + len(b)] = np.frombuffer(b, np.uint8)
        inputs.append(dict(buf=buf, conns=conns, grp=grp, st=st, lb=lb, rep=rep, sc=sc, wc=wc, wp=wp,
                           w_lb=w_lb, w_dec=w_dec, wr=wr, w_cb=w_cb, w_coff=w_coff))
    assert inputs[0]["wr"]["res"]["n_replies"] != inputs[1]["wr"]["res"]["n_replies"]
    c_cap = max(len(x["w_cb"]) for x in inputs) + 64
    with Arena(e) as ar:
        g, g_buf, d_conns, out = dev_buffers(ar, inputs[0]["buf"], inputs[0]["conns"], G, cap)
        g_grp, g_st = Guard(ar, G, R.PROPOSER_GROUP), Guard(ar, n_inst, R.ACCEPTOR_STATE)
        g_lb, g_snd = Guard(ar, n_inst, R.INST_STATE), Guard(ar, G, R.ACCEPT_SEND)
        d_rep, g_sc = ar.empty(G, R.ACCEPT_REPLY), Guard(ar, 1 + N, np.int32)
        g_lb2, g_dec = Guard(ar, n_inst, R.INST_STATE), Guard(ar, n_inst, np.uint8)
        g_recs, g_cs = Guard(ar, cap, R.REPLY_REC), Guard(ar, G, R.COMMIT_SEND)
        g_res = Guard(ar, 1, R.REPLY_RESULT)
        g_rout, g_roff = Guard(ar, cap * R.PROPOSE_REPLY_BYTES, np.uint8), Guard(ar, n_conns + 2, np.uint64)
        g_cout, g_coff = Guard(ar, c_cap, np.uint8), Guard(ar, N + 1, np.uint64)
        rb = e.reply_batch_dev(R.RB_DECIDED, g_snd, G, g["meta"], cap, g_dec, n_inst, base,
                               pad_client=n_conns, general=general)
        cb = _lib.MpxCommitBatch()
        cb.sends, cb.n_sends, cb.inst_base, cb.ipg = g_cs.ptr, G, base, ipg
        cb.groups, cb.n_groups = g_grp.ptr, G
        cb.cmd_op, cb.cmd_key, cb.cmd_val, cb.n_cmds = g["op"].ptr, g["key"].ptr, g["val"].ptr, cap
        cb.flags, cb.alive_mask = 0, 0xFFFF
        e.decode_client_streams_reserve(n_conns * slot, n_conns, G)
        e.build_replies_reserve(G)
        e.encode_replies_reserve(cap)
        e.encode_commits_reserve(G, 0)
        s = e.stream_create()
        e.graph_begin(s)
        e.decode_client_streams_dev(g_buf.ptr, n_conns * slot, d_conns.ptr, n_conns, G, out,
                                    g["conn_res"].ptr, g["res"].ptr, s)
        e.propose_handle_dev(g_grp.ptr, G, g["prop_off"].ptr, g["send_off"].ptr, g_st.ptr, g_lb.ptr,
                             n_inst, base, ipg, g_snd.ptr, s)
        e.accept_tally_dev(d_rep.ptr, G, g_lb.ptr, g_lb2.ptr, n_inst, base, g_sc.ptr, g_dec.ptr, s)
        e.build_replies_dev(rb, g_recs.ptr, cap, g_cs.ptr, g_res.ptr, s)
        e.encode_replies_dev(g_recs.ptr, cap, n_conns + 1, 1, 0, g_rout.ptr, g_roff.ptr, s)
        e.encode_commits_dev(cb, g_cout.ptr, c_cap, g_coff.ptr, s)
        gr = e.graph_end(s)
        try:
            for x in inputs + inputs[:1]:
                for y in list(g.values()) + [g_snd, g_lb2, g_dec, g_recs, g_cs, g_res, g_rout, g_roff,
                                             g_cout, g_coff]:
                    y.fill(s)
                g_buf.put(x["buf"], s)
                g_grp.put(x["grp"], s)
                g_st.put(x["st"], s)
                g_lb.put(x["lb"], s)
                g_sc.put(x["sc"], s)
                for dst, a in ((d_conns, x["conns"]), (d_rep, x["rep"])):
                    src = ar.put(a, s)
                    e.memcpy(dst.ptr, src.ptr, src.nbytes, D2D, s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                wr = x["wr"]
                assert g_snd.assert_margins().tobytes() == x["wp"][3].tobytes()
                assert np.array_equal(g_dec.assert_margins(), x["w_dec"])
                assert g_res.assert_margins()[0].tobytes() == wr["res"].tobytes()
                assert g_recs.assert_margins().tobytes() == wr["recs"].tobytes()
                assert g_cs.assert_margins().tobytes() == wr["commit_sends"].tobytes()
                roff, rout = g_roff.assert_margins(), g_rout.assert_margins()
                runs = _reply_bytes(wr["recs"], n_conns + 1)
                for k in range(n_conns + 1):
                    assert rout[int(roff[k]):int(roff[k + 1])].tobytes() == runs[k], k
                n_real = int(wr["res"]["n_replies"])
                assert int(roff[n_conns]) == n_real * R.PROPOSE_REPLY_BYTES  # the last run is the pad
                assert np.array_equal(g_coff.assert_margins(), x["w_coff"])
                assert g_cout.assert_margins()[:len(x["w_cb"])].tobytes() == x["w_cb"].tobytes()
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()


@pytest.mark.gpu
def test_closed_loop_with_no_record_built_on_the_host(mk_engine):
    """tests/test_gpu_client.py's closed loop with the host join replaced: client bytes in, the
    Accept frames through two followers, their replies into the leader's tally, then
    mpx_build_replies from the sends, the decided mask and meta, then mpx_encode_replies: every
    connection's reply run carries exactly its own CommandIds and Timestamps in its own order"""
    import client_translit as CL
    import proposer_translit as PT
    from test_gpu_client import _chain_input
    NR = 3
    e = mk_engine(NR, R.MODE_MIN)
    G, per_group, slot, ipg, base, D = 3, 5, 1024, 8, 300, 48
    n_inst, n_conns = G * ipg, G * per_group
    bufs, groups = _chain_input(21, G, per_group, slot)
    got = e.decode_client_streams(bufs, groups, G)
    want_ids = [[(p[0], p[4]) for p in CL.client_listener(b)[0]] for b in bufs]
    grp = PT.mk_groups([(D, 0, 0, 2, base + g * ipg, base + g * ipg - 1) for g in range(G)])
    lb = np.zeros(n_inst, R.INST_STATE)
    grp, st, lb, sends, send_off = e.propose_handle(grp, got["prop_off"], PT.nil_state(n_inst), base,
                                                    ipg, lb)
    assert len(sends) == G
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
        um, _ = e.unmarshal_frames(run, var)
        fg = np.zeros(G, R.ACCEPTOR_GROUP)
        fg["default_ballot"], fg["self_id"] = D, q
        _, rep, to, eff = e.accept_handle(um["accepts"], PT.nil_state(n_inst), fg, base, ipg)
        assert (eff & R.AH_REPLIED).all()
        replies.append(rep[::-1].copy())
    batch, _, _ = e.order_records(replies, n_inst, base)
    _, _, _, decided = e.accept_tally(batch, lb, base, base - 1, np.full(NR, base - 1, np.int32))
    assert int(decided.sum()) == G
    recs, cs, res = e.build_replies(R.RB_DECIDED, sends, got["meta"], decided, base,
                                    want_commit_sends=True)
    assert int(res["n_replies"]) == len(recs) == int(got["res"]["n_proposals"])
    assert int(res["n_slots"]) == G and (cs["flags"] == R.CS_SEND).all()
    rbytes, roff = e.encode_replies(recs, n_conns)
    for k in range(n_conns):
        run = rbytes[int(roff[k]):int(roff[k + 1])].tobytes()
        assert len(run) == R.PROPOSE_REPLY_BYTES * len(want_ids[k])
        ids = [(struct.unpack_from("<i", run, 25 * i + 1)[0], struct.unpack_from("<q", run, 25 * i + 13)[0])
               for i in range(len(want_ids[k]))]
        assert ids == want_ids[k], k


@pytest.mark.gpu
def test_classic_commit_sends_are_bcast_commits_list(mk_engine):
    """CLASSIC's leader: the commit_sends of a DECIDED call are the instances handleAcceptReply
    hands to bcastCommit (paxos.go:661), and mpx_encode_commits over them writes what
    commit_translit's bcastCommit sends for exactly those calls"""
    import commit_translit as CT
    NC = 5
    e = mk_engine(NC, R.MODE_CLASSIC)
    counts = [3, 0, 40, 1, 7, 2]
    case = mk_case(R.RB_DECIDED, counts, flags=[A, A, PR, A, RF, A], sel=[1, 1, 1, 0, 1, 1], base=70)
    want = check(e, case)
    m = len(case["meta"])
    rng = np.random.default_rng(3)
    op = rng.integers(0, 6, m).astype(np.uint8)
    key, val = rng.integers(-99, 99, m), rng.integers(-99, 99, m)
    wantc = T.build_replies(proto=T.CLASSIC, **case)
    assert [b[0] for b in wantc["bcast"]] == [70, 71, 72, 75]
    per = [[] for _ in range(NC)]
    for inst, ballot, cmds in wantc["bcast"]:
        command = [(int(op[j]), int(key[j]), int(val[j])) for j in cmds]
        for q, frame in CT.bcast_commit(NC, 0, False, [True] * NC, inst, ballot, command):
            per[q].append(frame)
    _, cs, _ = e.build_replies(R.RB_DECIDED, case["sends"], case["meta"], case["mask"], 70, cap=0,
                               want_commit_sends=True)
    assert cs.tobytes() == want["commit_sends"].tobytes()
    out, off = e.encode_commits(cs, CT.mk_self([0]), (op, key, val), 70, len(counts))
    for q in range(NC):
        assert out[int(off[q]):int(off[q + 1])].tobytes() == b"".join(per[q]), q

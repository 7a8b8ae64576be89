"""GPU tests of execute assembly (mpx_execute_gather, mpx_execute_gather_dev): executeCommands' walk
and the gather of its commands, bit-exact against tests/execute_translit.py (the Go loop over
Go-shaped objects). Every case runs the host form and the _dev form, the latter with its outputs on
devguard.Guard buffers exactly their capacity long (op at an odd address), and, whenever the call
is within the one-launch bounds, both the one-launch kernel and the general path (general=True, the
documented MPX_XG_GENERAL flag) against the same bytes. Shapes are the smallest that reach the
edges: the stop and mark passes take 1024 slots per workgroup in 64-slot units, the scan 4096
items per tile (over n_inst + 1 items), the gather 1024 commands per tile, four per thread. The
error cases are reported through the error word or refused before any launch: no case provokes a
fault."""
import ctypes as C
import struct

import numpy as np
import pytest

import execute_kat
import execute_translit as T
from devguard import Guard
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import D2D, Arena
from minpaxos_amd.engine import MpxError

N = 3
TILE = 1024
OUT = ("op", "key", "val", "mask", "executed", "inst_first", "ret_first", "grp_cmd_off", "res")


def _code(f, *a, **k):
    try:
        f(*a, **k)
    except MpxError as ex:
        return ex.code
    return R.OK


def mk_case(sizes, committed, executed, ipg, nil=(), base=100, gaps=True, sends=None, **extra):
    """slot idx has sizes[idx] commands (None or idx in nil: Cmds == nil), laid out from command 3
    with a gap of one command after every third slot, so first_cmd is rarely a multiple of 4;
    committed / executed: per group, relative to first_g - 1 (0 = none)"""
    n, G = len(sizes), len(committed)
    has = np.array([k is not None for k in sizes], bool)
    has[list(nil)] = False
    k = np.array([x or 0 for x in sizes], np.int64)
    step = k + (np.arange(n) % 3 == 2 if gaps else 0)
    inst = np.zeros(n, R.INST_CMDS)
    inst["first_cmd"] = 3 + np.concatenate([[0], np.cumsum(step)])[:n]
    inst["n_cmds"], inst["flags"] = np.where(has, k, 0), np.where(has, R.IC_HAS_CMDS, 0)
    inst["first_cmd"][~has] = 0
    at = 3 + int(step.sum())
    first = base + np.arange(G) * ipg - 1
    case = dict(inst=inst, committed_upto=(first + committed).astype(np.int32),
                executed=(first + executed).astype(np.int32), cmds=T.mk_cmds(at + 2, len(sizes)),
                inst_base=base, ipg=ipg, **extra)
    if sends is not None:
        case["sends"] = T.mk_sends(np.asarray(sends, np.int32))
    return case


def run_host(e, case, cap, general):
    return e.execute_gather(case["inst"], case["committed_upto"], case["executed"], case["cmds"],
                            case["inst_base"], case["ipg"], case.get("sends"), cap,
                            case.get("pad", False), general)


def dev_call(e, ar, case, cap, general, op_shift=1, kv_shift=0):
    """the call's inputs on the device and its outputs on guards; returns (batch, out, guards)"""
    inst, sends = case["inst"], case.get("sends")
    cu, ex = case["committed_upto"], case["executed"]
    op, key, val = case["cmds"]
    n, G, n_src = len(inst), len(cu), len(op)
    n_sends = 0 if sends is None else len(sends)
    g = dict(op=Guard(ar, cap, np.uint8, shift=op_shift), key=Guard(ar, cap, np.int64, shift=kv_shift),
             val=Guard(ar, cap, np.int64, shift=kv_shift), mask=Guard(ar, n, np.uint8, shift=5),
             executed=Guard(ar, G, np.int32).put(ex), inst_first=Guard(ar, n, np.uint64),
             ret_first=Guard(ar, n_sends, np.uint64), grp_cmd_off=Guard(ar, G + 1, np.uint64),
             res=Guard(ar, 1, R.EXECUTE_RESULT))
    d_sop = Guard(ar, n_src, np.uint8, shift=3).put(op)
    b = e.execute_batch_dev(ar.put(inst) if n else None, n, case["inst_base"], case["ipg"], G,
                            ar.put(cu) if G else None, g["executed"] if G else None,
                            g["executed"] if G else None, d_sop if n_src else None,
                            ar.put(key) if n_src else None, ar.put(val) if n_src else None, n_src,
                            ar.put(sends) if n_sends else None, n_sends, case.get("pad", False), general)
    o = e.execute_out_dev(g["op"] if cap else None, g["key"] if cap else None,
                          g["val"] if cap else None, cap, g["mask"] if n else None, g["inst_first"],
                          g["ret_first"] if sends is not None else None, g["grp_cmd_off"])
    return b, o, g


def read_dev(g, cap, padded, with_sends):
    res = g["res"].assert_margins()[0]
    k = cap if padded else min(int(res["n_cmds"]), cap)
    got = {name: g[name].assert_margins() for name in OUT[:8]}
    for name in ("op", "key", "val"):
        g[name].assert_untouched([(k, cap)])
        got[name] = got[name][:k]
    if not with_sends:
        got["ret_first"] = None
    got["res"] = res
    return got


def run_dev(e, case, cap, general, op_shift=1, kv_shift=0):
    """returns (outputs, code of the next synchronising call)"""
    with Arena(e) as ar:
        b, o, g = dev_call(e, ar, case, cap, general, op_shift, kv_shift)
        e.execute_gather_reserve(len(case["inst"]), len(case["committed_upto"]))
        e.execute_gather_dev(b, o, g["res"].ptr)
        code = _code(e.synchronize)
        return read_dev(g, cap, case.get("pad", False), case.get("sends") is not None), code


def same(got, want, what):
    for name in OUT:
        a, b = got[name], want[name]
        if a is None or b is None:
            assert a is None and b is None, (what, name)
            continue
        a, b = np.asarray(a), np.asarray(b)
        if a.tobytes() != b.tobytes():
            assert a.shape == b.shape, (what, name, a.shape, b.shape)
            diff = np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:5] if a.shape else []
            raise AssertionError(f"{what}: {name} differs at {list(diff)}: got "
                                 f"{a.reshape(-1)[diff] if a.shape else a} want "
                                 f"{b.reshape(-1)[diff] if b.shape else b}")


def paths_of(case, cap):
    """general = False always; True as well when the default would take the one-launch kernel"""
    one = len(case["inst"]) <= R.XG_ONE_LAUNCH_INST and cap <= R.XG_ONE_LAUNCH_CMDS
    return (False, True) if one else (False,)


def args_of(case):
    return {k: v for k, v in case.items() if k not in ("cap", "pad")}


def check(e, case, forms=("host", "dev"), shifts=((1, 0),)):
    want = T.execute_gather(**args_of(case))
    cap = case.get("cap", int(want["res"]["n_cmds"]))
    if "cap" in case or case.get("pad"):
        want = T.execute_gather(**dict(case, cap=cap))
    assert want["code"] == R.OK
    for general in paths_of(case, cap):
        if "host" in forms:
            same(run_host(e, case, cap, general), want, f"host general={general}")
        if "dev" in forms:
            for op_shift, kv_shift in shifts:
                got, code = run_dev(e, case, cap, general, op_shift, kv_shift)
                assert code == R.OK
                same(got, want, f"dev general={general} shifts={op_shift},{kv_shift}")
    return want


@pytest.fixture
def eng(mk_engine):
    return mk_engine(N, R.MODE_MIN)


# ---- the known answers ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", execute_kat.KAT_EXECUTE, ids=lambda c: c["name"])
def test_known_answers(eng, case):
    want = check(eng, execute_kat.kat_args(case), shifts=((1, 0), (0, 8), (4, 8)))
    execute_kat.check(case, want)
    execute_kat.check(case, run_host(eng, execute_kat.kat_args(case), case.get("cap", len(case["src"])),
                                     False))


# ---- shapes --------------------------------------------------------------------------------------
def shape_case(ipg, G, seed=0, big=True):
    """groups with every kind of cursor pair, a nil slot in about half of the walks, commands per
    instance from {0, 1, 2, 16, 17} and one instance of 5000"""
    rng = np.random.default_rng(500 + 7 * ipg + G + seed)
    n = ipg * G
    sizes = rng.choice([0, 1, 2, 16, 17], n, p=[0.15, 0.5, 0.25, 0.05, 0.05]).tolist()
    a, b = rng.integers(0, ipg + 1, G), rng.integers(0, ipg + 1, G)
    flip = rng.random(G) < 0.1                      # executed above committed
    ex = np.where(flip, np.maximum(a, b), np.minimum(a, b))
    cu = np.where(flip, np.minimum(a, b), np.maximum(a, b))
    nil = set()
    for g in range(G):
        if cu[g] > ex[g] and rng.random() < 0.5:
            nil.add(g * ipg + int(rng.integers(ex[g], cu[g])))
        if rng.random() < 0.5:
            nil.add(g * ipg + int(rng.integers(0, ipg)))
    runs = [g * ipg + int(ex[g]) for g in range(G) if cu[g] > ex[g] and g * ipg + int(ex[g]) not in nil]
    if big and runs:
        sizes[runs[0]] = 5000
    sends = rng.integers(98, 102 + n, min(n, 200))
    return mk_case(sizes, cu, ex, ipg, nil, sends=sends)


@pytest.mark.gpu
@pytest.mark.parametrize("n_groups", [1, 2, 3, 257])
@pytest.mark.parametrize("ipg", [1, 2, 63, 64, 65, 256, 1025])
def test_group_boundaries_inside_and_across_tiles(eng, ipg, n_groups):
    want = check(eng, shape_case(ipg, n_groups))
    if n_groups == 257 and ipg >= 63:
        assert 0 < int(want["res"]["n_groups"]) < 257 and int(want["mask"].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("total", [TILE - 1, TILE, TILE + 1, 4 * TILE - 1, 4 * TILE, 4 * TILE + 1])
def test_totals_and_instance_boundaries_around_the_gather_tile(eng, total):
    """an instance boundary at every position from 2 before to 2 after a tile boundary, with key /
    val outputs that start on a 16-byte line and in the middle of one, op at four alignments"""
    edge = TILE if total <= TILE + 1 else 4 * TILE
    for d in (-2, -1, 0, 1, 2):
        k = min(edge + d, total)
        sizes = [k - 7, 0, 7, total - k]
        check(eng, mk_case(sizes, [4], [0], 4), shifts=((1, 0), (2, 8), (3, 0), (0, 8)))
    # ... and built from instances of 16 and 17 commands
    sizes = [17] * (total // 17 - 1) + [16]
    sizes += [total - sum(sizes)]
    check(eng, mk_case(sizes, [len(sizes)], [0], len(sizes)))


@pytest.mark.gpu
def test_one_5000_command_instance(eng):
    """the replica batch: one launch by default"""
    want = check(eng, mk_case([5000], [1], [0], 1), shifts=((1, 0), (1, 8)))
    assert int(want["res"]["n_cmds"]) == 5000


@pytest.mark.gpu
def test_window_of_2_to_the_20_slots_in_one_group(eng):
    """the walk stops in tile 300 of 1024: the stop crosses many workgroups of one group"""
    n = 1 << 20
    stop = 300 * TILE + 77
    sizes = np.ones(n, np.int64)
    sizes[5::7] = 2
    done = 200 * TILE + 5
    case = mk_case(sizes.tolist(), [n - 3], [done], n, nil=(stop, stop + 100000, 17), gaps=False,
                   sends=[100 + done, 100 + done + 1, 100 + stop, 100 + n - 1])
    want = check(eng, case, forms=("dev",))
    assert int(want["executed"][0]) == 100 + stop - 1 and int(want["res"]["n_inst"]) == stop - done


@pytest.mark.gpu
def test_no_slot_at_all(eng):
    case = dict(inst=T.mk_inst([]), committed_upto=np.zeros(0, np.int32), executed=np.zeros(0, np.int32),
                cmds=T.mk_cmds(0), inst_base=7, ipg=0)
    check(eng, case)
    check(eng, dict(case, cap=TILE + 5, pad=True))
    check(eng, dict(case, cap=9000, pad=True, sends=T.mk_sends([7, 8])))


# ---- capacity and padding ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[700, 0, 1, 323, 41, 1300], [3, 1, 2]], ids=["2365", "6"])
def test_capacity_and_pad(eng, sizes):
    total = sum(sizes)
    for cap, pad in ((0, False), (total - 1, False), (total, False), (total + 1000, True),
                     (total, True), (total - 1, True), (0, True)):
        check(eng, mk_case(sizes, [len(sizes)], [0], len(sizes), cap=cap, pad=pad),
              shifts=((1, 0), (0, 8)))


@pytest.mark.gpu
def test_a_short_call_repeated_with_a_larger_cap(eng):
    """executed_in and executed_out apart: the cursors are not consumed by the short call"""
    case = mk_case([5, 3, 9], [3], [0], 3)
    short = eng.execute_gather(case["inst"], case["committed_upto"], case["executed"], case["cmds"],
                               100, 3, cap=4)
    assert int(short["res"]["n_cmds"]) == 17 and len(short["op"]) == 4
    same(run_host(eng, case, 17, False), T.execute_gather(**case), "again")


# ---- fuzz ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_fuzz(eng, seed):
    check(eng, T.fuzz_case(seed), shifts=((1 + seed % 3, 8 * (seed & 1)),))


# ---- rejections ----------------------------------------------------------------------------------
def _faulty(fault):
    case = mk_case([4, 2, 6, 0, 3, 1200, 1, 1, 5], [3, 2, 3], [0, 0, 1], 3)
    if fault == "committed_below":
        case["committed_upto"][1] -= 3
    elif fault == "committed_above":
        case["committed_upto"][0] += 1
    elif fault == "executed_below":
        case["executed"][2] = case["inst_base"] + 4
    elif fault == "executed_above":
        case["executed"][0] = case["inst_base"] + 3
    elif fault == "commands":
        case["inst"]["n_cmds"][2] = 5000              # past n_src
    elif fault == "first_cmd":
        case["inst"]["first_cmd"][7] = 1 << 40
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("fault", ["committed_below", "committed_above", "executed_below",
                                   "executed_above", "commands", "first_cmd"])
def test_faulty_group_or_instance_by_error_word_and_by_code(eng, fault):
    """the host form answers before any launch; the _dev form raises the error word, the group
    does nothing or the instance executes with no commands, and the others are exact"""
    case = _faulty(fault)
    assert T.execute_gather(**case)["code"] == R.E_INVAL
    want = T.execute_gather(dev=True, **case)
    assert want["code"] == R.E_INVAL and int(want["res"]["n_groups"]) >= 2
    cap = int(want["res"]["n_cmds"])
    for general in (False, True):
        assert _code(run_host, eng, case, cap, general) == R.E_INVAL
        got, code = run_dev(eng, case, cap, general)
        assert code == R.E_INVAL
        same(got, want, f"dev general={general}")
    # the handle is clean again
    check(eng, mk_case([2, 3], [2], [0], 2))


@pytest.mark.gpu
def test_an_unreached_faulty_instance_is_not_looked_at(eng):
    case = mk_case([4, 2, 6], [2], [0], 3)
    case["inst"]["n_cmds"][2] = 5000
    check(eng, case)


@pytest.mark.gpu
def test_argument_rejections(eng):
    e = eng
    case = mk_case([2, 3, 1, 1], [2, 2], [0, 0], 2, sends=[100])
    keep = [case["inst"], case["committed_upto"], case["executed"].copy(), *case["cmds"], case["sends"],
            np.zeros(8, np.uint8), np.zeros(8, np.int64), np.zeros(8, np.int64), np.zeros(4, np.uint8),
            np.zeros(4, np.uint64), np.zeros(1, np.uint64), np.zeros(3, np.uint64)]
    p = [x.ctypes.data_as(C.c_void_p) for x in keep]
    n_src = len(case["cmds"][0])
    res = _lib.MpxExecuteResult()

    def host(with_res=True, **kw):
        f = dict(inst=p[0], n_inst=4, inst_base=100, ipg=2, n_groups=2, committed_upto=p[1],
                 executed_in=p[2], executed_out=p[2], src_op=p[3], src_key=p[4], src_val=p[5],
                 n_src=n_src, sends=p[6], n_sends=1, flags=0, reserved=0)
        o = dict(op=p[7], key=p[8], val=p[9], cap=8, mask=p[10], inst_first=p[11], ret_first=p[12],
                 grp_cmd_off=p[13])
        f.update({k: v for k, v in kw.items() if k in f})
        o.update({k: v for k, v in kw.items() if k in o})
        keep[2][:] = case["executed"]
        return e.lib.mpx_execute_gather(e.h, C.byref(_lib.MpxExecuteBatch(**f)),
                                        C.byref(_lib.MpxExecuteOut(**o)),
                                        C.byref(res) if with_res else None)
    assert host() == R.OK and (res.n_cmds, res.n_inst, res.n_groups) == (7, 4, 2)
    for name in ("inst", "committed_upto", "executed_in", "executed_out", "src_op", "src_key", "src_val",
                 "sends", "op", "key", "val", "mask"):
        assert host(**{name: None}) == R.E_INVAL, name
    assert host(with_res=False) == R.E_INVAL
    assert e.lib.mpx_execute_gather(e.h, None, None, C.byref(res)) == R.E_INVAL
    assert host(n_inst=3) == R.E_INVAL and host(ipg=3) == R.E_INVAL
    assert host(ipg=0, n_inst=0) == R.E_INVAL
    assert host(flags=4) == R.E_INVAL and host(reserved=1) == R.E_INVAL
    assert host(sends=None, n_sends=0) == R.E_INVAL                 # ret_first without sends
    assert host(sends=None, n_sends=0, ret_first=None) == R.OK
    assert host(inst_first=None, ret_first=None, grp_cmd_off=None) == R.OK
    assert host(n_inst=0xFFFFFFFF, n_groups=1, ipg=0xFFFFFFFF) == R.E_UNSUPPORTED
    keep[0]["n_cmds"][:2] = 0x80000000          # 2^32 commands in all: refused before any is read
    assert host(n_src=1 << 40) == R.E_UNSUPPORTED
    keep[0]["n_cmds"][:2] = [2, 3]
    assert host() == R.OK and res.n_cmds == 7
    assert _code(e.execute_gather_reserve, 0xFFFFFFFF, 1) == R.E_UNSUPPORTED
    assert _code(e.execute_gather_reserve, 1, 0xFFFFFFFF) == R.E_UNSUPPORTED
    # the device form's alignment rules
    with Arena(e) as ar:
        b, o, g = dev_call(e, ar, case, 8, False, op_shift=0)
        e.execute_gather_reserve(4, 2)

        def dev(field=None, by=0, res_by=0):
            x, y = _lib.MpxExecuteBatch.from_buffer_copy(b), _lib.MpxExecuteOut.from_buffer_copy(o)
            for s in (x, y):
                if field and hasattr(s, field):
                    setattr(s, field, getattr(s, field) + by)
            return _code(e.execute_gather_dev, x, y, g["res"].ptr + res_by)
        for field, by in (("inst", 8), ("sends", 8), ("src_key", 4), ("src_val", 4), ("key", 4),
                          ("val", 4), ("inst_first", 4), ("ret_first", 4), ("grp_cmd_off", 4),
                          ("committed_upto", 2), ("executed_in", 2), ("executed_out", 2)):
            assert dev(field, by) == R.E_INVAL, field
        assert dev(res_by=4) == R.E_INVAL
        e.synchronize()
        for name, x in g.items():
            x.assert_margins()
            if name != "executed":
                x.assert_untouched([(0, x.count)])
        # op, src_op and mask may sit anywhere (one byte further is inside the guards' margins)
        assert dev("src_op", 0) == R.OK
        e.synchronize()
    del keep


@pytest.mark.gpu
def test_dev_form_needs_its_reserve_and_never_grows(mk_engine):
    e = mk_engine(N, R.MODE_CLASSIC)
    small = mk_case([2, 3], [1, 1], [0, 0], 1)
    big = mk_case([1] * 3000, [2] * 1500, [0] * 1500, 2)
    with Arena(e) as ar:
        b, o, g = dev_call(e, ar, small, 5, True)
        with pytest.raises(MpxError) as ei:
            e.execute_gather_dev(b, o, g["res"].ptr)
        assert ei.value.code == R.E_INVAL and "mpx_execute_gather_reserve" in str(ei.value)
        e.execute_gather_reserve(2, 1)      # two slots, but one group only
        assert _code(e.execute_gather_dev, b, o, g["res"].ptr) == R.E_INVAL
        e.execute_gather_reserve(1, 2)      # grows only: now two slots in two groups
        e.execute_gather_dev(b, o, g["res"].ptr)
        e.synchronize()
        assert g["res"].assert_margins()[0].tolist() == (5, 2, 2, 0)
        b2, o2, g2 = dev_call(e, ar, big, 3000, False)
        assert _code(e.execute_gather_dev, b2, o2, g2["res"].ptr) == R.E_INVAL
        e.synchronize()
        g2["op"].assert_untouched([(0, 3000)])
        g2["mask"].assert_untouched([(0, 3000)])
    check(e, big)
    # the stop words of 1500 groups were laid over what was other scratch: calls of both sizes
    # stay exact in any order
    check(e, small)
    check(e, shape_case(256, 3, big=False))
    check(e, big)


# ---- against existing code -----------------------------------------------------------------------
@pytest.mark.gpu
def test_cursors_equal_the_group_steps(mk_engine):
    """64 groups x 16 slots: mpx_group_step with empty reply lists and the same committed /
    executed / has_cmds leaves the same executed_out"""
    from minpaxos_amd import synth
    G, ipg = 64, 16
    e = mk_engine(5, R.MODE_MIN)
    rng = np.random.default_rng(64)
    b = synth.group_batch(G, ipg, 5, 2, 64, seed=9)
    b["recs"], b["grp_rec_off"] = np.zeros(0, R.ACCEPT_REPLY), np.zeros(G + 1, np.uint64)
    x, y = rng.integers(-1, ipg, G), rng.integers(-1, ipg, G)
    b["executed_in"], b["committed_in"] = np.minimum(x, y).astype(np.int32), np.maximum(x, y).astype(np.int32)
    b["executed_in"][:4], b["committed_in"][:4] = [5, ipg - 1, -1, 3], [2, ipg - 1, -1, 3]
    b["has_cmds"] = (rng.random(G * ipg) > 0.12).astype(np.uint8)
    step = e.group_step(b)
    assert np.array_equal(step["committed_out"], b["committed_in"])
    inst = np.zeros(G * ipg, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"] = b["cmd_off"][:-1], np.diff(b["cmd_off"].astype(np.int64))
    inst["flags"] = b["has_cmds"]
    first = np.arange(G, dtype=np.int32) * ipg
    for general in (False, True):
        got = e.execute_gather(inst, first + b["committed_in"], first + b["executed_in"],
                               (b["op"], b["key"], b["val"]), 0, ipg, general=general)
        assert np.array_equal(got["executed"] - first, step["executed_out"])
        assert len({int(v) for v in step["executed_out"] - b["executed_in"]}) > 4
        # ... and the commands it gathered are the ones the step wrote results for
        ran = np.repeat(got["mask"], 2).astype(bool)
        assert np.array_equal(got["val"], b["val"][ran]) and np.array_equal(got["op"], b["op"][ran])


# ---- the chain -----------------------------------------------------------------------------------
def _reply_bytes(recs, n_clients):
    """per client, ProposeReplyTS.Marshal of its records in order (OK = 1, Leader = 0)"""
    runs = [b""] * n_clients
    for r in recs:
        runs[int(r["client"])] += struct.pack("<Biqqi", 1, int(r["command_id"]), int(r["value"]),
                                              int(r["timestamp"]), 0)
    return runs


def _execute(state, op, key, val):
    """state.(*Command).Execute over a Python dict (state.go:77-102)"""
    ret = np.zeros(len(op), np.int64)
    for i in range(len(op)):
        if op[i] == R.OP_PUT:
            state[int(key[i])] = int(val[i])
            ret[i] = val[i]
        elif op[i] == R.OP_GET:
            ret[i] = state.get(int(key[i]), 0)
    return ret


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True])
def test_graph_from_commits_to_reply_bytes(mk_engine, general):
    """mpx_commit_handle_dev -> mpx_execute_gather_dev (pad) -> mpx_apply_dev(m = cap) ->
    mpx_build_replies_dev(MPX_RB_EXECUTED, mask, ret_first) -> mpx_encode_replies_dev, captured once
    into a graph and replayed on two inputs that commit different instances, against the commit,
    execute and reply transliterations and a Python dict State that lives across the replays"""
    import commit_translit as CT
    import reply_translit as RT
    e = mk_engine(N, R.MODE_MIN)
    G, ipg, base, n_clients = 3, 8, 50, 6
    n_inst = G * ipg
    rng = np.random.default_rng(77)
    sizes = rng.choice([0, 1, 2, 3], n_inst, p=[0.1, 0.4, 0.3, 0.2])
    first_cmd = np.concatenate([[0], np.cumsum(sizes + 1)])[:-1] + 1   # gaps: commands no slot names
    m = int(first_cmd[-1] + sizes[-1]) + 2
    inst = np.zeros(n_inst, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"], inst["flags"] = first_cmd, sizes, R.IC_HAS_CMDS
    inst["flags"][[5, ipg + 2]] = 0        # Cmds == nil although committed: the walk stops there
    op = rng.choice([R.OP_PUT, R.OP_GET, R.OP_NONE], m, p=[0.5, 0.4, 0.1]).astype(np.uint8)
    key, val = rng.integers(0, 12, m), rng.integers(1, 1 << 40, m)
    meta = np.zeros(m, R.PROPOSAL)
    meta["timestamp"], meta["command_id"] = rng.integers(1, 1 << 50, m), np.arange(m) + 1000
    meta["client"] = rng.integers(0, n_clients, m)
    sends = RT.mk_sends([(base + i, 4, R.PH_ACCEPT, int(first_cmd[i]), int(sizes[i])) for i in range(n_inst)])
    cap = int(sizes.sum()) + 5
    none = (base + np.arange(G) * ipg - 1).astype(np.int32)
    state, inputs = {}, []
    for commits in ((4, 7, 0), (8, 0, 3)):     # per group: Commits for its first so many instances
        msgs = CT.mk_msgs([(base + g * ipg + k, 9, 0, 1 + k) for g in range(G) for k in range(commits[g])])
        st = np.zeros(n_inst, R.ACCEPTOR_STATE)
        st["status"] = CT.NIL
        w_st, w_cu, w_eff, _ = CT.commit_handle(msgs, st, none, base, ipg)
        wx = T.execute_gather(inst, w_cu, none, (op, key, val), base, ipg, sends, cap, pad=True)
        assert 0 < int(wx["res"]["n_cmds"]) < cap
        ret = _execute(state, wx["op"], wx["key"], wx["val"])
        wr = RT.build_replies(R.RB_EXECUTED, sends, meta, wx["mask"], base, ret, wx["ret_first"],
                              cap=cap, pad_client=n_clients)
        assert int(wr["res"]["n_replies"]) == int(wx["res"]["n_cmds"])
        inputs.append(dict(msgs=msgs, st=st, w_st=w_st, w_cu=w_cu, w_eff=w_eff, wx=wx, ret=ret, wr=wr))
    assert inputs[0]["wx"]["res"]["n_cmds"] != inputs[1]["wx"]["res"]["n_cmds"]
    n_msgs = len(inputs[0]["msgs"])          # the captured call takes a host count
    assert len(inputs[1]["msgs"]) == n_msgs
    with Arena(e) as ar:
        d_msgs = ar.empty(n_msgs, R.ACCEPT_MSG)
        g_st, g_cu = Guard(ar, n_inst, R.ACCEPTOR_STATE), Guard(ar, G, np.int32)
        g_eff, g_ex = Guard(ar, n_msgs, np.uint8), Guard(ar, G, np.int32)
        d_inst, d_sends, d_meta = ar.put(inst), ar.put(sends), ar.put(meta)
        d_op, d_key, d_val = ar.put(op), ar.put(key), ar.put(val)
        g_op, g_key, g_val = Guard(ar, cap, np.uint8), Guard(ar, cap, np.int64), Guard(ar, cap, np.int64)
        g_mask, g_if = Guard(ar, n_inst, np.uint8), Guard(ar, n_inst, np.uint64)
        g_rf, g_go = Guard(ar, n_inst, np.uint64), Guard(ar, G + 1, np.uint64)
        g_xres, g_ret = Guard(ar, 1, R.EXECUTE_RESULT), Guard(ar, cap, np.int64)
        g_recs, g_rres = Guard(ar, cap, R.REPLY_REC), Guard(ar, 1, R.REPLY_RESULT)
        g_rout = Guard(ar, cap * R.PROPOSE_REPLY_BYTES, np.uint8)
        g_roff = Guard(ar, n_clients + 2, np.uint64)
        outs = [g_eff, g_op, g_key, g_val, g_mask, g_if, g_rf, g_go, g_xres, g_ret, g_recs, g_rres,
                g_rout, g_roff]
        xb = e.execute_batch_dev(d_inst, n_inst, base, ipg, G, g_cu, g_ex, g_ex, d_op, d_key, d_val, m,
                                 d_sends, n_inst, pad=True, general=general)
        xo = e.execute_out_dev(g_op, g_key, g_val, cap, g_mask, g_if, g_rf, g_go)
        rb = e.reply_batch_dev(R.RB_EXECUTED, d_sends, n_inst, d_meta, m, g_mask, n_inst, base, g_ret,
                               cap, g_rf, pad_client=n_clients)
        e.execute_gather_reserve(n_inst, G)
        e.apply_reserve(cap)
        e.build_replies_reserve(n_inst)
        e.encode_replies_reserve(cap)
        s = e.stream_create()
        e.graph_begin(s)
        e.commit_handle_dev(d_msgs.ptr, n_msgs, g_st.ptr, n_inst, base, g_cu.ptr, G, ipg, g_eff.ptr, None, s)
        e.execute_gather_dev(xb, xo, g_xres.ptr, s)
        e.apply_dev(g_op.ptr, g_key.ptr, g_val.ptr, cap, g_ret.ptr, None, s)
        e.build_replies_dev(rb, g_recs.ptr, cap, None, g_rres.ptr, s)
        e.encode_replies_dev(g_recs.ptr, cap, n_clients + 1, 1, 0, g_rout.ptr, g_roff.ptr, s)
        gr = e.graph_end(s)
        try:
            for x in inputs:
                for y in outs:
                    y.fill(s)
                src = ar.put(x["msgs"], s)
                e.memcpy(d_msgs.ptr, src.ptr, src.nbytes, D2D, s)
                g_st.put(x["st"], s)
                g_cu.put(none, s)
                g_ex.put(none, s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                wx, wr = x["wx"], x["wr"]
                assert np.array_equal(g_cu.assert_margins(), x["w_cu"])
                assert g_st.assert_margins().tobytes() == x["w_st"].tobytes()
                assert g_xres.assert_margins()[0].tobytes() == wx["res"].tobytes()
                assert np.array_equal(g_ex.assert_margins(), wx["executed"])
                for g, name in ((g_op, "op"), (g_key, "key"), (g_val, "val"), (g_mask, "mask"),
                                (g_if, "inst_first"), (g_rf, "ret_first"), (g_go, "grp_cmd_off")):
                    assert np.array_equal(g.assert_margins(), wx[name]), name
                assert np.array_equal(g_ret.assert_margins(), x["ret"])
                assert g_rres.assert_margins()[0].tobytes() == wr["res"].tobytes()
                assert g_recs.assert_margins().tobytes() == wr["recs"].tobytes()
                roff, rout = g_roff.assert_margins(), g_rout.assert_margins()
                runs = _reply_bytes(wr["recs"], n_clients + 1)
                for k in range(n_clients + 1):
                    assert rout[int(roff[k]):int(roff[k + 1])].tobytes() == runs[k], k
                n_real = int(wr["res"]["n_replies"])
                assert int(roff[n_clients]) == n_real * R.PROPOSE_REPLY_BYTES  # the last run is the pad
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()

"""GPU tests of store assembly (mpx_store_commands, mpx_store_compact and their _dev forms): the
batch's instance commands appended to the command arena and the arena's compaction, bit-exact
against tests/store_translit.py (the Go's assignments over Go-shaped objects). Every case runs the
host form and the _dev form, the latter with the arena, the window, the cursor and the result on
devguard.Guard buffers exactly their capacity long (op bytes at odd addresses, key / val at both
alignments mod 16), and, whenever the call is within the one-launch bounds, both the one-launch
kernel and the general path (general=True, the documented MPX_SC_GENERAL flag) against the same
bytes. Shapes are the smallest that reach the edges: the item passes take 256 items per workgroup,
the scans 4096 items per tile, the copy 1024 arena positions per tile, four per thread, cut at
multiples of four of the arena index. The error cases are reported through the error word or
refused before any launch: no case provokes a fault."""
import ctypes as C

import numpy as np
import pytest

import store_kat
import store_translit as T
import test_store_translit as TT
from devguard import Guard
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import Arena
from minpaxos_amd.engine import MpxError

N = 3
TILE = 1024
OUT = ("op", "key", "val", "used", "inst", "res")


def _code(f, *a, **k):
    try:
        f(*a, **k)
    except MpxError as ex:
        return ex.code
    return R.OK


def args_of(case):
    return {k: v for k, v in case.items() if k not in ("handler",)}


def want_of(case, **kw):
    return T.store_commands(**dict(case, **kw))


def run_host(e, case, general):
    arena = tuple(np.array(x, copy=True) for x in case["arena"])
    inst = case["inst"].copy()
    used, res = e.store_commands(case["kind"], case["items"], case["sources"], arena, case["used"], inst,
                                 case.get("inst_base", 0), case.get("effect"), case.get("perm"),
                                 case.get("store_mask", R.AH_STORED), general)
    return dict(op=arena[0], key=arena[1], val=arena[2], used=used, inst=inst, res=res)


def dev_sources(ar, sources):
    out = []
    for x in sources:
        off = x.get("cmd_off")
        k = len(x["op"])
        out.append(dict(cmd_off=None if off is None else ar.put(np.asarray(off, np.uint64)),
                        n_frames=0 if off is None else len(off) - 1,
                        op=Guard(ar, k, np.uint8, shift=3).put(x["op"]) if k else None,
                        key=ar.put(np.asarray(x["key"], np.int64)) if k else None,
                        val=ar.put(np.asarray(x["val"], np.int64)) if k else None,
                        n_cmds=k, n_recs=x["n_recs"]))
    return out


def dev_call(e, ar, case, general, op_shift=1, kv_shift=0, d_n=None):
    """the call's inputs on the device and its in/out arrays on guards; returns (batch, arena, guards)"""
    a_op, a_key, a_val = case["arena"]
    cap, n, n_inst = len(a_op), len(case["items"]), len(case["inst"])
    g = dict(op=Guard(ar, cap, np.uint8, shift=op_shift).put(a_op),
             key=Guard(ar, cap, np.int64, shift=kv_shift).put(a_key),
             val=Guard(ar, cap, np.int64, shift=kv_shift).put(a_val),
             used=Guard(ar, 1, np.uint64).put(np.array([case["used"]], np.uint64)),
             inst=Guard(ar, n_inst, R.INST_CMDS).put(case["inst"]), res=Guard(ar, 1, R.STORE_RESULT))
    eff, perm = case.get("effect"), case.get("perm")
    b = e.store_batch_dev(case["kind"], ar.put(case["items"]) if n else None, n,
                          dev_sources(ar, case["sources"]), n_inst, case.get("inst_base", 0),
                          None if eff is None or not n else Guard(ar, n, np.uint8, shift=5).put(eff),
                          None if perm is None or not n else ar.put(np.asarray(perm, np.uint32)),
                          None if d_n is None else ar.put(np.array([d_n], np.uint64)),
                          case.get("store_mask", R.AH_STORED), general)
    a = e.store_arena_dev(g["op"] if cap else None, g["key"] if cap else None, g["val"] if cap else None,
                          cap, g["used"])
    return b, a, g


def read_dev(g):
    got = {name: g[name].assert_margins() for name in OUT}
    got["used"], got["res"] = int(got["used"][0]), got["res"][0]
    return got


def run_dev(e, case, general, op_shift=1, kv_shift=0, d_n=None):
    """returns (outputs, code of the next synchronising call)"""
    with Arena(e) as ar:
        b, a, g = dev_call(e, ar, case, general, op_shift, kv_shift, d_n)
        e.store_commands_reserve(len(case["items"]))
        e.store_commands_dev(b, a, g["inst"] if len(case["inst"]) else None, g["res"])
        code = _code(e.synchronize)
        return read_dev(g), code


def same(got, want, what):
    for name in OUT:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.tobytes() != b.tobytes():
            assert a.shape == b.shape, (what, name, a.shape, b.shape)
            diff = np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:5] if a.shape else []
            raise AssertionError(f"{what}: {name} differs at {list(diff)}: got "
                                 f"{a.reshape(-1)[diff] if a.shape else a} want "
                                 f"{b.reshape(-1)[diff] if b.shape else b}")


def paths_of(case):
    """general = False always; True as well when the default would take the one-launch kernel"""
    one = len(case["items"]) <= R.SC_ONE_LAUNCH_ITEMS and \
        sum(len(s["op"]) for s in case["sources"]) <= R.SC_ONE_LAUNCH_CMDS
    return (False, True) if one else (False,)


def check(e, case, forms=("host", "dev"), shifts=((1, 0),)):
    want = want_of(case)
    assert want["code"] == R.OK
    for general in paths_of(case):
        if "host" in forms:
            same(run_host(e, case, general), want, f"host general={general}")
        if "dev" in forms:
            for op_shift, kv_shift in shifts:
                got, code = run_dev(e, case, general, op_shift, kv_shift)
                assert code == R.OK
                same(got, want, f"dev general={general} shifts={op_shift},{kv_shift}")
    return want


def mk_case(sizes, instances, stores=None, used=0, extra=3, base=100, inst=None, seed=0):
    """one connection's messages in arrival order: item i names instances[i] (relative to base) and
    frame i, of sizes[i] commands; it stores unless stores[i] is false"""
    n = len(sizes)
    stores = np.ones(n, bool) if stores is None else np.asarray(stores, bool)
    src = T.mk_source(sizes, seed=seed, gap=2)
    items = T.mk_msgs([(base + int(instances[i]), i) for i in range(n)])
    eff = np.where(stores, R.AH_STORED | R.AH_REPLIED, R.AH_REPLIED).astype(np.uint8)
    if inst is None:
        inst = T.mk_window(int(max(instances)) + 2 if n else 1, used, 0.3, np.random.default_rng(600 + seed))
    case = dict(kind=R.SC_MSGS, items=items, effect=eff, sources=[src], used=used, inst_base=base, inst=inst)
    total = int(want_of(dict(case, arena=T.mk_arena(0), used=0))["res"]["n_cmds"])
    case["arena"] = T.mk_arena(used + total + extra, seed)
    return case


@pytest.fixture
def eng(mk_engine):
    return mk_engine(N, R.MODE_MIN)


# ---- the known answers ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", store_kat.KAT_STORE, ids=lambda c: c["name"])
def test_known_answers(eng, case):
    args = store_kat.kat_args(case)
    want = check(eng, args, shifts=((1, 0), (0, 8), (3, 8)))
    store_kat.check(case, want)
    store_kat.check(case, run_host(eng, args, False))


@pytest.mark.gpu
def test_known_compaction(eng):
    c = store_kat.KAT_COMPACT
    for form in ("host", "dev"):
        got = run_compact(eng, c["inst"], store_kat.arena(c["cap"]), c["used"], c["to_cap"], form,
                          fill=tuple(np.zeros(c["to_cap"], t) for t in (np.uint8, np.int64, np.int64)))
        store_kat.check_compact(got)


# ---- shapes --------------------------------------------------------------------------------------
def shape_case(n, seed=0, used=5):
    """n items in runs of one to four per instance, a third not storing, commands per item from
    {0, 1, 2, 3}"""
    rng = np.random.default_rng(700 + n + seed)
    runs = rng.choice([1, 1, 2, 3, 4], n + 1)
    instances = np.repeat(np.arange(len(runs)) * 2, runs)[:n]
    sizes = rng.choice([0, 1, 2, 3], n, p=[0.15, 0.45, 0.25, 0.15])
    return mk_case(sizes, instances, rng.random(n) > 0.33, used=used, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_item_counts_around_the_wave_the_workgroup_and_the_scan_tile(eng, n):
    want = check(eng, shape_case(n), shifts=((1, 0), (2, 8)))
    if n >= 63:
        assert int(want["res"]["n_superseded"]) > 0 and int(want["res"]["n_stored"]) > n // 4


@pytest.mark.gpu
@pytest.mark.parametrize("total", [TILE - 1, TILE, TILE + 1, 8 * TILE - 1, 8 * TILE, 8 * TILE + 1])
def test_totals_and_item_boundaries_around_the_copy_tile(eng, total):
    """an item boundary at every position from 2 before to 2 after a tile boundary, from cursors
    at every residue mod 4 (the tiles are cut by the arena index), op at four alignments and key /
    val on a 16-byte line and in the middle of one"""
    edge = TILE if total <= TILE + 1 else 8 * TILE
    for d, used in ((-2, 0), (-1, 1), (0, 2), (1, 3), (2, 6)):
        k = min(edge + d, total)
        sizes = [k - 7, 0, 7, total - k]
        check(eng, mk_case(sizes, [0, 1, 2, 3], used=used, extra=0),
              shifts=((1, 0), (2, 8), (3, 0), (0, 8)))
    # ... and built from items of 16 and 17 commands, every fourth superseded
    sizes = [17] * (total // 17 - 1) + [16]
    sizes += [total - sum(sizes)]
    instances = np.arange(len(sizes)) - (np.arange(len(sizes)) % 4 == 1)
    check(eng, mk_case(sizes, instances, used=9))


@pytest.mark.gpu
def test_one_item_of_5000_commands(eng):
    """the replica batch: one launch by default"""
    want = check(eng, mk_case([5000], [0], used=3), shifts=((1, 0), (1, 8)))
    assert int(want["res"]["n_cmds"]) == 5000


@pytest.mark.gpu
@pytest.mark.parametrize("n,lo,hi", [(200, 60, 70), (1300, 250, 260), (4300, 4000, 4200)])
def test_a_run_of_one_instance_across_a_boundary(eng, n, lo, hi):
    """items lo .. hi - 1 name one instance and all store: the winner is the last of them, in a later
    wave / workgroup / scan tile than the first"""
    instances = np.arange(n) * 2
    instances[lo:hi] = instances[lo]
    sizes = np.ones(n, np.int64) + (np.arange(n) % 3 == 0)
    stores = np.ones(n, bool)
    stores[hi - 1] = n != 1300            # ... or the last but one, the last not storing
    want = check(eng, mk_case(sizes, instances, stores, used=2))
    assert int(want["res"]["n_superseded"]) == hi - lo - 1 - (n == 1300)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 2000])
def test_a_run_covering_the_whole_batch(eng, n):
    want = check(eng, mk_case(np.full(n, 2), np.zeros(n, np.int64), used=1))
    assert int(want["res"]["n_stored"]) == 1 and int(want["res"]["n_cmds"]) == 2
    assert int(want["res"]["n_superseded"]) == n - 1


@pytest.mark.gpu
def test_d_n_smaller_than_n(eng):
    for n, d_n in ((300, 123), (2000, 1500), (50, 0), (50, 70)):
        case = shape_case(n, seed=3)
        want = want_of(case, dev=True, d_n=d_n)
        assert want["code"] == R.OK
        for general in paths_of(case):
            got, code = run_dev(eng, case, general, d_n=d_n)
            assert code == R.OK
            same(got, want, f"d_n={d_n} general={general}")
    assert int(want_of(shape_case(300, seed=3), dev=True, d_n=123)["res"]["n_stored"]) < \
        int(want_of(shape_case(300, seed=3))["res"]["n_stored"])


@pytest.mark.gpu
def test_a_window_of_2_to_the_20_slots_with_100_items(eng):
    """nothing depends on n_inst: the untouched slots keep a poison pattern, byte for byte"""
    n_inst = 1 << 20
    rng = np.random.default_rng(20)
    instances = np.sort(rng.choice(n_inst, 60, replace=False))
    instances = np.repeat(instances, rng.choice([1, 2, 3], 60))[:100]
    inst = np.zeros(n_inst, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"], inst["flags"] = 0x0123456789ABCDEF, 0xDEADBEEF, 0xFFFFFFFE
    case = mk_case(rng.integers(0, 5, 100), instances, rng.random(100) > 0.2, used=7, inst=inst)
    want = check(eng, case)
    changed = np.flatnonzero(want["inst"]["flags"] == R.IC_HAS_CMDS)
    assert len(changed) == int(want["res"]["n_stored"]) and set(changed) <= set(instances.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 1500])
def test_full_by_one_changes_nothing(eng, n):
    case = shape_case(n, seed=5)
    total = int(want_of(case)["res"]["n_cmds"])
    case["arena"] = tuple(x[:case["used"] + total - 1].copy() for x in case["arena"])
    want = check(eng, case)
    assert int(want["res"]["flags"]) == R.SC_FULL and want["used"] == case["used"]
    assert want["inst"].tobytes() == case["inst"].tobytes()
    assert all(want[k].tobytes() == x.tobytes() for k, x in zip(("op", "key", "val"), case["arena"]))
    case["arena"] = T.mk_arena(case["used"] + total, 5)     # exactly full
    assert int(check(eng, case)["res"]["flags"]) == 0


# ---- fuzz ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(24))
def test_fuzz(eng, seed):
    check(eng, args_of(T.fuzz_case(seed)), shifts=((1 + seed % 3, 8 * (seed & 1)),))


# ---- rejections ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fault", TT.FAULTS)
def test_a_faulty_item_by_error_word_and_by_code(eng, fault):
    """the host form answers before any launch; the _dev form raises the error word, the item
    neither stores nor supersedes, and the others are exact"""
    case = TT.faulty(fault)
    code = R.E_NIL_INSTANCE if "window" in fault else R.E_INVAL
    want = want_of(case, dev=True)
    assert want["code"] == code
    for general in (False, True):
        assert _code(run_host, eng, case, general) == code
        got, got_code = run_dev(eng, case, general)
        assert got_code == code
        same(got, want, f"dev general={general}")
    check(eng, mk_case([2, 3], [0, 1]))      # the handle is clean again


@pytest.mark.gpu
def test_a_cursor_past_the_capacity(eng):
    case = dict(TT._two(), used=9)
    want = want_of(case, dev=True)
    for general in (False, True):
        assert _code(run_host, eng, case, general) == R.E_INVAL
        got, code = run_dev(eng, case, general)
        assert code == R.E_INVAL
        same(got, want, f"general={general}")


@pytest.mark.gpu
def test_argument_rejections(eng):
    e = eng
    case = mk_case([2, 3, 1], [0, 1, 1])
    two = dict(case, sources=[dict(case["sources"][0], n_recs=2), dict(case["sources"][0], n_recs=1)],
               perm=np.arange(3, dtype=np.uint32))
    inst, res = case["inst"].copy(), _lib.MpxStoreResult()
    arena = tuple(x.copy() for x in case["arena"])
    cur = np.array([0], np.uint64)
    keep = []

    def ptr_of(x, k, t):
        keep.append(np.ascontiguousarray(x, t))
        return keep[-1].ctypes.data_as(C.c_void_p)
    src1, _ = e._store_srcs(case["sources"], ptr_of)
    src2, _ = e._store_srcs(two["sources"], ptr_of)
    p = [x.ctypes.data_as(C.c_void_p) for x in (case["items"], case["effect"], two["perm"], *arena, cur, inst)]

    def host(with_res=True, **kw):
        f = dict(kind=R.SC_MSGS, flags=0, items=p[0], effect=p[1], n=3, d_n=None, perm=None, src=src1,
                 n_src=1, n_inst=len(inst), inst_base=100, store_mask=2, reserved=0)
        a = dict(op=p[3], key=p[4], val=p[5], cap=len(arena[0]), used=p[6])
        f.update({k: v for k, v in kw.items() if k in f})
        a.update({k: v for k, v in kw.items() if k in a})
        cur[0] = kw.get("cursor", 0)
        return e.lib.mpx_store_commands(e.h, C.byref(_lib.MpxStoreBatch(**f)), C.byref(_lib.MpxStoreArena(**a)),
                                        None if kw.get("no_inst") else p[7], C.byref(res) if with_res else None)
    assert host() == R.OK and (res.n_stored, res.n_cmds, res.n_superseded) == (2, 3, 1)
    for name in ("items", "effect", "src", "op", "key", "val", "used"):
        assert host(**{name: None}) == R.E_INVAL, name
    assert host(with_res=False) == R.E_INVAL and host(no_inst=True) == R.E_INVAL
    assert host(kind=2) == R.E_INVAL and host(flags=2) == R.E_INVAL and host(reserved=1) == R.E_INVAL
    assert host(n_src=0) == R.E_INVAL and host(n_src=17) == R.E_INVAL
    assert host(d_n=p[6]) == R.E_INVAL
    assert host(src=src2, n_src=2) == R.E_INVAL                     # two sources need perm
    assert host(src=src2, n_src=2, perm=p[2]) == R.OK
    assert host(n=4) == R.E_INVAL                                   # more items than records
    assert host(cursor=len(arena[0]) + 1) == R.E_INVAL
    assert host(kind=R.SC_SENDS, src=src2, n_src=2) == R.E_INVAL
    assert host(n=0xFFFFFFFF) == R.E_UNSUPPORTED
    assert _code(e.store_commands_reserve, 0xFFFFFFFF) == R.E_UNSUPPORTED
    assert _code(e.store_compact_reserve, 0xFFFFFFFF) == R.E_UNSUPPORTED
    # the device form's alignment rules
    with Arena(e) as ar:
        b, a, g = dev_call(e, ar, dict(two, used=0), False, op_shift=0)
        e.store_commands_reserve(3)

        def dev(field=None, by=0, inst_by=0, res_by=0, src_field=None):
            x, y = _lib.MpxStoreBatch.from_buffer_copy(b), _lib.MpxStoreArena.from_buffer_copy(a)
            for s in (x, y):
                if field and hasattr(s, field):
                    setattr(s, field, getattr(s, field) + by)
            if src_field:
                arr = (_lib.MpxStoreSrc * 2)(b.src[0], b.src[1])
                setattr(arr[1], src_field, getattr(arr[1], src_field) + by)
                x.src = arr
                keep.append(arr)
            return _code(e.store_commands_dev, x, y, g["inst"].ptr + inst_by, g["res"].ptr + res_by)
        for field, by in (("items", 8), ("perm", 2), ("d_n", 4), ("key", 4), ("val", 4), ("used", 4)):
            if field == "d_n":
                b.d_n = g["used"].ptr
            assert dev(field, by) == R.E_INVAL, field
            b.d_n = None
        for field in ("cmd_off", "key", "val"):
            assert dev(src_field=field, by=4) == R.E_INVAL, field
        assert dev(inst_by=8) == R.E_INVAL and dev(res_by=4) == R.E_INVAL
        e.synchronize()
        for name, x in g.items():
            x.assert_margins()
        g["res"].assert_untouched([(0, 1)])
        assert int(g["used"].payload()[0]) == 0
        # op bytes and effect may sit anywhere (one byte further is inside the guards' margins)
        assert dev(src_field="op", by=1) in (R.OK,)
        e.synchronize()
    del keep


@pytest.mark.gpu
def test_dev_forms_need_their_reserve_and_never_grow(mk_engine):
    e = mk_engine(N, R.MODE_CLASSIC)
    small, big = mk_case([2, 3], [0, 1]), shape_case(3000, seed=8)
    with Arena(e) as ar:
        b, a, g = dev_call(e, ar, small, True)
        with pytest.raises(MpxError) as ei:
            e.store_commands_dev(b, a, g["inst"], g["res"])
        assert ei.value.code == R.E_INVAL and "mpx_store_commands_reserve" in str(ei.value)
        to = e.store_arena_dev(ar.empty(8, np.uint8), ar.empty(8, np.int64), ar.empty(8, np.int64), 8,
                               ar.empty(1, np.uint64))
        with pytest.raises(MpxError) as ei:
            e.store_compact_dev(g["inst"], len(small["inst"]), a, to, g["res"])
        assert ei.value.code == R.E_INVAL and "mpx_store_compact_reserve" in str(ei.value)
        e.store_commands_reserve(2)
        e.store_commands_dev(b, a, g["inst"], g["res"])
        e.synchronize()
        assert g["res"].assert_margins()[0].tolist() == (2, 5, 0, 0)
        b2, a2, g2 = dev_call(e, ar, big, False)
        assert _code(e.store_commands_dev, b2, a2, g2["inst"], g2["res"]) == R.E_INVAL
        assert _code(e.store_compact_dev, g2["inst"], 1 << 16, a2, to, g2["res"]) == R.E_INVAL
        e.synchronize()
        g2["res"].assert_untouched([(0, 1)])
        assert g2["inst"].assert_margins().tobytes() == big["inst"].tobytes()
    check(e, big)
    check(e, small)


# ---- compaction ----------------------------------------------------------------------------------
def run_compact(e, inst, arena, used, to_cap, form, fill=None, kv_shift=0):
    """returns the outputs as store_translit.store_compact names them (+ code for the dev form)"""
    fill = T.mk_arena(to_cap, 77) if fill is None else fill
    if form == "host":
        inst, to = inst.copy(), tuple(x.copy() for x in fill)
        t_used, res = e.store_compact(inst, arena, used, to)
        full = int(res["flags"]) & R.SC_FULL
        return dict(op=to[0], key=to[1], val=to[2], used=None if full else t_used, inst=inst, res=res,
                    code=R.OK)
    with Arena(e) as ar:
        n, cap = len(inst), len(arena[0])
        f = e.store_arena_dev(Guard(ar, cap, np.uint8, shift=3).put(arena[0]) if cap else None,
                              ar.put(arena[1]) if cap else None, ar.put(arena[2]) if cap else None, cap,
                              ar.put(np.array([used], np.uint64)))
        g = dict(op=Guard(ar, to_cap, np.uint8, shift=1).put(fill[0]),
                 key=Guard(ar, to_cap, np.int64, shift=kv_shift).put(fill[1]),
                 val=Guard(ar, to_cap, np.int64, shift=kv_shift).put(fill[2]),
                 used=Guard(ar, 1, np.uint64), inst=Guard(ar, n, R.INST_CMDS).put(inst),
                 res=Guard(ar, 1, R.STORE_RESULT))
        t = e.store_arena_dev(g["op"] if to_cap else None, g["key"] if to_cap else None,
                              g["val"] if to_cap else None, to_cap, g["used"])
        e.store_compact_reserve(n)
        e.store_compact_dev(g["inst"] if n else None, n, f, t, g["res"])
        code = _code(e.synchronize)
        got = {name: g[name].assert_margins() for name in OUT}
        got["res"] = got["res"][0]
        if int(got["res"]["flags"]) & R.SC_FULL:
            g["used"].assert_untouched([(0, 1)])
            got["used"] = None
        else:
            got["used"] = int(got["used"][0])
        return dict(got, code=code)


def same_compact(got, want, what):
    assert got["used"] == want["used"], (what, got["used"], want["used"])
    same(dict(got, used=0), dict(want, used=0), what)


def compact_case(ipg, groups, seed=0):
    """a window of ipg * groups slots in an arena the batches of a few turns filled: about a quarter
    retired, some never filled, lengths from {0, 1, 2, 3, 17}"""
    rng = np.random.default_rng(800 + ipg * 7 + groups + seed)
    n = ipg * groups
    lens = rng.choice([0, 1, 2, 3, 17], n, p=[0.1, 0.4, 0.25, 0.2, 0.05])
    order = rng.permutation(n)                   # the slots were stored in some other order
    first = np.zeros(n, np.int64)
    first[order] = 3 + np.concatenate([[0], np.cumsum(lens[order] + (rng.random(n) < 0.2))])[:n]
    used = int(first.max() + lens.max()) + 2 if n else 5
    inst = np.zeros(n, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"] = first, lens
    inst["flags"] = np.where(rng.random(n) < 0.7, R.IC_HAS_CMDS, 0)
    never = rng.random(n) < 0.05
    inst["first_cmd"][never], inst["n_cmds"][never], inst["flags"][never] = 0xDEAD, 0xBEEF, 0
    return inst, T.mk_arena(used + 4, seed), used


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("ipg", [1, 65, 1025])
def test_compaction(eng, ipg, groups):
    inst, arena, used = compact_case(ipg, groups)
    total = int(inst["n_cmds"][inst["flags"] == R.IC_HAS_CMDS].sum())
    for to_cap in (total, total + 5) + ((total - 1,) if total else ()):
        fill = T.mk_arena(to_cap, 77)
        want = T.store_compact(inst, arena, used, to_cap, fill=fill)
        assert want["code"] == R.OK and (int(want["res"]["flags"]) == R.SC_FULL) == (to_cap < total)
        same_compact(run_compact(eng, inst, arena, used, to_cap, "host", fill), want, "host")
        for kv_shift in (0, 8):
            same_compact(run_compact(eng, inst, arena, used, to_cap, "dev", fill, kv_shift), want, "dev")


@pytest.mark.gpu
def test_compaction_of_an_empty_window(eng):
    arena = T.mk_arena(6)
    for form in ("host", "dev"):
        got = run_compact(eng, np.zeros(0, R.INST_CMDS), arena, 4, 3, form)
        assert got["used"] == 0 and got["res"].tolist() == (0, 0, 0, 0) and got["code"] == R.OK
        assert got["key"].tobytes() == T.mk_arena(3, 77)[1].tobytes()


@pytest.mark.gpu
def test_compaction_of_a_faulty_slot_by_error_word_and_by_code(eng):
    c = store_kat.KAT_COMPACT
    inst = c["inst"].copy()
    inst[2] = (5, 2, R.IC_HAS_CMDS)
    arena = store_kat.arena(8)
    with pytest.raises(MpxError) as ei:
        run_compact(eng, inst, arena, 6, 4, "host")
    assert ei.value.code == R.E_INVAL
    fill = T.mk_arena(4, 77)
    got = run_compact(eng, inst, arena, 6, 4, "dev", fill)
    assert got["code"] == R.E_INVAL
    same_compact(got, T.store_compact(inst, arena, 6, 4, dev=True, fill=fill), "dev")
    with pytest.raises(MpxError):
        run_compact(eng, c["inst"], arena, 9, 4, "host")           # the cursor past the capacity
    lib, res = eng.lib, _lib.MpxStoreResult()
    a = [x.copy() for x in arena]
    cur = np.array([6, 0], np.uint64)
    f = _lib.MpxStoreArena(*[x.ctypes.data_as(C.c_void_p) for x in a], 8, cur.ctypes.data_as(C.c_void_p))
    t = _lib.MpxStoreArena(a[0].ctypes.data + 4, a[1].ctypes.data_as(C.c_void_p),
                           a[2].ctypes.data_as(C.c_void_p), 4, cur.ctypes.data + 8)
    w = c["inst"].copy()
    assert lib.mpx_store_compact(eng.h, w.ctypes.data_as(C.c_void_p), 4, C.byref(f), C.byref(t),
                                 C.byref(res)) == R.E_INVAL          # from and to overlap
    assert lib.mpx_store_compact(eng.h, None, 4, C.byref(f), C.byref(t), C.byref(res)) == R.E_INVAL
    assert w.tobytes() == c["inst"].tobytes()


@pytest.mark.gpu
def test_store_then_compact_then_store(eng):
    """two turns' batches into one arena, the first turn's instances retired, the rest squeezed into
    a second arena, a third batch appended there: the windows and arenas equal the transliteration's
    at every step, host and _dev form alike"""
    turns = [shape_case(700, seed=s, used=0) for s in (11, 12, 13)]
    n_inst = max(len(c["inst"]) for c in turns)
    for form in ("host", "dev"):
        inst = np.zeros(n_inst, R.INST_CMDS)
        arena, used = T.mk_arena(6000, 1), 0
        w_inst, w_arena, w_used = inst.copy(), arena, 0
        for turn, c in enumerate(turns):
            if turn == 2:      # retire what the first turn stored, compact
                first = T.store_commands(**dict(turns[0], arena=T.mk_arena(6000, 1), used=0,
                                                inst=np.zeros(n_inst, R.INST_CMDS)))["inst"]
                retired = np.flatnonzero(first["flags"])[::2]
                inst["flags"][retired] = 0
                w_inst["flags"][retired] = 0
                fill = T.mk_arena(5000, 2)
                want = T.store_compact(w_inst, w_arena, w_used, 5000, fill=fill)
                got = run_compact(eng, inst, arena, used, 5000, form, fill)
                same_compact(got, want, f"{form} compact")
                assert 0 < want["used"] < w_used
                inst, arena, used = got["inst"], (got["op"], got["key"], got["val"]), got["used"]
                w_inst, w_arena, w_used = want["inst"], (want["op"], want["key"], want["val"]), want["used"]
            case = dict(c, arena=arena, used=used, inst=inst)
            want = want_of(dict(c, arena=w_arena, used=w_used, inst=w_inst))
            got = run_host(eng, case, False) if form == "host" else run_dev(eng, case, False)[0]
            same(got, want, f"{form} turn {turn}")
            inst, arena, used = got["inst"], (got["op"], got["key"], got["val"]), got["used"]
            w_inst, w_arena, w_used = want["inst"], (want["op"], want["key"], want["val"]), want["used"]
        assert used > 0 and int(inst["flags"].sum()) > 250


# ---- the chains ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True])
def test_graph_of_decode_propose_handle_and_store_sends(mk_engine, general):
    """mpx_decode_client_streams_dev -> mpx_propose_handle_dev -> mpx_store_commands_dev(MPX_SC_SENDS),
    captured once into a graph and replayed on two inputs (new connection lengths and bytes, same
    pointers), against the client, proposer and store transliterations: the installed instances'
    commands land in the arena and their slots name them, with no host step in between"""
    import client_translit as CL
    import proposer_translit as PT
    import test_gpu_client as TC
    from minpaxos_amd.devbuf import D2D
    NR = 5
    e = mk_engine(NR, R.MODE_MIN)
    G, per_group, slot, ipg, base, D = 3, 4, 1024, 8, 50, 32
    n_inst, n_conns = G * ipg, G * per_group
    rng = np.random.default_rng(5)
    used0, inst0 = 5, T.mk_window(n_inst, 5, 0.3, rng)
    inputs = []
    for seed in (11, 12):
        bufs, groups = TC._chain_input(seed, G, per_group, slot)
        wc = CL.decode_client_streams(bufs, groups, G)
        grp = PT.mk_groups([(D, 0, 0, 3, base + g * ipg, base + g * ipg - 1) for g in range(G)])
        st, lb = PT.nil_state(n_inst), np.zeros(n_inst, R.INST_STATE)
        wp = PT.propose_handle(R.MODE_MIN, NR, grp, wc["prop_off"], st, base, ipg, lb)
        assert len(wp[3]) == G and (wp[3]["flags"] == R.PH_ACCEPT).all()
        buf = np.zeros(n_conns * slot, np.uint8)
        conns = np.zeros(n_conns, R.CLIENT_CONN)
        for k, b in enumerate(bufs):
            conns[k] = (k * slot, len(b), groups[k])
            buf[k * slot:k * slot + len(b)] = np.frombuffer(b, np.uint8)
        inputs.append(dict(buf=buf, conns=conns, grp=grp, st=st, lb=lb, wc=wc, wp=wp))
    cap = n_conns * slot // 30
    a_cap = used0 + max(int(x["wc"]["res"]["n_proposals"]) for x in inputs) + 3
    arena0 = T.mk_arena(a_cap, 3)
    for x in inputs:
        wc = x["wc"]
        x["ws"] = T.store_commands(R.SC_SENDS, x["wp"][3], [dict(cmd_off=None, op=wc["op"], key=wc["key"],
                                                                val=wc["val"], n_recs=G)],
                                   arena0, used0, inst0, base)
        assert x["ws"]["code"] == R.OK and int(x["ws"]["res"]["n_stored"]) == G
    assert inputs[0]["ws"]["used"] != inputs[1]["ws"]["used"]
    with Arena(e) as ar:
        g, g_buf, d_conns, out = TC.dev_buffers(ar, inputs[0]["buf"], inputs[0]["conns"], G, cap)
        g_grp, g_st = Guard(ar, G, R.PROPOSER_GROUP), Guard(ar, n_inst, R.ACCEPTOR_STATE)
        g_lb, g_snd = Guard(ar, n_inst, R.INST_STATE), Guard(ar, G, R.ACCEPT_SEND)
        s_g = dict(op=Guard(ar, a_cap, np.uint8, shift=1), key=Guard(ar, a_cap, np.int64, shift=8),
                   val=Guard(ar, a_cap, np.int64), used=Guard(ar, 1, np.uint64),
                   inst=Guard(ar, n_inst, R.INST_CMDS), res=Guard(ar, 1, R.STORE_RESULT))
        sb = e.store_batch_dev(R.SC_SENDS, g_snd, G, [dict(cmd_off=None, n_frames=0, op=g["op"], key=g["key"],
                                                           val=g["val"], n_cmds=cap, n_recs=G)],
                               n_inst, base, general=general)
        sa = e.store_arena_dev(s_g["op"], s_g["key"], s_g["val"], a_cap, s_g["used"])
        e.decode_client_streams_reserve(len(inputs[0]["buf"]), n_conns, G)
        e.store_commands_reserve(G)
        s = e.stream_create()
        e.graph_begin(s)
        e.decode_client_streams_dev(g_buf.ptr, n_conns * slot, d_conns.ptr, n_conns, G, out,
                                    g["conn_res"].ptr, g["res"].ptr, s)
        e.propose_handle_dev(g_grp.ptr, G, g["prop_off"].ptr, g["send_off"].ptr, g_st.ptr, g_lb.ptr,
                             n_inst, base, ipg, g_snd.ptr, s)
        e.store_commands_dev(sb, sa, s_g["inst"], s_g["res"], s)
        gr = e.graph_end(s)
        try:
            for x in inputs + inputs[:1]:
                for y in list(g.values()) + [g_snd, s_g["res"]]:
                    y.fill(s)
                g_buf.put(x["buf"], s)
                g_grp.put(x["grp"], s)
                g_st.put(x["st"], s)
                g_lb.put(x["lb"], s)
                for name, a in zip(("op", "key", "val"), arena0):
                    s_g[name].put(a, s)
                s_g["used"].put(np.array([used0], np.uint64), s)
                s_g["inst"].put(inst0, s)
                src = ar.put(x["conns"], s)
                e.memcpy(d_conns.ptr, src.ptr, src.nbytes, D2D, s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                wc, wp = x["wc"], x["wp"]
                TC.same(TC.read_dev(g, int(wc["res"]["n_proposals"])), wc, cap, "replay")
                assert g_st.assert_margins().tobytes() == wp[1].tobytes()
                assert g_snd.assert_margins().tobytes() == wp[3].tobytes()
                same(read_dev(s_g), x["ws"], f"store general={general}")
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()


def _follower_turn(seed, state, NR, ipg, base, D, used0, inst0, arena0, cap, shorts_at):
    """one follower turn's input and what every station must leave: 24 Accept frames of one leader
    (every instance once, eight resends, which MIN ignores, four with a stale ballot), ten
    CommitShorts, the dict State the executed commands run against"""
    import acceptor_translit as AT
    import commit_translit as CT
    import execute_translit as XT
    import order_translit as OT
    import test_gpu_execute as TX
    import unmarshal_translit as U
    from minpaxos_amd import wire
    rng = np.random.default_rng(seed)

    def cmds():
        return [(int(rng.choice([R.OP_PUT, R.OP_GET])), int(rng.integers(0, 9)), int(rng.integers(1, 1 << 40)))
                for _ in range(int(rng.choice([0, 1, 2, 3, 5])))]
    rows = [(base + k, D, cmds()) for k in range(12)]
    rows += [(base + int(k), D, cmds()) for k in rng.integers(0, 12, 8)]
    rows += [(base + int(k), D - 1, cmds()) for k in rng.integers(0, 14, 4)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    buf = b"".join(wire.accept(R.MODE_MIN, 0, i, b, c, base - 1) for i, b, c in rows)
    var, _ = U.walk(R.MODE_MIN, buf)
    wu, counts = U.expected(R.MODE_MIN, buf, var)
    n = len(rows)
    assert counts["n_accepts"] == n == len(var)
    srt, perm, ores = OT.order_records([wu["accepts"]], ipg, base)
    st0 = AT.mk_state([(AT.NIL, 0, 0, 0)] * ipg)
    groups = AT.mk_groups([(D, 1)])
    w_st, _, _, w_eff = AT.accept_handle(R.MODE_MIN, NR, srt, st0, groups, base, ipg)
    ws = T.store_commands(R.SC_MSGS, srt, [dict(cmd_off=wu["cmd_off"], op=wu["op"], key=wu["key"],
                                                val=wu["val"], n_recs=n)],
                          arena0, used0, inst0, base, effect=w_eff, perm=perm)
    # (MIN ignores a resend of an accepted instance: of an instance's Accepts the first stores)
    assert ws["code"] == R.OK and int(ws["res"]["n_stored"]) == 12 and (w_eff == 0).sum() >= 8
    shorts = CT.mk_msgs([(base + k, D, 0, R.VALUE_KEEP) for k in shorts_at])
    none = np.array([base - 1], np.int32)
    w_st2, w_cu, _, _ = CT.commit_handle(shorts, w_st, none, base, ipg)
    wx = XT.execute_gather(ws["inst"], w_cu, none, (ws["op"], ws["key"], ws["val"]), base, ipg, None, cap,
                           pad=True)
    assert 0 < int(wx["res"]["n_cmds"]) < cap
    ret = TX._execute(state, wx["op"], wx["key"], wx["val"])
    return dict(buf=buf, var=var, wu=wu, counts=counts, srt=srt, perm=perm, ores=ores, st0=st0, groups=groups,
                w_eff=w_eff, ws=ws, shorts=shorts, none=none, w_st2=w_st2, w_cu=w_cu, wx=wx, ret=ret)


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True])
def test_graph_of_a_followers_turn(mk_engine, general):
    """mpx_unmarshal_frames_dev -> mpx_order_records_dev -> mpx_accept_handle_dev ->
    mpx_store_commands_dev (perm and &d_res->n from the order call) -> mpx_commit_handle_dev
    (CommitShorts) -> mpx_execute_gather_dev (pad) -> mpx_apply_dev(m = cap), captured once into a
    graph and replayed on two inputs, against the unmarshal, order, acceptor, store, commit and
    execute transliterations and a Python dict State that lives across the replays"""
    import test_gpu_unmarshal as TU
    from minpaxos_amd.devbuf import H2D
    NR, G, ipg, base, D, cap, used0 = 3, 1, 32, 100, 16, 64, 3
    e = mk_engine(NR, R.MODE_MIN)
    inst0 = T.mk_window(ipg, used0, 0.0, np.random.default_rng(1))
    a_cap = used0 + 24 * 5
    arena0 = T.mk_arena(a_cap, 4)
    state = {}
    inputs = [_follower_turn(31, state, NR, ipg, base, D, used0, inst0, arena0, cap, range(10)),
              _follower_turn(32, state, NR, ipg, base, D, used0, inst0, arena0, cap,
                             list(range(8)) + [10, 11])]
    assert int(inputs[0]["w_cu"][0]) != int(inputs[1]["w_cu"][0])
    n, n_sh = 24, 10
    size = -(-max(len(x["buf"]) for x in inputs) // 16) * 16
    caps = (n, 0, max(x["counts"]["n_cmds"] for x in inputs), 0, 0)
    with Arena(e) as ar:
        d_buf, d_var = ar.empty(size, np.uint8), ar.empty(n, R.VAR_FRAME)
        shape = {"cmd_off": n + 1, "log_inst_off": n + 1, "log_cmd_off": 1}
        g = {name: Guard(ar, shape.get(name, caps[TU.CAP_OF.get(name, 0)]), TU.DTYPES[name], name=name)
             for name in R.UNMARSHAL_ARRAYS}
        g_ures = Guard(ar, 1, R.UNMARSHAL_RESULT)
        out = _lib.MpxUnmarshalOut()
        for name in R.UNMARSHAL_ARRAYS:
            setattr(out, name, g[name].ptr)
        out.accept_cap, out.commit_cap, out.cmd_cap, out.log_inst_cap, out.log_cmd_cap = caps
        g_srt, g_perm = Guard(ar, n, R.ACCEPT_MSG), Guard(ar, n, np.uint32)
        g_ores = Guard(ar, 1, R.ORDER_RESULT)
        g_st, d_groups = Guard(ar, ipg, R.ACCEPTOR_STATE), ar.put(inputs[0]["groups"])
        g_rep, g_to, g_eff = Guard(ar, n, R.ACCEPT_REPLY), Guard(ar, n, np.int32), Guard(ar, n, np.uint8)
        s_g = dict(op=Guard(ar, a_cap, np.uint8, shift=1), key=Guard(ar, a_cap, np.int64, shift=8),
                   val=Guard(ar, a_cap, np.int64), used=Guard(ar, 1, np.uint64),
                   inst=Guard(ar, ipg, R.INST_CMDS), res=Guard(ar, 1, R.STORE_RESULT))
        d_shorts, g_cu, g_ex = ar.empty(n_sh, R.ACCEPT_MSG), Guard(ar, G, np.int32), Guard(ar, G, np.int32)
        g_eff2 = Guard(ar, n_sh, np.uint8)
        x_op, x_key, x_val = Guard(ar, cap, np.uint8), Guard(ar, cap, np.int64), Guard(ar, cap, np.int64)
        x_mask, x_res, g_ret = Guard(ar, ipg, np.uint8), Guard(ar, 1, R.EXECUTE_RESULT), Guard(ar, cap, np.int64)
        sb = e.store_batch_dev(R.SC_MSGS, g_srt, n, [dict(cmd_off=g["cmd_off"], n_frames=n, op=g["op"],
                                                          key=g["key"], val=g["val"], n_cmds=caps[2], n_recs=n)],
                               ipg, base, g_eff, g_perm, g_ores.ptr + R.ORDER_RESULT.fields["n"][1],
                               general=general)
        sa = e.store_arena_dev(s_g["op"], s_g["key"], s_g["val"], a_cap, s_g["used"])
        xb = e.execute_batch_dev(s_g["inst"], ipg, base, ipg, G, g_cu, g_ex, g_ex, s_g["op"], s_g["key"],
                                 s_g["val"], a_cap, pad=True, general=general)
        xo = e.execute_out_dev(x_op, x_key, x_val, cap, x_mask)
        e.unmarshal_frames_reserve(n, 1)
        e.order_records_reserve(n, ipg)
        e.store_commands_reserve(n)
        e.execute_gather_reserve(ipg, G)
        e.apply_reserve(cap)
        s = e.stream_create()
        e.graph_begin(s)
        e.unmarshal_frames_dev(d_buf.ptr, size, d_var.ptr, n, None, out, g_ures.ptr, s)
        e.order_records_dev([(g["accepts"].ptr, None, n)], ipg, base, 0, g_srt.ptr, g_perm.ptr, g_ores.ptr,
                            stream=s)
        e.accept_handle_dev(g_srt.ptr, n, g_st.ptr, g_st.ptr, ipg, base, d_groups.ptr, G, ipg, g_rep.ptr,
                            g_to.ptr, g_eff.ptr, s)
        e.store_commands_dev(sb, sa, s_g["inst"], s_g["res"], s)
        e.commit_handle_dev(d_shorts.ptr, n_sh, g_st.ptr, ipg, base, g_cu.ptr, G, ipg, g_eff2.ptr, None, s)
        e.execute_gather_dev(xb, xo, x_res.ptr, s)
        e.apply_dev(x_op.ptr, x_key.ptr, x_val.ptr, cap, g_ret.ptr, None, s)
        gr = e.graph_end(s)
        try:
            for x in inputs:
                for y in list(g.values()) + [g_srt, g_perm, g_ores, g_eff, s_g["res"], x_op, x_key, x_val,
                                             x_mask, x_res, g_ret]:
                    y.fill(s)
                b = np.frombuffer(x["buf"] + bytes(size - len(x["buf"])), np.uint8)
                e.memcpy(d_buf.ptr, b.ctypes.data_as(C.c_void_p), size, H2D, s)
                for d, h in ((d_var, x["var"]), (d_shorts, x["shorts"])):
                    e.memcpy(d.ptr, h.ctypes.data_as(C.c_void_p), h.nbytes, H2D, s)
                g_st.put(x["st0"], s)
                g_cu.put(x["none"], s)
                g_ex.put(x["none"], s)
                for name, a in zip(("op", "key", "val"), arena0):
                    s_g[name].put(a, s)
                s_g["used"].put(np.array([used0], np.uint64), s)
                s_g["inst"].put(inst0, s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                wu, k = x["wu"], x["counts"]["n_cmds"]
                assert g["accepts"].assert_margins().tobytes() == wu["accepts"].tobytes()
                assert np.array_equal(g["cmd_off"].assert_margins(), wu["cmd_off"])
                assert np.array_equal(g["key"].assert_margins()[:k], wu["key"])
                assert g_srt.assert_margins().tobytes() == x["srt"].tobytes()
                assert np.array_equal(g_perm.assert_margins(), x["perm"])
                assert g_ores.assert_margins()[0].tobytes() == x["ores"].tobytes()
                assert np.array_equal(g_eff.assert_margins(), x["w_eff"])
                same(read_dev(s_g), x["ws"], f"store general={general}")
                assert g_st.assert_margins().tobytes() == x["w_st2"].tobytes()
                assert np.array_equal(g_cu.assert_margins(), x["w_cu"])
                wx = x["wx"]
                assert x_res.assert_margins()[0].tobytes() == wx["res"].tobytes()
                assert np.array_equal(g_ex.assert_margins(), wx["executed"])
                for gd, name in ((x_op, "op"), (x_key, "key"), (x_val, "val"), (x_mask, "mask")):
                    assert np.array_equal(gd.assert_margins(), wx[name]), name
                assert np.array_equal(g_ret.assert_margins(), x["ret"])
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()

"""GPU tests of record assembly (mpx_record_log and its _dev form): a batch's durable-log bytes,
bit-exact against tests/record_translit.py (the Go's record sites over Go-shaped objects). Every
case runs the host form and the _dev form, the latter with out, item_off and the result on
devguard.Guard buffers exactly their capacity long, and, whenever the call is within the one-launch
bounds, both the one-launch kernel and the general path (general=True, the documented
MPX_LR_GENERAL flag) against the same bytes. Shapes are the smallest that reach the edges: the item
pass takes 256 items per workgroup, the scan 4096 per tile, the emit 8 KB windows of the output cut
at multiples of 8 KB of the ADDRESS (so at output byte 8192 - (out mod 16)), 256 items per turn.
The error cases are reported through the error word or refused before any launch: no case provokes
a fault."""
import ctypes as C

import numpy as np
import pytest

import record_kat
import record_translit as T
import test_record_translit as TT
from devguard import Guard
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd.devbuf import Arena
from minpaxos_amd.engine import MpxError

N = 3
WIN = 8192
OUT = ("out", "item_off", "res")
ARGS = ("kind", "fmt", "items", "sources", "effect", "perm", "mask", "inst_base")


def _code(f, *a, **k):
    try:
        f(*a, **k)
    except MpxError as ex:
        return ex.code
    return R.OK


def n_cmds_of(case):
    return sum(len(s["op"]) for s in case.get("sources", ()))


def cap_of(case, out_cap):
    return R.record_bound(len(case["items"]), n_cmds_of(case)) if out_cap is None else out_cap


def want_of(case, **kw):
    return T.record_log(**dict({k: case[k] for k in ARGS if k in case}, **kw))


def run_host(e, case, general, out_cap=None):
    out, item_off, res = e.record_log(case["kind"], case["fmt"], case["items"], case.get("sources", ()),
                                      case.get("effect"), case.get("perm"), case.get("mask"),
                                      case.get("inst_base", 0), cap_of(case, out_cap), general)
    return dict(out=out, item_off=item_off, res=res)


def dev_sources(ar, sources, op_shift, kv_shift):
    out = []
    for x in sources:
        off = x.get("cmd_off")
        k = len(x["op"])
        out.append(dict(cmd_off=None if off is None else ar.put(np.asarray(off, np.uint64)),
                        n_frames=0 if off is None else len(off) - 1,
                        op=Guard(ar, k, np.uint8, shift=op_shift).put(x["op"]) if k else None,
                        key=Guard(ar, k, np.int64, shift=kv_shift).put(x["key"]) if k else None,
                        val=Guard(ar, k, np.int64, shift=kv_shift).put(x["val"]) if k else None,
                        n_cmds=k, n_recs=x["n_recs"]))
    return out


def dev_call(e, ar, case, general, out_shift=0, op_shift=3, kv_shift=0, d_n=None, out_cap=None):
    """the call's inputs on the device and its outputs on guards; returns (batch, guards, cap)"""
    n, cap = len(case["items"]), cap_of(case, out_cap)
    g = dict(out=Guard(ar, cap, np.uint8, shift=out_shift), item_off=Guard(ar, n + 1, np.uint64),
             res=Guard(ar, 1, R.RECORD_RESULT))
    eff, perm, mask = case.get("effect"), case.get("perm"), case.get("mask")
    b = e.record_batch_dev(case["kind"], case["fmt"], ar.put(case["items"]) if n else None, n,
                           dev_sources(ar, case.get("sources", ()), op_shift, kv_shift),
                           None if eff is None or not n else Guard(ar, n, np.uint8, shift=5).put(eff),
                           None if perm is None or not n else ar.put(np.asarray(perm, np.uint32)),
                           None if mask is None else Guard(ar, len(mask), np.uint8, shift=7).put(mask),
                           0 if mask is None else len(mask), case.get("inst_base", 0),
                           None if d_n is None else ar.put(np.array([d_n], np.uint64)), general)
    return b, g, cap


def read_dev(g):
    got = {name: g[name].assert_margins() for name in OUT}
    got["res"] = got["res"][0]
    if int(got["res"]["flags"]) & R.LR_FULL:
        g["out"].assert_untouched([(0, g["out"].count)])     # every byte still holds the poison
        got["out"] = got["out"][:0]
    else:
        k = int(got["res"]["n_bytes"])
        g["out"].assert_untouched([(k, g["out"].count)])
        got["out"] = got["out"][:k]
    return got


def run_dev(e, case, general, out_shift=0, op_shift=3, kv_shift=0, d_n=None, out_cap=None):
    """returns (outputs, code of the next synchronising call)"""
    with Arena(e) as ar:
        b, g, cap = dev_call(e, ar, case, general, out_shift, op_shift, kv_shift, d_n, out_cap)
        e.record_log_reserve(len(case["items"]))
        e.record_log_dev(b, g["out"] if cap else None, cap, g["item_off"], g["res"])
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
    one = len(case["items"]) <= R.LR_ONE_LAUNCH_ITEMS and n_cmds_of(case) <= R.LR_ONE_LAUNCH_CMDS
    return (False, True) if one else (False,)


def check(e, case, forms=("host", "dev"), shifts=((0, 3, 0),), out_cap=None):
    """shifts: (out, op, key / val) byte shifts of the _dev form's buffers"""
    want = want_of(case, out_cap=out_cap)
    assert want["code"] == R.OK
    for general in paths_of(case):
        if "host" in forms:
            same(run_host(e, case, general, out_cap), want, f"host general={general}")
        if "dev" in forms:
            for sh in shifts:
                got, code = run_dev(e, case, general, *sh, out_cap=out_cap)
                assert code == R.OK
                same(got, want, f"dev general={general} shifts={sh}")
    return want


@pytest.fixture
def eng(mk_engine):
    return mk_engine(N, R.MODE_MIN)


# ---- the known answers ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", record_kat.KAT, ids=lambda c: c["name"])
def test_known_answers(eng, case):
    want = check(eng, case["args"], shifts=((0, 3, 0), (1, 0, 8), (15, 1, 8)))
    record_kat.check(case, want)
    record_kat.check(case, run_host(eng, case["args"], False))
    n = int(want["res"]["n_bytes"])
    short = check(eng, case["args"], out_cap=n - 1)
    assert int(short["res"]["flags"]) == R.LR_FULL and int(short["res"]["n_bytes"]) == n


# ---- shapes --------------------------------------------------------------------------------------
def shape_cases(n, every_second, seed=0):
    """n items of each kind: none records (where the kind can), or every second does"""
    rng = np.random.default_rng(900 + n + seed)
    sizes = rng.choice([0, 1, 2, 3], n, p=[0.15, 0.45, 0.25, 0.15]).tolist()
    rec = [(i % 2 == 1) and every_second for i in range(n)]
    yield T.msgs_case(R.LR_ACCEPTS, R.LOG_DURABLE, sizes, rec, seed=seed)
    # COMMITS: every item records; the others are CommitShorts
    yield T.msgs_case(R.LR_COMMITS, R.LOG_DURABLE_CLASSIC, [s if r else None for s, r in zip(sizes, rec)], rec,
                      seed=seed)
    flags = [R.PH_ACCEPT if r else (R.PH_PREPARE, R.PH_REFUSED, R.PH_NOT_LEADER)[i % 3] for i, r in enumerate(rec)]
    yield T.sends_case(R.LR_SENDS, R.LOG_DURABLE_CLASSIC, sizes, flags, seed)
    mask = np.ones(n + 1, np.uint8) if every_second else np.zeros(n + 1, np.uint8)
    yield T.sends_case(R.LR_DECIDED, R.LOG_DURABLE, sizes, [R.PH_ACCEPT if i % 4 else R.PH_PREPARE for i in range(n)],
                       seed, mask=mask)


@pytest.mark.gpu
@pytest.mark.parametrize("every_second", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_item_counts_around_the_wave_the_workgroup_and_the_scan_tile(eng, n, every_second):
    for case in shape_cases(n, every_second):
        want = check(eng, case, shifts=((n % 16, 1, 8 * (n & 1)),))
        if case["kind"] == R.LR_ACCEPTS:
            assert int(want["res"]["n_recs"]) == (n // 2 if every_second else 0)
        if case["kind"] == R.LR_COMMITS:
            assert int(want["res"]["n_recs"]) == n


def boundary_case(kind_fmt, at, tail=3):
    """COMMITS: CommitShorts and one Commit filling exactly `at` bytes, then a Commit of `tail`
    commands whose record starts at byte `at`, then one more CommitShort and Commit"""
    fmt = kind_fmt
    h = R.LR_HEADER_BYTES[fmt]
    a = next(a for a in range(17) if at - h - h * a >= 0 and (at - h - h * a) % 17 == 0)
    sizes = [None] * a + [(at - h - h * a) // 17, tail, None, 2]
    case = T.msgs_case(R.LR_COMMITS, fmt, sizes, [True] * len(sizes), seed=at)
    assert int(want_of(case)["item_off"][a + 1]) == at
    return case


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R.LOG_DURABLE, R.LOG_DURABLE_CLASSIC])
def test_record_header_and_command_bytes_straddling_the_window_boundary(eng, fmt):
    """a record starting at every byte from 30 before (CLASSIC: 23) to 2 after the first window
    boundary: the boundary falls 2 before to 2 after a record boundary, inside every byte of its
    header and inside every byte of its first command; out on a 16-byte line and 5 bytes into one"""
    h = R.LR_HEADER_BYTES[fmt]
    for out_shift in (0, 5):
        edge = WIN - out_shift
        for at in range(edge - h - 18, edge + 3):
            case = boundary_case(fmt, at)
            want = check(eng, case, forms=("dev",), shifts=((out_shift, 3, 0),))
            assert int(want["res"]["n_bytes"]) > edge
    check(eng, boundary_case(fmt, WIN - 7), forms=("host",))
    # ... and a second boundary: records of one command (29 / 22 bytes) over three windows
    check(eng, T.msgs_case(R.LR_COMMITS, fmt, [1] * 900, [True] * 900), shifts=((0, 3, 0), (9, 2, 8)))


@pytest.mark.gpu
def test_one_item_of_5000_commands(eng):
    """the replica batch, 85 KB over eleven windows: one launch by default"""
    want = check(eng, T.msgs_case(R.LR_ACCEPTS, R.LOG_DURABLE, [5000], [True]), shifts=((0, 3, 0), (7, 1, 8)))
    assert int(want["res"]["n_bytes"]) == 12 + 17 * 5000
    check(eng, T.sends_case(R.LR_SENDS, R.LOG_DURABLE_CLASSIC, [5000], [R.PH_ACCEPT]), shifts=((11, 3, 8),))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R.LOG_DURABLE, R.LOG_DURABLE_CLASSIC])
def test_alignments(eng, fmt):
    """out at every address mod 16, op at odd addresses, key / val at both alignments mod 16; with
    CLASSIC's 5-byte metadata every phase of a command against the dwords occurs"""
    rng = np.random.default_rng(77)
    sizes = rng.choice([0, 1, 2, 3, 9], 420).tolist()
    case = T.msgs_case(R.LR_COMMITS, fmt, [None if i % 7 == 3 else s for i, s in enumerate(sizes)], [True] * 420,
                       n_src=2)
    want = check(eng, case, forms=("host",))
    assert int(want["res"]["n_bytes"]) > 2 * WIN
    check(eng, case, forms=("dev",), shifts=[(s, 1 + 2 * (s % 4), 8 * (s & 1)) for s in range(16)])


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [2, 16])
def test_sources_through_the_order_calls_perm(eng, n_src):
    """the connections' Accepts merged and grouped by mpx_order_records: item i is record perm[i]"""
    rng = np.random.default_rng(50 + n_src)
    n_inst, base = 200, 40
    sources, accepts = [], []
    for s in range(n_src):
        k = int(rng.integers(1, 90))
        sizes = rng.choice([0, 1, 2, 5], k).tolist()
        sources.append(T.mk_source(sizes, seed=s, gap=s % 3))
        accepts.append(T.mk_msgs([(base + int(rng.integers(0, n_inst)), 5 + s, v) for v in range(k)]))
    srt, perm, res = eng.order_records(accepts, n_inst, base)
    n = len(srt)
    case = dict(kind=R.LR_ACCEPTS, fmt=R.LOG_DURABLE, items=srt, sources=sources, perm=perm,
                effect=np.where(rng.random(n) < 0.7, R.AH_STORED | R.AH_REPLIED, R.AH_REPLIED).astype(np.uint8))
    want = check(eng, case, shifts=((3, 1, 8),))
    assert int(want["res"]["n_recs"]) > n // 2 and not np.array_equal(perm, np.arange(n))


@pytest.mark.gpu
def test_commits_and_commit_shorts_merged_by_stream_offset(eng):
    """the unmarshalled Commits and the gathered CommitShorts of one connection, merged by their
    frames' stream offsets and grouped by instance: perm names a Commit's record in the first
    source and a CommitShort's in the second, which has no frames"""
    rng = np.random.default_rng(8)
    n_c, n_s = 300, 200
    sizes = rng.choice([0, 1, 2, 4], n_c).tolist()
    commits = T.mk_msgs([(int(rng.integers(0, 150)), 9, v) for v in range(n_c)])
    shorts = T.mk_msgs([(int(rng.integers(0, 150)), 9, R.VALUE_KEEP) for _ in range(n_s)])
    offset = rng.permutation(n_c + n_s)                       # every frame's place in the stream
    both = np.concatenate([commits, shorts])
    by_offset = np.argsort(offset, kind="stable")
    order = by_offset[np.argsort(both["instance"][by_offset], kind="stable")]
    eff = np.where(both["value_id"][order] == R.VALUE_KEEP, R.CH_INSTALLED, R.CH_CMDS).astype(np.uint8)
    empty = dict(cmd_off=None, op=np.zeros(0, np.uint8), key=np.zeros(0, np.int64), val=np.zeros(0, np.int64),
                 n_recs=n_s)
    for fmt in (R.LOG_DURABLE, R.LOG_DURABLE_CLASSIC):
        case = dict(kind=R.LR_COMMITS, fmt=fmt, items=both[order], effect=eff, perm=order.astype(np.uint32),
                    sources=[T.mk_source(sizes, seed=4), empty])
        want = check(eng, case, shifts=((13, 3, 8),))
        assert int(want["res"]["n_recs"]) == n_c + n_s and int(want["res"]["n_cmds"]) == sum(sizes)


@pytest.mark.gpu
def test_d_n_smaller_than_n(eng):
    for n, d_n in ((300, 123), (2000, 1500), (50, 0), (50, 70)):
        case = next(shape_cases(n, True, seed=3))
        want = want_of(case, dev=True, d_n=d_n)
        assert want["code"] == R.OK and len(set(want["item_off"][min(d_n, n):].tolist())) == 1
        for general in paths_of(case):
            got, code = run_dev(eng, case, general, d_n=d_n)
            assert code == R.OK
            same(got, want, f"d_n={d_n} general={general}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 1500])
def test_one_byte_short_changes_nothing(eng, n):
    """every output byte keeps its poison (read_dev checks each), res is complete and flagged"""
    for case in shape_cases(n, True, seed=5):
        total = int(want_of(case)["res"]["n_bytes"])
        want = check(eng, case, out_cap=total - 1, shifts=((0, 3, 0), (6, 1, 8)))
        assert int(want["res"]["flags"]) == R.LR_FULL and int(want["res"]["n_bytes"]) == total
        assert int(want["res"]["n_recs"]) > 0 and len(want["out"]) == 0
        assert int(check(eng, case, out_cap=total)["res"]["flags"]) == 0       # exactly full


@pytest.mark.gpu
def test_decided_over_a_window_of_2_to_the_20_slots_with_100_slots(eng):
    """nothing depends on n_inst"""
    n_inst, base = 1 << 20, -7
    rng = np.random.default_rng(20)
    rel = np.sort(rng.choice(n_inst, 100, replace=False))
    mask = np.zeros(n_inst, np.uint8)
    mask[rel[rng.random(100) < 0.7]] = 1
    mask[rng.choice(n_inst, 5000)] = 1                        # other instances were decided as well
    flags = np.where(rng.random(100) < 0.8, R.PH_ACCEPT, R.PH_REFUSED)
    rows = [(base + int(r), 20 + i % 3, int(f), 0, 2) for i, (r, f) in enumerate(zip(rel, flags))]
    for fmt in (R.LOG_DURABLE, R.LOG_DURABLE_CLASSIC):
        case = dict(kind=R.LR_DECIDED, fmt=fmt, items=T.mk_sends(rows), mask=mask, inst_base=base)
        want = check(eng, case)
        assert 30 < int(want["res"]["n_recs"]) < 100 and int(want["res"]["n_cmds"]) == 0


# ---- fuzz ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", TT.SEEDS)
def test_fuzz(eng, seed):
    check(eng, T.fuzz_case(seed), shifts=((seed % 16, 1 + seed % 3, 8 * (seed & 1)),))


# ---- the round trip ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 700, 3000])
def test_round_trip_through_the_durable_replay(eng, n):
    """batches of single-command items in MIN's format are what getDataFromStableStore reads: per
    instance, replay leaves the ballot, status and command of the instance's last record"""
    rng = np.random.default_rng(n)
    case = T.msgs_case(R.LR_ACCEPTS, R.LOG_DURABLE, [1] * n, (rng.random(n) < 0.8).tolist(), n_src=min(n, 3))
    case["items"]["instance"] = np.sort(rng.integers(0, n // 2 + 1, n))
    case["effect"][0] |= R.AH_STORED
    got = run_dev(eng, case, False, out_shift=0)[0]
    log = got["out"]
    assert len(log) % R.DURABLE_REC_BYTES == 0
    inst_cap = n // 2 + 2
    recs, op, key, val, last_rec = eng.replay_durable(log, inst_cap)[:5]
    recording = np.flatnonzero(case["effect"] & R.AH_STORED)
    assert len(recs) == len(recording)
    gr, goff, gop, gkey, gval = T.gathered(case)
    for i in range(inst_cap):
        mine = np.flatnonzero(case["items"]["instance"][recording] == i)
        assert int(last_rec[i]) == (int(mine[-1]) if len(mine) else -1)
        if len(mine):
            k = int(last_rec[i])
            assert (int(recs[k]["ballot"]), int(recs[k]["status"]), int(recs[k]["inst_no"])) == \
                (int(case["items"]["ballot"][recording[k]]), T.ACCEPTED, i)
            assert (int(op[k]), int(key[k]), int(val[k])) == (int(gop[k]), int(gkey[k]), int(gval[k]))


# ---- rejections ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fault", TT.FAULTS)
def test_a_faulty_item_by_error_word_and_by_code(eng, fault):
    """the host form answers before any launch; the _dev form raises the error word, the item
    records nothing, and the others are exact"""
    case = TT.faulty(fault)
    code = R.E_NIL_INSTANCE if "window" in fault else R.E_INVAL
    want = want_of(case, dev=True)
    assert want["code"] == code
    for general in (False, True):
        assert _code(run_host, eng, case, general) == code
        got, got_code = run_dev(eng, case, general)
        assert got_code == code
        same(got, want, f"dev general={general}")
    check(eng, TT._two())                    # the handle is clean again


@pytest.mark.gpu
def test_argument_rejections(eng):
    e = eng
    case = T.msgs_case(R.LR_ACCEPTS, R.LOG_DURABLE, [2, 3, 1], [True, False, True])
    two = dict(case, sources=[dict(case["sources"][0], n_recs=2), dict(case["sources"][0], n_recs=1)],
               perm=np.arange(3, dtype=np.uint32))
    sends = T.sends_case(R.LR_DECIDED, R.LOG_DURABLE, [1, 1, 1], [R.PH_ACCEPT] * 3, mask=np.ones(3, np.uint8))
    res = _lib.MpxRecordResult()
    out, ioff, cur = np.zeros(200, np.uint8), np.zeros(4, np.uint64), np.array([1], np.uint64)
    keep = []

    def ptr_of(x, k, t):
        keep.append(np.ascontiguousarray(x, t))
        return keep[-1].ctypes.data_as(C.c_void_p)
    src1, _ = e._store_srcs(case["sources"], ptr_of)
    src2, _ = e._store_srcs(two["sources"], ptr_of)
    p = [x.ctypes.data_as(C.c_void_p) for x in (case["items"], case["effect"], two["perm"], out, ioff, cur,
                                                sends["items"], sends["mask"])]

    def host(with_res=True, out_p=p[3], out_cap=200, **kw):
        f = dict(kind=R.LR_ACCEPTS, flags=0, format=R.LOG_DURABLE, reserved=0, items=p[0], effect=p[1],
                 mask=None, n=3, d_n=None, perm=None, src=src1, n_src=1, n_inst=0, inst_base=0, pad=0)
        f.update(kw)
        return e.lib.mpx_record_log(e.h, C.byref(_lib.MpxRecordBatch(**f)), out_p, out_cap, p[4],
                                    C.byref(res) if with_res else None)
    assert host() == R.OK and (res.n_recs, res.n_cmds, res.n_bytes, res.flags) == (2, 3, 75, 0)
    assert ioff.tolist() == [0, 46, 46, 75]
    for name in ("items", "effect", "src"):
        assert host(**{name: None}) == R.E_INVAL, name
    assert host(with_res=False) == R.E_INVAL and host(out_p=None) == R.E_INVAL
    assert host(out_p=None, out_cap=0) == R.OK and res.flags == R.LR_FULL and res.n_bytes == 75
    assert host(kind=4) == R.E_INVAL and host(flags=2) == R.E_INVAL and host(reserved=1) == R.E_INVAL
    assert host(format=R.LOG_CATCHUP) == R.E_INVAL and host(format=3) == R.E_INVAL
    assert host(format=R.LOG_DURABLE_CLASSIC) == R.E_UNSUPPORTED     # CLASSIC handleAccept is not covered
    assert host(kind=R.LR_COMMITS, format=R.LOG_DURABLE_CLASSIC) == R.OK and res.n_bytes == 15 + 17 * 3
    assert host(n_src=0) == R.E_INVAL and host(n_src=17) == R.E_INVAL
    assert host(d_n=p[5]) == R.E_INVAL
    assert host(src=src2, n_src=2) == R.E_INVAL                     # two sources need perm
    assert host(src=src2, n_src=2, perm=p[2]) == R.OK
    assert host(n=4) == R.E_INVAL                                   # more items than records
    assert host(kind=R.LR_SENDS, src=src2, n_src=2) == R.E_INVAL
    assert host(n=0xFFFFFFFF) == R.E_UNSUPPORTED
    decided = dict(kind=R.LR_DECIDED, items=p[6], effect=None, src=None, n_src=0, n_inst=3, inst_base=100)
    assert host(mask=p[7], **decided) == R.OK and res.n_bytes == 36
    assert host(mask=None, **decided) == R.E_INVAL
    assert host(mask=p[7], **dict(decided, n_src=17)) == R.E_INVAL
    assert host(mask=p[7], **dict(decided, n_inst=2)) == R.E_NIL_INSTANCE
    assert _code(e.record_log_reserve, 0xFFFFFFFF) == R.E_UNSUPPORTED
    # the device form's alignment rules
    with Arena(e) as ar:
        b, g, cap = dev_call(e, ar, two, False, op_shift=0)
        e.record_log_reserve(3)

        def dev(field=None, by=0, out_by=0, ioff_by=0, res_by=0, src_field=None):
            x = _lib.MpxRecordBatch.from_buffer_copy(b)
            if field:
                setattr(x, field, getattr(x, field) + by)
            if src_field:
                arr = (_lib.MpxStoreSrc * 2)(b.src[0], b.src[1])
                setattr(arr[1], src_field, getattr(arr[1], src_field) + by)
                x.src = arr
                keep.append(arr)
            return _code(e.record_log_dev, x, g["out"].ptr + out_by, cap - out_by, g["item_off"].ptr + ioff_by,
                         g["res"].ptr + res_by)
        for field, by in (("items", 8), ("perm", 2), ("d_n", 4)):
            if field == "d_n":
                b.d_n = g["item_off"].ptr
            assert dev(field, by) == R.E_INVAL, field
            b.d_n = None
        for field in ("cmd_off", "key", "val"):
            assert dev(src_field=field, by=4) == R.E_INVAL, field
        assert dev(ioff_by=4) == R.E_INVAL and dev(res_by=4) == R.E_INVAL
        e.synchronize()
        for x in g.values():
            x.assert_margins()
            x.assert_untouched([(0, x.count)])
        # out, op bytes and effect may sit anywhere (one byte further is inside the guards' margins)
        assert dev(src_field="op", by=1) == R.OK and dev(out_by=1) == R.OK and dev("effect", 1) == R.OK
        e.synchronize()
    del keep


@pytest.mark.gpu
def test_the_dev_form_needs_its_reserve_and_never_grows(mk_engine):
    e = mk_engine(N, R.MODE_CLASSIC)
    small, big = TT._two(), next(shape_cases(3000, True, seed=8))
    with Arena(e) as ar:
        b, g, cap = dev_call(e, ar, small, True)
        with pytest.raises(MpxError) as ei:
            e.record_log_dev(b, g["out"], cap, g["item_off"], g["res"])
        assert ei.value.code == R.E_INVAL and "mpx_record_log_reserve" in str(ei.value)
        e.record_log_reserve(2)
        e.record_log_dev(b, g["out"], cap, g["item_off"], g["res"])
        e.synchronize()
        assert g["res"].assert_margins()[0].tolist() == (2, 5, 24 + 85, 0)
        b2, g2, cap2 = dev_call(e, ar, big, False)
        assert _code(e.record_log_dev, b2, g2["out"], cap2, g2["item_off"], g2["res"]) == R.E_INVAL
        e.synchronize()
        for x in g2.values():
            x.assert_untouched([(0, x.count)])
    check(e, big)
    check(e, small)


# ---- the chains ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True])
def test_graph_of_decode_propose_handle_store_and_record_sends(mk_engine, general):
    """mpx_decode_client_streams_dev -> mpx_propose_handle_dev -> mpx_store_commands_dev(MPX_SC_SENDS)
    -> mpx_record_log_dev(MPX_LR_SENDS), captured once into a graph and replayed on two inputs (new
    connection lengths and bytes, same pointers), against the client, proposer and record
    transliterations: the leader's stable-store append with no host step in between"""
    import client_translit as CL
    import proposer_translit as PT
    import test_gpu_client as TC
    from minpaxos_amd.devbuf import D2D
    NR = 5
    e = mk_engine(NR, R.MODE_MIN)
    G, per_group, slot, ipg, base, D = 3, 4, 1024, 8, 50, 32
    n_inst, n_conns = G * ipg, G * per_group
    inputs = []
    for seed in (11, 12):
        bufs, groups = TC._chain_input(seed, G, per_group, slot)
        wc = CL.decode_client_streams(bufs, groups, G)
        grp = PT.mk_groups([(D, 0, 0, 3, base + g * ipg, base + g * ipg - 1) for g in range(G)])
        st, lb = PT.nil_state(n_inst), np.zeros(n_inst, R.INST_STATE)
        wp = PT.propose_handle(R.MODE_MIN, NR, grp, wc["prop_off"], st, base, ipg, lb)
        buf = np.zeros(n_conns * slot, np.uint8)
        conns = np.zeros(n_conns, R.CLIENT_CONN)
        for k, b in enumerate(bufs):
            conns[k] = (k * slot, len(b), groups[k])
            buf[k * slot:k * slot + len(b)] = np.frombuffer(b, np.uint8)
        wr = T.record_log(R.LR_SENDS, R.LOG_DURABLE, wp[3],
                          [dict(cmd_off=None, op=wc["op"], key=wc["key"], val=wc["val"], n_recs=G)])
        assert wr["code"] == R.OK and int(wr["res"]["n_recs"]) == G
        inputs.append(dict(buf=buf, conns=conns, grp=grp, st=st, lb=lb, wc=wc, wp=wp, wr=wr))
    assert inputs[0]["wr"]["out"].tobytes() != inputs[1]["wr"]["out"].tobytes()
    cap = n_conns * slot // 30
    a_cap = cap + 8
    o_cap = R.record_bound(G, cap)
    with Arena(e) as ar:
        g, g_buf, d_conns, out = TC.dev_buffers(ar, inputs[0]["buf"], inputs[0]["conns"], G, cap)
        g_grp, g_st = Guard(ar, G, R.PROPOSER_GROUP), Guard(ar, n_inst, R.ACCEPTOR_STATE)
        g_lb, g_snd = Guard(ar, n_inst, R.INST_STATE), Guard(ar, G, R.ACCEPT_SEND)
        s_g = dict(op=Guard(ar, a_cap, np.uint8, shift=1), key=Guard(ar, a_cap, np.int64, shift=8),
                   val=Guard(ar, a_cap, np.int64), used=Guard(ar, 1, np.uint64),
                   inst=Guard(ar, n_inst, R.INST_CMDS), res=Guard(ar, 1, R.STORE_RESULT))
        r_g = dict(out=Guard(ar, o_cap, np.uint8, shift=9), item_off=Guard(ar, G + 1, np.uint64),
                   res=Guard(ar, 1, R.RECORD_RESULT))
        src = [dict(cmd_off=None, n_frames=0, op=g["op"], key=g["key"], val=g["val"], n_cmds=cap, n_recs=G)]
        sb = e.store_batch_dev(R.SC_SENDS, g_snd, G, src, n_inst, base, general=general)
        sa = e.store_arena_dev(s_g["op"], s_g["key"], s_g["val"], a_cap, s_g["used"])
        rb = e.record_batch_dev(R.LR_SENDS, R.LOG_DURABLE, g_snd, G, src, general=general)
        e.decode_client_streams_reserve(len(inputs[0]["buf"]), n_conns, G)
        e.store_commands_reserve(G)
        e.record_log_reserve(G)
        s = e.stream_create()
        e.graph_begin(s)
        e.decode_client_streams_dev(g_buf.ptr, n_conns * slot, d_conns.ptr, n_conns, G, out,
                                    g["conn_res"].ptr, g["res"].ptr, s)
        e.propose_handle_dev(g_grp.ptr, G, g["prop_off"].ptr, g["send_off"].ptr, g_st.ptr, g_lb.ptr,
                             n_inst, base, ipg, g_snd.ptr, s)
        e.store_commands_dev(sb, sa, s_g["inst"], s_g["res"], s)
        e.record_log_dev(rb, r_g["out"], o_cap, r_g["item_off"], r_g["res"], s)
        gr = e.graph_end(s)
        try:
            for x in inputs + inputs[:1]:
                for y in list(g.values()) + [g_snd, s_g["res"]] + list(r_g.values()):
                    y.fill(s)
                g_buf.put(x["buf"], s)
                g_grp.put(x["grp"], s)
                g_st.put(x["st"], s)
                g_lb.put(x["lb"], s)
                for name, t in (("op", np.uint8), ("key", np.int64), ("val", np.int64)):
                    s_g[name].put(np.zeros(a_cap, t), s)
                s_g["used"].put(np.array([0], np.uint64), s)
                s_g["inst"].put(np.zeros(n_inst, R.INST_CMDS), s)
                src_conns = ar.put(x["conns"], s)
                e.memcpy(d_conns.ptr, src_conns.ptr, src_conns.nbytes, D2D, s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                assert g_snd.assert_margins().tobytes() == x["wp"][3].tobytes()
                assert int(s_g["res"].assert_margins()[0]["n_stored"]) == G
                same(read_dev(r_g), x["wr"], f"record general={general}")
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True])
def test_graph_of_a_followers_accepts_to_their_records(mk_engine, general):
    """mpx_unmarshal_frames_dev -> mpx_order_records_dev -> mpx_accept_handle_dev ->
    mpx_store_commands_dev -> mpx_record_log_dev(MPX_LR_ACCEPTS, perm and &d_res->n from the order
    call), captured once into a graph and replayed on two inputs: every storing Accept records, the
    resends MIN ignores and the stale ballots do not"""
    import store_translit as ST
    import test_gpu_store as TS
    import test_gpu_unmarshal as TU
    from minpaxos_amd.devbuf import H2D
    NR, G, ipg, base, D, cap, used0 = 3, 1, 32, 100, 16, 64, 3
    e = mk_engine(NR, R.MODE_MIN)
    inst0 = ST.mk_window(ipg, used0, 0.0, np.random.default_rng(1))
    a_cap = used0 + 24 * 5
    arena0 = ST.mk_arena(a_cap, 4)
    inputs = [TS._follower_turn(31, {}, NR, ipg, base, D, used0, inst0, arena0, cap, range(10)),
              TS._follower_turn(32, {}, NR, ipg, base, D, used0, inst0, arena0, cap, range(10))]
    n = 24
    for x in inputs:
        wu = x["wu"]
        x["wr"] = T.record_log(R.LR_ACCEPTS, R.LOG_DURABLE, x["srt"],
                               [dict(cmd_off=wu["cmd_off"], op=wu["op"], key=wu["key"], val=wu["val"], n_recs=n)],
                               effect=x["w_eff"], perm=x["perm"])
        assert x["wr"]["code"] == R.OK and int(x["wr"]["res"]["n_recs"]) == 12
    assert inputs[0]["wr"]["out"].tobytes() != inputs[1]["wr"]["out"].tobytes()
    size = -(-max(len(x["buf"]) for x in inputs) // 16) * 16
    caps = (n, 0, max(x["counts"]["n_cmds"] for x in inputs), 0, 0)
    o_cap = R.record_bound(n, caps[2])
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
        r_g = dict(out=Guard(ar, o_cap, np.uint8, shift=3), item_off=Guard(ar, n + 1, np.uint64),
                   res=Guard(ar, 1, R.RECORD_RESULT))
        src = [dict(cmd_off=g["cmd_off"], n_frames=n, op=g["op"], key=g["key"], val=g["val"], n_cmds=caps[2],
                    n_recs=n)]
        d_n = g_ores.ptr + R.ORDER_RESULT.fields["n"][1]
        sb = e.store_batch_dev(R.SC_MSGS, g_srt, n, src, ipg, base, g_eff, g_perm, d_n, general=general)
        sa = e.store_arena_dev(s_g["op"], s_g["key"], s_g["val"], a_cap, s_g["used"])
        rb = e.record_batch_dev(R.LR_ACCEPTS, R.LOG_DURABLE, g_srt, n, src, g_eff, g_perm, d_n=d_n,
                                general=general)
        e.unmarshal_frames_reserve(n, 1)
        e.order_records_reserve(n, ipg)
        e.store_commands_reserve(n)
        e.record_log_reserve(n)
        s = e.stream_create()
        e.graph_begin(s)
        e.unmarshal_frames_dev(d_buf.ptr, size, d_var.ptr, n, None, out, g_ures.ptr, s)
        e.order_records_dev([(g["accepts"].ptr, None, n)], ipg, base, 0, g_srt.ptr, g_perm.ptr, g_ores.ptr,
                            stream=s)
        e.accept_handle_dev(g_srt.ptr, n, g_st.ptr, g_st.ptr, ipg, base, d_groups.ptr, G, ipg, g_rep.ptr,
                            g_to.ptr, g_eff.ptr, s)
        e.store_commands_dev(sb, sa, s_g["inst"], s_g["res"], s)
        e.record_log_dev(rb, r_g["out"], o_cap, r_g["item_off"], r_g["res"], s)
        gr = e.graph_end(s)
        try:
            for x in inputs + inputs[:1]:
                for y in list(g.values()) + [g_srt, g_perm, g_ores, g_eff, s_g["res"]] + list(r_g.values()):
                    y.fill(s)
                b = np.frombuffer(x["buf"] + bytes(size - len(x["buf"])), np.uint8)
                e.memcpy(d_buf.ptr, b.ctypes.data_as(C.c_void_p), size, H2D, s)
                e.memcpy(d_var.ptr, x["var"].ctypes.data_as(C.c_void_p), x["var"].nbytes, H2D, s)
                g_st.put(x["st0"], s)
                for name, a in zip(("op", "key", "val"), arena0):
                    s_g[name].put(a, s)
                s_g["used"].put(np.array([used0], np.uint64), s)
                s_g["inst"].put(inst0, s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                assert g_srt.assert_margins().tobytes() == x["srt"].tobytes()
                assert np.array_equal(g_eff.assert_margins(), x["w_eff"])
                TS.same(TS.read_dev(s_g), x["ws"], f"store general={general}")
                same(read_dev(r_g), x["wr"], f"record general={general}")
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()


# ---- store assembly and record assembly resolve one batch alike ------------------------------------
def _shared_batch(faulty=False):
    """300 Commits over three connections of 100 records each, merged by a perm that is no identity
    and grouped by instance in runs of one or two; record r of a connection is its frame r. One
    item is a CommitShort (MPX_VALUE_KEEP), some carry no MPX_CH_CMDS, some name an empty frame.
    faulty: one storing item names frame n_frames of its source."""
    import store_translit as ST
    rng = np.random.default_rng(2024)
    n, per, base = 300, 100, 40
    sizes = rng.choice([0, 1, 2, 3], (3, per), p=[0.2, 0.4, 0.25, 0.15])
    sources = [T.mk_source(sizes[s].tolist(), seed=40 + s, gap=s) for s in range(3)]
    perm = rng.permutation(n).astype(np.uint32)
    instance = base + np.cumsum(rng.random(n) < 0.6)            # ascending, runs of equal instances
    value = (perm % per).astype(np.int64)
    eff = np.where(rng.random(n) < 0.85, R.CH_CMDS | R.CH_INSTALLED, R.CH_INSTALLED).astype(np.uint8)
    at_end, at_last = int(np.flatnonzero(perm == per)[0]), int(np.flatnonzero(perm == n - 1)[0])
    keep = next(i for i in range(n) if i not in (at_end, at_last))
    value[keep] = R.VALUE_KEEP
    eff[[at_end, at_last, keep]] |= R.CH_CMDS
    if faulty:
        value[next(i for i in range(n) if eff[i] & R.CH_CMDS and i != keep)] = per
    items = T.mk_msgs([(int(instance[i]), 9, int(value[i])) for i in range(n)])
    n_inst = int(instance[-1]) - base + 2
    record = dict(kind=R.LR_COMMITS, fmt=R.LOG_DURABLE, items=items, sources=sources, effect=eff, perm=perm)
    total = int(sizes.sum())
    store = dict(kind=R.SC_MSGS, items=items, sources=sources, effect=eff, perm=perm, store_mask=R.CH_CMDS,
                 handler="commit", arena=ST.mk_arena(5 + total, 6), used=5, inst_base=base,
                 inst=ST.mk_window(n_inst, 5, 0.3, np.random.default_rng(7)))
    storing = [i for i in range(n) if eff[i] & R.CH_CMDS and value[i] != R.VALUE_KEEP]
    winners = [i for k, i in enumerate(storing)
               if k + 1 == len(storing) or instance[storing[k + 1]] != instance[i]]
    if not faulty:
        assert not np.array_equal(perm, np.arange(n)) and len(winners) < len(storing) < n - 1
        assert at_end in storing and at_last in storing
        assert any(sizes[perm[i] // per, perm[i] % per] == 0 for i in winners)
    return store, record, winners


def _stored_equals_recorded(store, got_s, got_r, winners):
    """every winner's slot names as many commands as its record holds past the 12 metadata bytes,
    and the arena holds the commands the record bytes hold"""
    cmd = np.dtype([("op", "u1"), ("key", "<i8"), ("val", "<i8")])
    assert cmd.itemsize == 17
    for i in winners:
        slot = got_s["inst"][int(store["items"]["instance"][i]) - store["inst_base"]]
        lo, hi = int(got_r["item_off"][i]), int(got_r["item_off"][i + 1])
        k, first = int(slot["n_cmds"]), int(slot["first_cmd"])
        assert int(slot["flags"]) == R.IC_HAS_CMDS and k == (hi - lo - 12) // 17 and (hi - lo - 12) % 17 == 0, i
        rec = np.frombuffer(got_r["out"][lo + 12:hi].tobytes(), cmd)
        assert np.array_equal(rec["op"], got_s["op"][first:first + k]), i
        assert np.array_equal(rec["key"], got_s["key"][first:first + k]), i
        assert np.array_equal(rec["val"], got_s["val"][first:first + k]), i


@pytest.mark.gpu
def test_store_and_record_resolve_one_batch_alike(eng):
    """one MPX_SC_MSGS / MPX_LR_COMMITS batch through both calls, on the one-launch path and on the
    general path (300 items: two workgroups of the item pass): a perm entry equal to a source's
    rec_end, the last record of the last source, an empty frame and a CommitShort among the items"""
    import store_translit as ST
    import test_gpu_store as TS
    store, record, winners = _shared_batch()
    want_s, want_r = ST.store_commands(**store), want_of(record)
    assert want_s["code"] == R.OK and want_r["code"] == R.OK
    assert int(want_s["res"]["n_stored"]) == len(winners)
    _stored_equals_recorded(store, want_s, want_r, winners)
    for general in (False, True):
        got_s, code_s = TS.run_dev(eng, store, general, op_shift=1, kv_shift=8)
        got_r, code_r = run_dev(eng, record, general, out_shift=3)
        assert code_s == R.OK and code_r == R.OK
        TS.same(got_s, want_s, f"store general={general}")
        same(got_r, want_r, f"record general={general}")
        _stored_equals_recorded(store, got_s, got_r, winners)
        TS.same(TS.run_host(eng, store, general), want_s, f"store host general={general}")
        same(run_host(eng, record, general), want_r, f"record host general={general}")


@pytest.mark.gpu
def test_store_and_record_refuse_one_faulty_item_alike(eng):
    """value_id == n_frames of the item's source: both calls answer the same code, by the error word
    and before any launch, on both paths"""
    import store_translit as ST
    import test_gpu_store as TS
    store, record, _ = _shared_batch(faulty=True)
    want_s, want_r = ST.store_commands(**dict(store, dev=True)), want_of(record, dev=True)
    assert want_s["code"] == want_r["code"] == R.E_INVAL
    for general in (False, True):
        got_s, code_s = TS.run_dev(eng, store, general)
        got_r, code_r = run_dev(eng, record, general)
        assert code_s == code_r == R.E_INVAL
        TS.same(got_s, want_s, f"store general={general}")
        same(got_r, want_r, f"record general={general}")
        assert _code(TS.run_host, eng, store, general) == _code(run_host, eng, record, general) == R.E_INVAL

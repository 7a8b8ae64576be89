"""Instance-log encoding.

CPU: the oracle against Instance.Marshal / recordInstanceMetadata + recordCommands restated
with struct.pack (minpaxosprotomarsh.go:100-124, bareminpaxos.go:164-188, statemarsh.go:8-19),
including multi-byte varints and empty (nil) command slices; bcastAccept's per-peer CatchUpLog is
a suffix of one encoded run (bareminpaxos.go:488-513).
GPU: mpx_encode_log vs the oracle and the restatement, bit for bit, across the engine's 8 KB
output windows (logenc.hip kLogBlockBytes).

The edge cases of the encoder (edge_cases below) are written once, as generators that assert the
geometry they claim from the expected rec_off: 1-, 2- and 3-byte varints, random bytes in every
field, windows of nothing but empty records (the most records a window can overlap, which sizes
the emit kernel's LDS arrays), a probe record swept over a window boundary byte by byte, totals
at and around a whole number of windows, and record counts around the offset scan's tile. The
oracle is checked against the restatement on the CPU, the host form against the restatement on the
GPU, and tests/test_gpu_dev_forms.py runs the same cases through mpx_encode_log_dev.
"""
import struct

import numpy as np
import pytest

from oracle_lib import Oracle
from minpaxos_amd import records as R
from minpaxos_amd import synth


def put_varint(x):  # encoding/binary.PutVarint
    ux = (x << 1) ^ (-1 if x < 0 else 0)
    ux &= (1 << 64) - 1
    b = bytearray()
    while ux >= 0x80:
        b.append((ux & 0x7F) | 0x80)
        ux >>= 7
    b.append(ux)
    return bytes(b)


def cmd_bytes(op, key, val):
    return struct.pack("<Bqq", op, key, val)


def expected(fmt, recs, off, op, key, val):
    w, ro = bytearray(), []
    for i, r in enumerate(recs):
        ro.append(len(w))
        w += struct.pack("<ii", int(r["ballot"]), int(r["status"]))
        c0, c1 = int(off[i]), int(off[i + 1])
        w += put_varint(c1 - c0) if fmt == R.LOG_CATCHUP else struct.pack("<i", int(r["inst_no"]))
        for j in range(c0, c1):
            w += cmd_bytes(int(op[j]), int(key[j]), int(val[j]))
    ro.append(len(w))
    return bytes(w), ro


def sample():
    recs = np.zeros(4, R.LOG_REC)
    recs["ballot"] = [16, 16, -1, 33]
    recs["status"] = [R.COMMITTED, R.ACCEPTED, R.COMMITTED, R.PREPARED]
    recs["inst_no"] = [7, 8, 9, 10]
    cnt = [1, 0, 64, 3]  # 64 commands -> a 2-byte varint (zigzag 128)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    m = int(off[-1])
    rng = np.random.default_rng(3)
    op = rng.integers(0, 6, m).astype(np.uint8)
    key = rng.integers(-(1 << 62), 1 << 62, m).astype(np.int64)
    val = rng.integers(-(1 << 62), 1 << 62, m).astype(np.int64)
    key[0] = np.iinfo(np.int64).min
    return recs, off, op, key, val


@pytest.mark.parametrize("fmt", [R.LOG_CATCHUP, R.LOG_DURABLE])
def test_kat_formats(fmt):
    recs, off, op, key, val = sample()
    out, ro = Oracle().encode_log(fmt, recs, off, op, key, val)
    want, wro = expected(fmt, recs, off, op, key, val)
    assert out.tobytes() == want and list(ro) == wro
    if fmt == R.LOG_CATCHUP:
        assert out[int(ro[2]) + 8:int(ro[2]) + 10].tobytes() == bytes([0x80, 0x01])


def test_kat_catchup_suffix_per_peer():
    recs, off, op, key, val = synth.log_records(50, 4, ragged=True)
    out, ro = Oracle().encode_log(R.LOG_CATCHUP, recs, off, op, key, val)
    peer_commits = [-1, 10, 48]  # bcastAccept: from = 0 if peercommits < 0 else pc + 1
    for pc in peer_commits:
        frm = 0 if pc < 0 else pc + 1
        sub = Oracle().encode_log(R.LOG_CATCHUP, recs[frm:], off[frm:] - off[frm],
                                  op[int(off[frm]):], key[int(off[frm]):], val[int(off[frm]):])[0]
        assert out[int(ro[frm]):].tobytes() == sub.tobytes()


# ---- the encoder's edges, each written once ------------------------------------------------------
WINDOW = 8192     # logenc.hip kLogBlockBytes: one emit workgroup's output window
MAX_RECS = 912    # logenc.hip kLogMaxRecs: the most records one window can overlap
SCAN_TILE = 4096  # scan.hpp kScTile: records per tile of the offsets scan
FMTS = [R.LOG_CATCHUP, R.LOG_DURABLE]
FMT_IDS = ["catchup", "durable"]
I64_MIN = np.iinfo(np.int64).min
I32_MIN = np.iinfo(np.int32).min


def hdr_len(fmt, c):
    """bytes of a record's header: Ballot, Status and PutVarint(c) or instNo"""
    return 8 + len(put_varint(c)) if fmt == R.LOG_CATCHUP else 12


def rec_len(fmt, c):
    return hdr_len(fmt, c) + 17 * c


def mk_case(cnt, seed):
    """a run with cnt[i] commands in record i and random bytes in every field: op over 0..255,
    key / val over all of int64, ballot / status / inst_no over all of int32"""
    cnt = np.asarray(cnt, np.int64)
    n = len(cnt)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(cnt, out=off[1:])
    m = int(off[-1])
    rng = np.random.default_rng(seed)
    recs = np.zeros(n, R.LOG_REC)
    for f in ("ballot", "status", "inst_no"):
        recs[f] = rng.integers(-(1 << 31), 1 << 31, n)
    op = rng.integers(0, 256, m).astype(np.uint8)
    key = rng.integers(0, 1 << 64, m, dtype=np.uint64).view(np.int64)
    val = rng.integers(0, 1 << 64, m, dtype=np.uint64).view(np.int64)
    return recs, off, op, key, val


def filler(fmt, total):
    """command counts of one lead record of c < 60 commands followed by empty records, `total`
    bytes in all (every total from one record up is reachable: 17 is coprime to 9 and to 12)"""
    e = rec_len(fmt, 0)
    for c in range(60):
        rest = total - rec_len(fmt, c)
        if rest >= 0 and rest % e == 0:
            return [c] + [0] * (rest // e)
    raise AssertionError(f"no filler of {total} bytes")


def window_overlaps(ro):
    """per output window, the (first, end) record indices overlapping it"""
    ro = np.asarray(ro, np.int64)
    total = int(ro[-1])
    out = []
    for b0 in range(0, total, WINDOW):
        b1 = min(b0 + WINDOW, total)
        out.append((int(np.searchsorted(ro[1:], b0, "right")), int(np.searchsorted(ro[:-1], b1, "left"))))
    return out


def gen_varint(fmt):
    """63 | 64 and 8191 | 8192 commands: the last 1-byte, both ends of the 2-byte and the first
    3-byte varint, with short records between them"""
    cnt = [2, 63, 0, 64, 1, 8191, 8192, 3]

    def check(ro):
        got = [ro[i + 1] - ro[i] - 17 * c for i, c in enumerate(cnt)]
        assert got == ([9, 9, 9, 10, 9, 10, 11, 9] if fmt == R.LOG_CATCHUP else [12] * 8)
    yield "63_64_8191_8192", mk_case(cnt, 101), check


def gen_full_range(fmt):
    """random bytes in every field, and the values that sign handling gets wrong"""
    rng = np.random.default_rng(102)
    case = mk_case(rng.integers(0, 9, 700), 103)
    recs, off, op, key, val = case
    key[:3], val[:3] = [-1, I64_MIN, 0], [I64_MIN, 0, -1]
    op[:4] = [0, 5, 6, 255]
    recs["ballot"][:3], recs["status"][:3], recs["inst_no"][:3] = ([-1, I32_MIN, 0],) * 3

    def check(ro):
        assert op.max() == 255 and (op > 5).sum() > len(op) // 2 and ro[-1] > 4 * WINDOW
        assert key.min() < -(1 << 62) and key.max() > (1 << 62)
    yield "random_bytes", case, check


def gen_dense(fmt):
    """windows of nothing but empty records (9 bytes each in catch-up, 12 in durable): the most
    records a window can overlap. One lead record of c commands shifts the phase of the record
    starts against the window boundaries through every residue"""
    e = rec_len(fmt, 0)
    most = 0
    for c in range(e):
        cnt = np.array([c] + [0] * 2800)

        def check(ro, cnt=cnt, c=c):
            nonlocal most
            ov = window_overlaps(ro)
            assert ro[1] == e + 17 * c and set(np.diff(ro[1:])) == {e}
            assert sum(1 for a, b in ov if cnt[a:b].max() == 0) >= 3
            most = max(most, max(b - a for a, b in ov))
            if c == e - 1:  # every phase seen: some window held as many records as one can
                assert most == (WINDOW - 2) // e + 2
                assert most == MAX_RECS or fmt == R.LOG_DURABLE
        yield f"lead{c}", mk_case(cnt, 200 + c), check


def gen_sweep(fmt):
    """a probe record of 3 commands placed so that output byte 8192 is its byte p, for every p from
    the record's first byte to one past its last; then a catch-up probe of 64 commands with the
    boundary on each byte of its 2-byte varint"""
    probes = [(3, p) for p in range(rec_len(fmt, 3) + 1)]
    if fmt == R.LOG_CATCHUP:
        probes += [(64, 8), (64, 9)]
    for c, p in probes:
        lead = filler(fmt, WINDOW - p)
        cnt = lead + [c, 2, 0]

        def check(ro, k=len(lead), c=c, p=p):
            assert ro[k] == WINDOW - p and ro[k + 1] == WINDOW - p + rec_len(fmt, c)
            assert len(ro) == k + 4
        yield f"probe{c}_byte{p}", mk_case(cnt, 300 + p + c), check


def gen_totals(fmt):
    """totals of exactly one and two windows and a byte either side; a last record that starts
    exactly at a window boundary"""
    tail = [4, 7]
    for total in (WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW - 1, 2 * WINDOW, 2 * WINDOW + 1):
        cnt = filler(fmt, total - rec_len(fmt, 4) - rec_len(fmt, 7)) + tail

        def check(ro, total=total):
            assert ro[-1] == total
        yield f"total{total}", mk_case(cnt, 400 + total), check
    for at in (WINDOW, 2 * WINDOW):
        cnt = filler(fmt, at) + [2]

        def check(ro, at=at):
            assert ro[-2] == at and ro[-1] == at + rec_len(fmt, 2)
        yield f"last_starts_at{at}", mk_case(cnt, 500 + at), check


def gen_scan_tile(fmt):
    """record counts around the offsets scan's tile"""
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        cnt = np.random.default_rng(600 + n).integers(0, 4, n)

        def check(ro, n=n):
            assert len(ro) == n + 1
        yield f"n{n}", mk_case(cnt, 700 + n), check


FAMILIES = {"varint": gen_varint, "full_range": gen_full_range, "dense": gen_dense,
            "sweep": gen_sweep, "totals": gen_totals, "scan_tile": gen_scan_tile}
_edge_cache = {}


def edge_cases(family, fmt):
    """[(label, case, expected bytes, expected rec_off)] of one family in one format; the
    restatement runs once per process and every generator's geometry is asserted here"""
    if (family, fmt) not in _edge_cache:
        out = []
        for label, case, check in FAMILIES[family](fmt):
            want, ro = expected(fmt, *case)
            check(ro)
            out.append((label, case, want, ro))
        _edge_cache[family, fmt] = out
    return _edge_cache[family, fmt]


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_edges_oracle_vs_restatement(family, fmt):
    o = Oracle()
    cases = edge_cases(family, fmt)
    assert cases
    for label, case, want, ro in cases:
        out, oro = o.encode_log(fmt, *case)
        assert list(oro) == ro, label
        assert out.tobytes() == want, label


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_edges_gpu_host_form(mk_engine, family, fmt):
    e = mk_engine(5, R.MODE_MIN)
    for label, case, want, ro in edge_cases(family, fmt):
        out, gro = e.encode_log(fmt, *case)
        assert list(gro) == ro, label
        assert out.tobytes() == want, label


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_out_cap_too_small(mk_engine, fmt):
    """rec_off[n] > out_cap: MPX_E_INVAL, rec_off fully written, out left as it was passed"""
    import ctypes as C
    e = mk_engine(5, R.MODE_MIN)
    label, case, want, ro = edge_cases("totals", fmt)[1]
    recs, off, op, key, val = case
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for cap in (len(want) - 1, WINDOW // 2, 0):
        out = np.full(max(cap, 1), 0x5A, np.uint8)
        gro = np.full(len(recs) + 1, 0x5A5A5A5A5A5A5A5A, np.uint64)
        rc = e.lib.mpx_encode_log(e.h, fmt, p(recs), len(recs), p(off), p(op), p(key), p(val),
                                  len(op), p(out) if cap else None, cap, p(gro))
        assert rc == R.E_INVAL, cap
        assert list(gro) == ro, cap
        assert np.all(out == 0x5A), cap
    # the handle stays usable, and a capacity of exactly the encoding is enough
    out = np.full(len(want), 0x5A, np.uint8)
    gro = np.zeros(len(recs) + 1, np.uint64)
    rc = e.lib.mpx_encode_log(e.h, fmt, p(recs), len(recs), p(off), p(op), p(key), p(val),
                              len(op), p(out), len(out), p(gro))
    assert rc == 0 and list(gro) == ro and out.tobytes() == want


@pytest.mark.gpu
def test_catchup_suffix_per_peer_gpu(mk_engine):
    """bcastAccept's per-peer CatchUpLog: out[rec_off[from]:] is the encoding of the suffix run"""
    e = mk_engine(5, R.MODE_MIN)
    label, (recs, off, op, key, val), want, ro = edge_cases("full_range", R.LOG_CATCHUP)[0]
    out, gro = e.encode_log(R.LOG_CATCHUP, recs, off, op, key, val)
    assert out.tobytes() == want
    for frm in (0, 1, 350, len(recs) - 1, len(recs)):
        c0 = int(off[frm])
        sub, sro = e.encode_log(R.LOG_CATCHUP, recs[frm:], off[frm:] - off[frm], op[c0:],
                                key[c0:], val[c0:])
        assert out[int(gro[frm]):].tobytes() == sub.tobytes() == want[ro[frm]:], frm
        assert [int(x) + ro[frm] for x in sro] == ro[frm:], frm


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R.LOG_CATCHUP, R.LOG_DURABLE])
def test_logenc_parity(mk_engine, fmt):
    e, o = mk_engine(5, R.MODE_MIN), Oracle()
    cases = [sample()]
    for n, c, ragged in ((1, 1, False), (10, 4, True), (4000, 4, True), (100000, 4, False),
                         (300, 40, True)):
        cases.append(synth.log_records(n, c, seed=n + c, ragged=ragged))
    recs, off, op, key, val = synth.log_records(600, 2, seed=9, ragged=True)
    big = np.array(off, np.int64)
    big[300:] += 900  # one instance with 900 commands (many 4 KB blocks, 2-byte varint)
    m = int(big[-1])
    bop, bkey, bval = synth.commands(m, 1 << 10, 0.5, "uniform", seed=10)
    cases.append((recs, big.astype(np.uint64), bop, bkey, bval))
    empty = np.zeros(0, R.LOG_REC)
    cases.append((empty, np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.int64),
                  np.zeros(0, np.int64)))
    for recs, off, op, key, val in cases:
        got = e.encode_log(fmt, recs, off, op, key, val)
        want = o.encode_log(fmt, recs, off, op, key, val)
        assert np.array_equal(got[1], want[1]), len(recs)
        assert got[0].tobytes() == want[0].tobytes(), len(recs)

"""GPU tests of mpx_unmarshal_frames: Accept, Commit and PrepareReply payloads from the frames
mpx_decode_stream found to the records and SoA arrays the engine consumes, host and device forms,
MIN and CLASSIC, bit for bit against tests/unmarshal_translit.py. Shapes are the smallest that
reach each path: the heads and the log walk run a lane per frame in workgroups of 256, a scan tile
holds 4096 items, a gather workgroup takes 1024 output commands."""
import ctypes as C

import numpy as np
import pytest

import proposer_translit as P
import test_unmarshal_translit as KA
import unmarshal_translit as U
from devguard import Guard
from go_translit import GoBackend
from minpaxos_amd import _lib
from minpaxos_amd import records as R
from minpaxos_amd import wire as W
from minpaxos_amd.devbuf import H2D, Arena
from minpaxos_amd.engine import MpxError

pytestmark = pytest.mark.gpu
MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
MODES = [MIN, CLASSIC]
MODE_IDS = ["min", "classic"]
ACCEPT, COMMIT, PREPARE_REPLY = R.PEER_ACCEPT, R.PEER_COMMIT, R.PEER_PREPARE_REPLY
TILE = 1024
COUNTS = ("n_accepts", "n_commits", "n_cmds", "n_log_inst", "n_log_cmds", "n_var")
DTYPES = {"accepts": R.ACCEPT_MSG, "accept_last_committed": np.int32, "commits": R.ACCEPT_MSG,
          "cmd_off": np.uint64, "op": np.uint8, "key": np.int64, "val": np.int64,
          "log_inst_off": np.uint64, "log_recs": R.LOG_REC, "log_cmd_off": np.uint64,
          "log_op": np.uint8, "log_key": np.int64, "log_val": np.int64}
CAP_OF = {"accepts": 0, "accept_last_committed": 0, "commits": 1, "op": 2, "key": 2, "val": 2,
          "log_recs": 3, "log_op": 4, "log_key": 4, "log_val": 4}


def same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape,
                                                                 want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        diff = [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()][:5]
        raise AssertionError(f"{name} differs at {diff}: got {got[diff]} want {want[diff]}")


def full_caps(n):
    return (n["n_accepts"], n["n_commits"], n["n_cmds"], n["n_log_inst"], n["n_log_cmds"])


def prefix(want, n, caps):
    """what a call with these capacities leaves: every array cut to min(count, capacity)"""
    w = {k: v[:caps[CAP_OF[k]]] if k in CAP_OF else v for k, v in want.items()}
    w["log_cmd_off"] = want["log_cmd_off"][:min(n["n_log_inst"], caps[3]) + 1]
    return w


def same_all(what, got, res, want, n, caps=None):
    w = want if caps is None else prefix(want, n, caps)
    for name in R.UNMARSHAL_ARRAYS:
        same(f"{what}: {name}", got[name], w[name])
    assert {k: int(res[k]) for k in COUNTS} == n, what  # complete whatever the capacities


def um_dev(e, ar, buf, var, n, caps=None, op_shift=0, stream=None, g_buf=None):
    """the _dev form on guarded outputs, each exactly its capacity long; returns what the host
    form returns. n: the expected counts (they size the buffers)."""
    caps = full_caps(n) if caps is None else caps
    nv = len(var)
    d_buf = ar.put(np.frombuffer(buf, np.uint8)) if g_buf is None else g_buf
    d_var = ar.put(var)
    shape = {"cmd_off": nv + 1, "log_inst_off": nv + 1, "log_cmd_off": caps[3] + 1}
    g = {name: Guard(ar, shape.get(name, caps[CAP_OF.get(name, 0)]), DTYPES[name], name=name,
                     shift=op_shift if name in ("op", "log_op") else 0)
         for name in R.UNMARSHAL_ARRAYS}
    g_res = Guard(ar, 1, R.UNMARSHAL_RESULT)
    out = _lib.MpxUnmarshalOut()
    for name in R.UNMARSHAL_ARRAYS:
        setattr(out, name, g[name].ptr)
    out.accept_cap, out.commit_cap, out.cmd_cap, out.log_inst_cap, out.log_cmd_cap = caps
    e.unmarshal_frames_reserve(nv, n["n_log_inst"])
    e.unmarshal_frames_dev(d_buf.ptr, len(buf), d_var.ptr, nv, None, out, g_res.ptr, stream)
    e.stream_synchronize(stream)
    e.synchronize()
    got = {name: g[name].assert_margins() for name in R.UNMARSHAL_ARRAYS}
    li = min(n["n_log_inst"], caps[3])
    g["log_cmd_off"].assert_untouched([(li + 1, caps[3] + 1)])
    got["log_cmd_off"] = got["log_cmd_off"][:li + 1]
    for name, k in CAP_OF.items():  # nothing past the count either
        c = min(n[COUNTS[k]], caps[k])
        g[name].assert_untouched([(c, caps[k])])
        got[name] = got[name][:c]
    return got, g_res.assert_margins()[0]


def check(e, mode, buf, var=None, msgs=None, dev=True, op_shift=0):
    """host form and _dev form against the transliteration; returns (want, counts, var)"""
    if var is None:
        var, msgs = U.walk(mode, buf)
    want, n = U.flatten(mode, msgs) if msgs is not None else U.expected(mode, buf, var)
    got, res = e.unmarshal_frames(buf, var)
    same_all("host form", got, res, want, n)
    if dev:
        with Arena(e) as ar:
            got, res = um_dev(e, ar, buf, var, n, op_shift=op_shift)
            same_all("_dev form", got, res, want, n)
    return want, n, var


def rcmds(rng, k):
    return [(int(rng.integers(0, 6)), int(rng.integers(-(1 << 63), 1 << 63)),
             int(rng.integers(-(1 << 63), 1 << 63))) for _ in range(k)]


def frame(mode, rng, code, n_cmds, log_counts=()):
    """one variable-length frame with random fields; log_counts: commands per log instance"""
    f = [int(x) for x in rng.integers(-(1 << 31), 1 << 31, 5)]
    log = [(int(rng.integers(0, 99)), int(rng.integers(0, 4)), rcmds(rng, k))
           for k in log_counts] if mode == MIN else []
    if code == ACCEPT:
        return W.accept(mode, f[0], f[1], f[2], rcmds(rng, n_cmds), f[3], log)
    if code == COMMIT:
        return W.commit(f[0], f[1], f[2], rcmds(rng, n_cmds))
    return W.prepare_reply(mode, f[1], f[4] & 1, f[2], rcmds(rng, n_cmds), f[0] & 3, f[3], log)


# ---- known answers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_known_answers(mk_engine, mode):
    """the hand-traced answers of test_unmarshal_translit.py through the host form: the expected
    arrays come from the messages written out there, not from a second unmarshal"""
    e = mk_engine(3, mode)
    known = [k for k in KA.KNOWN if k[1] == mode]
    assert len(known) >= 5
    for k in known:
        name, _, _, offset, code, msg = k
        buf = KA.known_bytes(k)
        rec, _, _ = U.var_frame(mode, buf, offset)
        want, n = U.flatten(mode, [(code, msg)])
        got, res = e.unmarshal_frames(buf, np.array([rec], R.VAR_FRAME))
        same_all(name, got, res, want, n)
    stream = b"".join(KA.known_bytes(k) for k in known)
    var, _ = U.walk(mode, stream)
    want, n = U.flatten(mode, [(k[4], k[5]) for k in known])
    got, res = e.unmarshal_frames(stream, var)
    same_all("all known answers as one stream", got, res, want, n)
    if mode == MIN:  # the arrays test_known_var_frame_and_flattened_arrays writes out by hand
        assert got["log_recs"].tolist()[:4] == [(18, 3, 6, 0), (16, 3, 8, 0), (16, 2, 9, 0),
                                                (49, 3, 3, 0)]
        assert got["cmd_off"].tolist()[:6] == [0, 1, 1, 2, 4, 5]
        assert got["accepts"].tolist()[:3] == [(5, 33, 1, 0), (7, 18, 2, 1), (10, 16, 0, 2)]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_no_frames(mk_engine, mode):
    e = mk_engine(3, mode)
    got, res = e.unmarshal_frames(b"", np.zeros(0, R.VAR_FRAME))
    assert all(len(got[k]) == 0 for k in CAP_OF) and not any(int(res[k]) for k in COUNTS)
    assert got["cmd_off"].tolist() == got["log_inst_off"].tolist() == [0]
    assert got["log_cmd_off"].tolist() == [0]
    buf = W.accept_reply(mode, 1, 1, 2, 3) * 3  # bytes without a variable-length frame
    check(e, mode, buf)


# ---- frame counts: wave, workgroup, one past a scan tile --------------------------------------------
@pytest.mark.parametrize("nf", [1, 63, 64, 65, 255, 256, 257, 4097])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_frame_counts(mk_engine, mode, nf):
    rng = np.random.default_rng(nf)
    codes = [ACCEPT, COMMIT, PREPARE_REPLY]
    buf = b"".join(frame(mode, rng, codes[(i * 7 // 3) % 3], i % 3, [i % 2] * (i % 3 == 1))
                   for i in range(nf))
    want, n, _ = check(mk_engine(3, mode), mode, buf)
    assert n["n_var"] == nf and n["n_accepts"] + n["n_commits"] <= nf


# ---- command counts at the gather tile's edges -------------------------------------------------------
@pytest.mark.parametrize("k", [TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_commands_in_one_frame(mk_engine, mode, k):
    """a single frame of k commands; MIN: its log holds one instance of k commands as well"""
    rng = np.random.default_rng(k)
    buf = frame(mode, rng, ACCEPT, k, [k])
    want, n, _ = check(mk_engine(3, mode), mode, buf)
    assert n["n_cmds"] == k and n["n_log_cmds"] == (k if mode == MIN else 0)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_1025_commands_over_small_frames(mk_engine, mode):
    """frames of 1 to 3 commands: the tile holds hundreds of owners, and the 17-byte stride plus
    the headers puts commands at every byte phase mod 16"""
    rng = np.random.default_rng(5)
    ks, total = [], 0
    while total < TILE + 1:
        k = min(int(rng.integers(1, 4)), TILE + 1 - total)
        ks.append(k)
        total += k
    buf = b"".join(frame(mode, rng, [ACCEPT, COMMIT, PREPARE_REPLY][i % 3], k, [k % 3])
                   for i, k in enumerate(ks))
    want, n, var = check(mk_engine(3, mode), mode, buf)
    assert n["n_cmds"] == TILE + 1 and len(var) > 256
    phases = {(int(v["cmds_off"]) + 17 * j) % 16 for v in var for j in range(int(v["n_cmds"]))}
    assert phases == set(range(16))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_varint_steps(mk_engine, mode):
    """63 / 64 and 8191 / 8192 commands (V(n) of 1, 2 and 3 bytes) in a Command slice and, MIN, in
    a log instance"""
    rng = np.random.default_rng(9)
    steps = [63, 64, 8191, 8192]
    buf = b"".join(frame(mode, rng, [ACCEPT, PREPARE_REPLY][i % 2], k, [steps[3 - i], 0])
                   for i, k in enumerate(steps))
    buf += frame(mode, rng, COMMIT, 64)
    want, n, var = check(mk_engine(3, mode), mode, buf)
    assert sorted(int(x) for x in var["n_cmds"]) == [63, 64, 64, 8191, 8192]
    if mode == MIN:
        assert sorted(np.diff(want["log_cmd_off"].astype(np.int64)).tolist())[4:] == steps


def test_um_catch_up_logs(mk_engine):
    """logs of 0, 1, 2 and 300 instances, instances of 0 commands among them, and one frame whose
    log holds more commands than a gather tile"""
    rng = np.random.default_rng(11)
    big = [(j * 5) % 11 for j in range(300)]
    assert sum(big) > TILE and 0 in big
    logs = [[], [0], [3], [0, 2], [2, 0], big, [0] * 5]
    buf = b"".join(frame(MIN, rng, [ACCEPT, PREPARE_REPLY][i % 2], i % 3, lg)
                   for i, lg in enumerate(logs))
    want, n, var = check(mk_engine(3, MIN), MIN, buf)
    assert [int(x) for x in var["n_log"]] == [0, 1, 1, 2, 2, 300, 5]
    assert n["n_log_inst"] == 311 and n["n_log_cmds"] == sum(big) + 7
    # inst_no: the range ends at the frame's LastCommitted
    lo, hi = int(want["log_inst_off"][5]), int(want["log_inst_off"][6])
    lc = U.unmarshal(MIN, buf, int(var["offset"][5]))[1]["LastCommitted"]
    assert [U.wrap32(int(x)) for x in want["log_recs"]["inst_no"][lo:hi]] == \
        [U.wrap32(lc - 299 + j) for j in range(300)]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_mixed_codes_and_ranks(mk_engine, mode):
    """Accept, Commit and PrepareReply interleaved with fixed-size frames: the compacted outputs
    keep stream order and name their frames"""
    rng = np.random.default_rng(13)
    codes = [int(c) for c in rng.choice([ACCEPT, COMMIT, PREPARE_REPLY], 700)]
    parts = []
    for i, c in enumerate(codes):
        parts.append(frame(mode, rng, c, int(rng.integers(0, 4)), [1] * int(rng.integers(0, 3))))
        if i % 3 == 0:
            parts.append(W.accept_reply(mode, i, 1, 16, 2))
        if i % 50 == 0:
            parts.append(bytes([200]))
    e = mk_engine(5, mode)
    buf = b"".join(parts)
    want, n, var = check(e, mode, buf)
    assert [int(c) for c in var["code"]] == codes
    assert want["accepts"]["value_id"].tolist() == [i for i, c in enumerate(codes) if c == ACCEPT]
    assert want["commits"]["value_id"].tolist() == [i for i, c in enumerate(codes) if c == COMMIT]
    # the stream decoder finds the same frames
    _, pr, dvar, _, res = e.decode_stream(buf)
    assert int(res["stop_reason"]) == R.DECODE_END and len(dvar) == len(var)
    for f in ("offset", "length", "n_cmds", "cmds_off", "n_log", "log_off", "code"):
        assert np.array_equal(dvar[f], var[f]), f
    assert pr["value_id"].tolist() == [i for i, c in enumerate(codes) if c == PREPARE_REPLY]


# ---- capacities, alignment, the buffer's end ----------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_short_capacities(mk_engine, mode):
    """every capacity one short of its count, then 0: the counts stay complete and nothing is
    written at or past a capacity (the _dev outputs are guarded and exactly that long)"""
    e = mk_engine(3, mode)
    buf, _ = U.fuzz_stream(2, mode)
    var, msgs = U.walk(mode, buf)
    want, n = U.flatten(mode, msgs)
    full = full_caps(n)
    assert min(full[:3]) > 1 and (mode == CLASSIC or min(full) > 1)
    for caps in (tuple(max(c - 1, 0) for c in full), (0,) * 5, (1, 0, 5, 2, 3)):
        got, res = e.unmarshal_frames(buf, var, caps=caps)
        same_all(f"host form, caps {caps}", got, res, want, n, caps)
        with Arena(e) as ar:
            got, res = um_dev(e, ar, buf, var, n, caps=caps)
            same_all(f"_dev form, caps {caps}", got, res, want, n, caps)


@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_misaligned_op_outputs(mk_engine, mode, shift):
    rng = np.random.default_rng(17)
    buf = b"".join(frame(mode, rng, ACCEPT, k, [k + 1, 2]) for k in (5, TILE + 3, 0, 9))
    check(mk_engine(3, mode), mode, buf, op_shift=shift)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_buffer_ends_on_a_frames_last_byte(mk_engine, mode):
    """the buffer's last byte is the last byte of a Guard payload, at every length mod 16 (the
    kernels read whole 16-byte vectors, never one at or past len rounded up to 16: argued in
    unmarshal.hip). Only the results are asserted: a read does not trip a guard."""
    e = mk_engine(3, mode)
    rng = np.random.default_rng(19)
    seen = set()
    for k in range(16):
        buf = bytes(k) + frame(mode, rng, ACCEPT, 2, [1]) + frame(mode, rng, COMMIT, 3)
        seen.add(len(buf) % 16)
        var, msgs = U.walk(mode, buf)
        want, n = U.flatten(mode, msgs)
        with Arena(e) as ar:
            g_buf = Guard(ar, len(buf), np.uint8).put(np.frombuffer(buf, np.uint8))
            got, res = um_dev(e, ar, buf, var, n, g_buf=g_buf)
            same_all(f"pad {k}", got, res, want, n)
    assert seen == set(range(16))


def test_um_errors(mk_engine):
    e = mk_engine(3, MIN)
    rng = np.random.default_rng(23)
    buf = frame(MIN, rng, ACCEPT, 1, [1])
    var, msgs = U.walk(MIN, buf)
    want, n = U.flatten(MIN, msgs)
    with Arena(e) as ar:  # the _dev form needs its reserve
        d_buf, d_var = ar.put(np.frombuffer(buf, np.uint8)), ar.put(var)
        out = _lib.MpxUnmarshalOut()
        g_res = Guard(ar, 1, R.UNMARSHAL_RESULT)
        with pytest.raises(MpxError, match="mpx_unmarshal_frames_reserve"):
            e.unmarshal_frames_dev(d_buf.ptr, len(buf), d_var.ptr, 1, None, out, g_res.ptr)
        with pytest.raises(MpxError) as ei:  # a misaligned buffer is refused before any launch
            e.unmarshal_frames_dev(d_buf.ptr + 4, len(buf) - 4, d_var.ptr, 1, None, out, g_res.ptr)
        assert ei.value.code == R.E_INVAL
    bad = var.copy()
    bad["n_log"] = 2  # the frame's bytes hold one instance: the walk cannot end at the frame's end
    with pytest.raises(MpxError) as ei:
        e.unmarshal_frames(buf, bad)
    assert ei.value.code == R.E_INVAL
    bad = var.copy()
    bad["code"] = R.PEER_ACCEPT_REPLY
    with pytest.raises(MpxError) as ei:
        e.unmarshal_frames(buf, bad)
    assert ei.value.code == R.E_INVAL
    got, res = e.unmarshal_frames(buf, var)  # the engine is usable afterwards
    same_all("after the errors", got, res, want, n)


# ---- decode -> unmarshal on device buffers, captured once -----------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_device_chain_graph_replay(mk_engine, mode):
    """mpx_decode_stream_dev then mpx_unmarshal_frames_dev with n_var = var_cap and d_n_var
    pointing at the stream result's n_var, captured once and replayed on two different buffers
    written into the same device memory (frames of at most 64 bytes: one decode call frames the
    whole buffer)"""
    e = mk_engine(3, mode)
    rng = np.random.default_rng(29)

    def stream(nf):
        parts = []
        for i in range(nf):
            parts.append(frame(mode, rng, [ACCEPT, COMMIT, PREPARE_REPLY][int(rng.integers(0, 3))],
                               int(rng.integers(0, 3)), [0] * int(rng.integers(0, 2))))
            assert len(parts[-1]) <= 64
            if i % 4 == 0:
                parts.append(W.accept_reply(mode, i, 1, 16, 1))
        return b"".join(parts)
    a, b = stream(300), stream(140)
    size = max(len(a), len(b))
    bufs = [x + bytes([200]) * (size - len(x)) for x in (a, b)]  # unknown codes: 1-byte frames
    var_cap = 400
    wants = [U.expected(mode, x, U.walk(mode, x)[0]) for x in bufs]
    caps = tuple(max(w[1][k] for w in wants) for k in COUNTS[:5])
    n_off = R.STREAM_RESULT.fields["n_var"][1]
    with Arena(e) as ar:
        d_buf = ar.empty(size, np.uint8)
        g_var = Guard(ar, var_cap, R.VAR_FRAME)
        d_ar, d_oth = ar.empty(size, R.ACCEPT_REPLY), ar.empty(size, R.PEER_FRAME)
        d_pr = ar.empty(var_cap, R.PREPARE_REPLY_MIN if mode == MIN else R.PREPARE_REPLY)
        d_sres = ar.empty(1, R.STREAM_RESULT)
        dec = _lib.MpxDecodeOut(d_ar.ptr, size, d_pr.ptr, var_cap, g_var.ptr, var_cap, d_oth.ptr,
                                size)
        shape = {"cmd_off": var_cap + 1, "log_inst_off": var_cap + 1, "log_cmd_off": caps[3] + 1}
        g = {name: Guard(ar, shape.get(name, caps[CAP_OF.get(name, 0)]), DTYPES[name], name=name)
             for name in R.UNMARSHAL_ARRAYS}
        g_res = Guard(ar, 1, R.UNMARSHAL_RESULT)
        out = _lib.MpxUnmarshalOut()
        for name in R.UNMARSHAL_ARRAYS:
            setattr(out, name, g[name].ptr)
        out.accept_cap, out.commit_cap, out.cmd_cap, out.log_inst_cap, out.log_cmd_cap = caps
        e.decode_stream_reserve(size)
        e.unmarshal_frames_reserve(var_cap, caps[3])
        s = e.stream_create()
        e.graph_begin(s)
        e.memset(d_sres.ptr, 0, R.STREAM_RESULT.itemsize, s)
        e.decode_stream_dev(d_buf.ptr, size, 0, dec, d_sres.ptr, s)
        e.unmarshal_frames_dev(d_buf.ptr, size, g_var.ptr, var_cap, d_sres.ptr + n_off, out,
                               g_res.ptr, s)
        gr = e.graph_end(s)
        try:
            for rnd in (0, 1, 0):
                x = np.frombuffer(bufs[rnd], np.uint8)
                want, n = wants[rnd]
                e.memcpy(d_buf.ptr, x.ctypes.data_as(C.c_void_p), size, H2D, s)
                for gd in list(g.values()) + [g_var, g_res]:
                    gd.fill(s)
                e.graph_launch(gr, s)
                e.stream_synchronize(s)
                e.synchronize()
                sres = ar.get(d_sres)[0]
                assert int(sres["stop_reason"]) == R.DECODE_END and int(sres["n_var"]) == n["n_var"]
                got = {name: g[name].assert_margins() for name in R.UNMARSHAL_ARRAYS}
                res = g_res.assert_margins()[0]
                nv = n["n_var"]
                # past the processed frames the offsets repeat the totals
                assert (got["cmd_off"][nv:] == n["n_cmds"]).all()
                assert (got["log_inst_off"][nv:] == n["n_log_inst"]).all()
                got["cmd_off"], got["log_inst_off"] = got["cmd_off"][:nv + 1], got["log_inst_off"][:nv + 1]
                got["log_cmd_off"] = got["log_cmd_off"][:n["n_log_inst"] + 1]
                for name, k in CAP_OF.items():
                    got[name] = got[name][:n[COUNTS[k]]]
                same_all(f"replay on buffer {rnd}", got, res, want, n)
        finally:
            e.graph_destroy(gr)
            e.stream_destroy(s)
        e.synchronize()


# ---- identity with the encoder ---------------------------------------------------------------------
@pytest.mark.parametrize("n_rep", [3, 5])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_inverts_encode_accepts(mk_engine, mode, n_rep):
    """mpx_encode_accepts on a fuzzed batch; each destination's run through mpx_decode_stream and
    mpx_unmarshal_frames gives back the sends' instance, ballot, last_committed and commands, and
    exactly the catch-up range of the log the encoder was given"""
    e = mk_engine(n_rep, mode)
    a = P.fuzz_encode(3, n_rep, mode)
    out, off = e.encode_accepts(**a)
    op, key, val = a["cmds"]
    lrec, lcoff, lop, lkey, lval = a["log"]
    base, ipg = a["inst_base"], a["ipg"]
    sends = {int(s["instance"]): s for s in a["sends"] if int(s["flags"]) & R.PH_ACCEPT}
    frames = 0
    for q in range(n_rep):
        run = out[int(off[q]):int(off[q + 1])].tobytes()
        if not run:
            continue
        _, _, var, _, res = e.decode_stream(run)
        assert int(res["stop_reason"]) == R.DECODE_END
        got, r = e.unmarshal_frames(run, var)
        assert int(r["n_accepts"]) == len(var) == len(got["accepts"]) and int(r["n_commits"]) == 0
        for i, m in enumerate(got["accepts"]):
            s = sends[int(m["instance"])]
            g = (int(m["instance"]) - base) // ipg
            assert int(m["value_id"]) == i and int(m["ballot"]) == int(s["ballot"])
            assert int(m["leader_id"]) == int(a["groups"][g]["self_id"])
            c0, c1 = int(got["cmd_off"][i]), int(got["cmd_off"][i + 1])
            f0 = int(s["first_cmd"])
            assert c1 - c0 == int(s["n_cmds"])
            for x, y in ((got["op"], op), (got["key"], key), (got["val"], val)):
                assert np.array_equal(x[c0:c1], y[f0:f0 + c1 - c0])
            l0, l1 = int(got["log_inst_off"][i]), int(got["log_inst_off"][i + 1])
            if mode == CLASSIC:
                assert int(got["accept_last_committed"][i]) == -1 and l0 == l1 == 0
                continue
            lc = int(s["last_committed"])
            assert int(got["accept_last_committed"][i]) == lc
            first = base + g * ipg
            pc = int(np.asarray(a["peer_commits"]).reshape(-1, n_rep)[g, q])
            lo = first if pc < first else pc + 1  # bareminpaxos.go:496-506
            assert l1 - l0 == max(lc - lo + 1, 0)
            for j in range(l1 - l0):
                k = lo + j - base  # the window index the record was encoded from
                rec = got["log_recs"][l0 + j]
                assert (int(rec["ballot"]), int(rec["status"]), int(rec["inst_no"]), int(rec["pad"])) \
                    == (int(lrec[k]["ballot"]), int(lrec[k]["status"]), lo + j, 0)
                a0, a1 = int(got["log_cmd_off"][l0 + j]), int(got["log_cmd_off"][l0 + j + 1])
                b0, b1 = int(lcoff[k]), int(lcoff[k + 1])
                assert a1 - a0 == b1 - b0
                for x, y in ((got["log_op"], lop), (got["log_key"], lkey), (got["log_val"], lval)):
                    assert np.array_equal(x[a0:a1], y[b0:b1])
            frames += 1
    assert mode == CLASSIC or frames > 0


# ---- the Phase-2 round trip with the unmarshal station in it -----------------------------------------
def test_phase2_round_trip_unmarshalled(mk_engine):
    """the three-round loop of test_gpu_proposer.py::test_phase2_round_trip with the followers'
    struct.unpack_from bridge replaced by mpx_unmarshal_frames: propose_handle -> encode_accepts;
    four followers decode_stream -> unmarshal_frames -> accept_handle -> encode_accept_replies; the
    leader decode_stream -> accept_tally. Each follower also checks the Command and the catch-up
    log it received against what the leader proposed and committed."""
    N = 5
    e = mk_engine(N, MIN)
    rng = np.random.default_rng(77)
    ipg, base, D = 16, 200, 32
    grp = P.mk_groups([(D, 0, 0, 3, base, base - 1)])
    st = P.nil_state(ipg)
    lb = np.zeros(ipg, R.INST_STATE)
    fst = [P.nil_state(ipg) for _ in range(N)]
    counts = [None] * ipg
    log_cmds = [np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64)]
    committed = []  # the commands of every committed instance, by round
    cu, pcs = base - 1, np.full(N, base - 1, np.int32)
    for rnd in range(3):
        k = int(rng.integers(1, 6))
        cmds = P.mk_cmds(rng, k)
        grp["committed_upto"] = cu
        grp, st, lb, sends, _ = e.propose_handle(grp, np.array([0, k], np.uint64), st, base, ipg, lb)
        inst = base + rnd
        assert int(sends["flags"][0]) == R.PH_ACCEPT and int(sends["instance"][0]) == inst
        lrec = np.zeros(ipg, R.LOG_REC)
        lrec["status"] = [P.NIL if c is None else R.COMMITTED for c in counts]
        lrec["ballot"] = D
        lcoff = np.zeros(ipg + 1, np.uint64)
        lcoff[1:] = np.cumsum([0 if c is None else c for c in counts])
        out, off = e.encode_accepts(sends=sends, groups=grp, cmds=cmds, inst_base=base, ipg=ipg,
                                    peer_commits=pcs.reshape(1, N), log=(lrec, lcoff, *log_cmds))
        to_leader = []
        for q in range(1, N):
            run = out[int(off[q]):int(off[q + 1])].tobytes()
            _, _, var, _, res = e.decode_stream(run)
            assert int(res["stop_reason"]) == R.DECODE_END and len(var) == 1
            um, r = e.unmarshal_frames(run, var)
            msgs = um["accepts"]
            assert len(msgs) == 1 and msgs[0].tolist() == (inst, D, 0, 0)
            assert int(um["accept_last_committed"][0]) == cu
            # the Command the follower stores is what the leader proposed
            assert all(np.array_equal(x, y) for x, y in zip((um["op"], um["key"], um["val"]), cmds))
            # ... and its catch-up log is every committed instance past what the leader knows of it
            lo = max(int(pcs[q]) + 1, base)
            assert um["log_inst_off"].tolist() == [0, inst - lo]
            assert um["log_recs"]["inst_no"].tolist() == list(range(lo, inst))
            assert (um["log_recs"]["ballot"] == D).all()
            assert (um["log_recs"]["status"] == R.COMMITTED).all()
            for j, i in enumerate(range(lo - base, inst - base)):
                a0, a1 = int(um["log_cmd_off"][j]), int(um["log_cmd_off"][j + 1])
                for x, y in zip((um["log_op"], um["log_key"], um["log_val"]), committed[i]):
                    assert np.array_equal(x[a0:a1], y)
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
        committed.append(cmds)
        log_cmds = [np.concatenate([x, y]) for x, y in zip(log_cmds, cmds)]
        pcs = np.array([cu, cu, cu - 1, base - 1, cu], np.int32)  # 2 lags one, 3 knows nothing


# ---- fuzz ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", U.FUZZ_SEEDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_um_fuzz(mk_engine, mode, seed):
    buf, _ = U.fuzz_stream(seed, mode)
    check(mk_engine(3, mode), mode, buf, op_shift=seed % 4)

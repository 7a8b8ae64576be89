#!/usr/bin/env python3
"""Times the prepare side on device-resident buffers: mpx_prepare_handle_dev, then
mpx_encode_prepare_replies_dev on what it left; 3 warm-ups, the median and range of 20
event-timed calls of each, and of the two back to back. Shapes:

  a_min      65,536 groups x 1 Prepare, the follower as far as the leader: no log (MIN)
  a_classic  65,536 groups x 1 Prepare for an accepted instance of 4 commands (CLASSIC)
  b          65,536 groups x 1 Prepare, each reply with 4 commands and a 2-instance log (MIN)
  c          65,536 groups x 16 Prepares = 2^20 messages, rising ballots, no log (MIN)

The groups are put back (a device copy, outside the timed bracket) before every call, so every
call raises the ballots as the first one does. In the same run, the path the calls replace, wall
clock, median of 5: D2H of the state window, the slots' command ranges and the groups, the handler
as numpy over the batch, a gather of the referenced commands from a D2H copy of the arena, and the
frames built as numpy records and partitioned by destination.

After timing, the device bytes are compared with the replaced path's, whole, and the first 64
groups' records and frames with the transliteration.

    python tools/bench_prepare_handle.py [--shape a_min|a_classic|b|c|all] [--groups G]

One JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from minpaxos_amd import _lib  # noqa: E402
from minpaxos_amd import records as R  # noqa: E402
from minpaxos_amd.devbuf import D2D, Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

IPG, N, SAMPLE = 8, 5, 64
SHAPES = ("a_min", "a_classic", "b", "c")


def workload(shape, G):
    """(mode, msgs, groups, st, inst, arena): every group holds 4 instances of 4 commands; the
    arena is laid out as mpx_store_commands leaves it, turn t's instances of all groups back to
    back, so one group's instances lie 4 G commands apart"""
    mode = R.MODE_CLASSIC if shape == "a_classic" else R.MODE_MIN
    per = 16 if shape == "c" else 1
    g, t = np.divmod(np.arange(G * IPG), IPG)
    used = t < 4
    st = np.zeros(G * IPG, R.ACCEPTOR_STATE)
    st["status"], st["ballot"], st["value_id"] = R.STATUS_NIL, -1, R.VALUE_KEEP
    st["status"][used] = np.where(t[used] < 3, R.COMMITTED, R.ACCEPTED)
    st["ballot"][used] = 5
    inst = np.zeros(G * IPG, R.INST_CMDS)
    inst["first_cmd"][used] = t[used] * 4 * G + 4 * g[used]
    inst["n_cmds"][used] = 4
    inst["flags"][used] = R.IC_HAS_CMDS
    rng = np.random.default_rng(7)
    m = 16 * G
    arena = (rng.integers(1, 4, m).astype(np.uint8), rng.integers(0, 1 << 40, m).astype(np.int64),
             rng.integers(0, 1 << 40, m).astype(np.int64))
    first = np.arange(G, dtype=np.int64) * IPG
    groups = np.zeros(G, R.PROPOSER_GROUP)
    groups["default_ballot"], groups["self_id"] = 7, np.arange(G) % N
    groups["leader"], groups["prepare_oks"] = (np.arange(G) + 2) % N, 3
    groups["crt_instance"], groups["committed_upto"] = first + 3, first + 2
    msgs = np.zeros(G * per, R.PREPARE_MSG)
    gm = np.repeat(np.arange(G), per)
    msgs["leader_id"] = (gm + 1 + np.tile(np.arange(per), G)) % N
    msgs["ballot"] = 16 + np.tile(np.arange(per), G)
    if mode == R.MODE_MIN:
        msgs["key"] = gm
        msgs["arg"] = first[gm] + (0 if shape == "b" else 2)
    else:
        msgs["key"], msgs["arg"] = first[gm] + 3, 1
    return mode, msgs, groups, st, inst, arena


def rng_stats(ms):
    return {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4)}


def timed(eng, before, call, warmup=3, reps=20):
    for _ in range(warmup):
        before()
        call()
    eng.synchronize()
    e0, e1 = eng.event_create(True), eng.event_create(True)
    ms = []
    for _ in range(reps):
        before()
        eng.event_record(e0, eng.stream)
        call()
        eng.event_record(e1, eng.stream)
        eng.synchronize()
        ms.append(eng.event_elapsed_ms(e0, e1))
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms


def host_path(mode, msgs, groups, st, inst, arena, per):
    """the replaced path on host copies: handlePrepare over the batch as numpy, the gather of the
    referenced commands, the frames as records, the stable partition by leader. Every frame of a
    shape has one length, which is what lets numpy build them at all."""
    G = len(groups)
    n = len(msgs)
    g = msgs["key"].astype(np.int64) if mode == R.MODE_MIN else msgs["key"].astype(np.int64) // IPG
    bal = msgs["ballot"].reshape(G, per)
    if mode == R.MODE_MIN:
        # D before message j of a group: the running max of the earlier ballots and D0
        run = np.maximum.accumulate(np.concatenate([groups["default_ballot"][:, None], bal], axis=1),
                                    axis=1)
        ok = (run[:, :-1] < bal).reshape(-1)
        d_after = run[:, 1:].reshape(-1)
        crt = groups["crt_instance"].astype(np.int64)
        k = crt - np.arange(G) * IPG
        while True:  # :725-727, all groups at once
            more = st["status"][np.arange(G) * IPG + np.minimum(k, IPG - 1)] != R.STATUS_NIL
            if not more.any():
                break
            k += more
        crt = (np.arange(G) * IPG + k)[g]
        cu = groups["committed_upto"].astype(np.int64)[g]
        logged = cu > msgs["arg"]
        n_log = np.where(logged, cu - msgs["arg"], 0)
        assert (n_log == n_log[0]).all()
        m_log = int(n_log[0])
        slot = cu + 1
        n_cmd = 4 if m_log else 0
        body = [("code", "u1"), ("id", "<i4"), ("inst", "<i4"), ("ok", "u1"), ("ballot", "<i4"),
                ("lc", "<i4"), ("vn", "u1")]
    else:
        idx = msgs["key"].astype(np.int64)
        run = np.maximum.accumulate(np.concatenate([groups["default_ballot"][:, None], bal], axis=1),
                                    axis=1)
        ok = ~(msgs["ballot"] < st["ballot"][idx])
        slot, n_cmd, m_log = idx, 4, 0
        body = [("code", "u1"), ("inst", "<i4"), ("ok", "u1"), ("ballot", "<i4"), ("vn", "u1")]
    cmd = [("op", "u1"), ("k", "<i8"), ("v", "<i8")]
    for j in range(n_cmd):
        body += [(f"c{j}", cmd)]
    if mode == R.MODE_MIN:
        body += [("vm", "u1")]
        for i in range(m_log):
            body += [(f"b{i}", "<i4"), (f"s{i}", "<i4"), (f"vk{i}", "u1")] + \
                [(f"l{i}_{j}", cmd) for j in range(4)]
    f = np.zeros(n, np.dtype(body))
    f["code"], f["ok"], f["vn"] = R.PEER_PREPARE_REPLY, ok, 2 * n_cmd
    if mode == R.MODE_MIN:
        f["id"], f["inst"], f["ballot"], f["lc"] = groups["self_id"][g], crt - 1, d_after, cu
        f["vm"] = 2 * m_log
    else:
        f["inst"], f["ballot"] = msgs["key"], st["ballot"][idx]

    def put(name, at):
        f[name]["op"], f[name]["k"], f[name]["v"] = arena[0][at], arena[1][at], arena[2][at]
    for j in range(n_cmd):
        put(f"c{j}", inst["first_cmd"][slot].astype(np.int64) + j)
    for i in range(m_log):
        s = msgs["arg"].astype(np.int64) + 1 + i
        f[f"b{i}"], f[f"s{i}"], f[f"vk{i}"] = st["ballot"][s], st["status"][s], 8
        for j in range(4):
            put(f"l{i}_{j}", inst["first_cmd"][s].astype(np.int64) + j)
    order = np.argsort(msgs["leader_id"], kind="stable")
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(msgs["leader_id"], minlength=N)) * f.dtype.itemsize
    return f[order].view(np.uint8), off


def run(shape, G):
    import prepare_handle_translit as T
    mode, msgs, groups, st, inst, arena = workload(shape, G)
    n, per = len(msgs), len(msgs) // G
    rdt = R.PREPARE_REPLY_MIN if mode == R.MODE_MIN else R.PREPARE_REPLY
    with Engine(0, N, mode) as eng, Arena(eng) as ar:
        d = {k: ar.put(v) for k, v in dict(msgs=msgs, groups0=groups, groups=groups, st=st, inst=inst,
                                           sop=arena[0], skey=arena[1], sval=arena[2]).items()}
        d_rep, d_to = ar.empty(n, rdt), ar.empty(n, np.int32)
        d_eff, d_lf = ar.empty(n, np.uint8), ar.empty(n, np.int32)
        lf = d_lf.ptr if mode == R.MODE_MIN else None
        h_out, h_off = host_path(mode, msgs, groups, st, inst, arena, per)
        total = len(h_out)
        d_out, d_off = ar.empty(total, np.uint8), ar.empty(N + 1, np.uint64)
        b = _lib.MpxPrepareReplyBatch()
        b.replies, b.reply_to, b.log_from, b.n, b.n_dest = d_rep.ptr, d_to.ptr, lf, n, N
        b.inst_base, b.n_inst, b.st, b.inst = 0, G * IPG, d["st"].ptr, d["inst"].ptr
        b.src_op, b.src_key, b.src_val, b.n_src = d["sop"].ptr, d["skey"].ptr, d["sval"].ptr, len(arena[0])
        eng.encode_prepare_replies_reserve(n, G * IPG, N)

        def reset():
            eng.memcpy(d["groups"].ptr, d["groups0"].ptr, groups.nbytes, D2D, eng.stream)

        def handle():
            eng.prepare_handle_dev(d["msgs"].ptr, n, d["st"].ptr, G * IPG, 0, d["groups"].ptr, G, IPG,
                                   d_rep.ptr, d_to.ptr, d_eff.ptr, lf, None, None, eng.stream)

        def encode():
            eng.encode_prepare_replies_dev(b, d_out.ptr, total, d_off.ptr, eng.stream)

        def both():
            handle()
            encode()
        t_handle = rng_stats(timed(eng, reset, handle))
        t_encode = rng_stats(timed(eng, lambda: None, encode))
        t_both = rng_stats(timed(eng, reset, both))
        rep, to, eff = ar.get(d_rep), ar.get(d_to), ar.get(d_eff)
        got, off = ar.get(d_out), ar.get(d_off)
        g_after = ar.get(d["groups"])

        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            h_st, h_inst, h_grp = ar.get(d["st"]), ar.get(d["inst"]), ar.get(d["groups0"])
            h_arena = (ar.get(d["sop"]), ar.get(d["skey"]), ar.get(d["sval"]))
            r_out, r_off = host_path(mode, msgs, h_grp, h_st, h_inst, h_arena, per)
            wall.append((time.perf_counter() - t0) * 1e3)
        replaced = rng_stats(wall)
        same = bool(np.array_equal(off, r_off) and got.tobytes() == r_out.tobytes())

        S = min(SAMPLE, G)
        sub = T.run_batch(mode, N, msgs[:S * per], groups[:S], st[:S * IPG], 0, IPG, None,
                          inst[:S * IPG], arena)
        ok = rep[:S * per].tobytes() == sub["replies"].tobytes() and \
            np.array_equal(eff[:S * per], sub["effect"]) and \
            g_after[:S].tobytes() == sub["groups"].tobytes()
        for q in range(N):  # the sample's frames head every destination's run
            kq = int(sub["dest_off"][q + 1] - sub["dest_off"][q])
            ok = ok and got[int(off[q]):int(off[q]) + kq].tobytes() == \
                sub["bytes"][int(sub["dest_off"][q]):int(sub["dest_off"][q + 1])].tobytes()
    # bytes the two calls must move: the handler reads the messages, the groups and one state
    # record per slot it looks at, writes the outputs and the groups; the encoder reads the
    # handler's outputs and the referenced commands and writes the frames
    slots = n * (1 if mode != R.MODE_MIN else (4 if shape == "b" else 1))
    alg_handle = 16 * n + 2 * 32 * G + 16 * slots + (rdt.itemsize + 4 + 1 + (4 if lf else 0)) * n
    alg_encode = (rdt.itemsize + 4 + (4 if lf else 0)) * n + total
    return {"bench": "prepare_handle", "shape": shape, "mode": "classic" if mode else "min",
            "n_replicas": N, "groups": G, "messages": n, "warmup": 3, "timed_calls": 20,
            "frame_bytes": total // n, "out_bytes": total, "handle_dev": t_handle,
            "encode_dev": t_encode, "handle_then_encode_dev": t_both,
            "alg_bytes_handle": alg_handle, "alg_bytes_encode": alg_encode,
            "replaced_path_wall": replaced, "device_equals_replaced": same, "sample_groups": S,
            "sample_exact": bool(ok), "runtime": _lib.runtime_info()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=list(SHAPES) + ["all"])
    ap.add_argument("--groups", type=int, default=1 << 16)
    a = ap.parse_args()
    rc = 0
    for s in (SHAPES if a.shape == "all" else [a.shape]):
        res = run(s, a.groups)
        print(json.dumps(res), flush=True)
        if not (res["device_equals_replaced"] and res["sample_exact"]):
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())

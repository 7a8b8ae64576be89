#!/usr/bin/env python3
"""Times the commit side on device-resident buffers: 3 warm-ups, the median and range of 20
event-timed calls each, algorithmic bytes (every input read once, every output written once) over
the time as a fraction of the 8 TB/s HBM peak, and a sample checked against the transliteration
(tests/commit_translit.py) after timing.

Shapes:
  a  mpx_commit_handle_dev: 65,536 groups x 256 instances with one message each, half of them
     CommitShorts, seed 42, every watermark at first_g - 1 (the prefix walks the whole window).
     The call works in place, so the states and watermarks are restored by two device-to-device
     copies before every call, outside the timed bracket.
  b  mpx_encode_commits_dev, N = 5, not thrifty, 2^24 sends: four 17-byte CommitShorts each
  c  mpx_encode_commits_dev, N = 5, thrifty, 4 commands per send: two CommitShorts and two 82-byte
     Commits each, at the 65,536 sends of the yardstick's shape and at 2^22
  d  mpx_gather_commit_shorts_dev: 2^22 CommitShorts among as many Beacons and AcceptReplies
Yardsticks, taken in the same process (--yardsticks): mpx_accept_handle_dev and
mpx_encode_accept_replies_dev from tools/bench_acceptor.py (a, b) and mpx_encode_accepts_dev in
CLASSIC from tools/bench_proposer.py (c).

    python tools/bench_commit.py [--shape a|b|c|d|all] [--groups G] [--yardsticks]

One JSON line per shape and per yardstick.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from minpaxos_amd import _lib  # noqa: E402
from minpaxos_amd import records as R  # noqa: E402
from minpaxos_amd.devbuf import D2D, Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

HBM_PEAK = 8e12  # B/s, MI355X
N, IPG = 5, 256


def timed(eng, call, before=None, warmup=3, reps=20):
    for _ in range(warmup):
        if before:
            before()
        call()
    eng.synchronize()
    e0, e1 = eng.event_create(True), eng.event_create(True)
    ms = []
    for _ in range(reps):
        if before:
            before()
        eng.event_record(e0, eng.stream)
        call()
        eng.event_record(e1, eng.stream)
        eng.synchronize()
        ms.append(eng.event_elapsed_ms(e0, e1))
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms


def stats(ms, alg):
    med = statistics.median(ms)
    return {"ms_per_call": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "algorithmic_bytes": int(alg),
            "fraction_of_8TBps": round(alg / (med * 1e-3) / HBM_PEAK, 4)}


def shape_a(G, seed=42):
    import commit_translit as T
    rng = np.random.default_rng(seed)
    I = G * IPG
    st = np.zeros(I, R.ACCEPTOR_STATE)
    st["status"] = rng.integers(-1, 4, I)
    live = st["status"] != R.STATUS_NIL
    st["ballot"] = np.where(live, 16, 0)
    st["value_id"] = np.where(live, rng.integers(1, 1 << 31, I), 0)
    st["flags"] = np.where(live, rng.integers(0, 2, I), 0)
    msgs = np.zeros(I, R.ACCEPT_MSG)
    msgs["instance"] = np.arange(I)
    msgs["ballot"] = 32
    msgs["leader_id"] = rng.integers(0, N, I)
    msgs["value_id"] = np.where(rng.random(I) < 0.5, R.VALUE_KEEP, rng.integers(1, 1 << 31, I))
    cu = (np.arange(G) * IPG - 1).astype(np.int32)
    with Engine(0, N, R.MODE_CLASSIC) as eng, Arena(eng) as ar:
        d_msgs, d_st0, d_cu0 = ar.put(msgs), ar.put(st), ar.put(cu)
        d_st, d_cu = ar.empty(I, R.ACCEPTOR_STATE), ar.empty(G, np.int32)
        d_eff, d_log = ar.empty(I, np.uint8), ar.empty(I, R.LOG_REC)

        def restore():
            eng.memcpy(d_st.ptr, d_st0.ptr, d_st0.nbytes, D2D, eng.stream)
            eng.memcpy(d_cu.ptr, d_cu0.ptr, d_cu0.nbytes, D2D, eng.stream)
        out = {}
        for name, log in (("with_log_recs", d_log.ptr), ("without_log_recs", None)):
            ms = timed(eng, lambda: eng.commit_handle_dev(d_msgs.ptr, I, d_st.ptr, I, 0, d_cu.ptr,
                                                          G, IPG, d_eff.ptr, log, eng.stream),
                       before=restore)
            # 16 msg + 16 + 16 state + 1 effect (+ 16 log record), 4 + 4 watermark per group
            out[name] = stats(ms, I * (49 + (16 if log else 0)) + G * 8)
        S = min(64, G)
        want = T.commit_handle(msgs[:S * IPG], st[:S * IPG], cu[:S], 0, IPG)
        got = (ar.get(d_st, S * IPG), ar.get(d_cu, S), ar.get(d_eff, S * IPG),
               ar.get(d_log, S * IPG))
        ok = all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        ok = ok and bool((ar.get(d_cu) == np.arange(1, G + 1) * IPG - 1).all())
    return {"bench": "commit", "shape": "a", "groups": G, "ipg": IPG, "messages": I,
            "commit_handle": out, "sample_groups": S, "sample_bit_exact": bool(ok)}


def encode_shape(name, n_sends, thrifty, n_cmds, seed=42):
    import commit_translit as T
    rng = np.random.default_rng(seed)
    G = max(n_sends // IPG, 1)
    ipg = n_sends // G
    groups = T.mk_self(np.arange(G) % N)
    sends = np.zeros(n_sends, R.COMMIT_SEND)
    sends["instance"] = np.arange(n_sends)
    sends["ballot"] = 32
    sends["first_cmd"] = np.arange(n_sends, dtype=np.uint64) * n_cmds
    sends["n_cmds"] = n_cmds
    sends["flags"] = R.CS_SEND
    m = n_sends * n_cmds
    cmds = (rng.integers(0, 4, m).astype(np.uint8), rng.integers(-(1 << 62), 1 << 62, m),
            rng.integers(-(1 << 62), 1 << 62, m))
    full = R.commit_frame_bytes(n_cmds)
    per_send = 2 * R.COMMIT_SHORT_FRAME + 2 * full if thrifty else 4 * R.COMMIT_SHORT_FRAME
    total = n_sends * per_send
    with Engine(0, N, R.MODE_CLASSIC) as eng, Arena(eng) as ar:
        keep = [ar.put(x) for x in (sends, groups, *cmds)]
        b = _lib.MpxCommitBatch()
        b.sends, b.n_sends, b.inst_base, b.ipg, b.n_groups = keep[0].ptr, n_sends, 0, ipg, G
        b.groups = keep[1].ptr
        b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = keep[2].ptr, keep[3].ptr, keep[4].ptr, m
        b.flags, b.alive_mask = (R.AB_THRIFTY if thrifty else 0), 0xFFFF
        eng.encode_commits_reserve(n_sends)
        d_out, d_off = ar.empty(total, np.uint8), ar.empty(N + 1, np.uint64)
        ms = timed(eng, lambda: eng.encode_commits_dev(b, d_out.ptr, total, d_off.ptr, eng.stream))
        # a send read once, a group's self_id once, the commands a Commit carries once per call
        enc = stats(ms, n_sends * 32 + G * 32 + (17 * m if thrifty else 0) + total)
        off = ar.get(d_off)
        S = min(64 * ipg, n_sends)  # the sample's frames head every destination's run
        w_out, w_off = T.encode_commits(N, sends[:S], groups, cmds, 0, ipg, thrifty=thrifty)
        ok = int(off[-1]) == total
        for q in range(N):
            k = int(w_off[q + 1] - w_off[q])
            ok = ok and ar.get(d_out, k, int(off[q])).tobytes() == \
                w_out[int(w_off[q]):int(w_off[q + 1])].tobytes()
        del keep
    enc.update({"out_bytes": total, "frames": 4 * n_sends, "sample_sends": S,
                "sample_byte_exact": bool(ok)})
    return {"bench": "commit", "shape": name, "n_replicas": N, "sends": n_sends,
            "thrifty": thrifty, "cmds_per_send": n_cmds, "encode_commits": enc,
            "sample_bit_exact": bool(ok)}


def shape_d(K, seed=42):
    import commit_translit as T
    rng = np.random.default_rng(seed)
    # K triples of [CommitShort 17][Beacon 9][AcceptReply 14]: 40 bytes
    buf = rng.integers(0, 256, K * 40, dtype=np.uint8).reshape(K, 40)
    buf[:, 0], buf[:, 17], buf[:, 26] = R.PEER_COMMIT_SHORT, R.PEER_BEACON, R.PEER_ACCEPT_REPLY
    buf = buf.reshape(-1)
    oth = np.zeros(2 * K, R.PEER_FRAME)
    oth["offset"][0::2] = np.arange(K, dtype=np.uint32) * 40
    oth["offset"][1::2] = np.arange(K, dtype=np.uint32) * 40 + 17
    oth["code"][0::2], oth["code"][1::2] = R.PEER_COMMIT_SHORT, R.PEER_BEACON
    with Engine(0, N, R.MODE_MIN) as eng, Arena(eng) as ar:
        d_buf, d_oth = ar.put(buf), ar.put(oth)
        d_m, d_c = ar.empty(K, R.ACCEPT_MSG), ar.empty(K, np.int32)
        d_i, d_n = ar.empty(K, np.uint32), ar.empty(1, np.uint64)
        eng.encode_commits_reserve(0, 2 * K)
        ms = timed(eng, lambda: eng.gather_commit_shorts_dev(
            d_buf.ptr, len(buf), d_oth.ptr, 2 * K, None, d_m.ptr, d_c.ptr, d_i.ptr, K, d_n.ptr,
            eng.stream))
        # the frame list twice (the scan's two passes), 16 body bytes in and 24 record bytes out
        g = stats(ms, 2 * K * 8 * 2 + K * (16 + 24))
        S = min(1 << 12, K)
        want = T.gather_commit_shorts(buf[:S * 40].tobytes(), oth[:2 * S])
        got = (ar.get(d_m, S), ar.get(d_c, S), ar.get(d_i, S))
        ok = all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        ok = ok and int(ar.get(d_n)[0]) == K
    return {"bench": "commit", "shape": "d", "commit_shorts": K, "frames_listed": 2 * K,
            "stream_bytes": int(len(buf)), "gather_commit_shorts": g, "sample_frames": S,
            "sample_bit_exact": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "c", "d", "all"])
    ap.add_argument("--groups", type=int, default=1 << 16)
    ap.add_argument("--yardsticks", action="store_true")
    a = ap.parse_args()
    G = a.groups
    runs = {"a": [lambda: shape_a(G)],
            "b": [lambda: encode_shape("b", G * IPG, False, 0)],
            "c": [lambda: encode_shape("c", G, True, 4),
                  lambda: encode_shape("c_large", G * 64, True, 4)],
            "d": [lambda: shape_d(G * 64)]}
    rc = 0
    for s in (["a", "b", "c", "d"] if a.shape == "all" else [a.shape]):
        for fn in runs[s]:
            res = fn()
            res.update({"warmup": 3, "timed_calls": 20, "runtime": _lib.runtime_info()})
            print(json.dumps(res), flush=True)
            rc = rc or (0 if res["sample_bit_exact"] else 1)
    if a.yardsticks:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import bench_acceptor
        import bench_proposer
        print(json.dumps(bench_acceptor.run("min", G * IPG)), flush=True)
        print(json.dumps(bench_acceptor.run("classic", G * IPG)), flush=True)
        print(json.dumps(bench_proposer.run("c", G)), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())

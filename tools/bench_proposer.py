#!/usr/bin/env python3
"""Times the proposer side on device-resident buffers: mpx_propose_handle_dev and
mpx_encode_accepts_dev, 3 warm-ups, the median and range of 20 event-timed calls each.

Shapes:
  a  65,536 groups x one new instance x 4 commands, N = 5, MIN, every peer one instance behind
     (a one-instance CatchUpLog of 4 commands in every frame: 164 B frames, 4 per send)
  b  one group x 5000 commands, N = 3, MIN (two 85 KB frames)
  c  shape a in CLASSIC (83 B frames)
Algorithmic bytes: every input read once (sends, groups, peer commits, the new commands at 17 B,
the log records, offsets and commands a catch-up range covers, once per group) and every frame
byte written once; the fraction is of the 8 TB/s HBM peak. After timing, the frames of the first
64 groups are compared with the transliteration (tests/proposer_translit.py).

    python tools/bench_proposer.py [--shape a|b|c|all] [--groups G]

One JSON line per shape. Compare with `python bench.py --full --workload log` on the same box in
the same session: the catch-up log encoder does the same kind of work plus a partition.
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
from minpaxos_amd.devbuf import Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

HBM_PEAK = 8e12  # B/s, MI355X
SAMPLE = 64
IPG, USED, D = 4, 2, 32


def workload(G, n_cmds, n, seed=42):
    """G groups led by replica g % n, USED logged instances of 4 commands each, the next one
    proposed with n_cmds commands; every peer has committed all but the last logged instance"""
    rng = np.random.default_rng(seed)
    g = np.arange(G)
    first = g * IPG
    groups = np.zeros(G, R.PROPOSER_GROUP)
    groups["self_id"] = groups["leader"] = g % n
    groups["default_ballot"] = D + groups["self_id"]
    groups["prepare_oks"] = n
    groups["crt_instance"] = first + USED
    groups["committed_upto"] = first + USED - 1
    st = np.zeros(G * IPG, R.ACCEPTOR_STATE)
    st["status"] = np.where(np.arange(G * IPG) % IPG < USED, R.COMMITTED, R.STATUS_NIL)
    prop_off = (np.arange(G + 1) * n_cmds).astype(np.uint64)
    m = G * n_cmds
    cmds = (rng.integers(0, 4, m).astype(np.uint8), rng.integers(-(1 << 62), 1 << 62, m),
            rng.integers(-(1 << 62), 1 << 62, m))
    lrec = np.zeros(G * IPG, R.LOG_REC)
    lrec["status"], lrec["ballot"] = st["status"], D
    k = np.where(st["status"] == R.STATUS_NIL, 0, 4)
    lcoff = np.zeros(G * IPG + 1, np.uint64)
    lcoff[1:] = np.cumsum(k)
    lm = int(lcoff[-1])
    log = (lrec, lcoff, rng.integers(0, 4, lm).astype(np.uint8),
           rng.integers(-(1 << 62), 1 << 62, lm), rng.integers(-(1 << 62), 1 << 62, lm))
    pc = np.repeat((first + USED - 2).astype(np.int32), n).reshape(G, n)
    return groups, st, prop_off, cmds, log, pc


def timed(eng, call, warmup=3, reps=20):
    for _ in range(warmup):
        call()
    eng.synchronize()
    e0, e1 = eng.event_create(True), eng.event_create(True)
    ms = []
    for _ in range(reps):
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


def run(shape, G):
    import proposer_translit as P
    mode = R.MODE_CLASSIC if shape == "c" else R.MODE_MIN
    n = 3 if shape == "b" else 5
    G = 1 if shape == "b" else G
    n_cmds = 5000 if shape == "b" else 4
    groups, st, prop_off, cmds, log, pc = workload(G, n_cmds, n)
    frame = R.accept_frame_bytes(mode, n_cmds, [4])
    total = G * (n - 1) * frame
    with Engine(0, n, mode) as eng, Arena(eng) as ar:
        d_grp0, d_st0 = ar.put(groups), ar.put(st)
        d_grp, d_st = ar.put(groups), ar.put(st)
        d_lb = ar.full(G * IPG, R.INST_STATE, 0)
        d_poff, d_soff = ar.put(prop_off), ar.put(np.arange(G + 1, dtype=np.uint64))
        d_snd = ar.empty(G, R.ACCEPT_SEND)

        def propose():  # from the same input every time: the copies are part of the timed call
            eng.memcpy(d_grp.ptr, d_grp0.ptr, d_grp0.nbytes, 3, eng.stream)
            eng.memcpy(d_st.ptr, d_st0.ptr, d_st0.nbytes, 3, eng.stream)
            eng.propose_handle_dev(d_grp.ptr, G, d_poff.ptr, d_soff.ptr, d_st.ptr, d_lb.ptr,
                                   G * IPG, 0, IPG, d_snd.ptr, eng.stream)
        ms = timed(eng, propose)
        alg_ph = G * (32 * 2 + 16 + 16 * 2 + 16 + 32)  # group r/w, offsets, st r/w, lb, send
        ph = stats(ms, alg_ph)
        ph["note"] = "timed with two device-to-device copies that restore its input"
        sends = ar.get(d_snd)
        g2 = ar.get(d_grp)
        want = P.propose_handle(mode, n, groups[:SAMPLE], prop_off[:SAMPLE + 1], st[:SAMPLE * IPG],
                                0, IPG)
        S = min(SAMPLE, G)
        ph["sample_bit_exact"] = bool(sends[:S].tobytes() == want[3].tobytes() and
                                      g2[:S].tobytes() == want[0].tobytes())

        keep = [ar.put(x) for x in (pc, cmds[0], cmds[1], cmds[2], *log)]
        b = _lib.MpxAcceptBatch()
        b.sends, b.n_sends, b.inst_base, b.ipg, b.n_groups = d_snd.ptr, G, 0, IPG, G
        b.groups, b.peer_commits = d_grp.ptr, keep[0].ptr
        b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = keep[1].ptr, keep[2].ptr, keep[3].ptr, len(cmds[0])
        b.log_recs, b.log_cmd_off = keep[4].ptr, keep[5].ptr
        b.log_op, b.log_key, b.log_val, b.n_log_cmds = keep[6].ptr, keep[7].ptr, keep[8].ptr, len(log[2])
        b.flags, b.alive_mask = 0, 0xFFFF
        eng.encode_accepts_reserve(G, G * IPG, len(log[2]))
        d_out, d_off = ar.empty(total, np.uint8), ar.empty(n + 1, np.uint64)
        ms = timed(eng, lambda: eng.encode_accepts_dev(b, d_out.ptr, total, d_off.ptr, eng.stream))
        alg = G * (32 + 32 + 4 * n + 17 * n_cmds) + total
        if mode == R.MODE_MIN:
            alg += G * (16 + 16 + 17 * 4)  # the catch-up instance: record, two offsets, commands
        enc = stats(ms, alg)
        off = ar.get(d_off)
        sub = dict(sends=sends[:S], groups=g2[:S], cmds=cmds, inst_base=0, ipg=IPG,
                   peer_commits=pc[:S], log=tuple(x[:S * IPG + (1 if i == 1 else 0)] if i < 2 else x
                                                  for i, x in enumerate(log)))
        w_out, w_off = P.encode_accepts(mode, n, **sub)
        ok = int(off[-1]) == total
        for q in range(n):  # the sample's frames head every destination's run
            k = int(w_off[q + 1] - w_off[q])
            ok = ok and ar.get(d_out, k, int(off[q])).tobytes() == \
                w_out[int(w_off[q]):int(w_off[q + 1])].tobytes()
        enc.update({"frame_bytes": frame, "frames": G * (n - 1), "out_bytes": total,
                    "sample_groups": S, "sample_byte_exact": bool(ok)})
        del keep
    return {"bench": "proposer", "shape": shape, "mode": "classic" if shape == "c" else "min",
            "n_replicas": n, "groups": G, "cmds_per_instance": n_cmds, "warmup": 3,
            "timed_calls": 20, "propose_handle": ph, "encode_accepts": enc,
            "runtime": _lib.runtime_info()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "c", "all"])
    ap.add_argument("--groups", type=int, default=1 << 16)
    a = ap.parse_args()
    rc = 0
    for s in (["a", "b", "c"] if a.shape == "all" else [a.shape]):
        res = run(s, a.groups)
        print(json.dumps(res), flush=True)
        if not (res["propose_handle"]["sample_bit_exact"] and
                res["encode_accepts"]["sample_byte_exact"]):
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())

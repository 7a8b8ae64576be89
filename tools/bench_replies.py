#!/usr/bin/env python3
"""Times reply assembly (mpx_build_replies_dev) on device-resident buffers: 3 warm-ups, the median
and range of 20 event-timed calls, algorithmic bytes (32 B read per slot; 16 B read and 24 B written
per reply; 8 B more per reply with ret; 24 B written per pad record) over the time as a fraction of
the 5.2 TB/s copy ceiling tools/hbm_ceiling.hip measured (profiles/r01), and the
outputs checked after timing against a numpy expansion of the same inputs.

Shapes (they mirror tools/bench_client.py's):
  a   1024 slots x 2190 proposals (2.24 M replies): few full batches
  b   65,536 slots x 10 proposals: many short ones
  c   one slot x 5000: the one-launch path
Kinds: a and b run MPX_RB_DECIDED and MPX_RB_EXECUTED; b also runs DECIDED with the pad tail at
0 % and at 50 % of cap (every other slot unselected).
Yardsticks, in the same process:
  encode    mpx_encode_replies_dev on the records the call wrote: the sibling it feeds; for the
            padded runs both on the whole cap with n_clients + 1 clients (what a captured chain
            encodes) and on the replies alone: the difference is what the padding costs the encoder
  host      the path the call replaces: sends, mask, meta (and ret) copied to the host, a numpy
            gather, the records copied back; wall clock, 1 warm-up, median and range of 5

    python tools/bench_replies.py [--shape a|b|c|all] [--shrink K]

One JSON line per run. --shrink K divides the slot counts by 2^K (quick runs).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from minpaxos_amd import _lib  # noqa: E402
from minpaxos_amd import records as R  # noqa: E402
from minpaxos_amd.devbuf import D2H, H2D, Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

COPY_CEILING = 5.2e12  # B/s: tools/hbm_ceiling.hip's copy kernel on an MI355X
N = 5
N_CLIENTS = 4096


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


def stats(ms, alg=None):
    med = statistics.median(ms)
    out = {"ms_per_call": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    if alg is not None:
        out["algorithmic_bytes"] = int(alg)
        out["fraction_of_copy_ceiling"] = round(alg / (med * 1e-3) / COPY_CEILING, 5)
    return out


def expand(sends, meta, sel, ret):
    """the records of the selected slots, by numpy"""
    n = sends["n_cmds"].astype(np.int64) * sel
    j = np.repeat(sends["first_cmd"].astype(np.int64) - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + \
        np.arange(int(n.sum()))
    recs = np.zeros(len(j), R.REPLY_REC)
    recs["timestamp"], recs["command_id"] = meta["timestamp"][j], meta["command_id"][j]
    recs["client"] = meta["client"][j]
    if ret is not None:
        recs["value"] = ret[j]
    return recs


def run(shape, n_sends, per, kind, pad=None, seed=42):
    rng = np.random.default_rng(seed)
    m = n_sends * per
    sends = np.zeros(n_sends, R.ACCEPT_SEND)
    sends["instance"], sends["ballot"], sends["flags"] = np.arange(n_sends), 16, R.PH_ACCEPT
    sends["first_cmd"], sends["n_cmds"] = np.arange(n_sends, dtype=np.uint64) * per, per
    meta = np.zeros(m, R.PROPOSAL)
    meta["timestamp"] = rng.integers(0, 1 << 62, m)
    meta["command_id"] = rng.integers(-(1 << 31), 1 << 31, m)
    meta["client"] = rng.integers(0, N_CLIENTS, m)
    ret = rng.integers(-(1 << 62), 1 << 62, m) if kind == R.RB_EXECUTED else None
    sel = np.ones(n_sends, np.int64)
    if pad == 50:
        sel[1::2] = 0
    mask = sel.astype(np.uint8)
    want = expand(sends, meta, sel, ret)
    total = len(want)
    cap = m if pad is not None else total
    alg = 32 * n_sends + (40 + (8 if ret is not None else 0)) * total + 24 * (cap - total)
    res = {"bench": "replies", "shape": shape, "kind": {2: "decided", 3: "executed"}[kind],
           "slots": n_sends, "proposals_per_slot": per, "replies": total, "cap": cap,
           "pad_fraction": None if pad is None else round(1 - total / cap, 3),
           "path": "one launch" if n_sends <= R.RB_ONE_LAUNCH_SLOTS and cap <= R.RB_ONE_LAUNCH_REPLIES
           else "general"}
    with Engine(0, N, R.MODE_MIN) as eng, Arena(eng) as ar:
        d_sends, d_meta, d_mask = ar.put(sends), ar.put(meta), ar.put(mask)
        d_ret = None if ret is None else ar.put(ret)
        d_recs, d_cs, d_res = ar.empty(cap, R.REPLY_REC), ar.empty(n_sends, R.COMMIT_SEND), \
            ar.empty(1, R.REPLY_RESULT)
        b = eng.reply_batch_dev(kind, d_sends, n_sends, d_meta, m, d_mask, n_sends, 0, d_ret,
                                0 if ret is None else m, None,
                                None if pad is None else N_CLIENTS)
        eng.build_replies_reserve(n_sends)
        ms = timed(eng, lambda: eng.build_replies_dev(b, d_recs.ptr, cap, None, d_res.ptr, eng.stream))
        res["build"] = stats(ms, alg)
        ms = timed(eng, lambda: eng.build_replies_dev(b, d_recs.ptr, cap, d_cs.ptr, d_res.ptr,
                                                      eng.stream))
        res["build_with_commit_sends"] = stats(ms, alg + 32 * n_sends)
        got, r = ar.get(d_recs), ar.get(d_res)[0]
        cs = ar.get(d_cs)
        ok = (int(r["n_replies"]) == total and int(r["n_slots"]) == int(sel.sum()) and
              got[:total].tobytes() == want.tobytes() and
              np.array_equal(cs["flags"], sel.astype(np.uint32)) and
              np.array_equal(cs["first_cmd"], sends["first_cmd"]))
        if pad is not None:
            tail = got[total:]
            ok = ok and (tail["client"] == N_CLIENTS).all() and not tail["value"].any() and \
                not tail["timestamp"].any() and not tail["command_id"].any()
        # the sibling it feeds, on the records it wrote
        d_out = ar.empty(max(cap, 1) * R.PROPOSE_REPLY_BYTES, np.uint8)
        d_off = ar.empty(N_CLIENTS + 2, np.uint64)
        eng.encode_replies_reserve(cap)
        if pad is not None:
            ms = timed(eng, lambda: eng.encode_replies_dev(d_recs.ptr, cap, N_CLIENTS + 1, 1, 0,
                                                           d_out.ptr, d_off.ptr, eng.stream))
            res["encode_cap_with_pad_client"] = stats(ms)
        ms = timed(eng, lambda: eng.encode_replies_dev(d_recs.ptr, total, N_CLIENTS, 1, 0, d_out.ptr,
                                                       d_off.ptr, eng.stream))
        res["encode_replies_alone"] = stats(ms)
        # the path the call replaces
        h_sends, h_meta, h_mask = np.empty_like(sends), np.empty_like(meta), np.empty_like(mask)
        h_ret = None if ret is None else np.empty_like(ret)
        wall = []
        for i in range(6):
            t0 = time.perf_counter()
            for h, d in ((h_sends, d_sends), (h_meta, d_meta), (h_mask, d_mask), (h_ret, d_ret)):
                if h is not None:
                    eng.memcpy(h.ctypes.data_as(C.c_void_p), d.ptr, h.nbytes, D2H)
            eng.stream_synchronize(None)
            h_recs = expand(h_sends, h_meta, h_mask[h_sends["instance"]].astype(np.int64), h_ret)
            eng.memcpy(d_recs.ptr, h_recs.ctypes.data_as(C.c_void_p), h_recs.nbytes, H2D)
            eng.stream_synchronize(None)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        ok = ok and h_recs.tobytes() == want.tobytes()
        res["host_round_trip"] = dict(stats(wall), calls=len(wall), gather="numpy repeat + take")
    res["checked_against"] = "a numpy expansion of the inputs"
    res["bit_exact"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "c", "all"])
    ap.add_argument("--shrink", type=int, default=0)
    a = ap.parse_args()
    na, nb = max(1024 >> a.shrink, 1), max(65536 >> a.shrink, 2)
    runs = {"a": [lambda: run("a", na, 2190, R.RB_DECIDED), lambda: run("a", na, 2190, R.RB_EXECUTED)],
            "b": [lambda: run("b", nb, 10, R.RB_DECIDED), lambda: run("b", nb, 10, R.RB_EXECUTED),
                  lambda: run("b", nb, 10, R.RB_DECIDED, pad=0),
                  lambda: run("b", nb, 10, R.RB_DECIDED, pad=50)],
            "c": [lambda: run("c", 1, 5000, R.RB_DECIDED)]}
    rc = 0
    for s in (["a", "b", "c"] if a.shape == "all" else [a.shape]):
        for f in runs[s]:
            res = f()
            res.update({"warmup": 3, "timed_calls": 20, "runtime": _lib.runtime_info()})
            print(json.dumps(res), flush=True)
            rc = rc or (0 if res["bit_exact"] else 1)
    return rc


if __name__ == "__main__":
    sys.exit(main())

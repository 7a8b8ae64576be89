#!/usr/bin/env python3
"""Times record assembly (mpx_record_log_dev) on device-resident buffers: 3 warm-ups, the median and
range of 20 event-timed calls, algorithmic bytes (every item, effect byte and source command read
once: 16 B of record, 1 B of effect and 16 B of cmd_off per item, 17 B per recorded command; every
output byte written once) over the time as a fraction of the copy figure tools/hbm_ceiling.hip
measures (--ceiling GB/s, from the same job), and the outputs checked after timing against a numpy
rendering of the same inputs.

Shapes (MIN's format, every item recording):
  a   a replica batch: one Accept of 5000 commands (one launch)
  b   a replica batch: 5000 Accepts of one command each, general path (above the one-launch items)
  c   2^20 Accepts x 4 commands: general path
  d   2^20 CommitShorts (metadata only): general path
Yardsticks, in the same process:
  host      the path the call replaces: effects and records copied to the host, numpy picking the
            recording items and gathering their commands, mpx_encode_log(MPX_LOG_DURABLE) on them
            (host form); wall clock, 1 warm-up, median and range of 5
  encoder   mpx_encode_log_dev(MPX_LOG_DURABLE) on the same records with the commands already
            gathered: the encoder alone, without the item resolution; event-timed like the call

    python tools/bench_record.py [--shape a|b|c|d|all] [--shrink K] [--ceiling GBps]

One JSON line per run. --shrink K divides the item counts of c and d by 2^K (quick runs).
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
from minpaxos_amd.devbuf import D2H, Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

N = 5


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


def stats(ms, alg=None, ceiling=None):
    med = statistics.median(ms)
    out = {"ms_per_call": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    if alg is not None:
        out["algorithmic_bytes"] = int(alg)
        out["GBps"] = round(alg / (med * 1e-3) / 1e9, 1)
        if ceiling:
            out["fraction_of_copy_ceiling"] = round(alg / (med * 1e-3) / (ceiling * 1e9), 5)
    return out


def rendering(msgs, status, per, op, key, val):
    """the run of n records of `per` commands each, as bytes"""
    n = len(msgs)
    cmd = np.dtype([("op", "u1"), ("key", "<i8"), ("val", "<i8")])
    rec = np.dtype([("ballot", "<i4"), ("status", "<u4"), ("inst", "<i4"), ("cmds", cmd, (per,))])
    assert rec.itemsize == 12 + 17 * per
    w = np.zeros(n, rec)
    w["ballot"], w["status"], w["inst"] = msgs["ballot"], status, msgs["instance"]
    if per:
        w["cmds"]["op"], w["cmds"]["key"], w["cmds"]["val"] = (x.reshape(n, per) for x in (op, key, val))
    return w.view(np.uint8)


def run(shape, n, per, ceiling, kind, general=False, seed=42):
    rng = np.random.default_rng(seed)
    m = n * per
    short = kind == R.LR_COMMITS
    msgs = np.zeros(n, R.ACCEPT_MSG)
    msgs["instance"], msgs["ballot"] = np.arange(n) // 2, 7 + np.arange(n) % 5
    msgs["value_id"] = R.VALUE_KEEP if short else np.arange(n)
    eff = np.full(n, R.CH_INSTALLED if short else R.AH_STORED | R.AH_REPLIED, np.uint8)
    status = 3 if short else 2
    off = (np.arange(n + 1, dtype=np.uint64) * per)
    op = rng.choice([R.OP_PUT, R.OP_GET], m).astype(np.uint8)
    key, val = rng.integers(0, 1 << 20, m), rng.integers(0, 1 << 62, m)
    total = n * (12 + 17 * per)
    alg = 33 * n + 17 * m + total
    want = rendering(msgs, status, per, op, key, val)
    res = {"bench": "record", "shape": shape, "items": n, "cmds_per_item": per, "records": n, "bytes": total,
           "path": "one launch" if not general and n <= R.LR_ONE_LAUNCH_ITEMS and m <= R.LR_ONE_LAUNCH_CMDS
           else "general"}
    with Engine(0, N, R.MODE_MIN, kv_capacity=1 << 12) as eng, Arena(eng) as ar:
        d_msgs, d_eff, d_off = ar.put(msgs), ar.put(eff), ar.put(off)
        d_sop, d_skey, d_sval = (ar.put(x) if m else None for x in (op, key, val))
        d_out, d_ioff = ar.full(total, np.uint8, 0), ar.empty(n + 1, np.uint64)
        d_res = ar.empty(1, R.RECORD_RESULT)
        eng.record_log_reserve(n)
        src = [dict(cmd_off=d_off, n_frames=0 if short else n, op=d_sop, key=d_skey, val=d_sval, n_cmds=m,
                    n_recs=n)]
        b = eng.record_batch_dev(kind, R.LOG_DURABLE, d_msgs, n, src, d_eff, general=general)
        res["record"] = stats(timed(eng, lambda: eng.record_log_dev(b, d_out, total, d_ioff, d_res, eng.stream)),
                              alg, ceiling)
        r = ar.get(d_res)[0]
        ok = (int(r["n_recs"]), int(r["n_cmds"]), int(r["n_bytes"]), int(r["flags"])) == (n, m, total, 0)
        ok = ok and np.array_equal(ar.get(d_out), want)
        ok = ok and np.array_equal(ar.get(d_ioff), np.arange(n + 1, dtype=np.uint64) * (12 + 17 * per))
        # the encoder alone: the same records as mpx_log_recs, the commands already gathered
        recs = np.zeros(n, R.LOG_REC)
        recs["ballot"], recs["status"], recs["inst_no"] = msgs["ballot"], status, msgs["instance"]
        d_recs, d_roff = ar.put(recs), ar.empty(n + 1, np.uint64)
        eng.memset(d_out.ptr, 0, total, eng.stream)
        eng.encode_log_reserve(n, m)
        res["encoder_alone"] = stats(timed(eng, lambda: eng.encode_log_dev(
            R.LOG_DURABLE, d_recs.ptr, n, d_off.ptr, *(x.ptr if m else None for x in (d_sop, d_skey, d_sval)), m,
            d_out.ptr, d_roff.ptr, eng.stream)),
            32 * n + 17 * m + total, ceiling)
        ok = ok and np.array_equal(ar.get(d_out), want)
        # the path the call replaces
        h_msgs, h_eff = np.empty_like(msgs), np.empty_like(eff)
        wall = []
        for i in range(6):
            t0 = time.perf_counter()
            for h, d in ((h_msgs, d_msgs), (h_eff, d_eff)):
                eng.memcpy(h.ctypes.data_as(C.c_void_p), d.ptr, h.nbytes, D2H)
            eng.stream_synchronize(None)
            pick = np.arange(n) if short else np.flatnonzero(h_eff & R.AH_STORED)
            h_recs = np.zeros(len(pick), R.LOG_REC)
            h_recs["ballot"], h_recs["status"] = h_msgs["ballot"][pick], status
            h_recs["inst_no"] = h_msgs["instance"][pick]
            if short:
                h_off, g = np.zeros(len(pick) + 1, np.uint64), (op[:0], key[:0], val[:0])
            else:
                v = h_msgs["value_id"][pick].astype(np.int64)
                lo, k = off[v].astype(np.int64), (off[v + 1] - off[v]).astype(np.int64)
                h_off = np.concatenate([[0], np.cumsum(k)]).astype(np.uint64)
                h_src = np.repeat(lo - h_off[:-1].astype(np.int64), k) + np.arange(int(k.sum()))
                g = (op[h_src], key[h_src], val[h_src])
            h_out, _ = eng.encode_log(R.LOG_DURABLE, h_recs, h_off, *g)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        ok = ok and np.array_equal(np.frombuffer(h_out, np.uint8) if isinstance(h_out, bytes) else h_out, want)
        res["host_path"] = dict(stats(wall), calls=len(wall), loop="numpy pick + gather, mpx_encode_log")
    res["checked_against"] = "a numpy rendering of the inputs"
    res["bit_exact"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "c", "d", "all"])
    ap.add_argument("--shrink", type=int, default=0)
    ap.add_argument("--ceiling", type=float, default=0.0, help="tools/hbm_ceiling's copy figure, GB/s")
    a = ap.parse_args()
    big = max((1 << 20) >> a.shrink, 4)
    runs = {"a": lambda: run("a", 1, 5000, a.ceiling, R.LR_ACCEPTS),
            "b": lambda: run("b", 5000, 1, a.ceiling, R.LR_ACCEPTS),
            "c": lambda: run("c", big, 4, a.ceiling, R.LR_ACCEPTS),
            "d": lambda: run("d", big, 0, a.ceiling, R.LR_COMMITS)}
    rc = 0
    for s in (["a", "b", "c", "d"] if a.shape == "all" else [a.shape]):
        res = runs[s]()
        res.update({"warmup": 3, "timed_calls": 20, "copy_ceiling_GBps": a.ceiling or None,
                    "runtime": _lib.runtime_info()})
        print(json.dumps(res), flush=True)
        rc = rc or (0 if res["bit_exact"] else 1)
    return rc


if __name__ == "__main__":
    sys.exit(main())

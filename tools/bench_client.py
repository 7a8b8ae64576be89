#!/usr/bin/env python3
"""Times the client decode (mpx_decode_client_streams_dev) on device-resident buffers: 3 warm-ups,
the median and range of 20 event-timed calls, algorithmic bytes (every stream byte read once, 33 B
written per proposal, the 16 B read and 32 B written per connection) over the time as a fraction
of the 5.2 TB/s copy ceiling tools/hbm_ceiling.hip measured (profiles/r01), and the
outputs checked after timing against the arrays the streams were generated from.

Shapes:
  a   1024 connections x 64 KB of Proposes (2184 frames each): long reads from few clients
  b   65,536 connections x 10 Proposes (300 B in a 384-byte slot): many clients, short reads
Yardsticks, in the same process:
  peer      mpx_decode_peer_stream_dev on an AcceptReply-only stream of the same byte length: the
            sibling decoder
  host      the path the call replaces: the bytes copied to the host, framed there connection by
            connection (a numpy view per connection once its code bytes are seen to be PROPOSE at
            every 30th byte: the cheapest host loop there is for these streams, a general one is
            slower), and the SoA arrays copied back; wall clock, 1 warm-up, median and range of 5

    python tools/bench_client.py [--shape a|b|all] [--shrink K]

One JSON line per shape. --shrink K divides the connection counts by 2^K (quick runs).
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
FRAME = np.dtype([("code", "u1"), ("command_id", "<i4"), ("op", "u1"), ("key", "<i8"),
                  ("val", "<i8"), ("timestamp", "<i8")])
AR_FRAME = np.dtype([("code", "u1"), ("instance", "<i4"), ("ok", "u1"), ("ballot", "<i4"),
                     ("id", "<i4")])
assert FRAME.itemsize == R.CLIENT_PROPOSE_FRAME and AR_FRAME.itemsize == 14


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
            "fraction_of_copy_ceiling": round(alg / (med * 1e-3) / COPY_CEILING, 5)}


def run(name, n_conns, frames, n_groups, seed=42):
    rng = np.random.default_rng(seed)
    slot = -(-frames * FRAME.itemsize // R.CLIENT_ALIGN) * R.CLIENT_ALIGN
    n = n_conns * frames
    f = np.zeros(n, FRAME)
    f["command_id"] = rng.integers(-(1 << 31), 1 << 31, n)
    f["op"] = rng.integers(0, 6, n)
    f["key"] = rng.integers(0, 1 << 20, n)  # small keys: payload bytes that look like codes
    f["val"] = rng.integers(-(1 << 62), 1 << 62, n)
    f["timestamp"] = rng.integers(0, 1 << 62, n)
    buf = np.zeros(n_conns * slot, np.uint8)
    buf.reshape(n_conns, slot)[:, :frames * FRAME.itemsize] = \
        f.view(np.uint8).reshape(n_conns, frames * FRAME.itemsize)
    conns = np.zeros(n_conns, R.CLIENT_CONN)
    conns["offset"] = np.arange(n_conns, dtype=np.uint64) * slot
    conns["length"] = frames * FRAME.itemsize
    conns["group"] = np.arange(n_conns) * n_groups // n_conns
    alg = n_conns * frames * FRAME.itemsize + 33 * n + 48 * n_conns
    res = {"bench": "client", "shape": name, "connections": n_conns, "frames_per_connection": frames,
           "bytes": int(buf.nbytes), "proposals": n, "n_groups": n_groups}
    with Engine(0, N, R.MODE_MIN) as eng, Arena(eng) as ar:
        d_buf, d_conns = ar.put(buf), ar.put(conns)
        d_op, d_key, d_val = ar.empty(n, np.uint8), ar.empty(n, np.int64), ar.empty(n, np.int64)
        d_meta = ar.empty(n, R.PROPOSAL)
        d_po, d_so = ar.empty(n_groups + 1, np.uint64), ar.empty(n_groups + 1, np.uint64)
        d_cr, d_res = ar.empty(n_conns, R.CLIENT_CONN_RESULT), ar.empty(1, R.CLIENT_RESULT)
        out = _lib.MpxClientOut(d_op.ptr, d_key.ptr, d_val.ptr, d_meta.ptr, n, d_po.ptr, d_so.ptr)
        eng.decode_client_streams_reserve(len(buf), n_conns, n_groups)
        ms = timed(eng, lambda: eng.decode_client_streams_dev(
            d_buf.ptr, len(buf), d_conns.ptr, n_conns, n_groups, out, d_cr.ptr, d_res.ptr, eng.stream))
        res["client"] = stats(ms, alg)
        meta, cr, r = ar.get(d_meta), ar.get(d_cr), ar.get(d_res)[0]
        po = ar.get(d_po)
        first = np.searchsorted(conns["group"], np.arange(n_groups + 1)) * frames
        ok = (np.array_equal(ar.get(d_op), f["op"]) and np.array_equal(ar.get(d_key), f["key"]) and
              np.array_equal(ar.get(d_val), f["val"]) and
              np.array_equal(meta["timestamp"], f["timestamp"]) and
              np.array_equal(meta["command_id"], f["command_id"]) and
              np.array_equal(meta["client"], np.repeat(np.arange(n_conns), frames)) and
              int(r["n_proposals"]) == n and int(r["n_dropped"]) == 0 and int(r["n_partial"]) == 0 and
              np.array_equal(cr["first"], np.arange(n_conns) * frames) and
              (cr["consumed"] == frames * FRAME.itemsize).all() and
              (cr["n_proposals"] == frames).all() and (cr["stop_reason"] == R.DECODE_END).all() and
              np.array_equal(po, first.astype(np.uint64)))
        # the sibling decoder on an AcceptReply-only stream of the same byte length
        k = len(buf) // AR_FRAME.itemsize
        a = np.zeros(k, AR_FRAME)
        a["code"], a["instance"], a["ok"] = R.PEER_ACCEPT_REPLY, np.arange(k), 1
        peer = np.zeros(len(buf), np.uint8)
        peer[:k * AR_FRAME.itemsize] = a.view(np.uint8)
        peer[k * AR_FRAME.itemsize:] = 255  # unknown 1-byte frames up to the same length
        d_peer, d_ar = ar.put(peer), ar.empty(k, R.ACCEPT_REPLY)
        d_oth, d_dres = ar.empty(16, R.PEER_FRAME), ar.empty(1, R.DECODE_RESULT)
        eng.decode_reserve(len(peer))
        ms = timed(eng, lambda: eng.decode_peer_stream_dev(d_peer.ptr, len(peer), d_ar.ptr, k,
                                                           d_oth.ptr, 16, d_dres.ptr, eng.stream))
        res["peer"] = stats(ms, len(peer) + 16 * k)
        ok = ok and int(ar.get(d_dres)[0]["n_accept_replies"]) == k
        # the path the call replaces
        host = np.empty(len(buf), np.uint8)
        wall = []
        for i in range(6):
            t0 = time.perf_counter()
            eng.memcpy(host.ctypes.data_as(C.c_void_p), d_buf.ptr, host.nbytes, D2H)
            eng.stream_synchronize(None)
            parts = []
            for c in conns:
                o, ln = int(c["offset"]), int(c["length"])
                v = host[o:o + ln].view(FRAME)
                assert not v["code"].any()
                parts.append(v)
            allf = np.concatenate(parts)
            h_op, h_key = np.ascontiguousarray(allf["op"]), np.ascontiguousarray(allf["key"])
            h_val = np.ascontiguousarray(allf["val"])
            h_meta = np.zeros(n, R.PROPOSAL)
            h_meta["timestamp"], h_meta["command_id"] = allf["timestamp"], allf["command_id"]
            h_meta["client"] = np.repeat(np.arange(n_conns), frames)
            for d, h in ((d_op, h_op), (d_key, h_key), (d_val, h_val), (d_meta, h_meta)):
                eng.memcpy(d.ptr, h.ctypes.data_as(C.c_void_p), h.nbytes, H2D)
            eng.stream_synchronize(None)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        res["host_round_trip"] = {"ms_per_call": round(statistics.median(wall), 4),
                                  "ms_min": round(min(wall), 4), "ms_max": round(max(wall), 4),
                                  "calls": len(wall), "framing": "propose-only numpy view"}
    res["checked_against"] = "the generated proposals"
    res["bit_exact"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "all"])
    ap.add_argument("--shrink", type=int, default=0)
    a = ap.parse_args()
    runs = {"a": lambda: run("a", 1024 >> a.shrink, 2184, 16),
            "b": lambda: run("b", 65536 >> a.shrink, 10, 64)}
    rc = 0
    for s in (["a", "b"] if a.shape == "all" else [a.shape]):
        res = runs[s]()
        res.update({"warmup": 3, "timed_calls": 20, "runtime": _lib.runtime_info()})
        print(json.dumps(res), flush=True)
        rc = rc or (0 if res["bit_exact"] else 1)
    return rc


if __name__ == "__main__":
    sys.exit(main())

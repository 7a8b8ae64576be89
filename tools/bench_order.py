#!/usr/bin/env python3
"""Times batch assembly (mpx_order_records_dev) on device-resident buffers: 3 warm-ups, the median
and range of 20 event-timed calls, algorithmic bytes (every record read once and written once,
plus perm: 36 B per record) over the time as a fraction of the 8 TB/s HBM peak, and the outputs
checked after timing: against tests/order_translit.py where the call is small (shape b), against
numpy's stable argsort of the same key where Python's sorted() over 2^24 records would take
minutes (shapes a and c; the same stable sort, restated).

Shapes:
  a   four sources of 2^22 mpx_accept_reply each, every source ascending, n_inst = 2^22: the
      replies a 5-replica leader drains from its four peer connections
  b   one source of 5000 records in shuffled order, n_inst = 8192: one drained replica batch
      (above MPX_ORDER_ONE_LAUNCH_MAX, so the radix path whatever the flag says)
  b1  the same at 4096 records, where the one-launch kernel is eligible: timed on both paths
  c   two sources of 2^20 mpx_accept_msg each with 24-bit arrival keys (ascending per source, as
      stream offsets are), n_inst = 2^20: the Commit / CommitShort merge (64-bit keys, 44 bits)
Yardstick, in the same process: the path the call replaces, that is the records copied to the
host, numpy argsort(kind="stable") + take there, and the batch copied back (numpy's stable sort
stands in for the Go shim's sort.SliceStable); wall clock, 1 warm-up, the median and range of 5.

    python tools/bench_order.py [--shape a|b|b1|c|all] [--shrink K]

One JSON line per shape. --shrink K divides the record counts of a and c by 2^K (quick runs).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from minpaxos_amd import _lib  # noqa: E402
from minpaxos_amd import records as R  # noqa: E402
from minpaxos_amd.devbuf import D2H, H2D, Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

HBM_PEAK = 8e12  # B/s, MI355X
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


def stats(ms, alg):
    med = statistics.median(ms)
    return {"ms_per_call": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "algorithmic_bytes": int(alg),
            "fraction_of_8TBps": round(alg / (med * 1e-3) / HBM_PEAK, 5)}


def make_records(dtype, inst, rng):
    out = np.zeros(len(inst), dtype)
    w = out.view(np.uint32).reshape(len(inst), 4)
    w[:, 1:] = rng.integers(0, 1 << 32, (len(inst), 3), dtype=np.uint64).astype(np.uint32)
    out["instance"] = inst
    return out


def run(name, sources, arrivals, n_inst, bits, paths, full_translit):
    n = sum(len(s) for s in sources)
    dt = sources[0].dtype
    cat = np.concatenate(sources)
    key = cat["instance"].astype(np.uint64) << np.uint64(bits)
    if arrivals is not None:
        key |= np.concatenate(arrivals).astype(np.uint64)
    want_perm = np.argsort(key, kind="stable").astype(np.uint32)
    res = {"bench": "order", "shape": name, "records": n, "sources": len(sources),
           "n_inst": n_inst, "arrival_bits": bits, "record": "accept_reply" if dt == R.ACCEPT_REPLY
           else "accept_msg"}
    ok = True
    with Engine(0, N, R.MODE_MIN) as eng, Arena(eng) as ar:
        d_src = [ar.put(s) for s in sources]
        d_arr = [ar.put(a) for a in arrivals] if arrivals is not None else [None] * len(sources)
        srcs = [(d.ptr, a.ptr if a else None, len(s)) for d, a, s in zip(d_src, d_arr, sources)]
        d_out, d_perm = ar.empty(n, dt), ar.empty(n, np.uint32)
        d_res = ar.empty(1, R.ORDER_RESULT)
        eng.order_records_reserve(n, n_inst)
        for path in paths:
            general = path == "general"
            ms = timed(eng, lambda: eng.order_records_dev(srcs, n_inst, 0, bits, d_out.ptr,
                                                          d_perm.ptr, d_res.ptr, general=general,
                                                          stream=eng.stream))
            res[path] = stats(ms, n * 36)
            got_perm, got = ar.get(d_perm), ar.get(d_out)
            r = ar.get(d_res)[0]
            ok = ok and got_perm.tobytes() == want_perm.tobytes() and \
                got.tobytes() == cat[want_perm].tobytes() and int(r["n"]) == n and \
                int(r["n_runs"]) == len(np.unique(cat["instance"]))
            if full_translit:
                import order_translit as O
                w = O.order_records(sources, n_inst, 0, arrivals, bits)
                ok = ok and got.tobytes() == w[0].tobytes() and \
                    got_perm.tobytes() == w[1].tobytes() and r.tobytes() == w[2].tobytes()
        # the path the call replaces: D2H, a host stable sort, H2D
        host = np.empty(n, dt)
        d_cat = ar.put(cat)
        wall = []
        for i in range(6):
            t0 = time.perf_counter()
            eng.memcpy(host.ctypes.data_as(C.c_void_p), d_cat.ptr, host.nbytes, D2H)
            eng.stream_synchronize(None)
            batch = host.take(np.argsort(host["instance"], kind="stable"))
            eng.memcpy(d_out.ptr, batch.ctypes.data_as(C.c_void_p), batch.nbytes, H2D)
            eng.stream_synchronize(None)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        res["host_round_trip"] = {"ms_per_call": round(statistics.median(wall), 4),
                                  "ms_min": round(min(wall), 4), "ms_max": round(max(wall), 4),
                                  "calls": len(wall), "sorts_by": "instance only"}
    res["checked_against"] = "order_translit" if full_translit else "numpy stable argsort"
    res["bit_exact"] = bool(ok)
    return res


def shape_a(shrink, seed=42):
    rng = np.random.default_rng(seed)
    k = 1 << (22 - shrink)
    srcs = [make_records(R.ACCEPT_REPLY, np.arange(k, dtype=np.int32), rng) for _ in range(4)]
    return run("a", srcs, None, k, 0, ["auto"], False)


def shape_b(n, name, seed=42):
    rng = np.random.default_rng(seed)
    inst = rng.permutation(8192)[:n].astype(np.int32)
    inst[1::7] = inst[0::7][:len(inst[1::7])]  # some instances twice
    srcs = [make_records(R.ACCEPT_REPLY, inst, rng)]
    return run(name, srcs, None, 8192, 0, ["auto", "general"], True)


def shape_c(shrink, seed=42):
    rng = np.random.default_rng(seed)
    k = 1 << (20 - shrink)
    srcs = [make_records(R.ACCEPT_MSG, rng.integers(0, k, k).astype(np.int32), rng) for _ in range(2)]
    arrs = [np.sort(rng.integers(0, 1 << 24, k)).astype(np.uint32) for _ in range(2)]
    return run("c", srcs, arrs, k, 24, ["auto"], False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "b1", "c", "all"])
    ap.add_argument("--shrink", type=int, default=0)
    a = ap.parse_args()
    runs = {"a": lambda: shape_a(a.shrink), "b": lambda: shape_b(5000, "b"),
            "b1": lambda: shape_b(R.ORDER_ONE_LAUNCH_MAX, "b1"), "c": lambda: shape_c(a.shrink)}
    rc = 0
    for s in (["a", "b", "b1", "c"] if a.shape == "all" else [a.shape]):
        res = runs[s]()
        res.update({"warmup": 3, "timed_calls": 20, "runtime": _lib.runtime_info()})
        print(json.dumps(res), flush=True)
        rc = rc or (0 if res["bit_exact"] else 1)
    return rc


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times store assembly (mpx_store_commands_dev, mpx_store_compact_dev) on device-resident buffers:
3 warm-ups, the median and range of 20 event-timed calls (the append cursor is put back before
every call, outside the timed pair), algorithmic bytes (per item 16 B of record, 1 B of effect and
16 B of cmd_off read; per stored command 17 B read and 17 B written; per winner 16 B of
mpx_inst_cmds written; a compaction reads and writes 16 B per window slot besides) over the time as
a fraction of the copy figure tools/hbm_ceiling.hip measures (--ceiling GB/s, from the same job),
and the outputs checked after timing against a numpy rendering of the same inputs.

Shapes:
  a   a replica batch: one Accept of 5000 commands (one launch)
  b   a replica batch: 5000 Accepts of one command each, general path (above the one-launch items)
  c   2^20 items x 4 commands, every fourth superseded by the next: general path
  d   compaction of 2^20 slots x 4 commands with a quarter retired
Yardstick, in the same process:
  host      the path the call replaces: effects and records copied to the host, numpy picking the
            winners and taking their commands into the host's arrays, the appended
            commands and the window's slots copied back; wall clock, 1 warm-up, median and range of 5

    python tools/bench_store.py [--shape a|b|c|d|all] [--shrink K] [--ceiling GBps]

One JSON line per run. --shrink K divides the item or slot counts of c and d by 2^K (quick runs).
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

N = 5


def timed(eng, pre, call, warmup=3, reps=20):
    for _ in range(warmup):
        pre()
        call()
    eng.synchronize()
    e0, e1 = eng.event_create(True), eng.event_create(True)
    ms = []
    for _ in range(reps):
        pre()
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


def winners(instance, stores):
    """the storing items that no later storing item of their instance follows"""
    idx = np.flatnonzero(stores)
    nxt = np.append(instance[idx][1:], np.int64(-1 << 40))
    return idx[instance[idx] != nxt]


def run_store(shape, n, per, ceiling, general=False, supersede=False, seed=42):
    rng = np.random.default_rng(seed)
    m = n * per
    instance = np.arange(n, dtype=np.int64)
    if supersede:
        instance -= (np.arange(n) % 4 == 1)          # item 4k + 1 repeats instance 4k: 4k loses
    n_inst = int(instance.max()) + 1
    msgs = np.zeros(n, R.ACCEPT_MSG)
    msgs["instance"], msgs["ballot"], msgs["value_id"] = instance, 7, np.arange(n)
    eff = np.full(n, R.AH_STORED | R.AH_REPLIED, np.uint8)
    off = (np.arange(n + 1, dtype=np.uint64) * per)
    op = rng.choice([R.OP_PUT, R.OP_GET], m).astype(np.uint8)
    key, val = rng.integers(0, 1 << 20, m), rng.integers(0, 1 << 62, m)
    used0 = 5
    win = winners(instance, eff != 0)
    total = len(win) * per
    cap = used0 + total + 3
    alg = 33 * n + 34 * total + 16 * len(win)
    res = {"bench": "store", "shape": shape, "items": n, "cmds_per_item": per, "winners": int(len(win)),
           "commands": total, "window_slots": n_inst,
           "path": "one launch" if not general and n <= R.SC_ONE_LAUNCH_ITEMS and m <= R.SC_ONE_LAUNCH_CMDS
           else "general"}
    with Engine(0, N, R.MODE_MIN, kv_capacity=1 << 12) as eng, Arena(eng) as ar:
        d_msgs, d_eff, d_off = ar.put(msgs), ar.put(eff), ar.put(off)
        d_sop, d_skey, d_sval = ar.put(op), ar.put(key), ar.put(val)
        d_op, d_key, d_val = ar.full(cap, np.uint8, 0), ar.full(cap, np.int64, 0), ar.full(cap, np.int64, 0)
        d_inst = ar.full(n_inst, R.INST_CMDS, 0)
        d_used, d_used0 = ar.empty(1, np.uint64), ar.put(np.array([used0], np.uint64))
        d_res = ar.empty(1, R.STORE_RESULT)
        eng.store_commands_reserve(n)
        b = eng.store_batch_dev(R.SC_MSGS, d_msgs, n, [dict(cmd_off=d_off, n_frames=n, op=d_sop, key=d_skey,
                                                            val=d_sval, n_cmds=m, n_recs=n)],
                                n_inst, 0, d_eff, general=general)
        a = eng.store_arena_dev(d_op, d_key, d_val, cap, d_used)
        pre = lambda: eng.memcpy(d_used.ptr, d_used0.ptr, 8, 3, eng.stream)  # noqa: E731 (D2D)
        res["store"] = stats(timed(eng, pre, lambda: eng.store_commands_dev(b, a, d_inst, d_res, eng.stream)),
                             alg, ceiling)
        r = ar.get(d_res)[0]
        src = (win[:, None] * per + np.arange(per)[None, :]).reshape(-1)
        ok = (int(r["n_stored"]), int(r["n_cmds"]), int(r["n_superseded"]), int(r["flags"])) == \
            (len(win), total, n - len(win), 0)
        ok = ok and int(ar.get(d_used)[0]) == used0 + total
        ok = ok and np.array_equal(ar.get(d_op, total, used0), op[src])
        ok = ok and np.array_equal(ar.get(d_key, total, used0), key[src])
        ok = ok and np.array_equal(ar.get(d_val, total, used0), val[src])
        w_inst = np.zeros(n_inst, R.INST_CMDS)
        w_inst["first_cmd"][instance[win]] = used0 + np.arange(len(win)) * per
        w_inst["n_cmds"][instance[win]], w_inst["flags"][instance[win]] = per, R.IC_HAS_CMDS
        ok = ok and ar.get(d_inst).tobytes() == w_inst.tobytes()
        # the path the call replaces (the shim keeps the commands on the host)
        h_msgs, h_eff = np.empty_like(msgs), np.empty_like(eff)
        h_op, h_key, h_val = np.zeros(cap, np.uint8), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        h_inst = np.zeros(n_inst, R.INST_CMDS)
        wall = []
        for i in range(6):
            t0 = time.perf_counter()
            for h, d in ((h_msgs, d_msgs), (h_eff, d_eff)):
                eng.memcpy(h.ctypes.data_as(C.c_void_p), d.ptr, h.nbytes, D2H)
            eng.stream_synchronize(None)
            stores = (h_eff & R.AH_STORED) != 0
            hw = winners(h_msgs["instance"].astype(np.int64), stores)
            v = h_msgs["value_id"][hw].astype(np.int64)
            lo, k = off[v].astype(np.int64), (off[v + 1] - off[v]).astype(np.int64)
            new = used0 + np.concatenate([[0], np.cumsum(k)[:-1]])
            h_src = np.repeat(lo - (new - used0), k) + np.arange(int(k.sum()))
            at = used0 + len(h_src)
            h_op[used0:at], h_key[used0:at], h_val[used0:at] = op[h_src], key[h_src], val[h_src]
            rel = h_msgs["instance"][hw]
            h_inst["first_cmd"][rel], h_inst["n_cmds"][rel], h_inst["flags"][rel] = new, k, R.IC_HAS_CMDS
            for h, d in ((h_op, d_op), (h_key, d_key), (h_val, d_val), (h_inst, d_inst)):
                eng.memcpy(d.ptr, h.ctypes.data_as(C.c_void_p), h.nbytes, H2D)
            eng.stream_synchronize(None)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        ok = ok and h_inst.tobytes() == w_inst.tobytes() and np.array_equal(h_key[used0:at], key[src])
        res["host_round_trip"] = dict(stats(wall), calls=len(wall), loop="numpy winners + take")
    res["checked_against"] = "a numpy rendering of the inputs"
    res["bit_exact"] = bool(ok)
    return res


def run_compact(shape, n, per, ceiling, seed=43):
    rng = np.random.default_rng(seed)
    used = n * per + 7
    inst = np.zeros(n, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"] = 7 + rng.permutation(n).astype(np.uint64) * per, per
    inst["flags"] = np.where(np.arange(n) % 4 == 2, 0, R.IC_HAS_CMDS)       # a quarter retired
    op = rng.choice([R.OP_PUT, R.OP_GET], used).astype(np.uint8)
    key, val = rng.integers(0, 1 << 20, used), rng.integers(0, 1 << 62, used)
    keep = np.flatnonzero(inst["flags"])
    total = len(keep) * per
    alg = 32 * n + 34 * total
    res = {"bench": "store_compact", "shape": shape, "window_slots": n, "cmds_per_slot": per,
           "kept": int(len(keep)), "commands": total, "path": "general"}
    with Engine(0, N, R.MODE_MIN, kv_capacity=1 << 12) as eng, Arena(eng) as ar:
        d_inst, d_inst0 = ar.empty(n, R.INST_CMDS), ar.put(inst)
        f = eng.store_arena_dev(ar.put(op), ar.put(key), ar.put(val), used, ar.put(np.array([used], np.uint64)))
        d_op, d_key, d_val = ar.full(total, np.uint8, 0), ar.full(total, np.int64, 0), ar.full(total, np.int64, 0)
        d_used, d_res = ar.empty(1, np.uint64), ar.empty(1, R.STORE_RESULT)
        t = eng.store_arena_dev(d_op, d_key, d_val, total, d_used)
        eng.store_compact_reserve(n)
        pre = lambda: eng.memcpy(d_inst.ptr, d_inst0.ptr, inst.nbytes, 3, eng.stream)  # noqa: E731
        res["compact"] = stats(timed(eng, pre, lambda: eng.store_compact_dev(d_inst, n, f, t, d_res, eng.stream)),
                               alg, ceiling)
        r = ar.get(d_res)[0]
        src = (inst["first_cmd"][keep].astype(np.int64)[:, None] + np.arange(per)[None, :]).reshape(-1)
        ok = (int(r["n_stored"]), int(r["n_cmds"]), int(r["flags"])) == (len(keep), total, 0)
        ok = ok and int(ar.get(d_used)[0]) == total and np.array_equal(ar.get(d_key), key[src])
        ok = ok and np.array_equal(ar.get(d_op), op[src]) and np.array_equal(ar.get(d_val), val[src])
        w_inst = inst.copy()
        w_inst["first_cmd"][keep] = np.arange(len(keep)) * per
        ok = ok and ar.get(d_inst).tobytes() == w_inst.tobytes()
        # the path the call replaces: the window to the host, a numpy take, the arena and window back
        h_inst = np.empty_like(inst)
        wall = []
        for i in range(6):
            t0 = time.perf_counter()
            eng.memcpy(h_inst.ctypes.data_as(C.c_void_p), d_inst0.ptr, h_inst.nbytes, D2H)
            eng.stream_synchronize(None)
            hk = np.flatnonzero(h_inst["flags"] & R.IC_HAS_CMDS)
            k = h_inst["n_cmds"].astype(np.int64)[hk]
            first = h_inst["first_cmd"].astype(np.int64)[hk]
            new = np.concatenate([[0], np.cumsum(k)[:-1]])
            h_src = np.repeat(first - new, k) + np.arange(int(k.sum()))
            h_cmds = (op[h_src], key[h_src], val[h_src])
            h_inst["first_cmd"][hk] = new
            for h, d in zip(h_cmds + (h_inst,), (d_op, d_key, d_val, d_inst)):
                eng.memcpy(d.ptr, h.ctypes.data_as(C.c_void_p), h.nbytes, H2D)
            eng.stream_synchronize(None)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        ok = ok and np.array_equal(h_src, src) and h_inst.tobytes() == w_inst.tobytes()
        res["host_round_trip"] = dict(stats(wall), calls=len(wall), loop="numpy take")
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
    runs = {"a": lambda: run_store("a", 1, 5000, a.ceiling),
            "b": lambda: run_store("b", 5000, 1, a.ceiling),
            "c": lambda: run_store("c", big, 4, a.ceiling, supersede=True),
            "d": lambda: run_compact("d", big, 4, a.ceiling)}
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

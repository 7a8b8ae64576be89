#!/usr/bin/env python3
"""Times execute assembly (mpx_execute_gather_dev) on device-resident buffers: 3 warm-ups, the
median and range of 20 event-timed calls, algorithmic bytes (16 B read and 1 + 8 B written per
window slot: mpx_inst_cmds, mask, inst_first; 17 B read and 17 B written per gathered command; 17 B
written per pad command) over the time as a fraction of the 5.2 TB/s copy ceiling
tools/hbm_ceiling.hip measured (profiles/r01), and the outputs checked after timing
against a numpy walk of the same inputs.

Shapes:
  a   one group x 2^20 slots x 4 commands, the whole window executing: one replica's log
  b   65,536 groups x 256 slots x 4 commands, about half of each window executing, a nil slot in
      every fourth walk: the sharded engine
  c   one group x one instance of 5000 commands: the one-launch path
Yardsticks, in the same process:
  host      the path the call replaces: inst and the cursors copied to the host, a numpy walk and
            take on the host's command arrays, the gathered commands and the mask copied back;
            wall clock, 1 warm-up, median and range of 5
  apply     (a, c) mpx_apply_dev over the gathered commands with the exact m, and over cap = 2 x
            total with the pad tail (what a captured chain applies): the difference is what the
            padding costs the apply

    python tools/bench_execute.py [--shape a|b|c|all] [--shrink K]

One JSON line per run. --shrink K divides the slot or group counts by 2^K (quick runs).
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


def walk(inst, cu, ex, ipg):
    """executeCommands' walk by numpy (inst_base 0): (mask, executed_out, source index of every
    gathered command)"""
    n, G = len(inst), len(cu)
    idx = np.arange(n, dtype=np.int64)
    g = idx // ipg
    in_range = (idx > ex[g]) & (idx <= cu[g])
    bad = in_range & ((inst["flags"] & R.IC_HAS_CMDS) == 0)
    stop = np.where(bad, idx, n).reshape(G, ipg).min(axis=1)
    mask = in_range & (idx < stop[g])
    out = np.where(ex >= cu, ex, np.where(stop < n, stop - 1, cu)).astype(np.int32)
    k = inst["n_cmds"].astype(np.int64)[mask]
    first = inst["first_cmd"].astype(np.int64)[mask]
    src = np.repeat(first - np.concatenate([[0], np.cumsum(k)[:-1]]), k) + np.arange(int(k.sum()))
    return mask.astype(np.uint8), out, src


def run(shape, G, ipg, per, seed=42, apply_too=False):
    rng = np.random.default_rng(seed)
    n = G * ipg
    m = n * per
    inst = np.zeros(n, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"] = np.arange(n, dtype=np.uint64) * per, per
    inst["flags"] = R.IC_HAS_CMDS
    first = np.arange(G, dtype=np.int64) * ipg
    if shape == "b":
        ex = first - 1 + rng.integers(0, ipg // 4 + 1, G)
        cu = ex + ipg // 2 + rng.integers(-ipg // 8, ipg // 8 + 1, G)
        nil = rng.random(G) < 0.25
        at = (ex + 1 + rng.integers(0, np.maximum(cu - ex, 1)))[nil]
        inst["flags"][at] = 0
    else:
        ex, cu = first - 1, first + ipg - 1
    ex, cu = ex.astype(np.int32), cu.astype(np.int32)
    op = rng.choice([R.OP_PUT, R.OP_GET], m).astype(np.uint8)
    key, val = rng.integers(0, 1 << 20, m), rng.integers(0, 1 << 62, m)
    w_mask, w_ex, src = walk(inst, cu, ex, ipg)
    total = len(src)
    alg = (16 + 1 + 8) * n + 34 * total
    res = {"bench": "execute", "shape": shape, "groups": G, "ipg": ipg, "cmds_per_instance": per,
           "slots": n, "executed": int(w_mask.sum()), "commands": total,
           "path": "one launch" if n <= R.XG_ONE_LAUNCH_INST and total <= R.XG_ONE_LAUNCH_CMDS
           else "general"}
    with Engine(0, N, R.MODE_MIN, kv_capacity=1 << 22) as eng, Arena(eng) as ar:
        d_inst, d_cu, d_ex = ar.put(inst), ar.put(cu), ar.put(ex)
        d_sop, d_skey, d_sval = ar.put(op), ar.put(key), ar.put(val)
        cap = 2 * total
        d_op, d_key, d_val = ar.empty(cap, np.uint8), ar.empty(cap, np.int64), ar.empty(cap, np.int64)
        d_mask, d_if, d_exo = ar.empty(n, np.uint8), ar.empty(n, np.uint64), ar.empty(G, np.int32)
        d_go, d_res = ar.empty(G + 1, np.uint64), ar.empty(1, R.EXECUTE_RESULT)
        eng.execute_gather_reserve(n, G)

        def call(cap, pad):
            b = eng.execute_batch_dev(d_inst, n, 0, ipg, G, d_cu, d_ex, d_exo, d_sop, d_skey, d_sval, m,
                                      pad=pad)
            o = eng.execute_out_dev(d_op, d_key, d_val, cap, d_mask, d_if, None, d_go)
            return lambda: eng.execute_gather_dev(b, o, d_res.ptr, eng.stream)
        res["gather_padded_to_2x"] = stats(timed(eng, call(cap, True)), alg + 17 * (cap - total))
        tail = (ar.get(d_op, cap - total, total), ar.get(d_key, cap - total, total),
                ar.get(d_val, cap - total, total))
        ok = not tail[0].any() and not tail[2].any() and \
            np.array_equal(tail[1], np.arange(total, cap))
        res["gather"] = stats(timed(eng, call(total, False)), alg)
        r = ar.get(d_res)[0]
        ok = ok and (int(r["n_cmds"]), int(r["n_inst"])) == (total, int(w_mask.sum()))
        ok = ok and int(r["n_groups"]) == int((w_ex != ex).sum())
        ok = ok and np.array_equal(ar.get(d_mask), w_mask) and np.array_equal(ar.get(d_exo), w_ex)
        ok = ok and np.array_equal(ar.get(d_op, total), op[src])
        ok = ok and np.array_equal(ar.get(d_key, total), key[src])
        ok = ok and np.array_equal(ar.get(d_val, total), val[src])
        lens = np.where(w_mask, inst["n_cmds"], 0).astype(np.uint64)
        ok = ok and np.array_equal(ar.get(d_if), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64))
        ok = ok and np.array_equal(ar.get(d_go)[:-1], ar.get(d_if)[::ipg])
        if apply_too:
            d_ret = ar.empty(cap, np.int64)
            eng.apply_reserve(cap)
            call(cap, True)()
            ms = timed(eng, lambda: eng.apply_dev(d_op.ptr, d_key.ptr, d_val.ptr, total, d_ret.ptr, None,
                                                  eng.stream))
            res["apply_exact_m"] = stats(ms)
            ms = timed(eng, lambda: eng.apply_dev(d_op.ptr, d_key.ptr, d_val.ptr, cap, d_ret.ptr, None,
                                                  eng.stream))
            res["apply_cap_with_pad"] = stats(ms)
            ok = ok and not ar.get(d_ret, cap - total, total).any()   # NONE returns NIL
        # the path the call replaces (the shim keeps the commands on the host)
        h_inst, h_cu, h_ex = np.empty_like(inst), np.empty_like(cu), np.empty_like(ex)
        wall = []
        for i in range(6):
            t0 = time.perf_counter()
            for h, d in ((h_inst, d_inst), (h_cu, d_cu), (h_ex, d_ex)):
                eng.memcpy(h.ctypes.data_as(C.c_void_p), d.ptr, h.nbytes, D2H)
            eng.stream_synchronize(None)
            h_mask, h_exo, h_src = walk(h_inst, h_cu, h_ex, ipg)
            h_cmds = (op[h_src], key[h_src], val[h_src])
            for h, d in zip(h_cmds + (h_mask,), (d_op, d_key, d_val, d_mask)):
                eng.memcpy(d.ptr, h.ctypes.data_as(C.c_void_p), h.nbytes, H2D)
            eng.stream_synchronize(None)
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
        ok = ok and np.array_equal(h_src, src)
        res["host_round_trip"] = dict(stats(wall), calls=len(wall), gather="numpy walk + take")
    res["checked_against"] = "a numpy walk of the inputs"
    res["bit_exact"] = bool(ok)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "c", "all"])
    ap.add_argument("--shrink", type=int, default=0)
    a = ap.parse_args()
    runs = {"a": lambda: run("a", 1, max((1 << 20) >> a.shrink, 1), 4, apply_too=True),
            "b": lambda: run("b", max(65536 >> a.shrink, 1), 256, 4),
            "c": lambda: run("c", 1, 1, 5000, apply_too=True)}
    rc = 0
    for s in (["a", "b", "c"] if a.shape == "all" else [a.shape]):
        res = runs[s]()
        res.update({"warmup": 3, "timed_calls": 20, "runtime": _lib.runtime_info()})
        print(json.dumps(res), flush=True)
        rc = rc or (0 if res["bit_exact"] else 1)
    return rc


if __name__ == "__main__":
    sys.exit(main())

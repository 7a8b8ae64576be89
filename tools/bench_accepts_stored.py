#!/usr/bin/env python3
"""Times mpx_encode_accepts_stored_dev (the Accept frames with the catch-up log read from the
instance store) on device-resident buffers, over the three shapes of tools/bench_proposer.py:
3 warm-ups, the median and range of 20 event-timed calls. In the same run, on the same frames:

  stored     mpx_encode_accepts_stored_dev: st / lb / mpx_inst_cmds and the command arena
  dense      mpx_encode_accepts_dev with the dense window-ordered log already built (the
             encoder alone: the yardstick)
  replaced   wall clock of the path the stored form replaces: D2H of st, inst and the touched
             commands, the numpy build of the dense arrays, then the host form mpx_encode_accepts
             (its H2D, the encode, the bytes back); median of 5

The arena is laid out as mpx_store_commands leaves it after the preceding turns: turn t's
instances of all groups back to back in batch order, so the two logged instances of one group
lie 4 G commands apart and nothing is in window order. After timing, the stored form's bytes are
compared with the dense form's, whole, and the first 64 groups' frames with the transliteration.

    python tools/bench_accepts_stored.py [--shape a|b|c|all] [--groups G]

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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_proposer as BP  # noqa: E402
from minpaxos_amd import _lib  # noqa: E402
from minpaxos_amd import records as R  # noqa: E402
from minpaxos_amd.devbuf import Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

IPG, USED, D = BP.IPG, BP.USED, BP.D
SAMPLE = BP.SAMPLE


def store_of(G, st, log):
    """the dense log of BP.workload as the store USED turns of mpx_store_commands(SENDS) leave:
    inst[g * IPG + t] = {t * 4 G + 4 g, 4, HAS_CMDS}"""
    lrec, lcoff, lop, lkey, lval = log
    inst = np.zeros(G * IPG, R.INST_CMDS)
    g, t = np.divmod(np.arange(G * IPG), IPG)
    used = t < USED
    inst["first_cmd"][used] = (t[used] * 4 * G + 4 * g[used])
    inst["n_cmds"][used] = 4
    inst["flags"][used] = R.IC_HAS_CMDS
    n = USED * 4 * G
    at = np.zeros(n, np.int64)  # arena position -> dense log position
    w = np.flatnonzero(used)
    for j in range(4):
        at[inst["first_cmd"][w].astype(np.int64) + j] = lcoff[w].astype(np.int64) + j
    return inst, (lop[at], lkey[at], lval[at])


def rng_stats(ms):
    return {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4)}


def run(shape, G):
    import proposer_translit as P
    mode = R.MODE_CLASSIC if shape == "c" else R.MODE_MIN
    n = 3 if shape == "b" else 5
    G = 1 if shape == "b" else G
    n_cmds = 5000 if shape == "b" else 4
    groups, st, prop_off, cmds, log, pc = BP.workload(G, n_cmds, n)
    st["ballot"][st["status"] != R.STATUS_NIL] = D  # the logged instances' ballot, as log_recs has it
    frame = R.accept_frame_bytes(mode, n_cmds, [4])
    total = G * (n - 1) * frame
    inst, arena = store_of(G, st, log)
    with Engine(0, n, mode) as eng, Arena(eng) as ar:
        groups2, st2, lb, sends, _ = eng.propose_handle(groups, prop_off, st, 0, IPG,
                                                        np.full(G * IPG, R.STATUS_NIL, R.INST_STATE))
        lb["status"][st["status"] == R.COMMITTED] = R.COMMITTED  # what the tally left
        d = {k: ar.put(v) for k, v in dict(
            sends=sends, groups=groups2, pc=pc, op=cmds[0], key=cmds[1], val=cmds[2], st=st2, lb=lb,
            inst=inst, sop=arena[0], skey=arena[1], sval=arena[2], lrec=log[0], lcoff=log[1],
            lop=log[2], lkey=log[3], lval=log[4]).items()}
        sb = _lib.MpxAcceptStoreBatch()
        db = _lib.MpxAcceptBatch()
        for b in (sb, db):
            b.sends, b.n_sends, b.inst_base, b.ipg, b.n_groups = d["sends"].ptr, G, 0, IPG, G
            b.groups, b.peer_commits = d["groups"].ptr, d["pc"].ptr
            b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = d["op"].ptr, d["key"].ptr, d["val"].ptr, len(cmds[0])
            b.flags, b.alive_mask = 0, 0xFFFF
        sb.st, sb.lb, sb.inst = d["st"].ptr, d["lb"].ptr, d["inst"].ptr
        sb.src_op, sb.src_key, sb.src_val, sb.n_src = d["sop"].ptr, d["skey"].ptr, d["sval"].ptr, len(arena[0])
        db.log_recs, db.log_cmd_off = d["lrec"].ptr, d["lcoff"].ptr
        db.log_op, db.log_key, db.log_val, db.n_log_cmds = d["lop"].ptr, d["lkey"].ptr, d["lval"].ptr, len(log[2])
        eng.encode_accepts_stored_reserve(G, G * IPG)
        d_out, d_off = ar.empty(total, np.uint8), ar.empty(n + 1, np.uint64)
        d_out2, d_off2 = ar.empty(total, np.uint8), ar.empty(n + 1, np.uint64)
        stored = rng_stats(BP.timed(eng, lambda: eng.encode_accepts_stored_dev(
            sb, d_out.ptr, total, d_off.ptr, eng.stream)))
        dense = rng_stats(BP.timed(eng, lambda: eng.encode_accepts_dev(
            db, d_out2.ptr, total, d_off2.ptr, eng.stream)))
        # a second round of each, so that neither has the warmer box
        stored_again = rng_stats(BP.timed(eng, lambda: eng.encode_accepts_stored_dev(
            sb, d_out.ptr, total, d_off.ptr, eng.stream)))
        dense_again = rng_stats(BP.timed(eng, lambda: eng.encode_accepts_dev(
            db, d_out2.ptr, total, d_off2.ptr, eng.stream)))

        # the replaced path: every peer is one instance behind, so the touched slots are the last
        # logged instance of every group and their commands the arena's last turn
        t_lo = (USED - 1) * 4 * G
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            h_st, h_lb, h_inst = ar.get(d["st"]), ar.get(d["lb"]), ar.get(d["inst"])
            h_op = ar.get(d["sop"], len(arena[0]) - t_lo, t_lo)
            h_key = ar.get(d["skey"], len(arena[0]) - t_lo, t_lo)
            h_val = ar.get(d["sval"], len(arena[0]) - t_lo, t_lo)
            touched = np.arange(G) * IPG + USED - 1
            lrec = np.zeros(G * IPG, R.LOG_REC)
            lrec["status"] = R.STATUS_NIL
            lrec["ballot"][touched] = h_st["ballot"][touched]
            ls = h_lb["status"][touched]
            lrec["status"][touched] = np.where(ls != R.STATUS_NIL, ls, h_st["status"][touched])
            k = np.zeros(G * IPG, np.int64)
            k[touched] = h_inst["n_cmds"][touched]
            lcoff = np.zeros(G * IPG + 1, np.uint64)
            lcoff[1:] = np.cumsum(k)
            at = (h_inst["first_cmd"][touched].astype(np.int64)[:, None] - t_lo + np.arange(4)).reshape(-1)
            r_out, r_off = eng.encode_accepts(sends, groups2, cmds, 0, IPG, pc,
                                              (lrec, lcoff, h_op[at], h_key[at], h_val[at]),
                                              out_cap=total)
            wall.append((time.perf_counter() - t0) * 1e3)
        replaced = rng_stats(wall)

        off, off2 = ar.get(d_off), ar.get(d_off2)
        got, got2 = ar.get(d_out), ar.get(d_out2)
        S = min(SAMPLE, G)
        sub = dict(sends=sends[:S], groups=groups2[:S], cmds=cmds, inst_base=0, ipg=IPG,
                   peer_commits=pc[:S], log=tuple(x[:S * IPG + (1 if i == 1 else 0)] if i < 2 else x
                                                  for i, x in enumerate(log)))
        if mode == R.MODE_MIN:  # the sample's Status as the lb rule gives it
            sub["log"][0]["status"][st[:S * IPG]["status"] == R.COMMITTED] = R.COMMITTED
        w_out, w_off = P.encode_accepts(mode, n, **sub)
        ok = int(off[-1]) == total
        for q in range(n):  # the sample's frames head every destination's run
            kq = int(w_off[q + 1] - w_off[q])
            ok = ok and got[int(off[q]):int(off[q]) + kq].tobytes() == \
                w_out[int(w_off[q]):int(w_off[q + 1])].tobytes()
        same = bool(np.array_equal(off, off2) and got.tobytes() == got2.tobytes() and
                    r_out.tobytes() == got.tobytes() and np.array_equal(r_off, off))
    return {"bench": "accepts_stored", "shape": shape, "mode": "classic" if shape == "c" else "min",
            "n_replicas": n, "groups": G, "cmds_per_instance": n_cmds, "warmup": 3, "timed_calls": 20,
            "frame_bytes": frame, "frames": G * (n - 1), "out_bytes": total,
            "stored_dev": stored, "dense_dev": dense, "stored_dev_again": stored_again,
            "dense_dev_again": dense_again, "replaced_path_wall": replaced,
            "stored_equals_dense_and_replaced": same, "sample_groups": S,
            "sample_byte_exact": bool(ok), "runtime": _lib.runtime_info()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "c", "all"])
    ap.add_argument("--groups", type=int, default=1 << 16)
    a = ap.parse_args()
    rc = 0
    for s in (["a", "b", "c"] if a.shape == "all" else [a.shape]):
        res = run(s, a.groups)
        print(json.dumps(res), flush=True)
        if not (res["stored_equals_dense_and_replaced"] and res["sample_byte_exact"]):
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Times mpx_unmarshal_frames_dev on device-resident buffers: 3 warm-ups, the median and range of
20 event-timed calls.

Shapes, the three of tools/bench_proposer.py taken from the receiving side (the bytes are what
mpx_encode_accepts wrote for one destination, the frames what mpx_decode_stream found in them):
  a  65,536 Accepts of 4 commands, MIN, each one instance behind (a one-instance CatchUpLog of 4
     commands in every frame: 164 B frames)
  b  one 85 KB Accept of 5000 commands, MIN
  c  shape a in CLASSIC (83 B frames)
Algorithmic bytes: every frame byte and frame record read once, every output byte written once
(records, offsets, 17 B per command); the fraction is of the 8 TB/s HBM peak. After timing, the
outputs of the first 64 frames are compared with the transliteration (tests/unmarshal_translit.py).

    python tools/bench_unmarshal.py [--shape a|b|c|all] [--groups G]

One JSON line per shape. Compare with `python tools/bench_proposer.py` (mpx_encode_accepts_dev on
the matching shape) and `python bench.py --full --workload log` on the same box in the same session.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_proposer import IPG, stats, timed, workload  # noqa: E402
from minpaxos_amd import _lib  # noqa: E402
from minpaxos_amd import records as R  # noqa: E402
from minpaxos_amd.devbuf import Arena  # noqa: E402
from minpaxos_amd.engine import Engine  # noqa: E402

SAMPLE = 64
DTYPES = {"accepts": R.ACCEPT_MSG, "accept_last_committed": np.int32, "commits": R.ACCEPT_MSG,
          "cmd_off": np.uint64, "op": np.uint8, "key": np.int64, "val": np.int64,
          "log_inst_off": np.uint64, "log_recs": R.LOG_REC, "log_cmd_off": np.uint64,
          "log_op": np.uint8, "log_key": np.int64, "log_val": np.int64}


def received(eng, shape, G, n):
    """the run replica 1 receives from G groups led by replica 0, and its frames"""
    n_cmds = 5000 if shape == "b" else 4
    groups, st, prop_off, cmds, log, pc = workload(G, n_cmds, n)
    groups["self_id"] = groups["leader"] = 0
    groups["default_ballot"] = 32
    g2, _, _, sends, _ = eng.propose_handle(groups, prop_off, st, 0, IPG)
    out, off = eng.encode_accepts(sends, g2, cmds, 0, IPG, pc, log)
    run = np.ascontiguousarray(out[int(off[1]):int(off[2])])
    _, _, var, _, res = eng.decode_stream(run)
    assert int(res["stop_reason"]) == R.DECODE_END and len(var) == G
    return run, var


def run(shape, G):
    import unmarshal_translit as U
    mode = R.MODE_CLASSIC if shape == "c" else R.MODE_MIN
    n = 3 if shape == "b" else 5
    G = 1 if shape == "b" else G
    with Engine(0, n, mode) as eng, Arena(eng) as ar:
        buf, var = received(eng, shape, G, n)
        nv = len(var)
        m = int(var["n_cmds"].astype(np.int64).sum())
        li = int(var["n_log"].astype(np.int64).sum())
        lm = 4 * li  # every catch-up instance of the workload holds 4 commands
        count = {"accepts": nv, "accept_last_committed": nv, "commits": 0, "cmd_off": nv + 1,
                 "op": m, "key": m, "val": m, "log_inst_off": nv + 1, "log_recs": li,
                 "log_cmd_off": li + 1, "log_op": lm, "log_key": lm, "log_val": lm}
        d = {k: ar.empty(max(c, 1), DTYPES[k]) for k, c in count.items()}
        d_buf, d_var = ar.put(buf), ar.put(var)
        d_res = ar.empty(1, R.UNMARSHAL_RESULT)
        out = _lib.MpxUnmarshalOut()
        for k in R.UNMARSHAL_ARRAYS:
            setattr(out, k, d[k].ptr)
        out.accept_cap, out.commit_cap, out.cmd_cap, out.log_inst_cap, out.log_cmd_cap = nv, 0, m, li, lm
        eng.unmarshal_frames_reserve(nv, li)
        ms = timed(eng, lambda: eng.unmarshal_frames_dev(d_buf.ptr, len(buf), d_var.ptr, nv, None,
                                                         out, d_res.ptr, eng.stream))
        alg = len(buf) + 32 * nv + sum(c * np.dtype(DTYPES[k]).itemsize for k, c in count.items()) + 48
        um = stats(ms, alg)
        res = ar.get(d_res)[0]
        S = min(SAMPLE, nv)
        want, wn = U.expected(mode, buf.tobytes(), var[:S])
        ok = (int(res["n_var"]), int(res["n_accepts"]), int(res["n_cmds"]), int(res["n_log_inst"]),
              int(res["n_log_cmds"])) == (nv, nv, m, li, lm)
        for k in R.UNMARSHAL_ARRAYS:  # stream order: the sample's outputs head every array
            ok = ok and ar.get(d[k], len(want[k])).tobytes() == want[k].tobytes()
        um.update({"frames": nv, "buffer_bytes": len(buf), "commands": m, "log_instances": li,
                   "log_commands": lm, "sample_frames": S, "sample_bit_exact": bool(ok)})
    return {"bench": "unmarshal", "shape": shape, "mode": "classic" if shape == "c" else "min",
            "n_replicas": n, "warmup": 3, "timed_calls": 20, "unmarshal_frames": um,
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
        if not res["unmarshal_frames"]["sample_bit_exact"]:
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())

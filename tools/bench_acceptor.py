#!/usr/bin/env python3
"""Times the acceptor side on device-resident buffers: mpx_accept_handle_dev on 2^24 instances
with one Accept each (90 % acting, seed 42) and mpx_encode_accept_replies_dev on the replies it
produced, spread over 5 leader connections. Per mode: 3 warm-ups, the median of 20 event-timed
calls, algorithmic bytes over the time as a fraction of the 8 TB/s HBM peak, and a check of a
2^16-record sample against the transliteration (tests/acceptor_translit.py) after timing.

    python tools/bench_acceptor.py [--instances N] [--mode min|classic|both]

One JSON line per mode. Compare with `python bench.py --full --workload tally` on the same box in
the same session: the accept tally runs the same tile skeleton over comparable bytes.
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
N, D, SELF = 5, 32, 3
SAMPLE = 1 << 16


def workload(I, mode, seed=42):
    """one Accept at ballot D per instance; 90 % act (MIN: install and reply; CLASSIC: an OK
    reply), 10 % do not (MIN: a resend, ignored; CLASSIC: refused by a higher ballot)"""
    rng = np.random.default_rng(seed)
    acting = rng.random(I) < 0.9
    st = np.zeros(I, R.ACCEPTOR_STATE)
    st["status"] = np.where(acting, rng.integers(-1, 4, I), R.ACCEPTED)
    quiet_ballot = D if mode == R.MODE_MIN else D + 16
    st["ballot"] = np.where(acting, D - 16 * rng.integers(0, 2, I), quiet_ballot)
    # (MIN: an acting instance must not already be ACCEPTED at D)
    if mode == R.MODE_MIN:
        st["ballot"] = np.where(acting & (st["status"] == R.ACCEPTED), D - 16, st["ballot"])
    st["value_id"] = rng.integers(1, 1 << 31, I)
    st["flags"] = np.where(st["status"] == R.STATUS_NIL, 0, rng.integers(0, 2, I))
    msgs = np.zeros(I, R.ACCEPT_MSG)
    msgs["instance"] = np.arange(I)
    msgs["ballot"] = D
    msgs["leader_id"] = rng.integers(0, N, I)
    msgs["value_id"] = rng.integers(1, 1 << 31, I)
    groups = np.zeros(1, R.ACCEPTOR_GROUP)
    groups["default_ballot"], groups["self_id"] = D, SELF
    return msgs, st, groups, acting


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


def run(mode_name, I):
    import acceptor_translit as A
    mode = {"min": R.MODE_MIN, "classic": R.MODE_CLASSIC}[mode_name]
    F = R.ACCEPT_REPLY_FRAME[mode]
    msgs, st, groups, acting = workload(I, mode)
    with Engine(0, N, mode) as eng, Arena(eng) as ar:
        d_msgs, d_st, d_grp = ar.put(msgs), ar.put(st), ar.put(groups)
        d_out = ar.empty(I, R.ACCEPTOR_STATE)
        d_rep, d_to, d_eff = ar.empty(I, R.ACCEPT_REPLY), ar.empty(I, np.int32), ar.empty(I, np.uint8)
        ms = timed(eng, lambda: eng.accept_handle_dev(
            d_msgs.ptr, I, d_st.ptr, d_out.ptr, I, 0, d_grp.ptr, 1, I, d_rep.ptr, d_to.ptr,
            d_eff.ptr, eng.stream))
        med = statistics.median(ms)
        alg = I * 69  # 16 msg + 16 + 16 state + 16 reply + 4 + 1
        # the sample: the first SAMPLE instances are a window of their own
        S = min(SAMPLE, I)
        want = A.accept_handle(mode, N, msgs[:S], st[:S], groups, 0, S)
        got = (ar.get(d_out, S), ar.get(d_rep, S), ar.get(d_to, S), ar.get(d_eff, S))
        ok_step = all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
        eff = ar.get(d_eff)
        replied = int(np.count_nonzero(eff & R.AH_REPLIED))
        step = {"ms_per_call": round(med, 4), "ms_min": round(min(ms), 4),
                "ms_max": round(max(ms), 4), "algorithmic_bytes": alg,
                "fraction_of_8TBps": round(alg / (med * 1e-3) / HBM_PEAK, 4),
                "acting_fraction": round(float(acting.mean()), 4), "replied": replied,
                "sample_checked": S, "sample_bit_exact": bool(ok_step)}

        # the encoder on those replies
        eng.encode_accept_replies_reserve(I)
        d_bytes, d_off = ar.empty(I * F, np.uint8), ar.empty(N + 1, np.uint64)
        ms = timed(eng, lambda: eng.encode_accept_replies_dev(
            d_rep.ptr, d_to.ptr, I, N, d_bytes.ptr, d_off.ptr, eng.stream))
        med = statistics.median(ms)
        alg = I * 20 + replied * F  # 16 + 4 in per slot, one frame out per reply
        to = ar.get(d_to)
        off = ar.get(d_off)
        counts = np.bincount(to[to >= 0], minlength=N)
        ok_enc = np.array_equal(off, np.concatenate([[0], np.cumsum(counts)]) * F)
        w_out, w_off = A.encode_accept_replies(mode, ar.get(d_rep, S), to[:S], N)
        for d in range(N):  # the sample's frames head every destination's run
            k = int(w_off[d + 1] - w_off[d])
            ok_enc = ok_enc and ar.get(d_bytes, k, int(off[d])).tobytes() == \
                w_out[int(w_off[d]):int(w_off[d + 1])].tobytes()
        enc = {"ms_per_call": round(med, 4), "ms_min": round(min(ms), 4),
               "ms_max": round(max(ms), 4), "algorithmic_bytes": alg,
               "fraction_of_8TBps": round(alg / (med * 1e-3) / HBM_PEAK, 4),
               "destinations": N, "frame_bytes": F, "sample_checked": S,
               "sample_bit_exact": bool(ok_enc)}
    return {"bench": "acceptor", "mode": mode_name, "instances": I, "warmup": 3, "timed_calls": 20,
            "accept_handle": step, "encode_accept_replies": enc, "runtime": _lib.runtime_info()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1 << 24)
    ap.add_argument("--mode", default="both", choices=["min", "classic", "both"])
    a = ap.parse_args()
    rc = 0
    for m in (["min", "classic"] if a.mode == "both" else [a.mode]):
        res = run(m, a.instances)
        print(json.dumps(res), flush=True)
        if not (res["accept_handle"]["sample_bit_exact"] and
                res["encode_accept_replies"]["sample_bit_exact"]):
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())

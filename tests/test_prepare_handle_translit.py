"""The prepare side's transliteration (tests/prepare_handle_translit.py) against hand-worked bytes
(tests/prepare_handle_kat.py), against the existing Unmarshal transliteration, and the reach of
its fuzz generator. No GPU: what the GPU tests compare against is checked here first."""
import numpy as np
import pytest

import prepare_handle_kat as K
import prepare_handle_translit as T
import unmarshal_translit as U
from minpaxos_amd import records as R


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_kat(name):
    mode, kw, want = K.CASES[name]()
    N = kw.pop("N")
    got = T.run_batch(mode, N, **kw)
    assert got["frames"][0] == want["frame"]
    assert bytes(got["bytes"]) == want["frame"]
    assert int(got["dest_off"][want["reply_to"]]) == 0
    assert int(got["dest_off"][want["reply_to"] + 1]) == len(want["frame"])
    assert tuple(int(x) for x in got["replies"][0]) == want["reply"]
    assert int(got["reply_to"][0]) == want["reply_to"]
    assert int(got["effect"][0]) == want["effect"]
    if mode == R.MODE_MIN:
        assert int(got["log_from"][0]) == want["log_from"]
    g = got["groups"][0]
    assert tuple(int(g[f]) for f in ("default_ballot", "self_id", "leader", "prepare_oks",
                                     "crt_instance", "committed_upto")) == want["group"]


@pytest.mark.parametrize("mode", [R.MODE_MIN, R.MODE_CLASSIC])
@pytest.mark.parametrize("seed", [0, 5, 11])
def test_round_trip_through_unmarshal(mode, seed):
    """the transliteration's bytes, read back by PrepareReply.Unmarshal's transliteration, are
    the messages the handlers built"""
    kw = T.fuzz_case(seed, mode)
    got = T.run_batch(mode, 3, **kw)
    buf = bytes(got["bytes"])
    order = [i for d in range(3) for i in range(len(kw["msgs"])) if got["reply_to"][i] == d]
    pos = 0
    for i in order:
        code, m, end = U.unmarshal(mode, buf, pos)
        assert code == R.PEER_PREPARE_REPLY
        assert buf[pos:end] == got["frames"][i]
        rep = got["replies"][i]
        assert (m["Instance"], m["Ballot"], m["OK"]) == (int(rep["instance"]), int(rep["ballot"]),
                                                         int(rep["ok"]))
        vid = int(rep["value_id"])
        n = 0
        if vid != R.VALUE_KEEP and int(kw["inst"]["flags"][vid]) & R.IC_HAS_CMDS:
            n = int(kw["inst"]["n_cmds"][vid])
        assert len(m["Command"]) == n
        if mode == R.MODE_MIN:
            assert (m["Id"], m["LastCommitted"]) == (int(rep["id"]), int(rep["last_committed"]))
            want = max(0, int(rep["last_committed"]) - int(got["log_from"][i]) + 1)
            assert len(m["CatchUpLog"]) == want
            for j, (ballot, status, cmds) in enumerate(m["CatchUpLog"]):
                k = int(got["log_from"][i]) + j - kw["inst_base"]
                assert ballot == int(kw["st"]["ballot"][k])
        pos = end
    assert pos == len(buf)


def test_fuzz_generator_reach():
    """every branch of both handlers holds at least 0.02 of the fuzz messages"""
    for mode, names in ((R.MODE_MIN, T.MIN_BRANCHES), (R.MODE_CLASSIC, T.CLASSIC_BRANCHES)):
        census, total = {}, 0
        for seed in T.FUZZ_SEEDS:
            kw = T.fuzz_case(seed, mode)
            got = T.run_batch(mode, 3, **kw)
            total += len(kw["msgs"])
            for k, v in got["census"].items():
                census[k] = census.get(k, 0) + v
        for name in names:
            assert census.get(name, 0) >= 0.02 * total, (mode, name, census, total)


def test_out_of_order_and_panics():
    mode, kw, _ = K.CASES["min_command_and_log"]()
    kw.pop("N")
    bad = dict(kw, msgs=np.array([(0, 0x20, 0, 7)], R.PREPARE_MSG))  # the log would start at 8 < first
    with pytest.raises(T.GoPanic) as e:
        T.run_batch(mode, 3, **bad)
    assert e.value.code == R.E_NIL_INSTANCE
    st = kw["st"].copy()
    st["status"][3] = R.ACCEPTED  # crtInstance now reaches a full slot 13, committedUpTo + 1 fine
    st["status"][1] = T.NIL       # ... but instance 11 of the log is nil
    with pytest.raises(T.GoPanic) as e:
        T.run_batch(mode, 3, **dict(kw, st=st, groups=kw["groups"]))
    assert e.value.code == R.E_NIL_INSTANCE
    two = np.array([(1, 1, 0, 0), (0, 1, 0, 0)], R.PREPARE_MSG)
    with pytest.raises(T.GoPanic) as e:
        T.run_batch(mode, 3, **dict(kw, msgs=two))
    assert e.value.code == R.E_INVAL
    with pytest.raises(T.GoPanic) as e:
        T.run_batch(mode, 3, **dict(kw, msgs=np.array([(0, 0x20, 3, 9)], R.PREPARE_MSG)))
    assert e.value.code == R.E_BAD_ID


def test_boundary_sweep_inputs_sit_on_the_window_boundary():
    """the GPU sweep (test_gpu_prepare_handle.py) is only as good as its inputs: walked through the
    transliteration's frames, case d has the header of the record under test at byte 8192 + d, and
    over the sweep d = -30 .. 2 a record header starts on every byte of 8192 - 30 .. 8192 + 2 (the
    sweep's own range: the neighbouring headers are 60 bytes and more away) and a log command on
    every byte of 8192 - 47 .. 8192 + 11; the straddle case has a Command entry across byte 8192"""
    import proposer_translit as P
    heads, cmds = set(), set()
    for d in P.SWEEP:
        a, k = T.boundary_case(d)
        want = T.run_batch(R.MODE_MIN, 2, **a)
        assert len(want["frames"]) == 1 and want["census"] == dict(raised=1, log=1, command=1)
        recs, starts = P.log_starts(want["frames"][0], 18)
        assert recs[k] == P.WINDOW + d and len(want["frames"][0]) > P.WINDOW
        heads.update(recs)
        cmds.update(starts)
    assert heads >= set(range(P.WINDOW - 30, P.WINDOW + 3))
    assert cmds >= set(range(P.WINDOW - 47, P.WINDOW + 12))
    frame = T.run_batch(R.MODE_MIN, 2, **T.command_straddle_case())["frames"][0]
    own = [18 + 2 + 17 * j for j in range(482)]
    assert any(s < P.WINDOW < s + 17 for s in own)
    recs, _ = P.log_starts(frame, 18)
    assert recs[0] == own[-1] + 17 + 1 and len(recs) == 3

"""The reply transliteration (tests/reply_translit.py) against the hand-worked known answers of
tests/reply_kat.py, the faulty-slot treatment of both forms, and the reach of its fuzz generator:
CPU only."""
import numpy as np
import pytest

import reply_kat
import reply_translit as T
from minpaxos_amd import records as R

FUZZ_SEEDS = range(24)


def test_about_a_dozen_known_answers():
    assert len(reply_kat.KAT_REPLY) >= 12
    assert len({c["name"] for c in reply_kat.KAT_REPLY}) == len(reply_kat.KAT_REPLY)
    assert (reply_kat.FALSE_, reply_kat.DECIDED, reply_kat.EXECUTED) == \
        (R.RB_FALSE, R.RB_DECIDED, R.RB_EXECUTED)
    assert (reply_kat.ACCEPT, reply_kat.NOT_LEADER, reply_kat.REFUSED, reply_kat.PREPARE) == \
        (R.PH_ACCEPT, R.PH_NOT_LEADER, R.PH_REFUSED, R.PH_PREPARE)


@pytest.mark.parametrize("proto", [T.MIN, T.CLASSIC])
@pytest.mark.parametrize("case", reply_kat.KAT_REPLY, ids=lambda c: c["name"])
def test_known_answer(case, proto):
    got = T.build_replies(proto=proto, **reply_kat.kat_args(case))
    assert got["code"] == R.OK
    assert [tuple(int(x) for x in r) for r in got["recs"].tolist()] == case["want"]
    assert (int(got["res"]["n_replies"]), int(got["res"]["n_slots"])) == \
        (case["n_replies"], case["n_slots"])
    if case["cs_flags"] is not None:
        assert got["commit_sends"]["flags"].tolist() == case["cs_flags"]
        for s, row in enumerate(case["sends"]):
            c = got["commit_sends"][s]
            assert (int(c["instance"]), int(c["ballot"]), int(c["first_cmd"]), int(c["n_cmds"])) == \
                (row[0], row[1], row[3], row[4])
        # CLASSIC: bcastCommit ran for exactly the instances flagged MPX_CS_SEND
        if proto == T.CLASSIC and case["kind"] == R.RB_DECIDED:
            assert [b[0] for b in got["bcast"]] == \
                [row[0] for row, f in zip(case["sends"], case["cs_flags"]) if f]


def test_refusal_is_what_the_go_writes():
    """ProposeReplyTS{FALSE, -1, state.NIL, 0}: neither the proposal's id nor its timestamp"""
    got = T.build_replies(R.RB_FALSE, T.mk_sends([(-1, 0, R.PH_NOT_LEADER, 0, 1)]),
                          T.mk_meta([(1234, 77, 5)]))
    assert got["writers"] == {5: [(T.FALSE, -1, T.NIL, 0)]}


def test_writers_keep_each_clients_order():
    case = T.fuzz_case(4)
    got = T.build_replies(**{k: v for k, v in case.items() if k not in ("cap", "pad_client")})
    recs = got["recs"]
    for w, replies in got["writers"].items():
        mine = recs[recs["client"] == w]
        assert [(int(x["command_id"]), int(x["value"]), int(x["timestamp"])) for x in mine] == \
            [(cid, val, ts) for _, cid, val, ts in replies]


def test_faulty_slots_by_form():
    sends = T.mk_sends([(5, 1, R.PH_ACCEPT, 0, 2), (6, 1, R.PH_ACCEPT, 2, 9), (7, 1, R.PH_ACCEPT, 2, 1)])
    meta = T.mk_meta([(1, 1, 0), (2, 2, 0), (3, 3, 1)])
    assert T.build_replies(R.RB_DECIDED, sends, meta)["code"] == R.E_INVAL
    got = T.build_replies(R.RB_DECIDED, sends, meta, dev=True)
    assert got["code"] == R.E_INVAL and got["commit_sends"]["flags"].tolist() == [1, 0, 1]
    assert got["recs"]["command_id"].tolist() == [1, 2, 3] and int(got["res"]["n_slots"]) == 2
    # outside the window only matters with a mask
    sends = T.mk_sends([(5, 1, R.PH_ACCEPT, 0, 2), (9, 1, R.PH_ACCEPT, 2, 1)])
    assert T.build_replies(R.RB_DECIDED, sends, meta, inst_base=5)["code"] == R.OK
    mask = np.ones(4, np.uint8)
    assert T.build_replies(R.RB_DECIDED, sends, meta, mask, 5)["code"] == R.E_NIL_INSTANCE
    got = T.build_replies(R.RB_DECIDED, sends, meta, mask, 5, dev=True)
    assert got["code"] == R.E_NIL_INSTANCE and got["recs"]["command_id"].tolist() == [1, 2]
    # a result range outside ret
    ret = np.arange(3, dtype=np.int64)
    rf = np.array([0, 3], np.uint64)
    assert T.build_replies(R.RB_EXECUTED, sends, meta, ret=ret, ret_first=rf)["code"] == R.E_INVAL


def test_a_slot_the_mask_passes_over_reads_no_result():
    """execute_gather's ret_first puts an instance that did not execute where the executed ones
    before it end (the last slots: at n_ret itself); build_replies(EXECUTED) judges the result range
    of the slots it selects only"""
    import execute_translit as X
    sends = T.mk_sends([(100, 4, R.PH_ACCEPT, 0, 3), (101, 4, R.PH_ACCEPT, 3, 2), (102, 4, R.PH_ACCEPT, 5, 4)])
    meta = T.mk_meta([(j, j, j % 2) for j in range(9)])
    inst = np.zeros(3, R.INST_CMDS)
    inst["first_cmd"], inst["n_cmds"], inst["flags"] = [0, 3, 5], [3, 2, 4], R.IC_HAS_CMDS
    cmds = (np.ones(9, np.uint8), np.arange(9), np.arange(9))
    x = X.execute_gather(inst, [100], [99], cmds, 100, 3, sends=sends)
    assert x["mask"].tolist() == [1, 0, 0] and x["ret_first"].tolist() == [0, 3, 3]
    ret = np.array([11, 12, 13], np.int64)
    for dev in (False, True):
        got = T.build_replies(R.RB_EXECUTED, sends, meta, x["mask"], 100, ret, x["ret_first"], dev=dev)
        assert got["code"] == R.OK and got["recs"]["value"].tolist() == [11, 12, 13]
    assert T.build_replies(R.RB_EXECUTED, sends, meta, np.array([1, 0, 1], np.uint8), 100, ret,
                           x["ret_first"])["code"] == R.E_INVAL


def test_fuzz_generator_reaches_every_slot_kind():
    """over the fuzz seeds each slot kind is at least 0.02 of the slots"""
    census = {}
    kinds = set()
    for seed in FUZZ_SEEDS:
        case = T.fuzz_case(seed, census)
        kinds.add(case["kind"])
        want = T.build_replies(**case)
        assert want["code"] == R.OK
    assert kinds == {R.RB_FALSE, R.RB_DECIDED, R.RB_EXECUTED}
    for name in T.SLOT_KINDS:
        assert census.get(name, 0) >= 0.02 * census["slots"], (name, census)

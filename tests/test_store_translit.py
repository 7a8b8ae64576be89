"""CPU checks of the store-assembly reference model (tests/store_translit.py): the hand-traced
answers of tests/store_kat.py, the per-form treatment of faulty items, and the census of the fuzz
generator the GPU tests draw from (every branch of the assignments comes up often enough)."""
import numpy as np
import pytest

import store_kat
import store_translit as T
from minpaxos_amd import records as R


@pytest.mark.parametrize("case", store_kat.KAT_STORE, ids=lambda c: c["name"])
def test_known_answers(case):
    got = T.store_commands(**store_kat.kat_args(case))
    assert got["code"] == R.OK
    store_kat.check(case, got)
    # the device form answers the same where nothing is faulty
    dev = T.store_commands(dev=True, **store_kat.kat_args(case))
    assert all(np.asarray(dev[k]).tobytes() == np.asarray(got[k]).tobytes() for k in got if k != "code")


def test_known_compaction():
    c = store_kat.KAT_COMPACT
    got = T.store_compact(c["inst"], store_kat.arena(c["cap"]), c["used"], c["to_cap"])
    assert got["code"] == R.OK
    store_kat.check_compact(got)
    short = T.store_compact(c["inst"], store_kat.arena(c["cap"]), c["used"], c["to_cap"] - 1)
    assert short["code"] == R.OK and int(short["res"]["flags"]) == R.SC_FULL and short["used"] is None
    assert short["inst"].tobytes() == c["inst"].tobytes() and not short["key"].any()
    assert int(short["res"]["n_cmds"]) == 4 and int(short["res"]["n_stored"]) == 3


def _two():
    """two Accepts of two instances from one source, the first of them made faulty by the tests"""
    return dict(kind=R.SC_MSGS, items=T.mk_msgs([(10, 0), (11, 1)]), effect=np.array([2, 2], np.uint8),
                sources=[store_kat.source(0, [2, 3])], arena=store_kat.arena(8), used=1,
                inst=store_kat.window(4), inst_base=10)


def faulty(fault):
    a = _two()
    if fault == "value_id":
        a["items"]["value_id"][0] = 2
    elif fault == "range":
        a["sources"][0]["cmd_off"] = np.array([0, 9, 2, 5], np.uint64)   # frame 0 leaves the 5 commands
        a["items"]["value_id"][1] = 2
    elif fault == "decreasing":
        a["sources"][0]["cmd_off"] = np.array([3, 2, 5], np.uint64)
    elif fault == "perm":
        a["perm"] = np.array([7, 1], np.uint32)
    elif fault == "below_window":
        a["items"]["instance"][0] = 9
    elif fault == "above_window":
        a["items"]["instance"][0] = 14
    elif fault == "sends_range":
        a.update(kind=R.SC_SENDS, effect=None, items=T.mk_sends([(10, R.PH_ACCEPT, 4, 2), (11, R.PH_PREPARE, 1, 2)]),
                 sources=[dict(store_kat.source(0, [5]), cmd_off=None, n_recs=2)])
    return a


FAULTS = ("value_id", "range", "decreasing", "perm", "below_window", "above_window", "sends_range")


@pytest.mark.parametrize("fault", FAULTS)
def test_a_faulty_item_by_form(fault):
    a = faulty(fault)
    code = R.E_NIL_INSTANCE if "window" in fault else R.E_INVAL
    assert T.store_commands(**a) == dict(code=code)
    dev = T.store_commands(dev=True, **a)
    # the other item stored, the faulty one neither stored nor superseded
    assert dev["code"] == code and int(dev["res"]["n_stored"]) == 1 and int(dev["res"]["n_superseded"]) == 0
    assert int(dev["inst"]["flags"].sum()) == 1 and int(dev["inst"]["flags"][1]) == R.IC_HAS_CMDS
    assert dev["used"] == 1 + int(dev["res"]["n_cmds"])


def test_an_item_that_does_not_store_is_not_judged():
    a = faulty("value_id")
    a["effect"][0] = R.AH_REPLIED
    a["items"]["instance"][0] = -5
    got = T.store_commands(**a)
    assert got["code"] == R.OK and int(got["res"]["n_stored"]) == 1
    a["effect"][0], a["items"]["value_id"][0] = R.CH_CMDS, R.VALUE_KEEP
    assert T.store_commands(**a)["code"] == R.OK


def test_a_cursor_past_the_capacity():
    a = dict(_two(), used=9)
    assert T.store_commands(**a) == dict(code=R.E_INVAL)
    dev = T.store_commands(dev=True, **a)
    assert dev["code"] == R.E_INVAL and int(dev["res"]["flags"]) == R.SC_FULL and dev["used"] == 9
    assert not dev["inst"]["flags"].any()


def test_d_n_cuts_the_batch():
    a = _two()
    got = T.store_commands(dev=True, d_n=1, **a)
    assert int(got["res"]["n_stored"]) == 1 and got["used"] == 3 and int(got["inst"]["flags"][1]) == 0


def test_compaction_of_a_faulty_slot_by_form():
    c = store_kat.KAT_COMPACT
    inst = c["inst"].copy()
    inst[2] = (5, 2, R.IC_HAS_CMDS)                  # [5, 7) leaves [0, 6)
    assert T.store_compact(inst, store_kat.arena(8), 6, 4) == dict(code=R.E_INVAL)
    dev = T.store_compact(inst, store_kat.arena(8), 6, 4, dev=True)
    assert dev["code"] == R.E_INVAL and tuple(dev["inst"][2]) == (2, 0, R.IC_HAS_CMDS)
    assert dev["key"][:3].tolist() == [301, 302, 300] and dev["used"] == 3
    assert T.store_compact(c["inst"], store_kat.arena(8), 9, 4) == dict(code=R.E_INVAL)


def test_fuzz_census_over_24_seeds():
    """every branch is at least 0.02 of the items, by the transliteration alone"""
    census = T.new_census()
    kinds = set()
    for seed in range(24):
        case = T.fuzz_case(seed)
        kinds.add((case["kind"], len(case["sources"]), case.get("perm") is None))
        got = T.store_commands(census=census, **case)
        assert got["code"] == R.OK
        # the winners' lengths add up, the untouched slots are the input's
        assert int(got["res"]["n_stored"]) + int(got["res"]["n_superseded"]) > 0
        same = got["inst"] == case["inst"]
        assert int((~same).sum()) <= int(got["res"]["n_stored"])
    for b in T.BRANCHES:
        assert census[b] >= 0.02 * census["items"], (b, census)
    assert {k for k, _, _ in kinds} == {R.SC_MSGS, R.SC_SENDS}
    assert any(n > 1 for _, n, _ in kinds) and any(p for k, _, p in kinds if k == R.SC_MSGS)

"""CPU checks of the record-assembly reference model (tests/record_translit.py): the hand-worked
bytes of tests/record_kat.py, a second opinion from the durable-log encoding check of
tests/test_logenc.py on the recording items' records and pre-gathered commands, the per-form
treatment of faulty items, and the census of the fuzz generator the GPU tests draw from."""
import numpy as np
import pytest

import record_kat
import record_translit as T
import test_logenc
from minpaxos_amd import records as R

SEEDS = range(24)


@pytest.mark.parametrize("case", record_kat.KAT, ids=lambda c: c["name"])
def test_known_answers(case):
    got = T.record_log(**case["args"])
    assert got["code"] == R.OK
    record_kat.check(case, got)
    # the device form answers the same where nothing is faulty
    dev = T.record_log(dev=True, **case["args"])
    assert all(np.asarray(dev[k]).tobytes() == np.asarray(got[k]).tobytes() for k in got if k != "code")


@pytest.mark.parametrize("case", record_kat.KAT, ids=lambda c: c["name"])
def test_one_byte_short_writes_nothing(case):
    n = len(bytes.fromhex(case["out"]))
    got = T.record_log(out_cap=n - 1, **case["args"])
    assert got["code"] == R.OK and len(got["out"]) == 0 and int(got["res"]["flags"]) == R.LR_FULL
    assert int(got["res"]["n_bytes"]) == n and int(got["res"]["n_recs"]) == case["n_recs"]
    assert got["item_off"].tolist() == case["item_off"]


def test_accepts_have_no_classic_form():
    args = dict(record_kat.KAT[2]["args"], fmt=R.LOG_DURABLE_CLASSIC)
    assert T.record_log(**args) == dict(code=R.E_UNSUPPORTED)


def min_cases():
    return [c["args"] for c in record_kat.KAT if c["args"]["fmt"] == R.LOG_DURABLE] + \
        [c for c in map(T.fuzz_case, SEEDS) if c["fmt"] == R.LOG_DURABLE]


def test_second_opinion_from_the_durable_log_check():
    """MIN format: the recording items as LOG_REC records with their commands gathered, through
    test_logenc's restatement of MPX_LOG_DURABLE, give the same bytes and record starts"""
    kinds = set()
    for case in min_cases():
        got = T.record_log(**case)
        recs, off, op, key, val = T.gathered(case)
        want, ro = test_logenc.expected(R.LOG_DURABLE, recs, off, op, key, val)
        assert got["out"].tobytes() == want
        starts = got["item_off"][:-1][np.diff(got["item_off"].astype(np.int64)) > 0]
        assert starts.tolist() == ro[:-1] and int(got["res"]["n_recs"]) == len(recs)
        assert int(got["res"]["n_cmds"]) == len(op)
        kinds.add(case["kind"])
    assert kinds == {R.LR_ACCEPTS, R.LR_COMMITS, R.LR_SENDS, R.LR_DECIDED}


def test_classic_differs_from_min_only_in_the_metadata():
    """the same batch in both formats: the commands' bytes agree, the metadata is 5 bytes for 12"""
    for seed in SEEDS:
        case = T.fuzz_case(seed)
        if case["kind"] == R.LR_ACCEPTS:
            continue
        a = T.record_log(**dict(case, fmt=R.LOG_DURABLE))
        c = T.record_log(**dict(case, fmt=R.LOG_DURABLE_CLASSIC))
        n = int(a["res"]["n_recs"])
        assert int(c["res"]["n_recs"]) == n and int(c["res"]["n_cmds"]) == int(a["res"]["n_cmds"])
        assert int(a["res"]["n_bytes"]) - int(c["res"]["n_bytes"]) == 7 * n
        for i in np.flatnonzero(np.diff(a["item_off"].astype(np.int64))):
            ra = a["out"][int(a["item_off"][i]):int(a["item_off"][i + 1])]
            rc = c["out"][int(c["item_off"][i]):int(c["item_off"][i + 1])]
            assert ra[:4].tobytes() == rc[:4].tobytes() and ra[4] == rc[4] and not ra[5:8].any()
            assert ra[12:].tobytes() == rc[5:].tobytes()


def _two(kind=R.LR_ACCEPTS):
    return T.msgs_case(kind, R.LOG_DURABLE, [2, 3], [True, True])


def faulty(fault):
    a = _two()
    if fault == "value_id":
        a["items"]["value_id"][0] = 2
    elif fault == "range":
        a["sources"][0]["cmd_off"] = np.array([0, 9, 2, 5], np.uint64)    # frame 0 leaves the 5 commands
        a["items"]["value_id"][1] = 2
    elif fault == "decreasing":
        a["sources"][0]["cmd_off"] = np.array([3, 2, 5], np.uint64)
    elif fault == "perm":
        a["perm"] = np.array([7, 1], np.uint32)
    elif fault == "commit_value_id":
        a = _two(R.LR_COMMITS)
        a["items"]["value_id"][0] = 2
    elif fault == "sends_range":
        a = T.sends_case(R.LR_SENDS, R.LOG_DURABLE, [2, 2], [R.PH_ACCEPT, R.PH_ACCEPT])
        a["items"]["first_cmd"][0] = 8                                    # [8, 10) leaves the 9 commands
    elif fault in ("below_window", "above_window"):
        a = T.sends_case(R.LR_DECIDED, R.LOG_DURABLE, [1, 1], [R.PH_ACCEPT, R.PH_ACCEPT],
                         mask=np.ones(2, np.uint8))
        a["items"]["instance"][0] = 99 if fault == "below_window" else 102
    return a


FAULTS = ("value_id", "range", "decreasing", "perm", "commit_value_id", "sends_range", "below_window",
          "above_window")


@pytest.mark.parametrize("fault", FAULTS)
def test_a_faulty_item_by_form(fault):
    a = faulty(fault)
    code = R.E_NIL_INSTANCE if "window" in fault else R.E_INVAL
    assert T.record_log(**a) == dict(code=code)
    dev = T.record_log(dev=True, **a)
    # the other item recorded, the faulty one did not
    assert dev["code"] == code and int(dev["res"]["n_recs"]) == 1
    assert int(dev["item_off"][0]) == int(dev["item_off"][1]) == 0
    assert int(dev["item_off"][2]) == int(dev["res"]["n_bytes"]) == len(dev["out"]) > 0


def test_an_item_that_does_not_record_is_not_judged():
    a = faulty("value_id")
    a["effect"][0] = R.AH_REPLIED
    got = T.record_log(**a)
    assert got["code"] == R.OK and int(got["res"]["n_recs"]) == 1
    c = faulty("commit_value_id")
    c["effect"][0] = R.CH_INSTALLED                       # metadata only: its value is not resolved
    got = T.record_log(**c)
    assert got["code"] == R.OK and int(got["res"]["n_recs"]) == 2 and int(got["item_off"][1]) == 12
    d = faulty("below_window")
    d["items"]["flags"][0] = R.PH_PREPARE
    assert T.record_log(**d)["code"] == R.OK


def test_d_n_cuts_the_batch():
    got = T.record_log(dev=True, d_n=1, **_two())
    assert int(got["res"]["n_recs"]) == 1 and got["item_off"].tolist() == [0, 46, 46]


def test_a_replica_that_is_not_durable_records_nothing():
    for r in (T.MinReplica(durable=False), T.ClassicReplica(durable=False)):
        r.recordCommands([T.Command(1, 2, 3)])
        assert not r.StableStore


def test_fuzz_census_over_24_seeds():
    """every kind comes up, and each of its branches holds at least 0.02 of the kind's items, by the
    transliteration alone"""
    census = T.new_census()
    seen = set()
    for seed in SEEDS:
        case = T.fuzz_case(seed)
        got = T.record_log(census=census, **case)
        assert got["code"] == R.OK
        seen.add((case["kind"], case["fmt"], len(case.get("sources", ())), case.get("perm") is None))
        assert int(got["res"]["n_bytes"]) == len(got["out"]) == \
            R.LR_HEADER_BYTES[case["fmt"]] * int(got["res"]["n_recs"]) + 17 * int(got["res"]["n_cmds"])
    for kind, branches in T.BRANCHES.items():
        assert census[kind]["items"] > 0
        for b in branches:
            assert census[kind][b] >= 0.02 * census[kind]["items"], (kind, b, census[kind])
    assert {(k, f) for k, f, _, _ in seen} == {
        (R.LR_ACCEPTS, R.LOG_DURABLE), (R.LR_COMMITS, R.LOG_DURABLE), (R.LR_SENDS, R.LOG_DURABLE),
        (R.LR_DECIDED, R.LOG_DURABLE), (R.LR_COMMITS, R.LOG_DURABLE_CLASSIC),
        (R.LR_SENDS, R.LOG_DURABLE_CLASSIC), (R.LR_DECIDED, R.LOG_DURABLE_CLASSIC)}
    assert any(n > 1 for _, _, n, _ in seen) and any(p for k, _, _, p in seen if k <= R.LR_COMMITS)

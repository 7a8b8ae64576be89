"""The execute transliteration (tests/execute_translit.py) against the hand-worked known answers of
tests/execute_kat.py, the treatment of faulty groups and instances of both forms, and the reach of
its fuzz generator: CPU only."""
import numpy as np
import pytest

import execute_kat
import execute_translit as T
from minpaxos_amd import records as R

FUZZ_SEEDS = range(24)


def test_about_a_dozen_known_answers():
    assert len(execute_kat.KAT_EXECUTE) >= 12
    assert len({c["name"] for c in execute_kat.KAT_EXECUTE}) == len(execute_kat.KAT_EXECUTE)


@pytest.mark.parametrize("case", execute_kat.KAT_EXECUTE, ids=lambda c: c["name"])
def test_known_answer(case):
    got = T.execute_gather(**execute_kat.kat_args(case))
    assert got["code"] == R.OK
    execute_kat.check(case, got)


def test_call_order_is_group_then_instance_then_command():
    got = T.execute_gather(**{k: v for k, v in T.fuzz_case(3).items() if k not in ("cap", "pad")})
    assert got["order"] == sorted(got["order"]) and len(got["order"]) == int(got["res"]["n_cmds"])


def test_faulty_groups_and_instances_by_form():
    inst = T.mk_inst([(0, 2), (2, 9), (3, 1), (0, 1), (1, 1), (2, 1)])
    cmds = T.mk_cmds(4)
    # group 1's committedUpTo lies in group 0's window
    args = dict(inst=inst, cmds=cmds, inst_base=10, ipg=3, executed=[9, 12])
    assert T.execute_gather(committed_upto=[10, 11], **args)["code"] == R.E_INVAL
    got = T.execute_gather(committed_upto=[10, 11], dev=True, **args)
    assert got["code"] == R.E_INVAL and got["executed"].tolist() == [10, 12]
    assert got["mask"].tolist() == [1, 0, 0, 0, 0, 0]
    # instance 11's range leaves the source: only when the walk reaches it
    assert T.execute_gather(committed_upto=[10, 15], **args)["code"] == R.OK
    assert T.execute_gather(committed_upto=[11, 15], **args)["code"] == R.E_INVAL
    got = T.execute_gather(committed_upto=[12, 15], dev=True, **args)
    assert got["code"] == R.E_INVAL and got["mask"].tolist() == [1] * 6
    assert got["inst_first"].tolist() == [0, 2, 2, 3, 4, 5] and int(got["res"]["n_cmds"]) == 6
    # the cursors' legal range ends at first_g - 1 and first_g + ipg - 1
    assert T.execute_gather(committed_upto=[12, 15], **dict(args, executed=[8, 12]))["code"] == R.E_INVAL
    assert T.execute_gather(committed_upto=[13, 15], **args)["code"] == R.E_INVAL


def test_fuzz_generator_reaches_every_branch():
    """over the fuzz seeds each branch of the walk is at least 0.02 of the groups"""
    census = {}
    for seed in FUZZ_SEEDS:
        case = T.fuzz_case(seed, census)
        assert T.execute_gather(**case)["code"] == R.OK
    for name in T.BRANCHES:
        assert census.get(name, 0) >= 0.02 * census["groups"], (name, census)

"""Hand-worked known answers of execute assembly (KAT_EXECUTE), from the Go text of executeCommands
(bareminpaxos.go:1066-1098, paxos.go:675-706).

A case gives the call: inst as (first_cmd, n_cmds) per window slot or None for Cmds == nil, the
groups' committed and executed cursors, inst_base, ipg, and optionally sends (instance numbers),
cap and pad. It states what comes out: src = the source command index of every gathered command
in Execute's call order (before cap), mask, executed (the cursors after), inst_first, and where
given ret_first and grp_cmd_off; n_inst = instances executed, n_groups = groups whose cursor moved.

Reading one by hand: i starts at executed + 1; while i <= committedUpTo and instanceSpace[i].Cmds
!= nil the instance's commands run in order and i++; the first nil Cmds breaks. The cursor after is
i - 1."""

KAT_EXECUTE = [
    dict(name="no_stop",
         # 10, 11, 12 all have commands: everything up to committedUpTo = 12 runs
         inst=[(0, 2), (2, 1), (3, 2)], base=10, ipg=3, committed=[12], executed=[9],
         src=[0, 1, 2, 3, 4], mask=[1, 1, 1], executed_out=[12], inst_first=[0, 2, 3],
         grp_cmd_off=[0, 5], n_inst=3, n_groups=1),
    dict(name="stop_at_the_first",
         # instance 10's Cmds is nil: the very first test breaks, the cursor stays
         inst=[None, (2, 1), (3, 2)], base=10, ipg=3, committed=[12], executed=[9],
         src=[], mask=[0, 0, 0], executed_out=[9], inst_first=[0, 0, 0],
         grp_cmd_off=[0, 0], n_inst=0, n_groups=0),
    dict(name="stop_in_the_middle",
         # 11 is nil: 10 runs, 12 does not although it is committed and has commands
         inst=[(5, 2), None, (9, 3)], base=10, ipg=3, committed=[12], executed=[9],
         src=[5, 6], mask=[1, 0, 0], executed_out=[10], inst_first=[0, 2, 2],
         grp_cmd_off=[0, 2], n_inst=1, n_groups=1),
    dict(name="stop_at_the_last",
         inst=[(5, 2), (1, 1), None], base=10, ipg=3, committed=[12], executed=[9],
         src=[5, 6, 1], mask=[1, 1, 0], executed_out=[11], inst_first=[0, 2, 3],
         grp_cmd_off=[0, 3], n_inst=2, n_groups=1),
    dict(name="empty_non_nil_slice",
         # len(Cmds) == 0, Cmds != nil: no Execute, i++ all the same, 2 runs after it
         inst=[(3, 1), (4, 0), (7, 2)], base=0, ipg=3, committed=[2], executed=[-1],
         src=[3, 7, 8], mask=[1, 1, 1], executed_out=[2], inst_first=[0, 1, 1],
         grp_cmd_off=[0, 3], n_inst=3, n_groups=1),
    dict(name="executed_is_committed",
         # i = 12 > committedUpTo = 11: the loop body never runs
         inst=[(0, 1), (1, 1), (2, 1)], base=10, ipg=3, committed=[11], executed=[11],
         src=[], mask=[0, 0, 0], executed_out=[11], inst_first=[0, 0, 0],
         grp_cmd_off=[0, 0], n_inst=0, n_groups=0),
    dict(name="executed_above_committed",
         # MIN assigns committedUpTo = areply.Instance: it moved down to 10 after 12 had run
         inst=[(0, 1), (1, 1), (2, 1)], base=10, ipg=3, committed=[10], executed=[12],
         src=[], mask=[0, 0, 0], executed_out=[12], inst_first=[0, 0, 0],
         grp_cmd_off=[0, 0], n_inst=0, n_groups=0),
    dict(name="nothing_committed",
         # committedUpTo = first_g - 1 = -1 (a fresh replica): 0 <= -1 is false
         inst=[(0, 1), (1, 1)], base=0, ipg=2, committed=[-1], executed=[-1],
         src=[], mask=[0, 0], executed_out=[-1], inst_first=[0, 0],
         grp_cmd_off=[0, 0], n_inst=0, n_groups=0),
    dict(name="resumes_after_the_cursor",
         # 10 ran in an earlier call: it is not run again, and a nil slot below the cursor is not seen
         inst=[None, (4, 2), (0, 1)], base=10, ipg=3, committed=[12], executed=[10],
         src=[4, 5, 0], mask=[0, 1, 1], executed_out=[12], inst_first=[0, 0, 2],
         grp_cmd_off=[0, 3], n_inst=2, n_groups=1),
    dict(name="two_groups_with_different_stops",
         # group 0 = instances 20..22 stops at 21; group 1 = 23..25 is committed up to 24 only
         inst=[(0, 1), None, (1, 1), (6, 2), (2, 3), (5, 1)], base=20, ipg=3,
         committed=[22, 24], executed=[19, 22],
         src=[0, 6, 7, 2, 3, 4], mask=[1, 0, 0, 1, 1, 0], executed_out=[20, 24],
         inst_first=[0, 1, 1, 1, 3, 6], grp_cmd_off=[0, 1, 6], n_inst=3, n_groups=2),
    dict(name="cap_short_by_one",
         # five commands, room for four: the counts and the cursors stay complete
         inst=[(0, 2), (2, 1), (3, 2)], base=10, ipg=3, committed=[12], executed=[9], cap=4,
         src=[0, 1, 2, 3, 4], mask=[1, 1, 1], executed_out=[12], inst_first=[0, 2, 3],
         grp_cmd_off=[0, 5], n_inst=3, n_groups=1),
    dict(name="pad_tail",
         # two commands in a capacity of five: positions 2, 3, 4 are {NONE, key = position, 0}
         inst=[(7, 2), None], base=0, ipg=2, committed=[1], executed=[-1], cap=5, pad=True,
         src=[7, 8], mask=[1, 0], executed_out=[0], inst_first=[0, 2],
         grp_cmd_off=[0, 2], n_inst=1, n_groups=1, pad_keys=[2, 3, 4]),
    dict(name="ret_first_with_a_send_outside_the_window",
         # sends name 12 (not executed: its offset is still the sum before it), 10, 9 (below the
         # window), 13 (past it) and 11
         inst=[(0, 2), (2, 3), (5, 1)], base=10, ipg=3, committed=[11], executed=[9],
         sends=[12, 10, 9, 13, 11],
         src=[0, 1, 2, 3, 4], mask=[1, 1, 0], executed_out=[11], inst_first=[0, 2, 5],
         ret_first=[5, 0, 0, 0, 2], grp_cmd_off=[0, 5], n_inst=2, n_groups=1),
]


def kat_args(case):
    """the case as keyword arguments of execute_translit.execute_gather / Engine.execute_gather"""
    import numpy as np

    import execute_translit as T
    n_src = 12
    a = dict(inst=T.mk_inst(case["inst"]), committed_upto=np.array(case["committed"], np.int32),
             executed=np.array(case["executed"], np.int32), cmds=T.mk_cmds(n_src, 5),
             inst_base=case["base"], ipg=case["ipg"])
    if "sends" in case:
        a["sends"] = T.mk_sends(case["sends"])
    for k in ("cap", "pad"):
        if k in case:
            a[k] = case[k]
    return a


def check(case, got):
    """got (the dict of execute_translit.execute_gather or of Engine.execute_gather) is the case's
    stated answer"""
    op, key, val = kat_args(case)["cmds"]
    cap = case.get("cap", len(case["src"]))
    src = case["src"][:cap]
    pad_keys = case.get("pad_keys", [])
    assert got["op"].tolist() == op[src].tolist() + [0] * len(pad_keys)
    assert got["key"].tolist() == key[src].tolist() + pad_keys
    assert got["val"].tolist() == val[src].tolist() + [0] * len(pad_keys)
    assert got["mask"].tolist() == case["mask"]
    assert got["executed"].tolist() == case["executed_out"]
    assert got["inst_first"].tolist() == case["inst_first"]
    assert got["grp_cmd_off"].tolist() == case["grp_cmd_off"]
    if "ret_first" in case:
        assert got["ret_first"].tolist() == case["ret_first"]
    res = got["res"]
    assert (int(res["n_cmds"]), int(res["n_inst"]), int(res["n_groups"]), int(res["reserved"])) == \
        (len(case["src"]), case["n_inst"], case["n_groups"], 0)

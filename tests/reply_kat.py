"""Hand-worked known answers of reply assembly (KAT_REPLY), from the Go text of the three reply
loops: handlePropose's refusals (bareminpaxos.go:622-623, :682-683, paxos.go:390-391),
handleAcceptReply with !Dreply (bareminpaxos.go:1030-1042, paxos.go:644-655) and executeCommands
with Dreply (bareminpaxos.go:1076-1084, paxos.go:685-693).

A case gives the call: kind, sends as (instance, ballot, flags, first_cmd, n_cmds), meta as
(timestamp, command_id, client) per proposal, and optionally mask (from inst_base), ret, ret_first,
cap and pad_client. It states what comes out: want = the mpx_reply_rec (value, timestamp,
command_id, client) the call writes, n_replies, n_slots, and cs_flags = the MPX_CS_SEND flag per
slot (None for MPX_RB_FALSE, which takes no commit_sends).

Reading a reply by hand: a refusal is ProposeReplyTS{FALSE, -1, state.NIL, 0}: CommandId -1, Value
0, Timestamp 0, sent on propose.Reply (the client stays, the id and the timestamp do not). A
decide-time reply is {TRUE, ClientProposals[i].CommandId, state.NIL, ClientProposals[i].Timestamp}
for i over len(inst.Cmds). An execute-time reply carries val = Cmds[j].Execute(...) instead."""
FALSE_, DECIDED, EXECUTED = 1, 2, 3
ACCEPT, NOT_LEADER, REFUSED, PREPARE = 1, 2, 4, 8
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

# 5000 proposals of one refused batch: proposal j is (timestamp 10 + j, id j, client j % 7 + 1)
_FULL = [(10 + j, j, j % 7 + 1) for j in range(5000)]

KAT_REPLY = [
    dict(name="refusal_keeps_the_client_only",
         # not the leader: each proposal is answered by its own handlePropose call
         kind=FALSE_, sends=[(-1, 0, NOT_LEADER, 0, 2)], meta=[(1000, 7, 3), (1001, 8, 4)],
         want=[(0, 0, -1, 3), (0, 0, -1, 4)], n_replies=2, n_slots=1, cs_flags=None),
    dict(name="refused_answers_the_first_of_5000",
         # :671-685: the batch was drained from ProposeChan, only `propose` is answered
         kind=FALSE_, sends=[(40, 5, REFUSED, 0, 5000)], meta=_FULL,
         want=[(0, 0, -1, 1)], n_replies=1, n_slots=1, cs_flags=None),
    dict(name="false_passes_over_installed_slots",
         # an installed batch sends no FALSE; the refused one after it answers its first (id 13)
         kind=FALSE_, sends=[(7, 1, ACCEPT, 0, 2), (8, 1, REFUSED, 2, 2), (-1, 0, NOT_LEADER, 4, 1)],
         meta=[(1, 11, 0), (2, 12, 0), (3, 13, 5), (4, 14, 6), (5, 15, 7)],
         want=[(0, 0, -1, 5), (0, 0, -1, 7)], n_replies=2, n_slots=2, cs_flags=None),
    dict(name="slot_of_zero_commands",
         # len(inst.Cmds) == 0: the loop body never runs, the instance still commits
         kind=DECIDED, sends=[(3, 2, ACCEPT, 0, 1), (4, 2, ACCEPT, 1, 0), (5, 2, ACCEPT, 1, 1)],
         meta=[(100, 1, 9), (101, 2, 8)],
         want=[(0, 100, 1, 9), (0, 101, 2, 8)], n_replies=2, n_slots=3, cs_flags=[1, 1, 1]),
    dict(name="decided_beside_undecided",
         # instance 21 crossed the majority this turn, 20 and 22 did not
         kind=DECIDED, inst_base=20, mask=[0, 1, 0],
         sends=[(20, 6, ACCEPT, 0, 2), (21, 6, ACCEPT, 2, 2), (22, 6, ACCEPT, 4, 1)],
         meta=[(1, 1, 0), (2, 2, 0), (3, 3, 1), (4, 4, 2), (5, 5, 0)],
         want=[(0, 3, 3, 1), (0, 4, 4, 2)], n_replies=2, n_slots=1, cs_flags=[0, 1, 0]),
    dict(name="prepare_slot_decided_later",
         # CLASSIC installed it PREPARING (MPX_PH_PREPARE); once prepared and accepted it commits
         # like any other: the slot is kept from the earlier turn, mask byte 0x80 counts as set
         kind=DECIDED, inst_base=-2, mask=[0x80],
         sends=[(-2, 3, PREPARE, 0, 2)], meta=[(50, -5, 2), (51, -6, 2)],
         want=[(0, 50, -5, 2), (0, 51, -6, 2)], n_replies=2, n_slots=1, cs_flags=[1]),
    dict(name="decided_passes_over_refusals",
         kind=DECIDED, sends=[(-1, 0, NOT_LEADER, 0, 2), (9, 4, REFUSED, 2, 1), (10, 4, ACCEPT, 3, 1)],
         meta=[(1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 4, 3)],
         want=[(0, 4, 4, 3)], n_replies=1, n_slots=1, cs_flags=[0, 0, 1]),
    dict(name="executed_takes_ret_at_first_cmd",
         kind=EXECUTED, sends=[(0, 1, ACCEPT, 1, 2)], meta=[(9, 9, 9), (10, 1, 4), (11, 2, 5)],
         ret=[700, 701, 702],
         want=[(701, 10, 1, 4), (702, 11, 2, 5)], n_replies=2, n_slots=1, cs_flags=[1]),
    dict(name="ret_first_differs_from_first_cmd",
         # the apply ran over gathered commands: slot 0's results start at 3, slot 1's at 0
         kind=EXECUTED, sends=[(0, 1, ACCEPT, 0, 2), (1, 1, ACCEPT, 2, 3)],
         meta=[(1, 1, 0), (2, 2, 1), (3, 3, 2), (4, 4, 3), (5, 5, 4)],
         ret=[30, 31, 32, 10, 11], ret_first=[3, 0],
         want=[(10, 1, 1, 0), (11, 2, 2, 1), (30, 3, 3, 2), (31, 4, 4, 3), (32, 5, 5, 4)],
         n_replies=5, n_slots=2, cs_flags=[1, 1]),
    dict(name="extreme_field_values",
         kind=EXECUTED, inst_base=I32_MAX - 1, mask=[1, 1],
         sends=[(I32_MAX, I32_MAX, ACCEPT, 0, 2), (I32_MAX - 1, I32_MIN, ACCEPT, 2, 1)],
         meta=[(I64_MIN, I32_MIN, 0xFFFFFFFE), (I64_MAX, I32_MAX, 0), (-1, -1, 1)],
         ret=[I64_MAX, I64_MIN, -1],
         want=[(I64_MAX, I64_MIN, I32_MIN, 0xFFFFFFFE), (I64_MIN, I64_MAX, I32_MAX, 0), (-1, -1, -1, 1)],
         n_replies=3, n_slots=2, cs_flags=[1, 1]),
    dict(name="cap_short",
         # five replies, room for three: the counts stay complete
         kind=DECIDED, sends=[(0, 1, ACCEPT, 0, 2), (1, 1, ACCEPT, 2, 3)],
         meta=[(1, 1, 0), (2, 2, 1), (3, 3, 2), (4, 4, 3), (5, 5, 4)], cap=3,
         want=[(0, 1, 1, 0), (0, 2, 2, 1), (0, 3, 3, 2)], n_replies=5, n_slots=2, cs_flags=[1, 1]),
    dict(name="pad_tail",
         # two replies in a capacity of five: three pad records on client 9
         kind=DECIDED, sends=[(0, 1, ACCEPT, 0, 2)], meta=[(1, 1, 0), (2, 2, 1)], cap=5,
         pad_client=9,
         want=[(0, 1, 1, 0), (0, 2, 2, 1), (0, 0, 0, 9), (0, 0, 0, 9), (0, 0, 0, 9)],
         n_replies=2, n_slots=1, cs_flags=[1]),
    dict(name="pad_with_nothing_to_pad",
         # the capacity is already short: no pad record, no reply past it
         kind=FALSE_, sends=[(-1, 0, NOT_LEADER, 0, 3)], meta=[(1, 1, 4), (2, 2, 5), (3, 3, 6)],
         cap=2, pad_client=7,
         want=[(0, 0, -1, 4), (0, 0, -1, 5)], n_replies=3, n_slots=1, cs_flags=None),
]


def kat_args(case):
    """the case as keyword arguments of reply_translit.build_replies / Engine.build_replies"""
    import numpy as np

    import reply_translit as T
    a = dict(kind=case["kind"], sends=T.mk_sends(case["sends"]), meta=T.mk_meta(case["meta"]),
             inst_base=case.get("inst_base", 0))
    if "mask" in case:
        a["mask"] = np.array(case["mask"], np.uint8)
    if "ret" in case:
        a["ret"] = np.array(case["ret"], np.int64)
    if "ret_first" in case:
        a["ret_first"] = np.array(case["ret_first"], np.uint64)
    for k in ("cap", "pad_client"):
        if k in case:
            a[k] = case[k]
    return a

"""Hand-traced answers of store assembly (mpx_store_commands, mpx_store_compact): small calls whose
results were worked out by hand from the Go's assignments (tests/store_translit.py cites them), for
the CPU check of the transliteration and the GPU check of the engine.

TEST INFRASTRUCTURE. Source s holds commands j = 0, 1, ... with key 100 * (s + 1) + j, val = -key,
op = 1 + j % 3; the arena before the call holds key 300 + j, val = -key, op = 9. The window starts at
instance 10. A case names what the call appends ("tail": the keys, in order), the slots it writes
("slots": window index -> (first_cmd, n_cmds)), the cursor it leaves and its result record
(n_stored, n_cmds, n_superseded, flags)."""
import numpy as np

import store_translit as T
from minpaxos_amd import records as R

BASE = 10
ST, RP = R.AH_STORED, R.AH_REPLIED
KEEP = R.VALUE_KEEP


def _cmds(first_key, n, op=None):
    key = first_key + np.arange(n, dtype=np.int64)
    return ((1 + np.arange(n) % 3).astype(np.uint8) if op is None else np.full(n, op, np.uint8), key, -key)


def source(s, sizes, n_recs=None, extra=0):
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.uint64)
    op, key, val = _cmds(100 * (s + 1), int(off[-1]) + extra)
    return dict(cmd_off=off, op=op, key=key, val=val, n_recs=len(sizes) if n_recs is None else n_recs)


def window(n, rows=None):
    inst = np.zeros(n, R.INST_CMDS)
    for rel, (first, k, flags) in (rows or {}).items():
        inst[rel] = (first, k, flags)
    return inst


def msgs_case(name, msgs, effect, sources, want, used=0, cap=8, rows=None, perm=None, handler="accept",
              n_inst=4):
    return dict(name=name, kind=R.SC_MSGS, items=T.mk_msgs(msgs), effect=np.array(effect, np.uint8),
                sources=sources, used=used, cap=cap, inst=window(n_inst, rows),
                perm=None if perm is None else np.array(perm, np.uint32), handler=handler, want=want)


H = R.IC_HAS_CMDS
KAT_STORE = [
    msgs_case("one_accept", [(11, 0)], [ST | RP], [source(0, [2])],
              dict(tail=[100, 101], slots={1: (0, 2)}, used=2, res=(1, 2, 0, 0))),
    msgs_case("two_accepts_of_one_instance_the_second_wins", [(11, 0), (11, 1)], [ST | RP, ST | RP],
              [source(0, [2, 3])], dict(tail=[102, 103, 104], slots={1: (0, 3)}, used=3, res=(1, 3, 1, 0))),
    msgs_case("a_storing_item_then_a_non_storing_one_the_first_wins", [(11, 0), (11, 1)], [ST | RP, RP],
              [source(0, [2, 3])], dict(tail=[100, 101], slots={1: (0, 2)}, used=2, res=(1, 2, 0, 0))),
    msgs_case("an_ignored_resend", [(11, 0)], [0], [source(0, [2])],
              dict(tail=[], slots={}, used=6, res=(0, 0, 0, 0)), used=6, rows={1: (5, 1, H)}),
    msgs_case("a_commit_over_an_accepted_slot", [(11, 0)], [R.CH_CMDS], [source(0, [3])],
              dict(tail=[100, 101, 102], slots={1: (2, 3)}, used=5, res=(1, 3, 0, 0)), used=2,
              rows={1: (0, 2, H)}, handler="commit"),
    msgs_case("commit_shorts_on_a_nil_and_on_a_full_slot", [(10, KEEP), (11, KEEP), (12, KEEP)],
              [R.CH_INSTALLED, 0, R.CH_CMDS], [source(0, [2], n_recs=3)],
              dict(tail=[], slots={}, used=2, res=(0, 0, 0, 0)), used=2, rows={1: (0, 2, H)},
              handler="commit"),
    msgs_case("a_zero_command_accept", [(12, 0)], [ST], [source(0, [0])],
              dict(tail=[], slots={2: (3, 0)}, used=3, res=(1, 0, 0, 0)), used=3),
    msgs_case("two_sources_with_colliding_value_ids_through_perm", [(10, 0), (11, 0), (12, 1)],
              [ST, ST, ST], [source(0, [1, 2]), source(1, [3, 1])],
              dict(tail=[200, 201, 202, 100, 203], slots={0: (0, 3), 1: (3, 1), 2: (4, 1)}, used=5,
                   res=(3, 5, 0, 0)), perm=[2, 0, 3]),
    dict(name="sends_with_a_not_leader_and_a_refused_slot_between_two_accepts", kind=R.SC_SENDS,
         items=T.mk_sends([(10, R.PH_ACCEPT, 0, 2), (-1, R.PH_NOT_LEADER, 2, 1), (11, R.PH_REFUSED, 3, 2),
                           (12, R.PH_ACCEPT, 5, 1)]),
         effect=None, perm=None, handler="accept", used=0, cap=8, inst=window(4),
         sources=[dict(zip(("op", "key", "val"), _cmds(100, 7)), cmd_off=None, n_recs=4)],
         want=dict(tail=[100, 101, 105], slots={0: (0, 2), 2: (2, 1)}, used=3, res=(2, 3, 0, 0))),
    msgs_case("the_arena_short_by_one_command", [(11, 0), (11, 1)], [ST, ST], [source(0, [2, 3])],
              dict(tail=[], slots={}, used=2, res=(1, 3, 1, R.SC_FULL)), used=2, cap=4, rows={1: (0, 2, H)}),
    msgs_case("the_arena_exactly_full", [(11, 0), (11, 1)], [ST, ST], [source(0, [2, 3])],
              dict(tail=[102, 103, 104], slots={1: (2, 3)}, used=5, res=(1, 3, 1, 0)), used=2, cap=5,
              rows={1: (0, 2, H)}),
]

# compaction with a retired slot in the middle: its commands (arena 3, 4) are left behind
KAT_COMPACT = dict(name="compaction_with_a_retired_slot_in_the_middle",
                   inst=window(4, {0: (1, 2, H), 1: (3, 2, 0), 2: (5, 1, H), 3: (0, 1, H)}), used=6, cap=8,
                   to_cap=4, want=dict(keys=[301, 302, 305, 300], used=4, res=(3, 4, 0, 0),
                                       inst=[(0, 2, H), (3, 2, 0), (2, 1, H), (3, 1, H)]))


def arena(cap):
    return _cmds(300, cap, op=9)


def kat_args(case):
    """the arguments of store_translit.store_commands for a case"""
    return dict(kind=case["kind"], items=case["items"], sources=case["sources"], arena=arena(case["cap"]),
                used=case["used"], inst=case["inst"], inst_base=BASE, effect=case["effect"],
                perm=case["perm"], handler=case["handler"])


def check(case, got):
    """got: the outputs of the transliteration or of the engine (op, key, val, used, inst, res)"""
    w = case["want"]
    a_op, a_key, a_val = arena(case["cap"])
    u0, k = case["used"], len(w["tail"])
    a_key[u0:u0 + k] = w["tail"]
    a_val[u0:u0 + k] = -a_key[u0:u0 + k]
    a_op[u0:u0 + k] = [1 + (x % 100) % 3 for x in w["tail"]]
    assert np.array_equal(got["key"], a_key), (case["name"], got["key"])
    assert np.array_equal(got["val"], a_val) and np.array_equal(got["op"], a_op), case["name"]
    inst = case["inst"].copy()
    for rel, (first, n) in w["slots"].items():
        inst[rel] = (first, n, H)
    assert got["inst"].tobytes() == inst.tobytes(), (case["name"], got["inst"])
    assert int(got["used"]) == w["used"], (case["name"], got["used"])
    assert tuple(int(got["res"][f]) for f in R.STORE_RESULT.names) == w["res"], (case["name"], got["res"])


def check_compact(got):
    c, w = KAT_COMPACT, KAT_COMPACT["want"]
    k = len(w["keys"])
    assert got["key"][:k].tolist() == w["keys"] and got["val"][:k].tolist() == [-x for x in w["keys"]]
    assert got["op"][:k].tolist() == [9] * k
    assert not got["key"][k:].any() and not got["op"][k:].any()
    assert [tuple(int(v) for v in x) for x in got["inst"]] == w["inst"]
    assert int(got["used"]) == w["used"]
    assert tuple(int(got["res"][f]) for f in R.STORE_RESULT.names) == w["res"]
    assert c["to_cap"] == k

"""CPU tests of tests/unmarshal_translit.py, the restatement the unmarshal GPU tests compare
against: hand-traced known answers (the bytes are literals, the expected fields were worked out
from the Go text), the inverse property against every Marshal restatement the suite has, and the
reach of the fuzz generator."""
import numpy as np
import pytest

import proposer_translit as P
import unmarshal_translit as U
from minpaxos_amd import records as R
from minpaxos_amd import wire as W

MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
ACCEPT, COMMIT, PREPARE_REPLY = R.PEER_ACCEPT, R.PEER_COMMIT, R.PEER_PREPARE_REPLY

# one state.Command: Op u8, K i64, V i64
C123 = "01 0200000000000000 0300000000000000"   # PUT 2 3
CNEG = "02 ffffffffffffffff feffffffffffffff"   # GET -1 -2
T123, TNEG = (1, 2, 3), (2, -1, -2)

# (name, mode, bytes, offset of the frame, code, message)
KNOWN = [
    ("min_accept_one_command_empty_log", MIN,
     "09 01000000 05000000 21000000 04000000 02" + C123 + "00", 0, ACCEPT,
     dict(LeaderId=1, Instance=5, Ballot=33, LastCommitted=4, Command=[T123], CatchUpLog=[])),
    ("min_accept_empty_command_log_instance_of_0_commands", MIN,
     "09 02000000 07000000 12000000 06000000 00 02 12000000 03000000 00", 0, ACCEPT,
     dict(LeaderId=2, Instance=7, Ballot=18, LastCommitted=6, Command=[],
          CatchUpLog=[(18, 3, [])])),
    ("min_accept_log_of_two_negative_key_and_value", MIN,
     "09 00000000 0a000000 10000000 09000000 02" + C123 + "04 10000000 03000000 02" + CNEG +
     "10000000 02000000 00", 0, ACCEPT,
     dict(LeaderId=0, Instance=10, Ballot=16, LastCommitted=9, Command=[T123],
          CatchUpLog=[(16, 3, [TNEG]), (16, 2, [])])),
    ("min_commit_two_commands", MIN,
     "0a 00000000 03000000 10000000 04" + C123 + CNEG, 0, COMMIT,
     dict(LeaderId=0, Instance=3, Ballot=16, Command=[T123, TNEG])),
    ("min_prepare_reply_command_and_log", MIN,
     "0c 03000000 04000000 01 31000000 03000000 02" + C123 + "02 31000000 03000000 02" + C123, 0,
     PREPARE_REPLY,
     dict(Id=3, Instance=4, OK=1, Ballot=49, LastCommitted=3, Command=[T123],
          CatchUpLog=[(49, 3, [T123])])),
    ("min_prepare_reply_empty", MIN,
     "0c 01000000 00000000 00 ffffffff ffffffff 00 00", 0, PREPARE_REPLY,
     dict(Id=1, Instance=0, OK=0, Ballot=-1, LastCommitted=-1, Command=[], CatchUpLog=[])),
    ("classic_accept_one_command", CLASSIC,
     "09 01000000 05000000 21000000 02" + C123, 0, ACCEPT,
     dict(LeaderId=1, Instance=5, Ballot=33, Command=[T123])),
    ("classic_accept_empty_command_extreme_fields", CLASSIC,
     "09 04000000 ffffffff 00000080 00", 0, ACCEPT,
     dict(LeaderId=4, Instance=-1, Ballot=-(1 << 31), Command=[])),
    ("classic_commit_negative_key_and_value", CLASSIC,
     "0a ffffffff 02000000 11000000 02" + CNEG, 0, COMMIT,
     dict(LeaderId=-1, Instance=2, Ballot=17, Command=[TNEG])),
    ("classic_prepare_reply_two_commands", CLASSIC,
     "0c 09000000 01 22000000 04" + CNEG + C123, 0, PREPARE_REPLY,
     dict(Instance=9, OK=1, Ballot=34, Command=[TNEG, T123])),
    ("classic_prepare_reply_empty", CLASSIC,
     "0c 00000000 00 ffffffff 00", 0, PREPARE_REPLY,
     dict(Instance=0, OK=0, Ballot=-1, Command=[])),
    # PutVarint(64) = zig-zag 128 = 0x80 0x01: the first two-byte length
    ("min_accept_64_commands", MIN,
     "09 01000000 05000000 21000000 04000000 8001" + C123 * 64 + "00", 0, ACCEPT,
     dict(LeaderId=1, Instance=5, Ballot=33, LastCommitted=4, Command=[T123] * 64,
          CatchUpLog=[])),
    ("min_accept_log_instance_of_64_commands", MIN,
     "09 01000000 05000000 21000000 04000000 00 02 10000000 03000000 8001" + CNEG * 64, 0, ACCEPT,
     dict(LeaderId=1, Instance=5, Ballot=33, LastCommitted=4, Command=[],
          CatchUpLog=[(16, 3, [TNEG] * 64)])),
    ("classic_commit_64_commands", CLASSIC,
     "0a 00000000 01000000 10000000 8001" + C123 * 64, 0, COMMIT,
     dict(LeaderId=0, Instance=1, Ballot=16, Command=[T123] * 64)),
    # behind a 14-byte MIN AcceptReply: the frame's offset is not 0
    ("min_commit_behind_an_accept_reply", MIN,
     "0d 01000000 01 10000000 02000000" + "0a 00000000 03000000 10000000 02" + CNEG, 14, COMMIT,
     dict(LeaderId=0, Instance=3, Ballot=16, Command=[TNEG])),
]
KNOWN_IDS = [k[0] for k in KNOWN]


def known_bytes(k):
    return bytes.fromhex(k[2])


@pytest.mark.parametrize("k", KNOWN, ids=KNOWN_IDS)
def test_known_answers(k):
    _, mode, _, offset, code, want = k
    buf = known_bytes(k)
    got_code, got, end = U.unmarshal(mode, buf, offset)
    assert got_code == code and got == want and end == len(buf)


def test_known_answers_cover_the_listed_cases():
    assert len(KNOWN) >= 12
    modes = {(k[1], k[4]) for k in KNOWN}
    assert modes == {(m, c) for m in (MIN, CLASSIC) for c in (ACCEPT, COMMIT, PREPARE_REPLY)}
    msgs = [k[5] for k in KNOWN]
    assert any(m["Command"] == [] for m in msgs)
    assert any(any(ic[2] == [] for ic in m.get("CatchUpLog", [])) for m in msgs)
    assert any(len(m["Command"]) == 64 for m in msgs)
    assert any(any(len(ic[2]) == 64 for ic in m.get("CatchUpLog", [])) for m in msgs)
    assert any(c[1] < 0 and c[2] < 0 for m in msgs for c in m["Command"])


def test_known_var_frame_and_flattened_arrays():
    """the first five MIN answers as one stream: the frame record of the third, and the ABI's
    arrays of all five, written out by hand"""
    buf = b"".join(known_bytes(k) for k in KNOWN[:5])
    third = sum(len(known_bytes(k)) for k in KNOWN[:2])
    rec, code, _ = U.var_frame(MIN, buf, third)
    # 1 + 16 + V(1) + 17 + V(2) + (8 + V(1) + 17) + (8 + V(0)) = 71 bytes
    assert rec[:7] == (third, 71, 1, third + 18, 2, third + 36, ACCEPT) and code == ACCEPT
    var, msgs = U.walk(MIN, buf)
    assert len(var) == 5 and int(var["offset"][2]) == third
    a, n = U.flatten(MIN, msgs)
    assert a["accepts"].tolist() == [(5, 33, 1, 0), (7, 18, 2, 1), (10, 16, 0, 2)]
    assert a["accept_last_committed"].tolist() == [4, 6, 9]
    assert a["commits"].tolist() == [(3, 16, 0, 3)]
    assert a["cmd_off"].tolist() == [0, 1, 1, 2, 4, 5]
    assert a["op"].tolist() == [1, 1, 1, 2, 1]
    assert a["key"].tolist() == [2, 2, 2, -1, 2] and a["val"].tolist() == [3, 3, 3, -2, 3]
    assert a["log_inst_off"].tolist() == [0, 0, 1, 3, 3, 4]
    # inst_no = LastCommitted - m + 1 + j
    assert a["log_recs"].tolist() == [(18, 3, 6, 0), (16, 3, 8, 0), (16, 2, 9, 0), (49, 3, 3, 0)]
    assert a["log_cmd_off"].tolist() == [0, 0, 1, 1, 2]
    assert a["log_op"].tolist() == [2, 1] and a["log_key"].tolist() == [-1, 2]
    assert a["log_val"].tolist() == [-2, 3]
    assert n == dict(n_accepts=3, n_commits=1, n_cmds=5, n_log_inst=4, n_log_cmds=2, n_var=5)
    assert all(a[name].dtype == want for name, want in
               (("accepts", R.ACCEPT_MSG), ("log_recs", R.LOG_REC), ("cmd_off", np.uint64),
                ("op", np.uint8), ("key", np.int64), ("accept_last_committed", np.int32)))
    c, _ = U.flatten(CLASSIC, [(k[4], k[5]) for k in KNOWN[6:11]])
    assert c["accept_last_committed"].tolist() == [-1, -1] and len(c["log_recs"]) == 0
    assert c["log_inst_off"].tolist() == [0] * 6 and c["log_cmd_off"].tolist() == [0]


@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_unmarshal_inverts_the_wire_builders(mode):
    rng = np.random.default_rng(3)
    for _ in range(60):
        cmds = [(int(rng.integers(0, 6)), int(rng.integers(-(1 << 63), 1 << 63)),
                 int(rng.integers(-(1 << 63), 1 << 63)))
                for _ in range(int(rng.integers(0, 5)) * int(rng.integers(1, 20)))]
        log = [(int(rng.integers(-5, 99)), int(rng.integers(0, 4)), cmds[:int(rng.integers(0, 3))])
               for _ in range(int(rng.integers(0, 4)))] if mode == MIN else []
        f = [int(x) for x in rng.integers(-(1 << 31), 1 << 31, 5)]
        ok = int(rng.integers(0, 2))
        pad = bytes(int(rng.integers(0, 20)))  # the frame's offset moves
        code, m, end = U.unmarshal(mode, pad + W.accept(mode, f[0], f[1], f[2], cmds, f[3], log),
                                   len(pad))
        want = dict(LeaderId=f[0], Instance=f[1], Ballot=f[2], Command=cmds)
        if mode == MIN:
            want.update(LastCommitted=f[3], CatchUpLog=log)
        assert (code, m) == (ACCEPT, want)
        code, m, _ = U.unmarshal(mode, pad + W.commit(f[0], f[1], f[2], cmds), len(pad))
        assert (code, m) == (COMMIT, dict(LeaderId=f[0], Instance=f[1], Ballot=f[2], Command=cmds))
        code, m, _ = U.unmarshal(
            mode, pad + W.prepare_reply(mode, f[1], ok, f[2], cmds, f[4], f[3], log), len(pad))
        want = dict(Instance=f[1], OK=ok, Ballot=f[2], Command=cmds)
        if mode == MIN:
            want.update(Id=f[4], LastCommitted=f[3], CatchUpLog=log)
        assert (code, m) == (PREPARE_REPLY, want)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_unmarshal_inverts_bcast_accept(mode, seed):
    """every frame proposer_translit's bcastAccept writes comes back as the send's fields, its
    commands and the catch-up range of the log the sender was given"""
    N = 5
    a = P.fuzz_encode(seed, N, mode)
    _, off, per = P.encode_accepts(mode, N, want_frames=True, **a)
    sends = {int(s["instance"]): s for s in a["sends"] if int(s["flags"]) & R.PH_ACCEPT}
    op, key, val = a["cmds"]
    lrec, lcoff, lop, lkey, lval = a["log"]
    seen = 0
    for q in range(N):
        for frame in per[q]:
            code, m, end = U.unmarshal(mode, frame, 0)
            assert code == ACCEPT and end == len(frame)
            s = sends[m["Instance"]]
            g = (m["Instance"] - a["inst_base"]) // a["ipg"]
            c0 = int(s["first_cmd"])
            assert m["LeaderId"] == int(a["groups"][g]["self_id"])
            assert m["Ballot"] == int(s["ballot"])
            assert m["Command"] == [(int(op[j]), int(key[j]), int(val[j]))
                                    for j in range(c0, c0 + int(s["n_cmds"]))]
            if mode == MIN:
                lc = int(s["last_committed"])
                assert m["LastCommitted"] == lc
                lo = lc - len(m["CatchUpLog"]) + 1 - a["inst_base"]  # window index of record 0
                for j, (ballot, status, ic) in enumerate(m["CatchUpLog"]):
                    k = lo + j
                    assert (ballot, status) == (int(lrec[k]["ballot"]), int(lrec[k]["status"]))
                    assert ic == [(int(lop[x]), int(lkey[x]), int(lval[x]))
                                  for x in range(int(lcoff[k]), int(lcoff[k + 1]))]
                assert frame[1:] == P.accept_marshal_min(m["LeaderId"], m["Instance"], m["Ballot"],
                                                         lc, m["Command"], m["CatchUpLog"])
            else:
                assert frame[1:] == P.accept_marshal_classic(m["LeaderId"], m["Instance"],
                                                             m["Ballot"], m["Command"])
            seen += 1
    assert seen > 0


@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_fuzz_generator_reach(mode):
    """conditions on the generator (not measurements): of all variable-length frames over the
    seeds, each property the GPU fuzz relies on occurs in at least 2 %"""
    tot = None
    for seed in U.FUZZ_SEEDS:
        buf, st = U.fuzz_stream(seed, mode)
        var, msgs = U.walk(mode, buf)
        assert len(var) == st["frames"] and len(var) < len(buf) // 13
        tot = st if tot is None else {k: tot[k] + st[k] for k in st}
    n = tot["frames"]
    assert n >= 24 * 60
    want = ["empty_command", "varint2", "commit", "prepare_reply"]
    if mode == MIN:
        want += ["log", "log2"]
    else:
        assert tot["log"] == 0
    for k in want:
        assert tot[k] / n >= 0.02, (k, tot[k], n)

"""The Unmarshals of the variable-length peer messages, transliterated line by line from the Go
reference (the single restatement the unmarshal tests compare against).

  Accept.Unmarshal        MIN      src/minpaxosproto/minpaxosprotomarsh.go:470-507
                          CLASSIC  src/paxosproto/paxosprotomarsh.go:244-268
  Commit.Unmarshal        MIN      src/minpaxosproto/minpaxosprotomarsh.go:648-672
                          CLASSIC  src/paxosproto/paxosprotomarsh.go:403-430
  PrepareReply.Unmarshal  MIN      src/minpaxosproto/minpaxosprotomarsh.go:352-387
                          CLASSIC  src/paxosproto/paxosprotomarsh.go:152-176
  Instance.Unmarshal      src/minpaxosproto/minpaxosprotomarsh.go:126-153
  Command.Unmarshal       src/state/statemarsh.go:21-39
  binary.ReadVarint       encoding/binary

unmarshal(mode, buf, offset) reads the frame whose code byte is at `offset` (replicaListener has
consumed the code byte, genericsmr.go:402-446) and returns Python structures; flatten() lays a
list of them out as the arrays of mpx_unmarshal_out, in the order the frames were given.
"""
import struct

import numpy as np

from minpaxos_amd import records as R
from minpaxos_amd import wire as W

MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
ACCEPT, COMMIT, PREPARE_REPLY = R.PEER_ACCEPT, R.PEER_COMMIT, R.PEER_PREPARE_REPLY


class Wire:
    """the byteReader the Unmarshals read from"""

    def __init__(self, buf, pos):
        self.buf, self.pos = bytes(buf), pos

    def read(self, n):                                   # io.ReadAtLeast / io.ReadFull
        if self.pos + n > len(self.buf):
            raise EOFError("unexpected EOF")
        bs = self.buf[self.pos:self.pos + n]
        self.pos += n
        return bs


def i32(bs, at):
    """int32(uint32(bs[at]) | uint32(bs[at+1]) << 8 | ...)"""
    u = bs[at] | (bs[at + 1] << 8) | (bs[at + 2] << 16) | (bs[at + 3] << 24)
    return u - (1 << 32) if u >= 1 << 31 else u


def read_varint(wire):
    """encoding/binary.ReadVarint: ReadUvarint, then the zig-zag"""
    x, s = 0, 0
    for i in range(10):
        b = wire.read(1)[0]
        if b < 0x80:
            if i == 9 and b > 1:
                raise OverflowError("binary: varint overflows a 64-bit integer")
            ux = x | (b << s)
            v = ux >> 1
            if ux & 1:
                v = ~v
            return v
        x |= (b & 0x7F) << s
        s += 7
    raise OverflowError("binary: varint overflows a 64-bit integer")


def command_unmarshal(wire):                             # statemarsh.go:21-39
    op = wire.read(1)[0]                                 # :24-28
    k = struct.unpack("<q", wire.read(8))[0]             # :29-33
    v = struct.unpack("<q", wire.read(8))[0]             # :34-37
    return (op, k, v)


def commands_unmarshal(wire):
    alen1 = read_varint(wire)
    if alen1 < 0:
        raise ValueError("makeslice: len out of range")
    return [command_unmarshal(wire) for _ in range(alen1)]


def instance_unmarshal(wire):                            # minpaxosprotomarsh.go:126-153
    bs = wire.read(8)                                    # :135-138
    ballot = i32(bs, 0)                                  # :140
    status = i32(bs, 4)                                  # :141
    cmds = commands_unmarshal(wire)                      # :144-151
    return (ballot, status, cmds)


def catchup_unmarshal(wire):
    alen2 = read_varint(wire)
    if alen2 < 0:
        raise ValueError("makeslice: len out of range")
    return [instance_unmarshal(wire) for _ in range(alen2)]


def accept_unmarshal(mode, wire):
    if mode == MIN:                                      # minpaxosprotomarsh.go:470-507
        bs = wire.read(16)                               # :479-481
        m = dict(LeaderId=i32(bs, 0), Instance=i32(bs, 4), Ballot=i32(bs, 8),
                 LastCommitted=i32(bs, 12))              # :482-485
        m["Command"] = commands_unmarshal(wire)          # :487-495
        m["CatchUpLog"] = catchup_unmarshal(wire)        # :497-505
        return m
    bs = wire.read(12)                                   # paxosprotomarsh.go:244-268
    m = dict(LeaderId=i32(bs, 0), Instance=i32(bs, 4), Ballot=i32(bs, 8))
    m["Command"] = commands_unmarshal(wire)
    return m


def commit_unmarshal(mode, wire):
    """minpaxosprotomarsh.go:648-672 / paxosprotomarsh.go:403-430: the same twelve bytes"""
    bs = wire.read(12)
    m = dict(LeaderId=i32(bs, 0), Instance=i32(bs, 4), Ballot=i32(bs, 8))
    m["Command"] = commands_unmarshal(wire)
    return m


def prepare_reply_unmarshal(mode, wire):
    if mode == MIN:                                      # minpaxosprotomarsh.go:352-387
        bs = wire.read(17)                               # :360-362
        m = dict(Id=i32(bs, 0), Instance=i32(bs, 4), OK=bs[8], Ballot=i32(bs, 9),
                 LastCommitted=i32(bs, 13))              # :363-367
        m["Command"] = commands_unmarshal(wire)          # :368-376
        m["CatchUpLog"] = catchup_unmarshal(wire)        # :377-385
        return m
    bs = wire.read(9)                                    # paxosprotomarsh.go:152-176
    m = dict(Instance=i32(bs, 0), OK=bs[4], Ballot=i32(bs, 5))
    m["Command"] = commands_unmarshal(wire)
    return m


UNMARSHAL = {ACCEPT: accept_unmarshal, COMMIT: commit_unmarshal,
             PREPARE_REPLY: prepare_reply_unmarshal}


def unmarshal(mode, buf, offset=0):
    """the frame at buf[offset]: returns (code, message, end)"""
    code = buf[offset]
    wire = Wire(buf, offset + 1)
    return code, UNMARSHAL[code](mode, wire), wire.pos


# ---- frames --------------------------------------------------------------------------------------
def varint_len_at(buf, pos):
    k = 0
    while buf[pos + k] >= 0x80:
        k += 1
    return k + 1


def var_frame(mode, buf, offset):
    """the mpx_var_frame mpx_decode_stream leaves for the frame at `offset`, worked out from the
    message: returns (record tuple, code, message)"""
    code, m, end = unmarshal(mode, buf, offset)
    cmds_off = offset + R.VAR_HEADER[mode][code]
    cmds_off += varint_len_at(buf, cmds_off)
    n = len(m["Command"])
    log = m.get("CatchUpLog")
    log_off = cmds_off + 17 * n
    if log is not None:
        log_off += varint_len_at(buf, log_off)
    rec = (offset, end - offset, n, cmds_off, len(log or ()), log_off, code, (0,) * 7)
    return rec, code, m


def walk(mode, buf):
    """replicaListener's framing over a whole buffer (fixed-size frames skipped). Returns (var
    VAR_FRAME[], [(code, message)])"""
    body = R.PEER_BODY if mode == MIN else R.PEER_BODY_CLASSIC
    pos, recs, msgs = 0, [], []
    while pos < len(buf):
        code = buf[pos]
        if code in UNMARSHAL:
            rec, _, m = var_frame(mode, buf, pos)
            recs.append(rec)
            msgs.append((code, m))
            pos += rec[1]
        else:
            pos += 1 + (body.get(code) or 0)
    assert pos == len(buf)
    var = np.array(recs, dtype=R.VAR_FRAME) if recs else np.zeros(0, R.VAR_FRAME)
    return var, msgs


def wrap32(x):
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def flatten(mode, msgs):
    """[(code, message)] in var order -> (dict of R.UNMARSHAL_ARRAYS, counts dict)"""
    acc, alc, com = [], [], []
    cmd_off, log_inst_off, log_cmd_off = [0], [0], [0]
    cmds, lrec, lcmds = [], [], []
    for i, (code, m) in enumerate(msgs):
        if code == ACCEPT:
            acc.append((m["Instance"], m["Ballot"], m["LeaderId"], i))
            alc.append(m["LastCommitted"] if mode == MIN else -1)
        elif code == COMMIT:
            com.append((m["Instance"], m["Ballot"], m["LeaderId"], i))
        cmds += m["Command"]
        cmd_off.append(len(cmds))
        log = m.get("CatchUpLog", [])
        for j, (ballot, status, ic) in enumerate(log):
            # the sender's range ends at LastCommitted (bareminpaxos.go:496-506, :743)
            lrec.append((ballot, status, wrap32(m["LastCommitted"] - len(log) + 1 + j), 0))
            lcmds += ic
            log_cmd_off.append(len(lcmds))
        log_inst_off.append(len(lrec))

    def soa(c):
        return (np.array([x[0] for x in c], np.uint8), np.array([x[1] for x in c], np.int64),
                np.array([x[2] for x in c], np.int64))
    op, key, val = soa(cmds)
    lop, lkey, lval = soa(lcmds)
    a = {"accepts": np.array(acc, R.ACCEPT_MSG) if acc else np.zeros(0, R.ACCEPT_MSG),
         "accept_last_committed": np.array(alc, np.int32),
         "commits": np.array(com, R.ACCEPT_MSG) if com else np.zeros(0, R.ACCEPT_MSG),
         "cmd_off": np.array(cmd_off, np.uint64), "op": op, "key": key, "val": val,
         "log_inst_off": np.array(log_inst_off, np.uint64),
         "log_recs": np.array(lrec, R.LOG_REC) if lrec else np.zeros(0, R.LOG_REC),
         "log_cmd_off": np.array(log_cmd_off, np.uint64), "log_op": lop, "log_key": lkey,
         "log_val": lval}
    counts = dict(n_accepts=len(acc), n_commits=len(com), n_cmds=len(cmds), n_log_inst=len(lrec),
                  n_log_cmds=len(lcmds), n_var=len(msgs))
    return a, counts


def expected(mode, buf, var):
    """what mpx_unmarshal_frames returns for the frames `var` of buf"""
    return flatten(mode, [unmarshal(mode, buf, int(v["offset"]))[:2] for v in var])


# ---- the fuzz generator --------------------------------------------------------------------------
FUZZ_SEEDS = list(range(24))


def fuzz_stream(seed, mode, n_frames=160):
    """a peer stream of Accepts, Commits and PrepareReplies with fixed-size frames between them.
    Returns (bytes, stats): stats counts, over the variable-length frames, the properties
    test_fuzz_generator_reach asserts."""
    rng = np.random.default_rng(9000 + seed)
    out = []
    stats = dict(frames=0, empty_command=0, log=0, log2=0, varint2=0, commit=0, prepare_reply=0)

    def i32r():
        return int(rng.integers(-(1 << 31), 1 << 31))

    def cmds(k):
        return [(int(rng.integers(0, 6)), int(rng.integers(-(1 << 63), 1 << 63)),
                 int(rng.integers(-(1 << 63), 1 << 63))) for _ in range(k)]

    def count():
        u = rng.random()
        return 0 if u < 0.15 else int(rng.integers(64, 90)) if u < 0.22 else int(rng.integers(1, 7))

    for _ in range(n_frames):
        u = rng.random()
        if u < 0.25:  # a fixed-size frame or an unknown code between the variable ones
            v = rng.random()
            if v < 0.6:
                out.append(W.accept_reply(mode, i32r(), int(rng.integers(0, 2)), i32r(), 1))
            elif v < 0.9:
                code = [R.PEER_BEACON, R.PEER_PREPARE, R.PEER_COMMIT_SHORT][int(rng.integers(0, 3))]
                out.append(W.fixed(mode, code, int(rng.integers(0, 1 << 62))))
            else:
                out.append(bytes([int(rng.integers(14, 256))]))
            continue
        n = count()
        log = []
        if mode == MIN and rng.random() < 0.5:
            m = int(rng.integers(1, 5)) if rng.random() < 0.9 else int(rng.integers(64, 70))
            log = [(i32r(), int(rng.integers(0, 4)), cmds(count() if m < 64 else 0))
                   for _ in range(m)]
        kind = rng.random()
        c = cmds(n)
        if kind < 0.6:
            out.append(W.accept(mode, i32r(), i32r(), i32r(), c, i32r(), log))
        elif kind < 0.8:
            log = []
            out.append(W.commit(i32r(), i32r(), i32r(), c))
            stats["commit"] += 1
        else:
            out.append(W.prepare_reply(mode, i32r(), int(rng.integers(0, 2)), i32r(), c,
                                       int(rng.integers(0, 5)), i32r(), log))
            stats["prepare_reply"] += 1
        stats["frames"] += 1
        stats["empty_command"] += n == 0
        stats["log"] += len(log) > 0
        stats["log2"] += len(log) >= 2
        stats["varint2"] += n >= 64 or len(log) >= 64 or any(len(x[2]) >= 64 for x in log)
    return b"".join(out), stats

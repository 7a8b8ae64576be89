"""numpy mirrors of the packed records in include/mpx.h.

Each dtype is byte-identical to its C struct, so arrays can be handed to the C ABI
(ctypes) or viewed as int32 words for device tensors.
"""
import numpy as np

# minpaxosproto.InstanceStatus  src/minpaxosproto/minpaxosproto.go:8-15
PREPARING, PREPARED, ACCEPTED, COMMITTED = 0, 1, 2, 3
STATUS_NIL = -1  # instanceSpace[i] == nil

# state.Operation  src/state/state.go:10-19
OP_NONE, OP_PUT, OP_GET, OP_DELETE, OP_RLOCK, OP_WLOCK = 0, 1, 2, 3, 4, 5

MODE_MIN, MODE_CLASSIC = 0, 1
MAX_REPLICAS = 16

# mpx_prep_state.flags
PF_HAS_PROPOSALS, PF_REQUEUED, PF_PREPARED_NOW = 1, 2, 4
# mpx_prepare_effect.flags
EF_COUNTED, EF_SELECTED, EF_CATCHUP, EF_TRIGGER = 1, 2, 4, 8

# error codes
OK = 0
E_INVAL, E_NOMEM, E_HIP, E_RCCL, E_NIL_INSTANCE, E_BAD_ID, E_KV_FULL, E_NODEV, E_UNSUPPORTED = (
    -1, -2, -3, -4, -5, -6, -7, -8, -9)
ERROR_NAMES = {
    0: "OK", -1: "E_INVAL", -2: "E_NOMEM", -3: "E_HIP", -4: "E_RCCL", -5: "E_NIL_INSTANCE",
    -6: "E_BAD_ID", -7: "E_KV_FULL", -8: "E_NODEV", -9: "E_UNSUPPORTED",
}

# mpx_accept_reply  <- minpaxosproto.AcceptReply{Instance,OK,Ballot,Id}
ACCEPT_REPLY = np.dtype([("instance", "<i4"), ("ballot", "<i4"), ("id", "<i4"), ("ok", "u1"),
                         ("pad", "u1", (3,))])
# mpx_inst_state  <- Instance.Status + LeaderBookkeeping
INST_STATE = np.dtype([("status", "<i4"), ("accept_oks", "<i4"), ("nacks", "<i4"),
                       ("max_recv_ballot", "<i4")])
# mpx_prepare_reply  <- paxosproto.PrepareReply{Instance,OK,Ballot,Command}
PREPARE_REPLY = np.dtype([("instance", "<i4"), ("ballot", "<i4"), ("ok", "<u4"),
                          ("value_id", "<u4")])
# mpx_prep_state  <- paxos Instance{cmds,ballot,status,lb}
PREP_STATE = np.dtype([("ballot", "<i4"), ("status", "<i4"), ("prepare_oks", "<i4"),
                       ("nacks", "<i4"), ("max_recv_ballot", "<i4"), ("value_id", "<u4"),
                       ("flags", "<u4"), ("pad", "<u4")])
# mpx_prepare_reply_min  <- minpaxosproto.PrepareReply
PREPARE_REPLY_MIN = np.dtype([("id", "<i4"), ("instance", "<i4"), ("ballot", "<i4"),
                              ("last_committed", "<i4"), ("ok", "<u4"), ("value_id", "<u4")])
# mpx_group_prep_state  <- bareminpaxos PrepareBookkeeping + replica scalars
GROUP_PREP_STATE = np.dtype([("default_ballot", "<i4"), ("prepare_oks", "<i4"), ("nacks", "<i4"),
                             ("max_recv_ballot", "<i4"), ("highest_instance", "<i4"),
                             ("value_id", "<u4"), ("committed_upto", "<i4"),
                             ("triggered", "<u4")])
# mpx_prepare_effect
PREPARE_EFFECT = np.dtype([("flags", "<u4"), ("catchup_from", "<i4")])

# peer-stream frame codes (include/mpx.h MPX_PEER_*; genericsmrproto.go:7-18 and the RPC
# registration order of bareminpaxos.NewReplica, bareminpaxos.go:108-113)
PEER_BEACON, PEER_BEACON_REPLY, PEER_PREPARE, PEER_ACCEPT, PEER_COMMIT = 6, 7, 8, 9, 10
PEER_COMMIT_SHORT, PEER_PREPARE_REPLY, PEER_ACCEPT_REPLY = 11, 12, 13
# body bytes after the code byte (None = variable length; unknown codes have none)
PEER_BODY = {PEER_BEACON: 8, PEER_BEACON_REPLY: 8, PEER_PREPARE: 12, PEER_COMMIT_SHORT: 16,
             PEER_ACCEPT_REPLY: 13, PEER_ACCEPT: None, PEER_COMMIT: None, PEER_PREPARE_REPLY: None}
# CLASSIC framing (paxosproto, registration order paxos.go:93-98): Prepare 13, AcceptReply 9
PEER_BODY_CLASSIC = {**PEER_BODY, PEER_PREPARE: 13, PEER_ACCEPT_REPLY: 9}
DECODE_END, DECODE_PARTIAL, DECODE_VARIABLE, DECODE_MALFORMED, DECODE_LONG = 0, 1, 2, 3, 4
DECODE_WINDOW = 64
DECODE_MAX_BYTES = 0x7FFFFFFF
# mpx_var_frame / mpx_stream_result (mpx_decode_stream)
VAR_FRAME = np.dtype([("offset", "<u4"), ("length", "<u4"), ("n_cmds", "<u4"),
                      ("cmds_off", "<u4"), ("n_log", "<u4"), ("log_off", "<u4"), ("code", "u1"),
                      ("pad", "u1", (7,))])
STREAM_RESULT = np.dtype([("consumed", "<u8"), ("next", "<u8"), ("n_accept_replies", "<u8"),
                          ("n_prepare_replies", "<u8"), ("n_var", "<u8"), ("n_other", "<u8"),
                          ("stop_reason", "<i4"), ("stop_code", "<i4")])
# mpx_peer_frame / mpx_decode_result
PEER_FRAME = np.dtype([("offset", "<u4"), ("code", "u1"), ("pad", "u1", (3,))])
DECODE_RESULT = np.dtype([("consumed", "<u8"), ("n_accept_replies", "<u8"), ("n_other", "<u8"),
                          ("stop_reason", "<i4"), ("stop_code", "<i4")])

# mpx_reply_rec: one client reply (genericsmrproto.ProposeReplyTS fields + connection index)
REPLY_REC = np.dtype([("value", "<i8"), ("timestamp", "<i8"), ("command_id", "<i4"),
                      ("client", "<u4")])
PROPOSE_REPLY_BYTES = 25

# mpx_log_rec / log formats (instance-log encoding)
LOG_CATCHUP, LOG_DURABLE = 0, 1
# mpx_replay_durable: getDataFromStableStore reads 12 metadata bytes + one 17-byte Command
DURABLE_REC_BYTES = 29
LOG_REC = np.dtype([("ballot", "<i4"), ("status", "<i4"), ("inst_no", "<i4"), ("pad", "<u4")])

# the acceptor side (mpx_accept_handle / mpx_encode_accept_replies)
# mpx_accept_msg  <- minpaxosproto.Accept / paxosproto.Accept header (Command -> value_id)
ACCEPT_MSG = np.dtype([("instance", "<i4"), ("ballot", "<i4"), ("leader_id", "<i4"),
                       ("value_id", "<u4")])
# mpx_acceptor_state  <- the acceptor's view of instanceSpace[i] (flags: PF_HAS_PROPOSALS in,
# PF_REQUEUED out)
ACCEPTOR_STATE = np.dtype([("status", "<i4"), ("ballot", "<i4"), ("value_id", "<u4"),
                           ("flags", "<u4")])
# mpx_acceptor_group  <- r.defaultBallot, r.Id
ACCEPTOR_GROUP = np.dtype([("default_ballot", "<i4"), ("self_id", "<i4")])
# effect[i] of mpx_accept_handle
AH_REPLIED, AH_STORED, AH_REQUEUE = 1, 2, 4
# frame bytes of one AcceptReply on a peer connection (code byte + Marshal), by mode
ACCEPT_REPLY_FRAME = {MODE_MIN: 14, MODE_CLASSIC: 10}

# the proposer side (mpx_propose_handle / mpx_encode_accepts)
# mpx_proposer_group  <- r.defaultBallot, r.Id, r.Leader, prepareOKs, r.crtInstance, r.committedUpTo
PROPOSER_GROUP = np.dtype([("default_ballot", "<i4"), ("self_id", "<i4"), ("leader", "<i4"),
                           ("prepare_oks", "<i4"), ("crt_instance", "<i4"),
                           ("committed_upto", "<i4"), ("pad", "<u4", (2,))])
# mpx_accept_send  <- one run of handlePropose: a batch of proposals and what became of it
ACCEPT_SEND = np.dtype([("instance", "<i4"), ("ballot", "<i4"), ("last_committed", "<i4"),
                        ("flags", "<u4"), ("first_cmd", "<u8"), ("n_cmds", "<u4"), ("pad", "<u4")])
PROPOSE_MAX_BATCH = 5000
PH_ACCEPT, PH_NOT_LEADER, PH_REFUSED, PH_PREPARE = 1, 2, 4, 8
AB_THRIFTY = 1
# mpx_encode_accepts_stored reads the catch-up log from the instance store instead of LOG_REC
# arrays: ACCEPTOR_STATE (ballot, status), optionally INST_STATE (the status once the tally has
# committed), INST_CMDS and the command arena they point into (below)

# the prepare side (mpx_gather_prepares / mpx_prepare_handle / mpx_encode_prepare_replies)
# mpx_prepare_msg  <- minpaxosproto.Prepare / paxosproto.Prepare. key: CLASSIC the Instance, MIN the
# group of the connection; arg: CLASSIC ToInfinity (the wire byte), MIN LastCommitted
PREPARE_MSG = np.dtype([("key", "<i4"), ("ballot", "<i4"), ("leader_id", "<i4"), ("arg", "<i4")])
PRH_OK, PRH_RAISED, PRH_LOG = 1, 2, 4
# the Prepare frame's body after the code byte, and the PrepareReply frame's fixed head, by mode
PREPARE_BODY = {MODE_MIN: 12, MODE_CLASSIC: 13}
PREPARE_REPLY_HEAD = {MODE_MIN: 18, MODE_CLASSIC: 10}
assert PREPARE_MSG.itemsize == 16

# the commit side (mpx_commit_handle / mpx_encode_commits / mpx_gather_commit_shorts)
VALUE_KEEP = 0xFFFFFFFF  # value_id of a CommitShort record (no Command; nil Cmds on a nil instance)
CH_INSTALLED, CH_CMDS, CH_REQUEUE = 1, 2, 4
# mpx_commit_send  <- one decided instance whose Commit goes out (CS_SEND: not skipped)
COMMIT_SEND = np.dtype([("instance", "<i4"), ("ballot", "<i4"), ("first_cmd", "<u8"),
                        ("n_cmds", "<u4"), ("flags", "<u4"), ("pad", "<u4", (2,))])
CS_SEND = 1
COMMIT_SHORT_FRAME = 17
assert COMMIT_SEND.itemsize == 32


# batch assembly (mpx_order_records): mpx_order_result, the call flag and the result flag
ORDER_RESULT = np.dtype([("n", "<u8"), ("n_runs", "<u8"), ("lo", "<i4"), ("hi", "<i4"),
                         ("flags", "<u4"), ("pad", "<u4")])
ORDER_MAX_SRC = 16
ORDER_ONE_LAUNCH_MAX = 4096
ORDER_GENERAL = 1
ORD_WAS_ORDERED = 1
assert ORDER_RESULT.itemsize == 32


# the client side (mpx_decode_client_streams): frame codes of a client connection
# (genericsmrproto.go:7-18), frame bytes with the code, and the four records of the call
CLIENT_PROPOSE, CLIENT_READ, CLIENT_PROPOSE_AND_READ = 0, 2, 4
CLIENT_PROPOSE_FRAME, CLIENT_READ_FRAME = 30, 13
CLIENT_ALIGN = 128
CLIENT_MAX_CONNS = CLIENT_MAX_GROUPS = 1 << 20
CLIENT_CONN = np.dtype([("offset", "<u8"), ("length", "<u4"), ("group", "<u4")])
PROPOSAL = np.dtype([("timestamp", "<i8"), ("command_id", "<i4"), ("client", "<u4")])
CLIENT_CONN_RESULT = np.dtype([("first", "<u8"), ("consumed", "<u4"), ("n_proposals", "<u4"),
                               ("n_dropped", "<u4"), ("stop_reason", "<i4"), ("stop_code", "<i4"),
                               ("pad", "<u4")])
CLIENT_RESULT = np.dtype([("n_proposals", "<u8"), ("n_dropped", "<u8"), ("n_partial", "<u8"),
                          ("n_sends", "<u8")])
assert CLIENT_CONN.itemsize == 16 and PROPOSAL.itemsize == 16
assert CLIENT_CONN_RESULT.itemsize == 32 and CLIENT_RESULT.itemsize == 32


# reply assembly (mpx_build_replies): the kinds, the call flag, the one-launch bounds and
# mpx_reply_result
RB_FALSE, RB_DECIDED, RB_EXECUTED = 1, 2, 3
RB_GENERAL = 1
RB_NO_PAD = 0xFFFFFFFF
RB_ONE_LAUNCH_SLOTS, RB_ONE_LAUNCH_REPLIES = 1024, 8192
REPLY_RESULT = np.dtype([("n_replies", "<u8"), ("n_slots", "<u8")])
assert REPLY_RESULT.itemsize == 16


# execute assembly (mpx_execute_gather): mpx_inst_cmds (where a window slot's Cmds live in the
# source command arrays; flags 0 = Cmds == nil or a nil instance), the call flags, the one-launch
# bounds and mpx_execute_result
INST_CMDS = np.dtype([("first_cmd", "<u8"), ("n_cmds", "<u4"), ("flags", "<u4")])
IC_HAS_CMDS = 1
XG_PAD, XG_GENERAL = 1, 2
XG_ONE_LAUNCH_INST, XG_ONE_LAUNCH_CMDS = 1024, 8192
EXECUTE_RESULT = np.dtype([("n_cmds", "<u8"), ("n_inst", "<u8"), ("n_groups", "<u8"),
                           ("reserved", "<u8")])
assert INST_CMDS.itemsize == 16 and EXECUTE_RESULT.itemsize == 32


# store assembly (mpx_store_commands / mpx_store_compact): the kinds, the call flag, the result
# flag, the one-launch bounds, mpx_store_result and the host layout of mpx_store_src
SC_MSGS, SC_SENDS = 0, 1
SC_GENERAL = 1
SC_FULL = 1
SC_MAX_SRC = 16
SC_ONE_LAUNCH_ITEMS, SC_ONE_LAUNCH_CMDS = 1024, 8192
STORE_RESULT = np.dtype([("n_stored", "<u8"), ("n_cmds", "<u8"), ("n_superseded", "<u8"),
                         ("flags", "<u8")])
STORE_SRC = np.dtype([("cmd_off", "<u8"), ("n_frames", "<u8"), ("op", "<u8"), ("key", "<u8"),
                      ("val", "<u8"), ("n_cmds", "<u8"), ("n_recs", "<u8")])
assert STORE_RESULT.itemsize == 32 and STORE_SRC.itemsize == 56


# record assembly (mpx_record_log): the kinds, the CLASSIC metadata format (beside LOG_DURABLE), the
# call flag, the result flag, the one-launch bounds, the metadata bytes per format and
# mpx_record_result
LR_ACCEPTS, LR_COMMITS, LR_SENDS, LR_DECIDED = 0, 1, 2, 3
LOG_DURABLE_CLASSIC = 2
LR_GENERAL = 1
LR_FULL = 1
LR_ONE_LAUNCH_ITEMS, LR_ONE_LAUNCH_CMDS = 1024, 8192
LR_HEADER_BYTES = {1: 12, LOG_DURABLE_CLASSIC: 5}
RECORD_RESULT = np.dtype([("n_recs", "<u8"), ("n_cmds", "<u8"), ("n_bytes", "<u8"), ("flags", "<u8")])
assert RECORD_RESULT.itemsize == 32


def record_bound(n, m):
    """mpx_record_bound: the most bytes n items carrying m commands can record, either format"""
    return 12 * n + 17 * m


def commit_frame_bytes(n_cmds):
    """one full Commit on a peer connection (code byte + Marshal)"""
    return 13 + varint_len(n_cmds) + 17 * n_cmds


# mpx_unmarshal_frames: mpx_unmarshal_result, and the arrays of mpx_unmarshal_out in the order a
# trimmed result carries them (engine.Engine.unmarshal_frames)
UNMARSHAL_RESULT = np.dtype([("n_accepts", "<u8"), ("n_commits", "<u8"), ("n_cmds", "<u8"),
                             ("n_log_inst", "<u8"), ("n_log_cmds", "<u8"), ("n_var", "<u8")])
UNMARSHAL_ARRAYS = ("accepts", "accept_last_committed", "commits", "cmd_off", "op", "key", "val",
                    "log_inst_off", "log_recs", "log_cmd_off", "log_op", "log_key", "log_val")
# bytes from a variable-length frame's code byte to V(len(Command)), by mode and code
VAR_HEADER = {MODE_MIN: {PEER_ACCEPT: 17, PEER_COMMIT: 13, PEER_PREPARE_REPLY: 18},
              MODE_CLASSIC: {PEER_ACCEPT: 13, PEER_COMMIT: 13, PEER_PREPARE_REPLY: 10}}
assert UNMARSHAL_RESULT.itemsize == 48


def varint_len(x):
    """bytes of binary.PutVarint(x), x >= 0"""
    u, n = x << 1, 1
    while u >= 0x80:
        u >>= 7
        n += 1
    return n


def log_instance_bytes(n_cmds):
    """Instance.Marshal: Ballot, Status, V(k), k Commands"""
    return 8 + varint_len(n_cmds) + 17 * n_cmds


def accept_frame_bytes(mode, n_cmds, log_cmd_counts=()):
    """one Accept on a peer connection (code byte + Marshal); MIN: log_cmd_counts = len(Cmds) of
    every CatchUpLog instance"""
    if mode == MODE_MIN:
        return (17 + varint_len(n_cmds) + 17 * n_cmds + varint_len(len(log_cmd_counts)) +
                sum(log_instance_bytes(k) for k in log_cmd_counts))
    return 13 + varint_len(n_cmds) + 17 * n_cmds


assert PROPOSER_GROUP.itemsize == 32 and ACCEPT_SEND.itemsize == 32
assert ACCEPT_MSG.itemsize == 16 and ACCEPTOR_STATE.itemsize == 16
assert ACCEPTOR_GROUP.itemsize == 8
assert LOG_REC.itemsize == 16
assert REPLY_REC.itemsize == 24
assert PEER_FRAME.itemsize == 8 and DECODE_RESULT.itemsize == 32
assert VAR_FRAME.itemsize == 32 and STREAM_RESULT.itemsize == 56
assert ACCEPT_REPLY.itemsize == 16 and INST_STATE.itemsize == 16
assert PREPARE_REPLY.itemsize == 16 and PREP_STATE.itemsize == 32
assert PREPARE_REPLY_MIN.itemsize == 24 and GROUP_PREP_STATE.itemsize == 32
assert PREPARE_EFFECT.itemsize == 8

# mpx_config.apply_path / apply_hot_min (include/mpx.h)
APPLY_AUTO, APPLY_SORTED, APPLY_PARTITIONED, APPLY_SMALL = 0, 1, 2, 3
APPLY_NO_HOT = 0xFFFFFFFF
FLAG_STEP_ONE_LAUNCH = 1  # mpx_config.flags: one kernel per group step (mpx.h)
APPLY_SMALL_MAX = 16384

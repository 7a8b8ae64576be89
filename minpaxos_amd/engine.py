"""Python handle over the C ABI (numpy in, numpy out; device pointers for the *_dev paths).

Names and argument meaning follow the reference handlers they replace:
  accept_tally        <- bareminpaxos / paxos  handleAcceptReply
  prepare_select      <- paxos.handlePrepareReply          (CLASSIC, per instance)
  prepare_select_min  <- bareminpaxos.handlePrepareReply   (MIN, per group)
  apply               <- executeCommands -> state.Command.Execute (+ state.Conflict)
  conflict_batch      <- state.ConflictBatch
  committed_prefix    <- updateCommittedUpTo
  group_step          <- handleAcceptReply + executeCommands for many replicas at once
  decode_peer_stream  <- genericsmr.replicaListener framing + AcceptReply.Unmarshal
  encode_replies      <- the ProposeReplyTS fan-out (ReplyProposeTS per executed command)
  accept_handle       <- bareminpaxos / paxos  handleAccept (the acceptor's half of Phase 2)
  encode_accept_replies <- replyAccept -> SendMsg: the AcceptReply frames per leader connection
  propose_handle      <- bareminpaxos / paxos  handlePropose (which proposals become an instance)
  encode_accepts      <- bcastAccept -> SendMsg: the Accept frames per peer connection
  encode_accepts_stored  the same frames, the catch-up log read from the instance store
  unmarshal_frames    <- Accept / Commit / PrepareReply.Unmarshal (+ Instance, Command) of the
                         frames decode_stream found: records and SoA arrays
  commit_handle       <- bareminpaxos / paxos  handleCommit, handleCommitShort and
                         updateCommittedUpTo for a commit-only batch
  encode_commits      <- bcastCommit -> SendMsg: the CommitShort / Commit frames per peer
  gather_commit_shorts <- CommitShort.Unmarshal of the frames decode_stream listed
  gather_prepares     <- Prepare.Unmarshal of the frames decode_stream listed
  prepare_handle      <- bareminpaxos / paxos  handlePrepare (the follower's half of Phase 1)
  encode_prepare_replies <- replyPrepare -> SendMsg: the PrepareReply frames per leader
                         connection, Command and CatchUpLog read from the instance store
  order_records       <- the shim's sort.SliceStable by Instance over the drained connections:
                         the batch order every handler above asks for
  decode_client_streams <- genericsmr.clientListener + Propose.Unmarshal over many connections:
                         the proposals, their reply metadata and the per-group offsets
  build_replies       <- the three reply loops (handlePropose's refusals, handleAcceptReply with
                         !Dreply, executeCommands with Dreply): the records encode_replies takes,
                         and CLASSIC's bcastCommit list
  execute_gather      <- executeCommands' walk (which instances run) and the gather of their
                         commands for apply, with build_replies' executed mask and ret_first
  store_commands      <- where handleAccept / handleCommit / handlePropose assign an instance's
                         Cmds: the batch's commands appended to a command arena, the slots'
                         INST_CMDS written; store_compact squeezes retired instances out of it
  record_log          <- the handlers' recordInstanceMetadata (+ recordCommands): a batch's durable-log
                         bytes as one run, MIN's 12-byte or CLASSIC's 5-byte metadata
  replay_durable      <- getDataFromStableStore (bareminpaxos.go:122-161)
  encode_log         <- Instance.Marshal (bcastAccept's CatchUpLog) / recordInstanceMetadata +
                         recordCommands (the durable log)
Errors come back as MpxError carrying the reference-level reason (e.g. E_NIL_INSTANCE where the
Go handler would dereference a nil *Instance).
"""
import ctypes as C

import numpy as np

from . import _lib
from . import records as R


class MpxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{R.ERROR_NAMES.get(code, code)}: {msg}")
        self.code = code


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def device_count():
    lib = _lib.load()
    c = C.c_int(0)
    lib.mpx_device_count(C.byref(c))
    return c.value


def step_one_launch_fits(n_replicas, ipg, kv_per_group):
    """True when a fast group-step variant takes the batch shape, which MPX_FLAG_STEP_ONE_LAUNCH
    requires (the variant choice of step.hip fast_variant / mpx.h)"""
    recs = max(n_replicas - 1, 1) * ipg
    K = kv_per_group or 512
    return ((ipg <= 256 and recs <= 1024 and K <= 1024) or (ipg <= 256 and recs <= 2048 and K <= 256)
            or (ipg <= 512 and recs <= 2048 and K <= 512))


class Engine:
    def __init__(self, device=0, n_replicas=5, mode=R.MODE_MIN, kv_capacity=0, kv_per_group=0,
                 max_groups=0, apply_path=R.APPLY_AUTO, apply_fast_min=0, apply_hot_min=0,
                 apply_chunk=0, step_one_launch=False):
        """apply_* are the handle's mpx_apply settings (mpx_config): the pipeline choice
        (R.APPLY_AUTO / _SMALL / _SORTED / _PARTITIONED), AUTO's partitioned threshold, the hot
        key sample threshold (R.APPLY_NO_HOT: none) and the chunk size; 0 = default.
        step_one_launch: MPX_FLAG_STEP_ONE_LAUNCH (one kernel per group step; every group must
        fit the fast kernel, see mpx.h)"""
        self.lib = _lib.load()
        if isinstance(mode, str):
            mode = {"min": R.MODE_MIN, "classic": R.MODE_CLASSIC}[mode.lower()]
        self.n_replicas = n_replicas
        self.mode = mode
        self.kv_per_group = kv_per_group or 512
        self.step_one_launch = bool(step_one_launch)
        flags = R.FLAG_STEP_ONE_LAUNCH if step_one_launch else 0
        cfg = _lib.MpxConfig(n_replicas, mode, kv_capacity, kv_per_group, flags, max_groups,
                             apply_chunk, apply_path, apply_fast_min, apply_hot_min, 0)
        h = C.c_void_p()
        rc = self.lib.mpx_open(device, C.byref(cfg), C.byref(h))
        if rc != 0:
            raise MpxError(rc, f"mpx_open(device={device})")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.mpx_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.mpx_last_error(self.h)
            raise MpxError(rc, f"{what}: {msg.decode() if msg else ''}")

    @property
    def stream(self):
        return self.lib.mpx_stream(self.h)

    def synchronize(self):
        self._check(self.lib.mpx_synchronize(self.h), "mpx_synchronize")

    # ---- A1 / A2 ----------------------------------------------------------------------------
    def accept_tally(self, recs, st, inst_base=0, committed_upto=-1, peer_commits=None,
                     want_decided=True):
        recs = _c(recs, R.ACCEPT_REPLY)
        st = np.array(st, dtype=R.INST_STATE, copy=True)
        pc = np.zeros(self.n_replicas, np.int32) if peer_commits is None else \
            np.array(peer_commits, dtype=np.int32, copy=True)
        cu = C.c_int32(committed_upto)
        dec = np.zeros(len(st), np.uint8) if want_decided else None
        rc = self.lib.mpx_accept_tally(self.h, _ptr(recs), len(recs), _ptr(st), len(st), inst_base,
                                       C.byref(cu), _ptr(pc), _ptr(dec))
        self._check(rc, "mpx_accept_tally")
        return st, cu.value, pc, dec

    def accept_tally_dev(self, d_recs, n, d_st_in, d_st_out, n_inst, inst_base, d_scalars,
                         d_decided=None, stream=None):
        rc = self.lib.mpx_accept_tally_dev(self.h, d_recs, n, d_st_in, d_st_out, n_inst,
                                           inst_base, d_scalars, d_decided, stream)
        self._check(rc, "mpx_accept_tally_dev")

    def committed_prefix(self, st, inst_base, committed_upto):
        st = _c(st, R.INST_STATE)
        cu = C.c_int32(committed_upto)
        self._check(self.lib.mpx_committed_prefix(self.h, _ptr(st), len(st), inst_base,
                                                  C.byref(cu)), "mpx_committed_prefix")
        return cu.value

    # ---- A4 ---------------------------------------------------------------------------------
    def prepare_select(self, recs, st, inst_base=0, default_ballot=-1, want_prepared=True):
        recs = _c(recs, R.PREPARE_REPLY)
        st = np.array(st, dtype=R.PREP_STATE, copy=True)
        db = C.c_int32(default_ballot)
        prep = np.zeros(len(st), np.uint8) if want_prepared else None
        rc = self.lib.mpx_prepare_select(self.h, _ptr(recs), len(recs), _ptr(st), len(st),
                                         inst_base, C.byref(db), _ptr(prep))
        self._check(rc, "mpx_prepare_select")
        return st, db.value, prep

    def prepare_select_dev(self, d_recs, n, d_st_in, d_st_out, n_inst, inst_base,
                           d_default_ballot, d_prepared=None, stream=None):
        rc = self.lib.mpx_prepare_select_dev(self.h, d_recs, n, d_st_in, d_st_out, n_inst,
                                             inst_base, d_default_ballot, d_prepared, stream)
        self._check(rc, "mpx_prepare_select_dev")

    # ---- A3 ---------------------------------------------------------------------------------
    def prepare_select_min(self, recs, grp_rec_off, gst, peer_commits=None, want_effects=True):
        recs = _c(recs, R.PREPARE_REPLY_MIN)
        off = _c(grp_rec_off, np.uint64)
        gst = np.array(gst, dtype=R.GROUP_PREP_STATE, copy=True)
        g = len(gst)
        pc = np.zeros(g * self.n_replicas, np.int32) if peer_commits is None else \
            np.array(peer_commits, dtype=np.int32, copy=True).reshape(-1)
        eff = np.zeros(len(recs), R.PREPARE_EFFECT) if want_effects else None
        rc = self.lib.mpx_prepare_select_min(self.h, _ptr(recs), len(recs), _ptr(off), _ptr(gst),
                                             g, _ptr(pc), _ptr(eff))
        self._check(rc, "mpx_prepare_select_min")
        return gst, pc, eff

    def prepare_select_min_dev(self, d_recs, n, d_off, d_gst, n_groups, d_peer, d_eff=None,
                               stream=None):
        rc = self.lib.mpx_prepare_select_min_dev(self.h, d_recs, n, d_off, d_gst, n_groups,
                                                 d_peer, d_eff, stream)
        self._check(rc, "mpx_prepare_select_min_dev")

    # ---- A5 / A6 ----------------------------------------------------------------------------
    def apply_buffers(self, max_m):
        """mpx_apply_buffers: numpy views of the engine's pinned op / key / val / ret / conf
        arrays (valid until they grow or the engine closes) for mpx_apply_staged"""
        io = _lib.MpxApplyIo()
        self._check(self.lib.mpx_apply_buffers(self.h, max_m, C.byref(io)), "mpx_apply_buffers")

        def view(ptr, ct, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(io.cap,)).view(dt)
        return {"op": view(io.op, C.c_uint8, np.uint8), "key": view(io.key, C.c_int64, np.int64),
                "val": view(io.val, C.c_int64, np.int64), "ret": view(io.ret, C.c_int64, np.int64),
                "conf": view(io.conf, C.c_uint8, np.uint8), "cap": int(io.cap)}

    def apply_staged(self, m):
        """mpx_apply_staged: apply the first m commands of the apply_buffers arrays"""
        self._check(self.lib.mpx_apply_staged(self.h, m), "mpx_apply_staged")

    def apply(self, op, key, val, want_conf=True):
        op = _c(op, np.uint8)
        key = _c(key, np.int64)
        val = _c(val, np.int64)
        m = len(op)
        ret = np.zeros(m, np.int64)
        conf = np.zeros(m, np.uint8) if want_conf else None
        rc = self.lib.mpx_apply(self.h, _ptr(op), _ptr(key), _ptr(val), m, _ptr(ret), _ptr(conf))
        self._check(rc, "mpx_apply")
        return ret, conf

    def debug_kv_set_epoch(self, epoch):
        """TEST-ONLY: the KV table's call epoch, its slots untouched (mpx_debug_kv_set_epoch)"""
        self._check(self.lib.mpx_debug_kv_set_epoch(self.h, epoch), "mpx_debug_kv_set_epoch")

    def debug_kv_set_small_tag(self, tag):
        """TEST-ONLY: the tag of the last replica-batch call (mpx_debug_kv_set_small_tag)"""
        self._check(self.lib.mpx_debug_kv_set_small_tag(self.h, tag), "mpx_debug_kv_set_small_tag")

    def debug_kv_state(self):
        """TEST-ONLY: the KV table's per-slot state words (uint32, cap + 1 of them)"""
        n = C.c_size_t(0)
        self._check(self.lib.mpx_debug_kv_state(self.h, None, 0, C.byref(n)), "mpx_debug_kv_state")
        out = np.zeros(n.value, np.uint32)
        self._check(self.lib.mpx_debug_kv_state(self.h, _ptr(out), len(out), C.byref(n)),
                    "mpx_debug_kv_state")
        return out

    def apply_reserve(self, max_cmds):
        self._check(self.lib.mpx_apply_reserve(self.h, max_cmds), "mpx_apply_reserve")

    def apply_dev(self, d_op, d_key, d_val, m, d_ret, d_conf=None, stream=None):
        self._check(self.lib.mpx_apply_dev(self.h, d_op, d_key, d_val, m, d_ret, d_conf, stream),
                    "mpx_apply_dev")

    def kv_size(self):
        n = C.c_size_t(0)
        self._check(self.lib.mpx_kv_size(self.h, C.byref(n)), "mpx_kv_size")
        return n.value

    def kv_export(self):
        """Present (key, value) pairs sorted by key."""
        n = self.kv_size()
        keys = np.zeros(max(n, 1), np.int64)
        vals = np.zeros(max(n, 1), np.int64)
        got = C.c_size_t(0)
        self._check(self.lib.mpx_kv_export(self.h, _ptr(keys), _ptr(vals), n, C.byref(got)),
                    "mpx_kv_export")
        k = min(n, got.value)
        order = np.argsort(keys[:k], kind="stable")
        return keys[:k][order], vals[:k][order]

    def kv_import(self, keys, vals):
        keys = _c(keys, np.int64)
        vals = _c(vals, np.int64)
        self._check(self.lib.mpx_kv_import(self.h, _ptr(keys), _ptr(vals), len(keys)),
                    "mpx_kv_import")

    def kv_clear(self):
        self._check(self.lib.mpx_kv_clear(self.h), "mpx_kv_clear")

    def conflict_batch(self, op, key, inst_off):
        op = _c(op, np.uint8)
        key = _c(key, np.int64)
        off = _c(inst_off, np.uint64)
        n_inst = len(off) - 1
        out = np.zeros(max(n_inst - 1, 1), np.uint8)
        self._check(self.lib.mpx_conflict_batch(self.h, _ptr(op), _ptr(key), _ptr(off), n_inst,
                                                _ptr(out)), "mpx_conflict_batch")
        return out[:max(n_inst - 1, 0)]

    def conflict_batch_dev(self, d_op, d_key, d_inst_off, n_inst, d_out, stream=None):
        self._check(self.lib.mpx_conflict_batch_dev(self.h, d_op, d_key, d_inst_off, n_inst,
                                                    d_out, stream), "mpx_conflict_batch_dev")

    # ---- fused group step -------------------------------------------------------------------
    def group_step(self, b, kv_cnt=None, kv_key=None, kv_val=None, ret=None, want_conf=True,
                   want_decided=True):
        """b: dict from synth.group_batch (or the same fields). Returns a dict of outputs."""
        G, ipg, N = int(b["n_groups"]), int(b["ipg"]), self.n_replicas
        K = self.kv_per_group
        recs = _c(b["recs"], R.ACCEPT_REPLY)
        off = _c(b["grp_rec_off"], np.uint64)
        st = np.array(b["st_in"], dtype=R.INST_STATE, copy=True)
        ci = _c(b["committed_in"], np.int32)
        ei = _c(b["executed_in"], np.int32)
        pi = _c(b["peer_in"], np.int32)
        op, key, val = _c(b["op"], np.uint8), _c(b["key"], np.int64), _c(b["val"], np.int64)
        coff = _c(b["cmd_off"], np.uint32)
        has = _c(b["has_cmds"], np.uint8) if b.get("has_cmds") is not None else None
        m = len(op)
        ret = np.zeros(m, np.int64) if ret is None else np.array(ret, np.int64, copy=True)
        conf = np.zeros(m, np.uint8) if want_conf else None
        kc = np.zeros(G, np.uint32) if kv_cnt is None else np.array(kv_cnt, np.uint32, copy=True)
        kk = np.zeros(G * K, np.int64) if kv_key is None else np.array(kv_key, np.int64, copy=True)
        kv = np.zeros(G * K, np.int64) if kv_val is None else np.array(kv_val, np.int64, copy=True)
        co = np.zeros(G, np.int32)
        eo = np.zeros(G, np.int32)
        po = np.zeros(G * N, np.int32)
        dec = np.zeros(G * ipg, np.uint8) if want_decided else None
        nd = np.zeros(G, np.uint32)
        gb = _lib.MpxGroupBatch(G, ipg, *[C.cast(_ptr(x), C.c_void_p) if x is not None else None
                                          for x in (recs, off, st, st, ci, co, ei, eo, pi, po, op,
                                                    key, val, coff, has, ret, conf, kc, kk, kv,
                                                    kc, kk, kv, dec, nd)])
        self._check(self.lib.mpx_group_step(self.h, C.byref(gb)), "mpx_group_step")
        return dict(st_out=st, committed_out=co, executed_out=eo, peer_out=po, ret=ret,
                    conf_prev=conf, kv_cnt=kc, kv_key=kk, kv_val=kv, decided=dec, n_decided=nd)

    def group_step_dev(self, gb, stream=None):
        self._check(self.lib.mpx_group_step_dev(self.h, C.byref(gb), stream), "mpx_group_step_dev")

    def group_step_totals_dev(self, gb, d_totals, stream=None):
        """mpx_group_step_totals_dev: the group step with its totals from the same kernels"""
        self._check(self.lib.mpx_group_step_totals_dev(self.h, C.byref(gb), d_totals, stream),
                    "mpx_group_step_totals_dev")

    def step_totals_dev(self, gb, d_totals, stream=None):
        """d_totals[0..2] = decided instances, executed instances, executed commands"""
        self._check(self.lib.mpx_step_totals_dev(self.h, C.byref(gb), d_totals, stream),
                    "mpx_step_totals_dev")

    # ---- peer stream framing ------------------------------------------
    def decode_peer_stream(self, buf, ar_cap=None, other_cap=None):
        """Frame one peer connection's bytes. Returns (accept_replies, other_frames, result):
        AcceptReplies in arrival order (mpx_accept_reply), the other fixed-size frames as
        (offset, code), and the mpx_decode_result (consumed, counts, stop reason / code)."""
        buf = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else \
            _c(buf, np.uint8)
        n = len(buf)
        ar_cap = n // 14 + 1 if ar_cap is None else ar_cap
        other_cap = n + 1 if other_cap is None else other_cap
        ar = np.zeros(max(ar_cap, 1), R.ACCEPT_REPLY)
        oth = np.zeros(max(other_cap, 1), R.PEER_FRAME)
        res = np.zeros(1, R.DECODE_RESULT)
        self._check(self.lib.mpx_decode_peer_stream(self.h, _ptr(buf), n, _ptr(ar), ar_cap,
                                                    _ptr(oth), other_cap, _ptr(res)),
                    "mpx_decode_peer_stream")
        r = res[0]
        return (ar[:min(int(r["n_accept_replies"]), ar_cap)],
                oth[:min(int(r["n_other"]), other_cap)], r)

    def decode_stream(self, buf, caps=None):
        """Frame one peer connection's bytes with the engine's protocol (MIN / CLASSIC),
        variable-length messages included. Returns (accept_replies, prepare_replies,
        var_frames, other_frames, mpx_stream_result)."""
        buf = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else \
            _c(buf, np.uint8)
        n = len(buf)
        ca, cp, cv, co = caps or (n // 10 + 1, n // 10 + 1, n // 13 + 1, n + 1)
        ar = np.zeros(max(ca, 1), R.ACCEPT_REPLY)
        pr = np.zeros(max(cp, 1), R.PREPARE_REPLY_MIN if self.mode == R.MODE_MIN
                      else R.PREPARE_REPLY)
        var = np.zeros(max(cv, 1), R.VAR_FRAME)
        oth = np.zeros(max(co, 1), R.PEER_FRAME)
        res = np.zeros(1, R.STREAM_RESULT)
        out = _lib.MpxDecodeOut(_ptr(ar), ca, _ptr(pr), cp, _ptr(var), cv, _ptr(oth), co)
        self._check(self.lib.mpx_decode_stream(self.h, _ptr(buf), n, C.byref(out), _ptr(res)),
                    "mpx_decode_stream")
        r = res[0]
        return (ar[:min(int(r["n_accept_replies"]), ca)], pr[:min(int(r["n_prepare_replies"]), cp)],
                var[:min(int(r["n_var"]), cv)], oth[:min(int(r["n_other"]), co)], r)

    def decode_stream_reserve(self, max_len):
        self._check(self.lib.mpx_decode_stream_reserve(self.h, max_len),
                    "mpx_decode_stream_reserve")

    def decode_stream_dev(self, d_buf, n, start, out, d_res, stream=None):
        """out: _lib.MpxDecodeOut of device pointers; d_res: device mpx_stream_result (in/out)"""
        self._check(self.lib.mpx_decode_stream_dev(self.h, d_buf, n, start, C.byref(out), d_res,
                                                   stream), "mpx_decode_stream_dev")

    def decode_reserve(self, max_len):
        self._check(self.lib.mpx_decode_reserve(self.h, max_len), "mpx_decode_reserve")

    def decode_peer_stream_dev(self, d_buf, n, d_ar, ar_cap, d_other, other_cap, d_res,
                               stream=None):
        self._check(self.lib.mpx_decode_peer_stream_dev(self.h, d_buf, n, d_ar, ar_cap, d_other,
                                                        other_cap, d_res, stream),
                    "mpx_decode_peer_stream_dev")

    # ---- client reply fan-out -----------------------------------------
    def encode_replies(self, recs, n_clients, ok=1, leader=0):
        """recs: REPLY_REC in execution order. Returns (bytes uint8[25 n], client_off u64[C+1]):
        client c's connection receives out[client_off[c]:client_off[c+1]]."""
        recs = _c(recs, R.REPLY_REC)
        n = len(recs)
        out = np.zeros(max(n * R.PROPOSE_REPLY_BYTES, 1), np.uint8)
        off = np.zeros(n_clients + 1, np.uint64)
        self._check(self.lib.mpx_encode_replies(self.h, _ptr(recs), n, n_clients, ok, leader,
                                                _ptr(out), _ptr(off)), "mpx_encode_replies")
        return out[:n * R.PROPOSE_REPLY_BYTES], off

    def encode_replies_reserve(self, max_n):
        self._check(self.lib.mpx_encode_replies_reserve(self.h, max_n),
                    "mpx_encode_replies_reserve")

    def encode_replies_dev(self, d_recs, n, n_clients, ok, leader, d_out, d_off, stream=None):
        self._check(self.lib.mpx_encode_replies_dev(self.h, d_recs, n, n_clients, ok, leader,
                                                    d_out, d_off, stream),
                    "mpx_encode_replies_dev")

    # ---- the acceptor side: handleAccept and the AcceptReply bytes ----------------------------
    def accept_handle(self, msgs, st, groups, inst_base=0, ipg=None):
        """msgs: ACCEPT_MSG grouped by instance, ascending; st: ACCEPTOR_STATE of the window
        (copied); groups: ACCEPTOR_GROUP, group g owning window indices [g*ipg, (g+1)*ipg)
        (ipg defaults to the whole window: one log). Returns (st, replies ACCEPT_REPLY[n],
        reply_to int32[n], effect uint8[n]), the last three slot-aligned with msgs."""
        msgs = _c(msgs, R.ACCEPT_MSG)
        st = np.array(st, dtype=R.ACCEPTOR_STATE, copy=True)
        groups = _c(np.atleast_1d(groups), R.ACCEPTOR_GROUP)
        n = len(msgs)
        ipg = (len(st) // len(groups) if len(groups) else 0) if ipg is None else ipg
        rep = np.zeros(max(n, 1), R.ACCEPT_REPLY)
        to = np.zeros(max(n, 1), np.int32)
        eff = np.zeros(max(n, 1), np.uint8)
        rc = self.lib.mpx_accept_handle(self.h, _ptr(msgs), n, _ptr(st), len(st), inst_base,
                                        _ptr(groups), len(groups), ipg, _ptr(rep), _ptr(to),
                                        _ptr(eff))
        self._check(rc, "mpx_accept_handle")
        return st, rep[:n], to[:n], eff[:n]

    def accept_handle_dev(self, d_msgs, n, d_st_in, d_st_out, n_inst, inst_base, d_groups,
                          n_groups, ipg, d_replies, d_reply_to, d_effect, stream=None):
        rc = self.lib.mpx_accept_handle_dev(self.h, d_msgs, n, d_st_in, d_st_out, n_inst,
                                            inst_base, d_groups, n_groups, ipg, d_replies,
                                            d_reply_to, d_effect, stream)
        self._check(rc, "mpx_accept_handle_dev")

    def encode_accept_replies(self, replies, reply_to, n_dest=None):
        """replies: ACCEPT_REPLY, reply_to: int32 destination per reply (< 0: skipped). Returns
        (bytes uint8, dest_off u64[n_dest+1]): destination d's connection receives
        out[dest_off[d]:dest_off[d+1]], its AcceptReply frames in array order."""
        replies = _c(replies, R.ACCEPT_REPLY)
        reply_to = _c(reply_to, np.int32)
        n = len(replies)
        n_dest = self.n_replicas if n_dest is None else n_dest
        out = np.zeros(max(n * R.ACCEPT_REPLY_FRAME[self.mode], 1), np.uint8)
        off = np.zeros(n_dest + 1, np.uint64)
        self._check(self.lib.mpx_encode_accept_replies(self.h, _ptr(replies), _ptr(reply_to), n,
                                                       n_dest, _ptr(out), _ptr(off)),
                    "mpx_encode_accept_replies")
        return out[:int(off[-1])], off

    def encode_accept_replies_reserve(self, max_n):
        self._check(self.lib.mpx_encode_accept_replies_reserve(self.h, max_n),
                    "mpx_encode_accept_replies_reserve")

    def encode_accept_replies_dev(self, d_replies, d_reply_to, n, n_dest, d_out, d_off,
                                  stream=None):
        self._check(self.lib.mpx_encode_accept_replies_dev(self.h, d_replies, d_reply_to, n,
                                                           n_dest, d_out, d_off, stream),
                    "mpx_encode_accept_replies_dev")

    # ---- the proposer side: handlePropose and the Accept bytes --------------------------------
    def propose_handle(self, groups, prop_off, st, inst_base=0, ipg=None, lb=None):
        """groups: PROPOSER_GROUP (copied; crt_instance comes back advanced); prop_off u64[G+1]:
        group g's drained proposals; st: ACCEPTOR_STATE of the window (copied); lb: optional
        INST_STATE of the window (copied). Returns (groups, st, lb, sends ACCEPT_SEND, send_off
        u64[G+1])."""
        groups = np.array(np.atleast_1d(groups), dtype=R.PROPOSER_GROUP, copy=True)
        prop_off = _c(prop_off, np.uint64)
        st = np.array(st, dtype=R.ACCEPTOR_STATE, copy=True)
        lb = None if lb is None else np.array(lb, dtype=R.INST_STATE, copy=True)
        G = len(groups)
        ipg = (len(st) // G if G else 0) if ipg is None else ipg
        n = [int(prop_off[g + 1]) - int(prop_off[g]) for g in range(G)]
        cap = sum(-(-x // R.PROPOSE_MAX_BATCH) for x in n if x > 0)
        sends = np.zeros(max(cap, 1), R.ACCEPT_SEND)
        send_off = np.zeros(G + 1, np.uint64)
        rc = self.lib.mpx_propose_handle(self.h, _ptr(groups), G, _ptr(prop_off), _ptr(st),
                                         _ptr(lb), len(st), inst_base, ipg, _ptr(send_off),
                                         _ptr(sends), cap)
        self._check(rc, "mpx_propose_handle")
        return groups, st, lb, sends[:cap], send_off

    def propose_handle_dev(self, d_groups, n_groups, d_prop_off, d_send_off, d_st, d_lb, n_inst,
                           inst_base, ipg, d_sends, stream=None):
        rc = self.lib.mpx_propose_handle_dev(self.h, d_groups, n_groups, d_prop_off, d_send_off,
                                             d_st, d_lb, n_inst, inst_base, ipg, d_sends, stream)
        self._check(rc, "mpx_propose_handle_dev")

    def encode_accepts(self, sends, groups, cmds, inst_base=0, ipg=None, peer_commits=None,
                       log=None, thrifty=False, alive_mask=0xFFFF, out_cap=None):
        """sends: ACCEPT_SEND; groups: PROPOSER_GROUP; cmds: (op, key, val) the new commands;
        peer_commits: int32[G, N] (MIN); log: (recs LOG_REC[n_inst], cmd_off u64[n_inst+1], op,
        key, val) the window's log (MIN). Returns (bytes uint8, dest_off u64[N+1]): peer q's
        connection receives out[dest_off[q]:dest_off[q+1]]."""
        sends = _c(sends, R.ACCEPT_SEND)
        groups = _c(np.atleast_1d(groups), R.PROPOSER_GROUP)
        op, key, val = _c(cmds[0], np.uint8), _c(cmds[1], np.int64), _c(cmds[2], np.int64)
        G, N = len(groups), self.n_replicas
        keep = [sends, groups, op, key, val]
        b = _lib.MpxAcceptBatch()
        b.sends, b.n_sends, b.inst_base = _ptr(sends), len(sends), inst_base
        b.groups, b.n_groups = _ptr(groups), G
        b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = _ptr(op), _ptr(key), _ptr(val), len(op)
        b.flags = R.AB_THRIFTY if thrifty else 0
        b.alive_mask = alive_mask
        n_inst = 0
        if log is not None:
            lrec, lcoff = _c(log[0], R.LOG_REC), _c(log[1], np.uint64)
            lop, lkey, lval = _c(log[2], np.uint8), _c(log[3], np.int64), _c(log[4], np.int64)
            keep += [lrec, lcoff, lop, lkey, lval]
            n_inst = len(lrec)
            b.log_recs, b.log_cmd_off = _ptr(lrec), _ptr(lcoff)
            b.log_op, b.log_key, b.log_val, b.n_log_cmds = _ptr(lop), _ptr(lkey), _ptr(lval), len(lop)
        if peer_commits is not None:
            pc = _c(peer_commits, np.int32)
            keep.append(pc)
            b.peer_commits = _ptr(pc)
        if ipg is None and log is None:
            raise ValueError("encode_accepts: ipg is needed when no log gives the window's size")
        b.ipg = (n_inst // G if G else 0) if ipg is None else ipg
        if out_cap is None:  # every frame with its largest possible catch-up log
            sel = sends[(sends["flags"] & R.PH_ACCEPT) != 0]
            logb = 0
            if log is not None and n_inst:
                k = np.diff(lcoff.astype(np.int64))
                per = 18 * b.ipg + 17 * int(k.reshape(G, -1).sum(axis=1).max()) if G else 0
                logb = per
            out_cap = int((28 * len(sel) + 17 * int(sel["n_cmds"].sum()) + logb * len(sel)) * N)
        out = np.zeros(max(out_cap, 1), np.uint8)
        off = np.zeros(N + 1, np.uint64)
        rc = self.lib.mpx_encode_accepts(self.h, C.byref(b), _ptr(out), out_cap, _ptr(off))
        self._check(rc, "mpx_encode_accepts")
        del keep
        return out[:int(off[-1])], off

    def encode_accepts_reserve(self, max_sends, max_n_inst, max_log_cmds=0):
        self._check(self.lib.mpx_encode_accepts_reserve(self.h, max_sends, max_n_inst,
                                                        max_log_cmds),
                    "mpx_encode_accepts_reserve")

    def encode_accepts_dev(self, batch, d_out, out_cap, d_dest_off, stream=None):
        """batch: _lib.MpxAcceptBatch of device pointers"""
        self._check(self.lib.mpx_encode_accepts_dev(self.h, C.byref(batch), d_out, out_cap,
                                                    d_dest_off, stream),
                    "mpx_encode_accepts_dev")

    def encode_accepts_stored(self, sends, groups, cmds, inst_base=0, ipg=None, peer_commits=None,
                              st=None, lb=None, inst=None, arena=None, thrifty=False,
                              alive_mask=0xFFFF, out_cap=None):
        """encode_accepts with the catch-up log read from the instance store: st ACCEPTOR_STATE
        [n_inst] (ballot, status), lb optional INST_STATE[n_inst] (its non-nil status wins), inst
        INST_CMDS[n_inst] and arena (op, key, val) they point into (MIN; CLASSIC reads none of
        them). Returns (bytes uint8, dest_off u64[N+1]) like encode_accepts."""
        sends = _c(sends, R.ACCEPT_SEND)
        groups = _c(np.atleast_1d(groups), R.PROPOSER_GROUP)
        op, key, val = _c(cmds[0], np.uint8), _c(cmds[1], np.int64), _c(cmds[2], np.int64)
        G, N = len(groups), self.n_replicas
        keep = [sends, groups, op, key, val]
        b = _lib.MpxAcceptStoreBatch()
        b.sends, b.n_sends, b.inst_base = _ptr(sends), len(sends), inst_base
        b.groups, b.n_groups = _ptr(groups), G
        b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = _ptr(op), _ptr(key), _ptr(val), len(op)
        b.flags = R.AB_THRIFTY if thrifty else 0
        b.alive_mask = alive_mask
        n_inst = 0
        if st is not None:
            st = _c(st, R.ACCEPTOR_STATE)
            keep.append(st)
            n_inst, b.st = len(st), _ptr(st)
        if lb is not None:
            lb = _c(lb, R.INST_STATE)
            keep.append(lb)
            b.lb = _ptr(lb)
        if inst is not None:
            inst = _c(inst, R.INST_CMDS)
            keep.append(inst)
            b.inst = _ptr(inst)
        if arena is not None:
            sop, skey, sval = _c(arena[0], np.uint8), _c(arena[1], np.int64), _c(arena[2], np.int64)
            keep += [sop, skey, sval]
            b.src_op, b.src_key, b.src_val, b.n_src = _ptr(sop), _ptr(skey), _ptr(sval), len(sop)
        if peer_commits is not None:
            pc = _c(peer_commits, np.int32)
            keep.append(pc)
            b.peer_commits = _ptr(pc)
        if ipg is None and st is None:
            raise ValueError("encode_accepts_stored: ipg is needed when no st gives the window's size")
        b.ipg = (n_inst // G if G else 0) if ipg is None else ipg
        if out_cap is None:  # every frame with its group's largest possible catch-up log
            sel = sends[(sends["flags"] & R.PH_ACCEPT) != 0]
            logb = 0
            if inst is not None and n_inst and G:
                k = np.where(inst["flags"] & R.IC_HAS_CMDS, inst["n_cmds"], 0).astype(np.int64)
                logb = 18 * b.ipg + 17 * int(k.reshape(G, -1).sum(axis=1).max())
            out_cap = int((28 * len(sel) + 17 * int(sel["n_cmds"].sum()) + logb * len(sel)) * N)
        out = np.zeros(max(out_cap, 1), np.uint8)
        off = np.zeros(N + 1, np.uint64)
        rc = self.lib.mpx_encode_accepts_stored(self.h, C.byref(b), _ptr(out), out_cap, _ptr(off))
        self._check(rc, "mpx_encode_accepts_stored")
        del keep
        return out[:int(off[-1])], off

    def encode_accepts_stored_reserve(self, max_sends, max_n_inst):
        self._check(self.lib.mpx_encode_accepts_stored_reserve(self.h, max_sends, max_n_inst),
                    "mpx_encode_accepts_stored_reserve")

    def encode_accepts_stored_dev(self, batch, d_out, out_cap, d_dest_off, stream=None):
        """batch: _lib.MpxAcceptStoreBatch of device pointers"""
        self._check(self.lib.mpx_encode_accepts_stored_dev(self.h, C.byref(batch), d_out, out_cap,
                                                           d_dest_off, stream),
                    "mpx_encode_accepts_stored_dev")

    # ---- Accept / Commit / PrepareReply payloads: Unmarshal in a batch -------------------------
    def unmarshal_frames(self, buf, var, caps=None):
        """buf: the bytes decode_stream framed; var: its VAR_FRAME records. Returns (arrays,
        mpx_unmarshal_result): a dict of R.UNMARSHAL_ARRAYS, each trimmed to its count. caps
        (optional): (accept, commit, cmd, log_inst, log_cmd) capacities, None = what the frames
        need; arrays come back trimmed to min(count, capacity)."""
        buf = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else \
            _c(buf, np.uint8)
        var = _c(var, R.VAR_FRAME)
        n, nv = len(buf), len(var)
        need = (int((var["code"] == R.PEER_ACCEPT).sum()), int((var["code"] == R.PEER_COMMIT).sum()),
                int(var["n_cmds"].astype(np.int64).sum()), int(var["n_log"].astype(np.int64).sum()),
                n // 17)
        ca, cc, cm, cl, clm = [w if c is None else c for c, w in zip(caps or (None,) * 5, need)]
        a = {"accepts": np.zeros(ca, R.ACCEPT_MSG), "accept_last_committed": np.zeros(ca, np.int32),
             "commits": np.zeros(cc, R.ACCEPT_MSG), "cmd_off": np.zeros(nv + 1, np.uint64),
             "op": np.zeros(cm, np.uint8), "key": np.zeros(cm, np.int64),
             "val": np.zeros(cm, np.int64), "log_inst_off": np.zeros(nv + 1, np.uint64),
             "log_recs": np.zeros(cl, R.LOG_REC), "log_cmd_off": np.zeros(cl + 1, np.uint64),
             "log_op": np.zeros(clm, np.uint8), "log_key": np.zeros(clm, np.int64),
             "log_val": np.zeros(clm, np.int64)}
        out = _lib.MpxUnmarshalOut()
        for name in R.UNMARSHAL_ARRAYS:
            setattr(out, name, _ptr(a[name]) if len(a[name]) else None)
        out.accept_cap, out.commit_cap, out.cmd_cap = ca, cc, cm
        out.log_inst_cap, out.log_cmd_cap = cl, clm
        res = np.zeros(1, R.UNMARSHAL_RESULT)
        self._check(self.lib.mpx_unmarshal_frames(self.h, _ptr(buf), n, _ptr(var), nv,
                                                  C.byref(out), _ptr(res)),
                    "mpx_unmarshal_frames")
        r = res[0]
        na, nc = min(int(r["n_accepts"]), ca), min(int(r["n_commits"]), cc)
        m, li = min(int(r["n_cmds"]), cm), min(int(r["n_log_inst"]), cl)
        lm = min(int(r["n_log_cmds"]), clm)
        trim = {"accepts": na, "accept_last_committed": na, "commits": nc, "op": m, "key": m,
                "val": m, "log_recs": li, "log_cmd_off": li + 1, "log_op": lm, "log_key": lm,
                "log_val": lm}
        return {k: v[:trim.get(k, len(v))] for k, v in a.items()}, r

    def unmarshal_frames_reserve(self, max_var, max_log_inst):
        self._check(self.lib.mpx_unmarshal_frames_reserve(self.h, max_var, max_log_inst),
                    "mpx_unmarshal_frames_reserve")

    def unmarshal_frames_dev(self, d_buf, n, d_var, n_var, d_n_var, out, d_res, stream=None):
        """out: _lib.MpxUnmarshalOut of device pointers; d_n_var: optional device u64 (the frame
        count mpx_decode_stream_dev left); d_res: device mpx_unmarshal_result"""
        self._check(self.lib.mpx_unmarshal_frames_dev(self.h, d_buf, n, d_var, n_var, d_n_var,
                                                      C.byref(out), d_res, stream),
                    "mpx_unmarshal_frames_dev")

    # ---- the commit side: handleCommit[Short], the Commit bytes, CommitShort records -----------
    def commit_handle(self, msgs, st, committed_upto, inst_base=0, ipg=None, want_log=True):
        """msgs: ACCEPT_MSG grouped by instance, ascending (value_id R.VALUE_KEEP = CommitShort);
        st: ACCEPTOR_STATE of the window (copied); committed_upto: int32 per group (copied).
        Returns (st, committed_upto, effect uint8[n], log_recs LOG_REC[n] or None)."""
        msgs = _c(msgs, R.ACCEPT_MSG)
        st = np.array(st, dtype=R.ACCEPTOR_STATE, copy=True)
        cu = np.array(np.atleast_1d(committed_upto), dtype=np.int32, copy=True)
        n, G = len(msgs), len(cu)
        ipg = (len(st) // G if G else 0) if ipg is None else ipg
        eff = np.zeros(max(n, 1), np.uint8)
        log = np.zeros(max(n, 1), R.LOG_REC) if want_log else None
        rc = self.lib.mpx_commit_handle(self.h, _ptr(msgs), n, _ptr(st), len(st), inst_base,
                                        _ptr(cu), G, ipg, _ptr(eff), _ptr(log))
        self._check(rc, "mpx_commit_handle")
        return st, cu, eff[:n], (log[:n] if want_log else None)

    def commit_handle_dev(self, d_msgs, n, d_st, n_inst, inst_base, d_committed_upto, n_groups,
                          ipg, d_effect, d_log_recs=None, stream=None):
        rc = self.lib.mpx_commit_handle_dev(self.h, d_msgs, n, d_st, n_inst, inst_base,
                                            d_committed_upto, n_groups, ipg, d_effect, d_log_recs,
                                            stream)
        self._check(rc, "mpx_commit_handle_dev")

    def encode_commits(self, sends, groups, cmds, inst_base=0, ipg=1, thrifty=False,
                       alive_mask=0xFFFF, out_cap=None):
        """sends: COMMIT_SEND (slots without R.CS_SEND are skipped); groups: PROPOSER_GROUP (only
        self_id is read), group g owning window indices [g*ipg, (g+1)*ipg); cmds: (op, key, val).
        Returns (bytes uint8, dest_off u64[N+1]): peer q's connection receives
        out[dest_off[q]:dest_off[q+1]], CommitShort and Commit frames in send order."""
        sends = _c(sends, R.COMMIT_SEND)
        groups = _c(np.atleast_1d(groups), R.PROPOSER_GROUP)
        op, key, val = _c(cmds[0], np.uint8), _c(cmds[1], np.int64), _c(cmds[2], np.int64)
        N = self.n_replicas
        b = _lib.MpxCommitBatch()
        b.sends, b.n_sends, b.inst_base, b.ipg = _ptr(sends), len(sends), inst_base, ipg
        b.groups, b.n_groups = _ptr(groups), len(groups)
        b.cmd_op, b.cmd_key, b.cmd_val, b.n_cmds = _ptr(op), _ptr(key), _ptr(val), len(op)
        b.flags = R.AB_THRIFTY if thrifty else 0
        b.alive_mask = alive_mask
        if out_cap is None:  # every send as a full Commit to every peer
            sel = sends[(sends["flags"] & R.CS_SEND) != 0]
            out_cap = int((18 * len(sel) + 17 * int(sel["n_cmds"].sum())) * N)
        out = np.zeros(max(out_cap, 1), np.uint8)
        off = np.zeros(N + 1, np.uint64)
        rc = self.lib.mpx_encode_commits(self.h, C.byref(b), _ptr(out), out_cap, _ptr(off))
        self._check(rc, "mpx_encode_commits")
        return out[:int(off[-1])], off

    def encode_commits_reserve(self, max_sends, max_other=0):
        self._check(self.lib.mpx_encode_commits_reserve(self.h, max_sends, max_other),
                    "mpx_encode_commits_reserve")

    def encode_commits_dev(self, batch, d_out, out_cap, d_dest_off, stream=None):
        """batch: _lib.MpxCommitBatch of device pointers"""
        self._check(self.lib.mpx_encode_commits_dev(self.h, C.byref(batch), d_out, out_cap,
                                                    d_dest_off, stream),
                    "mpx_encode_commits_dev")

    def gather_commit_shorts(self, buf, other, cap=None):
        """buf: the bytes decode_stream framed; other: its PEER_FRAME records. Returns (msgs
        ACCEPT_MSG, count int32, frame_index uint32, n_shorts): the CommitShort frames in stream
        order, trimmed to min(n_shorts, cap)."""
        buf = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else \
            _c(buf, np.uint8)
        other = _c(other, R.PEER_FRAME)
        cap = int((other["code"] == R.PEER_COMMIT_SHORT).sum()) if cap is None else cap
        msgs = np.zeros(max(cap, 1), R.ACCEPT_MSG)
        cnt = np.zeros(max(cap, 1), np.int32)
        idx = np.zeros(max(cap, 1), np.uint32)
        ns = np.zeros(1, np.uint64)
        rc = self.lib.mpx_gather_commit_shorts(self.h, _ptr(buf), len(buf), _ptr(other),
                                               len(other), _ptr(msgs), _ptr(cnt), _ptr(idx), cap,
                                               _ptr(ns))
        self._check(rc, "mpx_gather_commit_shorts")
        k = min(int(ns[0]), cap)
        return msgs[:k], cnt[:k], idx[:k], int(ns[0])

    def gather_commit_shorts_dev(self, d_buf, n, d_other, n_other, d_n_other, d_msgs, d_count,
                                 d_frame_index, cap, d_n_shorts, stream=None):
        self._check(self.lib.mpx_gather_commit_shorts_dev(self.h, d_buf, n, d_other, n_other,
                                                          d_n_other, d_msgs, d_count,
                                                          d_frame_index, cap, d_n_shorts, stream),
                    "mpx_gather_commit_shorts_dev")

    # ---- the prepare side: Prepare records, handlePrepare, the PrepareReply bytes --------------
    def _reply_dtype(self):
        return R.PREPARE_REPLY_MIN if self.mode == R.MODE_MIN else R.PREPARE_REPLY

    def gather_prepares(self, buf, other, group=0, cap=None):
        """buf: the bytes decode_stream framed; other: its PEER_FRAME records; group: the Replica
        the connection belongs to (MIN: it fills key). Returns (msgs PREPARE_MSG, frame_index
        uint32, n_prepares): the Prepare frames in stream order, trimmed to min(n_prepares, cap)."""
        buf = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else \
            _c(buf, np.uint8)
        other = _c(other, R.PEER_FRAME)
        cap = int((other["code"] == R.PEER_PREPARE).sum()) if cap is None else cap
        msgs = np.zeros(max(cap, 1), R.PREPARE_MSG)
        idx = np.zeros(max(cap, 1), np.uint32)
        ns = np.zeros(1, np.uint64)
        rc = self.lib.mpx_gather_prepares(self.h, _ptr(buf), len(buf), _ptr(other), len(other),
                                          group, _ptr(msgs), _ptr(idx), cap, _ptr(ns))
        self._check(rc, "mpx_gather_prepares")
        k = min(int(ns[0]), cap)
        return msgs[:k], idx[:k], int(ns[0])

    def gather_prepares_dev(self, d_buf, n, d_other, n_other, d_n_other, group, d_msgs,
                            d_frame_index, cap, d_n_prepares, stream=None):
        self._check(self.lib.mpx_gather_prepares_dev(self.h, d_buf, n, d_other, n_other, d_n_other,
                                                     group, d_msgs, d_frame_index, cap,
                                                     d_n_prepares, stream),
                    "mpx_gather_prepares_dev")

    def prepare_handle(self, msgs, st, groups, inst_base=0, ipg=None, gps=None,
                       peer_commits=None):
        """msgs: PREPARE_MSG grouped by key, ascending; st: ACCEPTOR_STATE of the window (read
        only); groups: PROPOSER_GROUP (copied). gps / peer_commits (MIN, optional, copied): the
        GROUP_PREP_STATE array and the int32 [G * N] rows a raised ballot resets. Returns a dict:
        groups, replies (PREPARE_REPLY_MIN or PREPARE_REPLY), reply_to int32, effect uint8,
        log_from int32 (MIN, else None), gps, peer_commits."""
        msgs = _c(msgs, R.PREPARE_MSG)
        st = _c(st, R.ACCEPTOR_STATE)
        groups = np.array(np.atleast_1d(groups), dtype=R.PROPOSER_GROUP, copy=True)
        n, G = len(msgs), len(groups)
        ipg = (len(st) // G if G else 0) if ipg is None else ipg
        minm = self.mode == R.MODE_MIN
        if gps is not None:
            gps = np.array(gps, dtype=R.GROUP_PREP_STATE, copy=True)
        if peer_commits is not None:
            peer_commits = np.array(peer_commits, dtype=np.int32, copy=True)
        rep = np.zeros(max(n, 1), self._reply_dtype())
        to = np.zeros(max(n, 1), np.int32)
        eff = np.zeros(max(n, 1), np.uint8)
        lf = np.zeros(max(n, 1), np.int32) if minm else None
        rc = self.lib.mpx_prepare_handle(self.h, _ptr(msgs), n, _ptr(st), len(st), inst_base,
                                         _ptr(groups), G, ipg, _ptr(gps), _ptr(peer_commits),
                                         _ptr(rep), _ptr(to), _ptr(eff), _ptr(lf))
        self._check(rc, "mpx_prepare_handle")
        return {"groups": groups, "replies": rep[:n], "reply_to": to[:n], "effect": eff[:n],
                "log_from": lf[:n] if minm else None, "gps": gps, "peer_commits": peer_commits}

    def prepare_handle_dev(self, d_msgs, n, d_st, n_inst, inst_base, d_groups, n_groups, ipg,
                           d_replies, d_reply_to, d_effect, d_log_from=None, d_gps=None,
                           d_peer_commits=None, stream=None):
        rc = self.lib.mpx_prepare_handle_dev(self.h, d_msgs, n, d_st, n_inst, inst_base, d_groups,
                                             n_groups, ipg, d_gps, d_peer_commits, d_replies,
                                             d_reply_to, d_effect, d_log_from, stream)
        self._check(rc, "mpx_prepare_handle_dev")

    def encode_prepare_replies(self, replies, reply_to, log_from=None, n_dest=None, inst_base=0,
                               st=None, lb=None, inst=None, arena=None, out_cap=None):
        """replies / reply_to / log_from: prepare_handle's outputs; st ACCEPTOR_STATE[n_inst], lb
        optional INST_STATE[n_inst], inst INST_CMDS[n_inst] and arena (op, key, val) they point
        into. Returns (bytes uint8, dest_off u64[n_dest+1]): leader d's connection receives
        out[dest_off[d]:dest_off[d+1]], PrepareReply frames in array order."""
        replies = _c(replies, self._reply_dtype())
        reply_to = _c(reply_to, np.int32)
        n_dest = self.n_replicas if n_dest is None else n_dest
        keep = [replies, reply_to]
        b = _lib.MpxPrepareReplyBatch()
        b.replies, b.reply_to, b.n, b.n_dest = _ptr(replies), _ptr(reply_to), len(replies), n_dest
        b.inst_base = inst_base
        if log_from is not None:
            log_from = _c(log_from, np.int32)
            keep.append(log_from)
            b.log_from = _ptr(log_from)
        if st is not None:
            st = _c(st, R.ACCEPTOR_STATE)
            keep.append(st)
            b.st = _ptr(st)
        if lb is not None:
            lb = _c(lb, R.INST_STATE)
            keep.append(lb)
            b.lb = _ptr(lb)
        if inst is not None:
            inst = _c(inst, R.INST_CMDS)
            keep.append(inst)
            b.inst, b.n_inst = _ptr(inst), len(inst)
        if arena is not None:
            sop, skey, sval = _c(arena[0], np.uint8), _c(arena[1], np.int64), _c(arena[2], np.int64)
            keep += [sop, skey, sval]
            b.src_op, b.src_key, b.src_val, b.n_src = _ptr(sop), _ptr(skey), _ptr(sval), len(sop)
        if out_cap is None:  # every frame with every instance of the window in its log
            k = 0
            if inst is not None and len(inst):
                k = int(np.where(inst["flags"] & R.IC_HAS_CMDS, inst["n_cmds"], 0).astype(np.int64).sum())
            out_cap = len(replies) * (28 + 18 * b.n_inst + 2 * 17 * k)
        out = np.zeros(max(out_cap, 1), np.uint8)
        off = np.zeros(n_dest + 1, np.uint64)
        rc = self.lib.mpx_encode_prepare_replies(self.h, C.byref(b), _ptr(out), out_cap, _ptr(off))
        self._check(rc, "mpx_encode_prepare_replies")
        del keep
        return out[:int(off[-1])], off

    def encode_prepare_replies_reserve(self, max_n, max_n_inst, n_dest=None):
        n_dest = self.n_replicas if n_dest is None else n_dest
        self._check(self.lib.mpx_encode_prepare_replies_reserve(self.h, max_n, max_n_inst, n_dest),
                    "mpx_encode_prepare_replies_reserve")

    def encode_prepare_replies_dev(self, batch, d_out, out_cap, d_dest_off, stream=None):
        """batch: _lib.MpxPrepareReplyBatch of device pointers"""
        self._check(self.lib.mpx_encode_prepare_replies_dev(self.h, C.byref(batch), d_out, out_cap,
                                                            d_dest_off, stream),
                    "mpx_encode_prepare_replies_dev")

    # ---- batch assembly: several connections' records as one legal handler batch -------------
    def order_records(self, sources, n_inst, inst_base=0, arrivals=None, arrival_bits=0,
                      want_perm=True, general=False):
        """sources: record arrays of one 16-byte dtype (ACCEPT_REPLY or ACCEPT_MSG), each in
        arrival order; arrivals: None, or one uint32 array per source. Returns (records, perm
        uint32 or None, result ORDER_RESULT scalar): the stable sort by instance (then arrival)
        of the concatenation. general: R.ORDER_GENERAL, the radix path at any size."""
        srcs = [np.ascontiguousarray(s) for s in sources]
        dt = srcs[0].dtype if srcs else R.ACCEPT_REPLY
        assert all(s.dtype == dt for s in srcs) and dt.itemsize == 16
        arrs = [None] * len(srcs) if arrivals is None else \
            [None if a is None else _c(a, np.uint32) for a in arrivals]
        assert all(a is None or len(a) == len(s) for a, s in zip(arrs, srcs))
        arr = (_lib.MpxOrderSrc * max(len(srcs), 1))()
        for i, s in enumerate(srcs):
            arr[i].recs, arr[i].n = _ptr(s) if len(s) else None, len(s)
            arr[i].arrival = _ptr(arrs[i]) if len(s) else None
        n = sum(len(s) for s in srcs)
        out = np.zeros(max(n, 1), dt)
        perm = np.zeros(max(n, 1), np.uint32) if want_perm else None
        res = _lib.MpxOrderResult()
        rc = self.lib.mpx_order_records(self.h, arr, len(srcs), n_inst, inst_base, arrival_bits,
                                        R.ORDER_GENERAL if general else 0, _ptr(out), _ptr(perm),
                                        C.byref(res))
        self._check(rc, "mpx_order_records")
        r = np.zeros((), R.ORDER_RESULT)
        for f in R.ORDER_RESULT.names:
            r[f] = getattr(res, f)
        return out[:n], (perm[:n] if want_perm else None), r

    def order_records_reserve(self, max_n, max_n_inst):
        self._check(self.lib.mpx_order_records_reserve(self.h, max_n, max_n_inst),
                    "mpx_order_records_reserve")

    def order_records_dev(self, srcs, n_inst, inst_base, arrival_bits, d_out, d_perm, d_res,
                          general=False, stream=None):
        """srcs: (d_recs, d_arrival or None, n) per source, device pointers"""
        arr = (_lib.MpxOrderSrc * max(len(srcs), 1))()
        for i, (d_recs, d_arr, n) in enumerate(srcs):
            arr[i].recs, arr[i].arrival, arr[i].n = d_recs, d_arr, n
        rc = self.lib.mpx_order_records_dev(self.h, arr, len(srcs), n_inst, inst_base,
                                            arrival_bits, R.ORDER_GENERAL if general else 0,
                                            d_out, d_perm, d_res, stream)
        self._check(rc, "mpx_order_records_dev")

    # ---- client bytes in: Propose decode over many connections --------------------------------
    @staticmethod
    def client_layout(bufs, groups=None):
        """Lay per-connection byte strings out at R.CLIENT_ALIGN-byte offsets. Returns (buf uint8,
        conns CLIENT_CONN)."""
        conns = np.zeros(len(bufs), R.CLIENT_CONN)
        at = 0
        for k, b in enumerate(bufs):
            conns[k] = (at, len(b), 0 if groups is None else groups[k])
            at += -(-len(b) // R.CLIENT_ALIGN) * R.CLIENT_ALIGN
        buf = np.zeros(at, np.uint8)
        for k, b in enumerate(bufs):
            o = int(conns["offset"][k])
            buf[o:o + len(b)] = np.frombuffer(bytes(b), np.uint8)
        return buf, conns

    def decode_client_streams(self, bufs, groups=None, n_groups=1, prop_cap=None, buf=None,
                              conns=None):
        """bufs: one bytes per client connection (its unread bytes, after the connection-type
        byte); groups: the connections' groups, non-decreasing. Or a ready layout (buf, conns).
        Returns a dict: op, key, val, meta (PROPOSAL) trimmed to min(n_proposals, prop_cap),
        prop_off, send_off (u64[n_groups + 1]), conn_res (CLIENT_CONN_RESULT per connection) and
        res (CLIENT_RESULT scalar)."""
        if buf is None:
            buf, conns = self.client_layout(bufs, groups)
        buf, conns = _c(buf, np.uint8), _c(conns, R.CLIENT_CONN)
        n, nc = len(buf), len(conns)
        cap = n // R.CLIENT_PROPOSE_FRAME if prop_cap is None else prop_cap
        op, key, val = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.int64), \
            np.zeros(max(cap, 1), np.int64)
        meta = np.zeros(max(cap, 1), R.PROPOSAL)
        po, so = np.zeros(n_groups + 1, np.uint64), np.zeros(n_groups + 1, np.uint64)
        cres = np.zeros(max(nc, 1), R.CLIENT_CONN_RESULT)
        out = _lib.MpxClientOut(_ptr(op), _ptr(key), _ptr(val), _ptr(meta), cap,
                                _ptr(po) if n_groups else None, _ptr(so) if n_groups else None)
        res = _lib.MpxClientResult()
        rc = self.lib.mpx_decode_client_streams(self.h, _ptr(buf), n, _ptr(conns), nc, n_groups,
                                                C.byref(out), _ptr(cres), C.byref(res))
        self._check(rc, "mpx_decode_client_streams")
        r = np.zeros((), R.CLIENT_RESULT)
        for f in R.CLIENT_RESULT.names:
            r[f] = getattr(res, f)
        k = min(int(r["n_proposals"]), cap)
        return dict(op=op[:k], key=key[:k], val=val[:k], meta=meta[:k], prop_off=po, send_off=so,
                    conn_res=cres[:nc], res=r)

    def decode_client_streams_reserve(self, max_len, max_conns, max_groups):
        self._check(self.lib.mpx_decode_client_streams_reserve(self.h, max_len, max_conns,
                                                               max_groups),
                    "mpx_decode_client_streams_reserve")

    def decode_client_streams_dev(self, d_buf, n, d_conns, n_conns, n_groups, out, d_conn_res,
                                  d_res, stream=None):
        """out: _lib.MpxClientOut of device pointers; d_conns: device CLIENT_CONN array"""
        rc = self.lib.mpx_decode_client_streams_dev(self.h, d_buf, n, d_conns, n_conns, n_groups,
                                                    C.byref(out), d_conn_res, d_res, stream)
        self._check(rc, "mpx_decode_client_streams_dev")

    # ---- reply assembly: the client reply records from sends, masks, ret and meta --------------
    def build_replies(self, kind, sends, meta, mask=None, inst_base=0, ret=None, ret_first=None,
                      cap=None, pad_client=None, want_commit_sends=False, general=False):
        """kind: R.RB_FALSE / RB_DECIDED / RB_EXECUTED; sends: ACCEPT_SEND; meta: PROPOSAL of the
        proposal arrays first_cmd indexes; mask: optional uint8 per window index from inst_base;
        ret: int64 (EXECUTED); ret_first: optional u64 per slot. cap: None = what the call needs
        (with pad_client: that and one more). Returns (recs REPLY_REC trimmed to what was written,
        commit_sends COMMIT_SEND or None, result REPLY_RESULT scalar)."""
        sends, meta = _c(sends, R.ACCEPT_SEND), _c(meta, R.PROPOSAL)
        mask = None if mask is None else _c(mask, np.uint8)
        ret = None if ret is None else _c(ret, np.int64)
        ret_first = None if ret_first is None else _c(ret_first, np.uint64)
        n = len(sends)
        if cap is None:
            cap = int(sends["n_cmds"].astype(np.int64).sum()) + (pad_client is not None)
        recs = np.zeros(max(cap, 1), R.REPLY_REC)
        cs = np.zeros(max(n, 1), R.COMMIT_SEND) if want_commit_sends else None
        b = _lib.MpxReplyBatch(_ptr(sends) if n else None, n, inst_base,
                               0 if mask is None else len(mask), _ptr(meta) if len(meta) else None,
                               len(meta), _ptr(mask), _ptr(ret), 0 if ret is None else len(ret),
                               _ptr(ret_first), kind, R.RB_GENERAL if general else 0,
                               R.RB_NO_PAD if pad_client is None else pad_client, 0)
        res = _lib.MpxReplyResult()
        rc = self.lib.mpx_build_replies(self.h, C.byref(b), _ptr(recs) if cap else None, cap,
                                        _ptr(cs), C.byref(res))
        self._check(rc, "mpx_build_replies")
        r = np.zeros((), R.REPLY_RESULT)
        r["n_replies"], r["n_slots"] = res.n_replies, res.n_slots
        k = cap if pad_client is not None else min(int(res.n_replies), cap)
        return recs[:k], (cs[:n] if want_commit_sends else None), r

    def build_replies_reserve(self, max_sends):
        self._check(self.lib.mpx_build_replies_reserve(self.h, max_sends),
                    "mpx_build_replies_reserve")

    def build_replies_dev(self, batch, d_recs, cap, d_commit_sends, d_res, stream=None):
        """batch: _lib.MpxReplyBatch of device pointers (reply_batch_dev builds one)"""
        self._check(self.lib.mpx_build_replies_dev(self.h, C.byref(batch), d_recs, cap,
                                                   d_commit_sends, d_res, stream),
                    "mpx_build_replies_dev")

    @staticmethod
    def reply_batch_dev(kind, d_sends, n_sends, d_meta, n_props, d_mask=None, n_inst=0,
                        inst_base=0, d_ret=None, n_ret=0, d_ret_first=None, pad_client=None,
                        general=False):
        """the mpx_reply_batch of a build_replies_dev call; every d_* is a device pointer or a
        devbuf.DevArray"""
        p = [getattr(x, "ptr", x) for x in (d_sends, d_meta, d_mask, d_ret, d_ret_first)]
        return _lib.MpxReplyBatch(p[0], n_sends, inst_base, n_inst, p[1], n_props, p[2], p[3],
                                  n_ret, p[4], kind, R.RB_GENERAL if general else 0,
                                  R.RB_NO_PAD if pad_client is None else pad_client, 0)

    # ---- execute assembly: executeCommands' walk and the gather of its commands ----------------
    def execute_gather(self, inst, committed_upto, executed, cmds, inst_base=0, ipg=None,
                       sends=None, cap=None, pad=False, general=False, want_inst_first=True,
                       want_grp_cmd_off=True):
        """inst: INST_CMDS per window slot; committed_upto, executed: int32 per group (executed is
        copied); cmds: (op, key, val) source arrays; sends: optional ACCEPT_SEND, for ret_first.
        cap: None = what the call needs. Returns a dict: op, key, val (trimmed to what was
        written), mask, executed, inst_first, ret_first, grp_cmd_off (None where not asked for) and
        res (EXECUTE_RESULT scalar)."""
        inst = _c(inst, R.INST_CMDS)
        cu = _c(np.atleast_1d(committed_upto), np.int32)
        ex = np.array(np.atleast_1d(executed), dtype=np.int32, copy=True)
        op, key, val = _c(cmds[0], np.uint8), _c(cmds[1], np.int64), _c(cmds[2], np.int64)
        sends = None if sends is None else _c(sends, R.ACCEPT_SEND)
        n, G, n_src = len(inst), len(cu), len(op)
        ipg = (n // G if G else 0) if ipg is None else ipg
        if cap is None:
            cap = int(inst["n_cmds"].astype(np.int64).sum())
        o_op, o_key, o_val = (np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.int64),
                              np.zeros(max(cap, 1), np.int64))
        mask = np.zeros(max(n, 1), np.uint8)
        ifirst = np.zeros(max(n, 1), np.uint64) if want_inst_first else None
        rf = None if sends is None else np.zeros(max(len(sends), 1), np.uint64)
        goff = np.zeros(G + 1, np.uint64) if want_grp_cmd_off else None
        b = _lib.MpxExecuteBatch(_ptr(inst) if n else None, n, inst_base, ipg, G, _ptr(cu), _ptr(ex),
                                 _ptr(ex), _ptr(op) if n_src else None,
                                 _ptr(key) if n_src else None, _ptr(val) if n_src else None, n_src,
                                 _ptr(sends), 0 if sends is None else len(sends),
                                 (R.XG_PAD if pad else 0) | (R.XG_GENERAL if general else 0), 0)
        out = _lib.MpxExecuteOut(_ptr(o_op) if cap else None, _ptr(o_key) if cap else None,
                                 _ptr(o_val) if cap else None, cap, _ptr(mask), _ptr(ifirst),
                                 _ptr(rf), _ptr(goff))
        res = _lib.MpxExecuteResult()
        rc = self.lib.mpx_execute_gather(self.h, C.byref(b), C.byref(out), C.byref(res))
        self._check(rc, "mpx_execute_gather")
        r = np.zeros((), R.EXECUTE_RESULT)
        r["n_cmds"], r["n_inst"], r["n_groups"], r["reserved"] = (res.n_cmds, res.n_inst,
                                                                  res.n_groups, res.reserved)
        k = cap if pad else min(int(res.n_cmds), cap)
        return dict(op=o_op[:k], key=o_key[:k], val=o_val[:k], mask=mask[:n], executed=ex,
                    inst_first=None if ifirst is None else ifirst[:n],
                    ret_first=None if rf is None else rf[:len(sends)], grp_cmd_off=goff, res=r)

    def execute_gather_reserve(self, max_n_inst, max_n_groups):
        self._check(self.lib.mpx_execute_gather_reserve(self.h, max_n_inst, max_n_groups),
                    "mpx_execute_gather_reserve")

    def execute_gather_dev(self, batch, out, d_res, stream=None):
        """batch: _lib.MpxExecuteBatch, out: _lib.MpxExecuteOut, both of device pointers
        (execute_batch_dev / execute_out_dev build them)"""
        self._check(self.lib.mpx_execute_gather_dev(self.h, C.byref(batch), C.byref(out), d_res,
                                                    stream), "mpx_execute_gather_dev")

    @staticmethod
    def execute_batch_dev(d_inst, n_inst, inst_base, ipg, n_groups, d_committed_upto, d_executed_in,
                          d_executed_out, d_src_op, d_src_key, d_src_val, n_src, d_sends=None,
                          n_sends=0, pad=False, general=False):
        """the mpx_execute_batch of an execute_gather_dev call; every d_* is a device pointer or a
        devbuf.DevArray"""
        p = [getattr(x, "ptr", x) for x in (d_inst, d_committed_upto, d_executed_in, d_executed_out,
                                            d_src_op, d_src_key, d_src_val, d_sends)]
        return _lib.MpxExecuteBatch(p[0], n_inst, inst_base, ipg, n_groups, p[1], p[2], p[3], p[4],
                                    p[5], p[6], n_src, p[7], n_sends,
                                    (R.XG_PAD if pad else 0) | (R.XG_GENERAL if general else 0), 0)

    @staticmethod
    def execute_out_dev(d_op, d_key, d_val, cap, d_mask, d_inst_first=None, d_ret_first=None,
                        d_grp_cmd_off=None):
        p = [getattr(x, "ptr", x) for x in (d_op, d_key, d_val, d_mask, d_inst_first, d_ret_first,
                                            d_grp_cmd_off)]
        return _lib.MpxExecuteOut(p[0], p[1], p[2], cap, p[3], p[4], p[5], p[6])

    # ---- store assembly: instance commands into a command arena, and its compaction ------------
    @staticmethod
    def _store_srcs(sources, ptr_of):
        """the mpx_store_src array of sources = [dict(cmd_off=, op=, key=, val=, n_recs=)];
        returns (ctypes array, what must stay alive)"""
        arr = (_lib.MpxStoreSrc * max(len(sources), 1))()
        keep = []
        for s, x in enumerate(sources):
            off = x.get("cmd_off")
            n_cmds = x["n_cmds"] if "n_cmds" in x else len(x["op"])
            n_frames = x["n_frames"] if "n_frames" in x else (0 if off is None else len(off) - 1)
            p = [ptr_of(x.get(k), keep, t) for k, t in (("cmd_off", np.uint64), ("op", np.uint8),
                                                        ("key", np.int64), ("val", np.int64))]
            arr[s] = _lib.MpxStoreSrc(p[0], n_frames, p[1], p[2], p[3], n_cmds, x["n_recs"])
        return arr, keep

    def store_commands(self, kind, items, sources, arena, used, inst, inst_base=0, effect=None,
                       perm=None, store_mask=R.AH_STORED, general=False):
        """kind: R.SC_MSGS (items ACCEPT_MSG, effect uint8 per item) or R.SC_SENDS (items
        ACCEPT_SEND); sources: a list of dicts cmd_off / op / key / val / n_recs (SENDS: the
        proposal arrays, cmd_off None); arena: (op, key, val) arrays of one capacity, appended to IN
        PLACE from `used`; inst: INST_CMDS window, written IN PLACE. Returns (used after the call,
        result STORE_RESULT scalar)."""
        items = _c(items, R.ACCEPT_SEND if kind == R.SC_SENDS else R.ACCEPT_MSG)
        effect = None if effect is None else _c(effect, np.uint8)
        perm = None if perm is None else _c(perm, np.uint32)
        a_op, a_key, a_val = arena
        assert a_op.dtype == np.uint8 and a_key.dtype == np.int64 and a_val.dtype == np.int64
        assert inst.dtype == R.INST_CMDS and inst.flags.c_contiguous

        def ptr_of(x, keep, t):
            if x is None or not len(x):
                return None
            keep.append(_c(x, t))
            return _ptr(keep[-1])
        src, keep = self._store_srcs(sources, ptr_of)
        cur = np.array([used], np.uint64)
        n, cap = len(items), len(a_op)
        b = _lib.MpxStoreBatch(kind, R.SC_GENERAL if general else 0, _ptr(items) if n else None,
                               _ptr(effect), n, None, _ptr(perm), src, len(sources), len(inst),
                               inst_base, store_mask, 0)
        ar = _lib.MpxStoreArena(_ptr(a_op) if cap else None, _ptr(a_key) if cap else None,
                                _ptr(a_val) if cap else None, cap, _ptr(cur))
        res = _lib.MpxStoreResult()
        rc = self.lib.mpx_store_commands(self.h, C.byref(b), C.byref(ar),
                                         _ptr(inst) if len(inst) else None, C.byref(res))
        self._check(rc, "mpx_store_commands")
        del keep
        return int(cur[0]), self._store_result(res)

    @staticmethod
    def _store_result(res):
        r = np.zeros((), R.STORE_RESULT)
        for f in R.STORE_RESULT.names:
            r[f] = getattr(res, f)
        return r

    def store_commands_reserve(self, max_n):
        self._check(self.lib.mpx_store_commands_reserve(self.h, max_n), "mpx_store_commands_reserve")

    def store_commands_dev(self, batch, arena, d_inst, d_res, stream=None):
        """batch: _lib.MpxStoreBatch, arena: _lib.MpxStoreArena, both of device pointers
        (store_batch_dev / store_arena_dev build them)"""
        self._check(self.lib.mpx_store_commands_dev(self.h, C.byref(batch), C.byref(arena),
                                                    getattr(d_inst, "ptr", d_inst),
                                                    getattr(d_res, "ptr", d_res), stream),
                    "mpx_store_commands_dev")

    @staticmethod
    def store_batch_dev(kind, d_items, n, sources, n_inst, inst_base=0, d_effect=None, d_perm=None,
                        d_n=None, store_mask=R.AH_STORED, general=False):
        """the mpx_store_batch of a store_commands_dev call; sources: a list of dicts of device
        pointers (or devbuf.DevArrays) cmd_off / op / key / val with n_frames, n_cmds, n_recs. The
        batch keeps its source array alive."""
        def ptr_of(x, keep, t):
            return getattr(x, "ptr", x)
        src, _ = Engine._store_srcs(sources, ptr_of)
        p = [getattr(x, "ptr", x) for x in (d_items, d_effect, d_n, d_perm)]
        b = _lib.MpxStoreBatch(kind, R.SC_GENERAL if general else 0, p[0], p[1], n, p[2], p[3], src,
                               len(sources), n_inst, inst_base, store_mask, 0)
        b._src_keep = src
        return b

    @staticmethod
    def store_arena_dev(d_op, d_key, d_val, cap, d_used):
        p = [getattr(x, "ptr", x) for x in (d_op, d_key, d_val, d_used)]
        return _lib.MpxStoreArena(p[0], p[1], p[2], cap, p[3])

    def store_compact(self, inst, src_arena, used, dst_arena):
        """inst: INST_CMDS window, rewritten IN PLACE; src_arena / dst_arena: (op, key, val) arrays;
        used: the source arena's cursor. Returns (the target's cursor, result STORE_RESULT)."""
        assert inst.dtype == R.INST_CMDS and inst.flags.c_contiguous
        f_used, t_used = np.array([used], np.uint64), np.zeros(1, np.uint64)

        def arena(a, cur):
            cap = len(a[0])
            assert a[0].dtype == np.uint8 and a[1].dtype == np.int64 and a[2].dtype == np.int64
            return _lib.MpxStoreArena(_ptr(a[0]) if cap else None, _ptr(a[1]) if cap else None,
                                      _ptr(a[2]) if cap else None, cap, _ptr(cur))
        f, t = arena(src_arena, f_used), arena(dst_arena, t_used)
        res = _lib.MpxStoreResult()
        rc = self.lib.mpx_store_compact(self.h, _ptr(inst) if len(inst) else None, len(inst),
                                        C.byref(f), C.byref(t), C.byref(res))
        self._check(rc, "mpx_store_compact")
        return int(t_used[0]), self._store_result(res)

    def store_compact_reserve(self, max_n_inst):
        self._check(self.lib.mpx_store_compact_reserve(self.h, max_n_inst), "mpx_store_compact_reserve")

    def store_compact_dev(self, d_inst, n_inst, src_arena, dst_arena, d_res, stream=None):
        """src_arena, dst_arena: _lib.MpxStoreArena of device pointers (store_arena_dev)"""
        self._check(self.lib.mpx_store_compact_dev(self.h, getattr(d_inst, "ptr", d_inst), n_inst,
                                                   C.byref(src_arena), C.byref(dst_arena),
                                                   getattr(d_res, "ptr", d_res), stream),
                    "mpx_store_compact_dev")

    # ---- record assembly: a batch's durable-log bytes ---------------------------------------------
    def record_log(self, kind, fmt, items, sources=(), effect=None, perm=None, mask=None,
                   inst_base=0, out_cap=None, general=False, want_item_off=True):
        """kind: R.LR_ACCEPTS / R.LR_COMMITS (items ACCEPT_MSG, effect uint8 per item), R.LR_SENDS or
        R.LR_DECIDED (items ACCEPT_SEND; DECIDED: mask uint8 per window slot from inst_base); fmt:
        R.LOG_DURABLE / R.LOG_DURABLE_CLASSIC; sources as store_commands takes them. out_cap: the
        output's capacity (default: the bound of the call's sizes). Returns (the run's bytes, empty
        when it did not fit; item_off u64[n + 1] or None; result RECORD_RESULT scalar)."""
        items = _c(items, R.ACCEPT_MSG if kind in (R.LR_ACCEPTS, R.LR_COMMITS) else R.ACCEPT_SEND)
        effect = None if effect is None else _c(effect, np.uint8)
        perm = None if perm is None else _c(perm, np.uint32)
        mask = None if mask is None else _c(mask, np.uint8)

        def ptr_of(x, keep, t):
            if x is None or not len(x):
                return None
            keep.append(_c(x, t))
            return _ptr(keep[-1])
        src, keep = self._store_srcs(sources, ptr_of)
        n = len(items)
        if out_cap is None:
            out_cap = R.record_bound(n, sum(x["n_cmds"] if "n_cmds" in x else len(x["op"])
                                            for x in sources))
        out = np.zeros(out_cap, np.uint8)
        item_off = np.zeros(n + 1, np.uint64) if want_item_off else None
        b = _lib.MpxRecordBatch(kind, R.LR_GENERAL if general else 0, fmt, 0,
                                _ptr(items) if n else None, _ptr(effect), _ptr(mask), n, None,
                                _ptr(perm), src if len(sources) else None, len(sources),
                                0 if mask is None else len(mask), inst_base, 0)
        res = _lib.MpxRecordResult()
        rc = self.lib.mpx_record_log(self.h, C.byref(b), _ptr(out) if out_cap else None, out_cap,
                                     _ptr(item_off), C.byref(res))
        self._check(rc, "mpx_record_log")
        del keep
        r = self._record_result(res)
        return out[:0 if int(r["flags"]) & R.LR_FULL else int(r["n_bytes"])], item_off, r

    @staticmethod
    def _record_result(res):
        r = np.zeros((), R.RECORD_RESULT)
        for f in R.RECORD_RESULT.names:
            r[f] = getattr(res, f)
        return r

    def record_log_reserve(self, max_n):
        self._check(self.lib.mpx_record_log_reserve(self.h, max_n), "mpx_record_log_reserve")

    def record_log_dev(self, batch, d_out, out_cap, d_item_off, d_res, stream=None):
        """batch: _lib.MpxRecordBatch of device pointers (record_batch_dev builds it)"""
        self._check(self.lib.mpx_record_log_dev(self.h, C.byref(batch), getattr(d_out, "ptr", d_out),
                                                out_cap, getattr(d_item_off, "ptr", d_item_off),
                                                getattr(d_res, "ptr", d_res), stream),
                    "mpx_record_log_dev")

    @staticmethod
    def record_batch_dev(kind, fmt, d_items, n, sources=(), d_effect=None, d_perm=None, d_mask=None,
                         n_inst=0, inst_base=0, d_n=None, general=False):
        """the mpx_record_batch of a record_log_dev call; sources: a list of dicts of device
        pointers (or devbuf.DevArrays) cmd_off / op / key / val with n_frames, n_cmds, n_recs. The
        batch keeps its source array alive."""
        def ptr_of(x, keep, t):
            return getattr(x, "ptr", x)
        src, _ = Engine._store_srcs(sources, ptr_of)
        p = [getattr(x, "ptr", x) for x in (d_items, d_effect, d_mask, d_n, d_perm)]
        b = _lib.MpxRecordBatch(kind, R.LR_GENERAL if general else 0, fmt, 0, p[0], p[1], p[2], n,
                                p[3], p[4], src if len(sources) else None, len(sources), n_inst,
                                inst_base, 0)
        b._src_keep = src
        return b

    # ---- instance-log encoding ------------------------------------
    def encode_log(self, fmt, recs, cmd_off, op, key, val):
        """Returns (bytes, rec_off u64[n+1]) of the run in format fmt (R.LOG_CATCHUP /
        R.LOG_DURABLE); record i is bytes[rec_off[i]:rec_off[i+1]]."""
        recs = _c(recs, R.LOG_REC)
        off = _c(cmd_off, np.uint64)
        op, key, val = _c(op, np.uint8), _c(key, np.int64), _c(val, np.int64)
        n, m = len(recs), len(op)
        cap = self.lib.mpx_encode_log_bound(n, m)
        out = np.zeros(max(cap, 1), np.uint8)
        ro = np.zeros(n + 1, np.uint64)
        self._check(self.lib.mpx_encode_log(self.h, fmt, _ptr(recs), n, _ptr(off), _ptr(op),
                                            _ptr(key), _ptr(val), m, _ptr(out), cap, _ptr(ro)),
                    "mpx_encode_log")
        return out[:int(ro[-1])], ro

    def encode_log_reserve(self, max_n, max_m):
        self._check(self.lib.mpx_encode_log_reserve(self.h, max_n, max_m),
                    "mpx_encode_log_reserve")

    def encode_log_dev(self, fmt, d_recs, n, d_cmd_off, d_op, d_key, d_val, m, d_out, d_rec_off,
                       stream=None):
        self._check(self.lib.mpx_encode_log_dev(self.h, fmt, d_recs, n, d_cmd_off, d_op, d_key,
                                                d_val, m, d_out, d_rec_off, stream),
                    "mpx_encode_log_dev")

    # ---- durable-log replay (read side) ---------------------------------
    def replay_durable(self, log, inst_cap, default_ballot=0, committed_up_to=-1, rec_base=0,
                       last_rec=None):
        """getDataFromStableStore (bareminpaxos.go:122-161) over a durable log of 29-byte
        records. Returns (recs, op, key, val, last_rec, default_ballot, committed_up_to):
        last_rec[i] is the file index of the last record naming instance i (-1: none). A store
        replayed in chunks passes each chunk's first file index as rec_base and the previous
        chunk's last_rec."""
        log = _c(log, np.uint8)
        n = len(log) // R.DURABLE_REC_BYTES
        recs = np.zeros(n, R.LOG_REC)
        op = np.zeros(n, np.uint8)
        key = np.zeros(n, np.int64)
        val = np.zeros(n, np.int64)
        last = np.full(inst_cap, -1, np.int32) if last_rec is None else \
            np.array(last_rec, np.int32, copy=True)
        sc = np.array([default_ballot, committed_up_to], np.int32)
        self._check(self.lib.mpx_replay_durable(self.h, _ptr(log), len(log), inst_cap, rec_base,
                                                _ptr(recs),
                                                _ptr(op), _ptr(key), _ptr(val), _ptr(last),
                                                _ptr(sc)),
                    "mpx_replay_durable")
        return recs, op, key, val, last, int(sc[0]), int(sc[1])

    def replay_durable_reserve(self, max_len, inst_cap):
        """scratch for the binned slot maximum of replay_durable_dev calls up to max_len bytes
        over inst_cap slots (without it the device form takes one atomic per record)"""
        self._check(self.lib.mpx_replay_durable_reserve(self.h, max_len, inst_cap),
                    "mpx_replay_durable_reserve")

    def replay_durable_dev(self, d_log, nbytes, inst_cap, d_recs, d_op, d_key, d_val, d_last,
                           d_scalars, stream=None, rec_base=0):
        self._check(self.lib.mpx_replay_durable_dev(self.h, d_log, nbytes, inst_cap, rec_base,
                                                    d_recs, d_op,
                                                    d_key, d_val, d_last, d_scalars, stream),
                    "mpx_replay_durable_dev")

    # ---- multi-GPU ----------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        lib = _lib.load()
        buf = (C.c_ubyte * 128)()
        rc = lib.mpx_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise MpxError(rc, "mpx_comm_unique_id")
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        self._check(self.lib.mpx_comm_init(self.h, nranks, rank, C.cast(buf, C.c_void_p)),
                    "mpx_comm_init")

    def watermarks_allreduce(self, committed, executed):
        c = np.array(committed, np.int32, copy=True)
        e = np.array(executed, np.int32, copy=True)
        self._check(self.lib.mpx_watermarks_allreduce(self.h, _ptr(c), _ptr(e), len(c)),
                    "mpx_watermarks_allreduce")
        return c, e

    def watermarks_allreduce_dev(self, d_wm, n_groups, stream=None):
        self._check(self.lib.mpx_watermarks_allreduce_dev(self.h, d_wm, n_groups, stream),
                    "mpx_watermarks_allreduce_dev")

    def step_allreduce_dev(self, d_wm, n_groups, d_totals, n_totals, stream=None):
        """max of the watermark vector and sum of the step totals over ranks, one RCCL group"""
        self._check(self.lib.mpx_step_allreduce_dev(self.h, d_wm, n_groups, d_totals, n_totals,
                                                    stream), "mpx_step_allreduce_dev")

    def step_allreduce_oop_dev(self, d_wm_send, d_wm_recv, n_groups, d_totals, n_totals,
                               stream=None):
        """the step exchange out of place: max over ranks of d_wm_send (foreign groups -1 for
        good) into d_wm_recv, sum of d_totals in place (mpx_step_allreduce_oop_dev)"""
        self._check(self.lib.mpx_step_allreduce_oop_dev(self.h, d_wm_send, d_wm_recv, n_groups,
                                                        d_totals, n_totals, stream),
                    "mpx_step_allreduce_oop_dev")

    # ---- device memory / streams / events of the engine's HIP runtime -----------------------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._check(self.lib.mpx_dev_alloc(self.h, nbytes, C.byref(p)), "mpx_dev_alloc")
        return p.value

    def dev_free(self, ptr):
        self._check(self.lib.mpx_dev_free(self.h, ptr), "mpx_dev_free")

    def memcpy(self, dst, src, nbytes, kind, stream=None):
        self._check(self.lib.mpx_memcpy_async(self.h, dst, src, nbytes, kind, stream),
                    "mpx_memcpy_async")

    def memset(self, ptr, byte_value, nbytes, stream=None):
        self._check(self.lib.mpx_memset_async(self.h, ptr, byte_value, nbytes, stream),
                    "mpx_memset_async")

    def stream_create(self):
        s = C.c_void_p()
        self._check(self.lib.mpx_stream_create(self.h, C.byref(s)), "mpx_stream_create")
        return s.value

    def stream_destroy(self, s):
        self._check(self.lib.mpx_stream_destroy(self.h, s), "mpx_stream_destroy")

    def stream_synchronize(self, s=None):
        self._check(self.lib.mpx_stream_synchronize(self.h, s), "mpx_stream_synchronize")

    def event_create(self, timing=True):
        ev = C.c_void_p()
        self._check(self.lib.mpx_event_create(self.h, 1 if timing else 0, C.byref(ev)),
                    "mpx_event_create")
        return ev.value

    def group_step_events(self, ev0=None, ev1=None):
        """record ev0 / ev1 around the fast kernel of every later group step (None: off)"""
        self._check(self.lib.mpx_group_step_events(self.h, ev0, ev1), "mpx_group_step_events")

    def event_destroy(self, ev):
        self._check(self.lib.mpx_event_destroy(self.h, ev), "mpx_event_destroy")

    def event_record(self, ev, stream=None):
        self._check(self.lib.mpx_event_record(self.h, ev, stream), "mpx_event_record")

    def stream_wait_event(self, stream, ev):
        self._check(self.lib.mpx_stream_wait_event(self.h, stream, ev), "mpx_stream_wait_event")

    def graph_begin(self, stream=None):
        """capture every call issued on `stream` (and streams joined to it) into a graph"""
        self._check(self.lib.mpx_graph_begin(self.h, stream), "mpx_graph_begin")

    def graph_end(self, stream=None):
        x = C.c_void_p()
        self._check(self.lib.mpx_graph_end(self.h, stream, C.byref(x)), "mpx_graph_end")
        return x.value

    def graph_launch(self, graph, stream=None):
        self._check(self.lib.mpx_graph_launch(self.h, graph, stream), "mpx_graph_launch")

    def graph_destroy(self, graph):
        self._check(self.lib.mpx_graph_destroy(self.h, graph), "mpx_graph_destroy")

    def event_elapsed_ms(self, ev0, ev1):
        ms = C.c_float(0.0)
        self._check(self.lib.mpx_event_elapsed_ms(self.h, ev0, ev1, C.byref(ms)),
                    "mpx_event_elapsed_ms")
        return ms.value

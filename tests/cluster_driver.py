"""A replica's turn as the chain of engine calls INTEGRATION.md and DESIGN §13-§23 describe, N
replicas exchanging only the bytes those calls wrote, compared with cluster_model.py after every
station of every replica.

TEST INFRASTRUCTURE for test_cluster_translit.py (TranslitBackend, on the CPU) and
test_gpu_cluster.py (EngineBackend, the real Engine). The driver is backend-agnostic: both backends
answer the host forms' names with the host forms' arguments and results.

What the driver does itself is plumbing, never a protocol effect:
  * it carries st / lb / inst / the arena and its cursor / the groups / committed_upto / peer_commits
    / the executed cursor from call to call exactly as the calls return them, and copies
    committed_upto (the tally's and commit_handle's output) into the proposer groups' field;
  * it keeps the proposal arrays of all turns back to back and every MPX_PH_ACCEPT slot of
    propose_handle at its window index with first_cmd moved by the arrays' length (INTEGRATION: "one
    mpx_commit_send per window slot"), so an instance decided or executed turns after it was
    proposed still finds its proposals;
  * it cuts the ordered AcceptReplies at the group boundaries for accept_tally, whose host form
    takes one log per call, and blanks the slots of other leaders' groups when it builds MIN's
    refusals, because encode_replies writes one Leader per call;
  * it moves byte runs between the replicas as the schedule (cluster_model.Cluster) says.
Where the host still acts: CLASSIC's handleAccept record (paxos.go:513-517) is no kind of
mpx_record_log, so the driver writes it in plain Python (`classic_accept_record`); the
bytes of that station are not compared, the state it leads to is.
"""
import struct

import numpy as np

import cluster_model as M
from go_translit import GoPanic
from minpaxos_amd import records as R

MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC
NIL = R.STATUS_NIL


class Divergence(AssertionError):
    """the first place the backend and the model part: which turn, replica and station"""


# ---- the backends ------------------------------------------------------------------------------------
class EngineBackend:
    """the real Engine; store_commands answers like the transliteration (new arrays, not in place)"""

    def __init__(self, engine):
        self.e = engine

    def __getattr__(self, name):
        return getattr(self.e, name)

    def store_commands(self, kind, items, sources, arena, used, inst, inst_base=0, effect=None,
                       perm=None, store_mask=R.AH_STORED, handler=None):
        arena = tuple(np.array(a, copy=True) for a in arena)
        inst = np.array(inst, dtype=R.INST_CMDS, copy=True)
        used, res = self.e.store_commands(kind, items, sources, arena, used, inst, inst_base,
                                          effect=effect, perm=perm, store_mask=store_mask)
        assert not int(res["flags"]) & R.SC_FULL
        return arena, used, inst

    def record_log(self, *a, **kw):
        out, _, res = self.e.record_log(*a, **kw)
        assert not int(res["flags"]) & R.LR_FULL
        return out.tobytes()

    def build_replies(self, *a, **kw):
        recs, cs, _ = self.e.build_replies(*a, **kw)
        return recs, cs

    def unmarshal_frames(self, buf, var):
        return self.e.unmarshal_frames(buf, var)[0]

    def gather_commit_shorts(self, buf, other):
        return self.e.gather_commit_shorts(buf, other)[:3]

    def order_records(self, sources, n_inst, inst_base=0, arrivals=None, arrival_bits=0):
        return self.e.order_records(sources, n_inst, inst_base, arrivals, arrival_bits)[:2]

    def raises(self):
        from minpaxos_amd.engine import MpxError
        return MpxError


class TranslitBackend:
    """the batch transliterations (and GoBackend / the oracle where a station has no transliteration
    of its own: framing, the tally, apply, the reply bytes), one per replica, on the CPU"""

    def __init__(self, N, mode):
        import acceptor_translit
        import accepts_stored_translit
        import client_translit
        import commit_translit
        import execute_translit
        import order_translit
        import proposer_translit
        import record_translit
        import reply_translit
        import store_translit
        import unmarshal_translit
        from go_translit import GoBackend
        from oracle_lib import Oracle
        self.N, self.mode = N, mode
        self.go, self.orc = GoBackend(N, mode), Oracle(N, mode)
        self.A, self.AS, self.C, self.CT, self.X, self.O, self.P, self.L, self.RT, self.S, self.U = (
            acceptor_translit, accepts_stored_translit, client_translit, commit_translit,
            execute_translit, order_translit, proposer_translit, record_translit, reply_translit,
            store_translit, unmarshal_translit)

    def raises(self):
        return GoPanic

    @staticmethod
    def _ok(d):
        if d.get("code", R.OK) != R.OK:
            raise GoPanic(d["code"], "the transliteration refuses the call")
        return d

    def decode_client_streams(self, bufs, groups=None, n_groups=1):
        return self.C.decode_client_streams(bufs, groups, n_groups)

    def propose_handle(self, groups, prop_off, st, inst_base=0, ipg=None, lb=None):
        return self.P.propose_handle(self.mode, self.N, groups, prop_off, st, inst_base, ipg, lb)[:5]

    def store_commands(self, kind, items, sources, arena, used, inst, inst_base=0, effect=None,
                       perm=None, store_mask=R.AH_STORED, handler="accept"):
        """handler: which of handleAccept / handleCommit the MSGS items went through (the engine
        reads it from the items: only a Commit finds a slot it must keep)"""
        d = self._ok(self.S.store_commands(kind, items, sources, arena, used, inst, inst_base, effect,
                                           perm, store_mask, handler=handler))
        assert not int(d["res"]["flags"]) & R.SC_FULL
        return (d["op"], d["key"], d["val"]), d["used"], d["inst"]

    def record_log(self, kind, fmt, items, sources=(), effect=None, perm=None, mask=None, inst_base=0):
        return self._ok(self.L.record_log(kind, fmt, items, sources, effect, perm, mask,
                                          inst_base))["out"].tobytes()

    def encode_accepts_stored(self, sends, groups, cmds, inst_base=0, ipg=None, peer_commits=None,
                              st=None, lb=None, inst=None, arena=None, thrifty=False):
        return self.AS.encode_accepts_stored(self.mode, self.N, sends, groups, cmds, inst_base, ipg,
                                             peer_commits, st, lb, inst, arena, thrifty)

    def encode_accepts(self, sends, groups, cmds, inst_base=0, ipg=None, thrifty=False):
        return self.P.encode_accepts(self.mode, self.N, sends, groups, cmds, inst_base, ipg,
                                     thrifty=thrifty)

    def build_replies(self, kind, sends, meta, mask=None, inst_base=0, ret=None, ret_first=None,
                      cap=None, want_commit_sends=False):
        d = self._ok(self.RT.build_replies(kind, sends, meta, mask, inst_base, ret, ret_first, cap,
                                           proto=self.mode))
        return d["recs"], d["commit_sends"] if want_commit_sends else None

    def encode_replies(self, recs, n_clients, ok=1, leader=0):
        return self.orc.encode_replies(recs, n_clients, ok, leader)

    def decode_stream(self, buf):
        return self.orc.decode_stream(bytes(buf))

    def unmarshal_frames(self, buf, var):
        return self.U.expected(self.mode, bytes(buf), var)[0]

    def order_records(self, sources, n_inst, inst_base=0, arrivals=None, arrival_bits=0):
        return self.O.order_records(sources, n_inst, inst_base, arrivals, arrival_bits)[:2]

    def accept_handle(self, msgs, st, groups, inst_base=0, ipg=None):
        return self.A.accept_handle(self.mode, self.N, msgs, st, groups, inst_base, ipg)

    def encode_accept_replies(self, replies, reply_to):
        return self.A.encode_accept_replies(self.mode, replies, reply_to, self.N)

    def accept_tally(self, recs, st, inst_base=0, committed_upto=-1, peer_commits=None):
        return self.go.accept_tally(recs, st, inst_base, committed_upto, peer_commits)

    def encode_commits(self, sends, groups, cmds, inst_base=0, ipg=1, thrifty=False):
        return self.CT.encode_commits(self.N, sends, groups, cmds, inst_base, ipg, thrifty)

    def gather_commit_shorts(self, buf, other):
        return self.CT.gather_commit_shorts(bytes(buf), other)

    def commit_handle(self, msgs, st, committed_upto, inst_base=0, ipg=None):
        return self.CT.commit_handle(msgs, st, committed_upto, inst_base, ipg, per_message=False)

    def execute_gather(self, inst, committed_upto, executed, cmds, inst_base=0, ipg=None, sends=None):
        return self._ok(self.X.execute_gather(inst, committed_upto, executed, cmds, inst_base, ipg,
                                              sends))

    def apply(self, op, key, val):
        return self.go.apply(op, key, val)

    def kv_export(self):
        return self.go.kv_export()

    def replay_durable(self, log, inst_cap, default_ballot=0):
        return self.orc.replay_durable(log, inst_cap, default_ballot)


# ---- one replica's arrays ---------------------------------------------------------------------------
class Rep:
    def __init__(self, be, sc, r, arena_cap):
        N, G, ipg = sc["N"], sc["G"], sc["ipg"]
        self.be, self.r = be, r
        n_inst = G * ipg
        first = np.arange(G, dtype=np.int32) * ipg
        self.st = np.zeros(n_inst, R.ACCEPTOR_STATE)
        self.st["status"] = NIL
        self.lb = np.zeros(n_inst, R.INST_STATE)
        self.lb["status"] = NIL
        self.inst = np.zeros(n_inst, R.INST_CMDS)
        self.arena = (np.zeros(arena_cap, np.uint8), np.zeros(arena_cap, np.int64),
                      np.zeros(arena_cap, np.int64))
        self.used = 0
        self.pg = np.zeros(G, R.PROPOSER_GROUP)
        self.ag = np.zeros(G, R.ACCEPTOR_GROUP)
        for g in range(G):
            lead = g % N
            self.pg[g] = (M.default_ballot(g, N), r, lead, (N >> 1) + 1 if lead == r else 0,
                          first[g], first[g] - 1, (0, 0))
            self.ag[g] = (M.default_ballot(g, N), r)
        self.cu = (first - 1).astype(np.int32)
        self.pc = np.repeat((first - 1).astype(np.int32)[:, None], N, axis=1).copy()
        self.ex = (first - 1).astype(np.int32)
        self.wsends = np.zeros(n_inst, R.ACCEPT_SEND)
        self.p_op, self.p_key, self.p_val = (np.zeros(0, np.uint8), np.zeros(0, np.int64),
                                             np.zeros(0, np.int64))
        self.p_meta = np.zeros(0, R.PROPOSAL)
        self.durable = bytearray()
        self.conn_groups = [g for (r2, g) in sc["clients"] if r2 == r]


def classic_accept_record(msgs, eff, st_before, sources, perm):
    """THE HOST'S PART: recordInstanceMetadata + recordCommands of paxos.go:513-517, the
    status being the instance's at that message: COMMITTED only in the reordered-ACCEPT branch
    (:503-508), where the slot was COMMITTED under the message's own ballot before it came"""
    rec_end = np.cumsum([int(s["n_recs"]) for s in sources])
    out = bytearray()
    for i, m in enumerate(msgs):
        if not int(eff[i]) & R.AH_STORED:
            continue
        s0 = st_before[int(m["instance"])]
        kept = int(s0["status"]) == R.COMMITTED and int(s0["ballot"]) == int(m["ballot"])
        out += struct.pack("<IB", int(m["ballot"]) & 0xFFFFFFFF, R.COMMITTED if kept else R.ACCEPTED)
        s = int(np.searchsorted(rec_end, int(perm[i]), side="right"))
        src, v = sources[s], int(m["value_id"])
        for j in range(int(src["cmd_off"][v]), int(src["cmd_off"][v + 1])):
            out += struct.pack("<Bqq", int(src["op"][j]), int(src["key"][j]), int(src["val"][j]))
    return bytes(out)


# ---- the driver ---------------------------------------------------------------------------------------
class Driver:
    """runs a scenario turn by turn next to the model; `step` raises Divergence at the first byte
    run or state field that differs, naming the turn, the replica and the station"""

    def __init__(self, sc, backends, compare=True):
        self.sc, self.mode, self.N, self.G, self.ipg = sc, sc["mode"], sc["N"], sc["G"], sc["ipg"]
        self.n_inst = self.G * self.ipg
        total = sum(len(b) for per in sc["client_bytes"] for row in per for b in row) // \
            R.CLIENT_PROPOSE_FRAME
        self.reps = [Rep(backends[r], sc, r, total + 16) for r in range(self.N)]
        self.model = M.cluster_of(sc)
        self.wire = {k: {(p, q): bytearray() for p in range(self.N) for q in range(self.N) if p != q}
                     for k in M.KINDS}
        self.turn = 0
        self.compare = compare
        self.fmt = R.LOG_DURABLE if self.mode == MIN else R.LOG_DURABLE_CLASSIC
        self.checked = {k: 0 for k in ("accept", "accept_reply", "commit", "client", "durable")}

    # -- comparison --
    def _same(self, what, r, station, got, want):
        got, want = bytes(got), bytes(want)
        if self.compare and got != want:
            at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            raise Divergence(f"turn {self.turn}, replica {r}, station {station}: {what} differ at byte "
                             f"{at} (backend {len(got)} bytes, model {len(want)}): "
                             f"{got[max(at - 8, 0):at + 24].hex()} != {want[max(at - 8, 0):at + 24].hex()}")

    def _put(self, kind, r, station, out, off, log):
        """a station's byte runs onto the connections, each against the model's run"""
        for q in range(self.N):
            run = out[int(off[q]):int(off[q + 1])].tobytes()
            if q == r:
                assert not run
                continue
            self._same(f"{kind} bytes to replica {q}", r, station, run, log[kind].get((r, q), b""))
            self.checked[kind] += len(run)
            self.wire[kind][(r, q)] += run

    def _clients(self, r, station, recs, ok, leader, got):
        rep = self.reps[r]
        if len(recs):
            out, off = rep.be.encode_replies(recs, len(rep.conn_groups), ok, leader)
            for k in range(len(rep.conn_groups)):
                got.setdefault(k, bytearray()).extend(out[int(off[k]):int(off[k + 1])].tobytes())

    def _check_clients(self, r, station, got, log):
        for k in range(len(self.reps[r].conn_groups)):
            self._same(f"reply bytes to client connection {k}", r, station, got.get(k, b""),
                       log["client"][station].get((r, k), b""))
            self.checked["client"] += len(got.get(k, b""))

    def _durable(self, r, station, run, log, compared=True):
        self.reps[r].durable += run
        if compared:
            self._same("durable-log bytes", r, station, run, log["durable"][station][r])
            self.checked["durable"] += len(run)

    def _read(self, r, kind):
        """the bytes every delivering connection holds for this station: [(peer, bytes)]"""
        got = []
        for p in range(self.N):
            if p == r or self.model.hold is not None and bool(self.model.hold[self.turn][p][r]):
                continue
            buf = bytes(self.wire[kind][(p, r)])
            self.wire[kind][(p, r)] = bytearray()
            if buf:
                got.append((p, buf))
        return got

    # -- the stations --
    def propose(self, r, log):
        rep, be, sc = self.reps[r], self.reps[r].be, self.sc
        d = be.decode_client_streams(sc["client_bytes"][self.turn][r], rep.conn_groups, self.G)
        assert int(d["res"]["n_dropped"]) == 0 and int(d["res"]["n_partial"]) == 0
        rep.pg["committed_upto"] = rep.cu
        rep.pg, rep.st, rep.lb, sends, send_off = be.propose_handle(
            rep.pg, d["prop_off"], rep.st, 0, self.ipg, rep.lb)
        cmds = (d["op"], d["key"], d["val"])
        src = [dict(cmd_off=None, op=d["op"], key=d["key"], val=d["val"], n_recs=len(sends))]
        rep.arena, rep.used, rep.inst = be.store_commands(R.SC_SENDS, sends, src, rep.arena, rep.used,
                                                          rep.inst, 0)
        self._durable(r, "propose", be.record_log(R.LR_SENDS, self.fmt, sends, src), log)
        if self.mode == MIN:
            out, off = be.encode_accepts_stored(sends, rep.pg, cmds, 0, self.ipg, peer_commits=rep.pc,
                                                st=rep.st, lb=rep.lb, inst=rep.inst, arena=rep.arena,
                                                thrifty=sc["thrifty"])
        else:
            out, off = be.encode_accepts(sends, rep.pg, cmds, 0, self.ipg, thrifty=sc["thrifty"])
        self._put("accept", r, "propose", out, off, log)
        got = {}
        refusing = (sends["flags"] & (R.PH_NOT_LEADER | R.PH_REFUSED)) != 0
        slot_group = np.searchsorted(send_off[1:], np.arange(len(sends)), side="right")
        leaders = rep.pg["leader"][slot_group] if self.mode == MIN else np.zeros(len(sends), np.int32)
        for L in sorted(set(int(x) for x in leaders[refusing])):   # one Leader per encode_replies
            part = sends.copy()
            part["flags"][leaders != L] = 0
            recs, _ = be.build_replies(R.RB_FALSE, part, d["meta"])
            self._clients(r, "propose", recs, 0, L, got)
        self._check_clients(r, "propose", got, log)
        # the turn's proposals behind the earlier ones, its instances at their window slots
        base = len(rep.p_op)
        for s in sends[(sends["flags"] & R.PH_ACCEPT) != 0]:
            rep.wsends[int(s["instance"])] = s
            rep.wsends["first_cmd"][int(s["instance"])] += base
        rep.p_op, rep.p_key, rep.p_val, rep.p_meta = (
            np.concatenate([rep.p_op, d["op"]]), np.concatenate([rep.p_key, d["key"]]),
            np.concatenate([rep.p_val, d["val"]]), np.concatenate([rep.p_meta, d["meta"]]))

    def accept(self, r, log):
        rep, be = self.reps[r], self.reps[r].be
        recs, sources = [], []
        for p, buf in self._read(r, "accept"):
            _, _, var, _, res = be.decode_stream(buf)
            assert int(res["stop_reason"]) == R.DECODE_END and int(res["consumed"]) == len(buf)
            a = be.unmarshal_frames(buf, var)
            recs.append(a["accepts"])
            sources.append(dict(cmd_off=a["cmd_off"], op=a["op"], key=a["key"], val=a["val"],
                                n_recs=len(a["accepts"])))
        if not recs:
            self._durable(r, "accept", b"", log, self.mode == MIN)
            self._put("accept_reply", r, "accept", np.zeros(0, np.uint8), np.zeros(self.N + 1, np.uint64), log)
            return
        msgs, perm = be.order_records(recs, self.n_inst, 0)
        st_before = rep.st
        rep.st, replies, to, eff = be.accept_handle(msgs, rep.st, rep.ag, 0, self.ipg)
        rep.arena, rep.used, rep.inst = be.store_commands(R.SC_MSGS, msgs, sources, rep.arena,
                                                          rep.used, rep.inst, 0, effect=eff, perm=perm)
        if self.mode == MIN:
            self._durable(r, "accept", be.record_log(R.LR_ACCEPTS, self.fmt, msgs, sources, effect=eff,
                                                     perm=perm), log)
        else:
            self._durable(r, "accept", classic_accept_record(msgs, eff, st_before, sources, perm), log,
                          compared=False)
        out, off = be.encode_accept_replies(replies, to)
        self._put("accept_reply", r, "accept", out, off, log)

    def tally(self, r, log):
        rep, be = self.reps[r], self.reps[r].be
        recs = []
        for p, buf in self._read(r, "accept_reply"):
            ar, _, _, _, res = be.decode_stream(buf)
            assert int(res["stop_reason"]) == R.DECODE_END and int(res["consumed"]) == len(buf)
            recs.append(ar)
        decided = np.zeros(self.n_inst, np.uint8)
        if recs:
            ordered, _ = be.order_records(recs, self.n_inst, 0)
            cut = np.searchsorted(ordered["instance"], np.arange(self.G + 1) * self.ipg)
            for g in range(self.G):
                if cut[g] == cut[g + 1]:
                    continue
                w = slice(g * self.ipg, (g + 1) * self.ipg)
                rep.lb[w], cu, rep.pc[g], decided[w] = be.accept_tally(
                    ordered[cut[g]:cut[g + 1]], rep.lb[w], g * self.ipg, int(rep.cu[g]), rep.pc[g])
                rep.cu[g] = cu
        self._durable(r, "tally", be.record_log(R.LR_DECIDED, self.fmt, rep.wsends, mask=decided,
                                                inst_base=0), log)
        want_cs = self.mode == CLASSIC
        recs, cs = be.build_replies(R.RB_DECIDED, rep.wsends, rep.p_meta, mask=decided, inst_base=0,
                                    cap=0 if self.sc["dreply"] else None, want_commit_sends=want_cs)
        got = {}
        if not self.sc["dreply"]:
            self._clients(r, "tally", recs, 1, r if self.mode == MIN else 0, got)
        self._check_clients(r, "tally", got, log)
        if want_cs:
            out, off = be.encode_commits(cs, rep.pg, (rep.p_op, rep.p_key, rep.p_val), 0, self.ipg,
                                         thrifty=self.sc["thrifty"])
            self._put("commit", r, "tally", out, off, log)

    def commit(self, r, log):
        rep, be = self.reps[r], self.reps[r].be
        recs, sources, arrivals = [], [], []
        inbox = self._read(r, "commit")
        obits = max(max((len(b) for _, b in inbox), default=1).bit_length(), 1)
        for rank, (p, buf) in enumerate(inbox):
            _, _, var, oth, res = be.decode_stream(buf)
            assert int(res["stop_reason"]) == R.DECODE_END and int(res["consumed"]) == len(buf)
            a = be.unmarshal_frames(buf, var)
            shorts, _, fidx = be.gather_commit_shorts(buf, oth)
            recs += [a["commits"], shorts]
            sources += [dict(cmd_off=a["cmd_off"], op=a["op"], key=a["key"], val=a["val"],
                             n_recs=len(a["commits"])),
                        dict(cmd_off=None, op=np.zeros(0, np.uint8), key=np.zeros(0, np.int64),
                             val=np.zeros(0, np.int64), n_recs=len(shorts))]
            # arrival: the connection, then the frame's offset in its stream
            arrivals += [((rank << obits) | var["offset"][a["commits"]["value_id"]]).astype(np.uint32),
                         ((rank << obits) | oth["offset"][fidx]).astype(np.uint32)]
        if not recs:
            self._durable(r, "commit", b"", log)
            return
        msgs, perm = be.order_records(recs, self.n_inst, 0, arrivals,
                                      obits + max(len(inbox) - 1, 1).bit_length())
        rep.st, rep.cu, eff, _ = be.commit_handle(msgs, rep.st, rep.cu, 0, self.ipg)
        rep.arena, rep.used, rep.inst = be.store_commands(
            R.SC_MSGS, msgs, sources, rep.arena, rep.used, rep.inst, 0, effect=eff, perm=perm,
            store_mask=R.CH_CMDS, handler="commit")
        self._durable(r, "commit", be.record_log(R.LR_COMMITS, self.fmt, msgs, sources, effect=eff,
                                                 perm=perm), log)

    def execute(self, r, log):
        rep, be = self.reps[r], self.reps[r].be
        x = be.execute_gather(rep.inst, rep.cu, rep.ex, rep.arena, 0, self.ipg, sends=rep.wsends)
        rep.ex = x["executed"]
        ret = be.apply(x["op"], x["key"], x["val"])[0] if len(x["op"]) else np.zeros(0, np.int64)
        got = {}
        if self.sc["dreply"]:
            recs, _ = be.build_replies(R.RB_EXECUTED, rep.wsends, rep.p_meta, mask=x["mask"],
                                       inst_base=0, ret=ret, ret_first=x["ret_first"])
            self._clients(r, "execute", recs, 1, r if self.mode == MIN else 0, got)
        self._check_clients(r, "execute", got, log)
        self._durable(r, "execute", b"", log)

    # -- a turn --
    def step(self):
        """a turn, station by station: the model's replicas walk the station, then the backend's
        (inside a station the replicas only write what later stations read, so the order among them
        is immaterial), then every replica's state is compared. The model's panic is the backend's
        refusal, at the same station."""
        t = self.turn
        log = self.model.begin(self.sc["client_bytes"][t])
        for name in M.Cluster.STATIONS:
            try:
                self.model.station(name)
            except GoPanic as e:
                return self._refused(name, e)
            for r in range(self.N):
                try:
                    getattr(self, name)(r, log)
                except Divergence:
                    raise
                except (self.reps[r].be.raises(), GoPanic) as e:
                    raise Divergence(f"turn {t}, replica {r}, station {name}: the backend refuses "
                                     f"where the model goes on: {e}")
            if self.compare:
                for r in range(self.N):
                    self.check_state(r, name)
        self.model.end()
        self.turn += 1
        return log

    def _refused(self, name, panic):
        """the model panicked (in these scenarios: a proposal that finds its window full,
        bareminpaxos.go:627 / paxos.go:395 indexing past instanceSpace): every replica that leads a
        group must have propose_handle refuse with the same code"""
        if name != "propose":
            raise Divergence(f"turn {self.turn}, station {name}: the model panics: {panic}")
        codes = {}
        for r in range(self.N):
            rep, be = self.reps[r], self.reps[r].be
            d = be.decode_client_streams(self.sc["client_bytes"][self.turn][r], rep.conn_groups, self.G)
            rep.pg["committed_upto"] = rep.cu
            try:
                be.propose_handle(rep.pg, d["prop_off"], rep.st, 0, self.ipg, rep.lb)
            except (be.raises(), GoPanic) as e:
                codes[r] = e.code
        leaders = {g % self.N for g in range(self.G)}
        if set(codes) != leaders or set(codes.values()) != {panic.code}:
            raise Divergence(f"turn {self.turn}: the model panics ({panic}), the backend answers {codes}")
        self.refused = (self.turn, panic.code)
        return None

    # -- state --
    def check_state(self, r, station):
        """the engine's windows mapped back to Go shapes, against the model's replica r of every
        group"""
        rep, N, ipg = self.reps[r], self.N, self.ipg

        def same(what, got, want, g, i=None):
            if got != want:
                where = f"group {g}" + ("" if i is None else f", instance {i}")
                raise Divergence(f"turn {self.turn}, replica {r}, {station}: {what} of {where}: backend "
                                 f"{got}, model {want}")
        for g in range(self.G):
            x = self.model.rep[g][r]
            lead = g % N == r
            for k in range(ipg):
                i = g * ipg + k
                m = x.space[k]
                st_status, lb_status = int(rep.st["status"][i]), int(rep.lb["status"][i])
                status = lb_status if lb_status != NIL else st_status
                same("status", status, NIL if m is None else m.Status, g, i)
                has = bool(int(rep.inst["flags"][i]) & R.IC_HAS_CMDS)
                if m is None:
                    same("Cmds", has, False, g, i)
                    continue
                same("ballot", int(rep.st["ballot"][i]), m.Ballot, g, i)
                # the one flag a slot may carry between stations: Lb.ClientProposals != nil
                same("flags", int(rep.st["flags"][i]), R.PF_HAS_PROPOSALS if m.Lb is not None and
                     m.Lb.ClientProposals is not None else 0, g, i)
                same("Cmds != nil", has, m.Cmds is not None, g, i)
                if has:
                    a, n = int(rep.inst["first_cmd"][i]), int(rep.inst["n_cmds"][i])
                    cmds = list(zip(rep.arena[0][a:a + n].tolist(), rep.arena[1][a:a + n].tolist(),
                                    rep.arena[2][a:a + n].tolist()))
                    same("Cmds", cmds, [tuple(c) for c in m.Cmds], g, i)
                if lead and m.Lb is not None:
                    same("Lb", (int(rep.lb["accept_oks"][i]), int(rep.lb["nacks"][i]),
                                int(rep.lb["max_recv_ballot"][i])),
                         (m.Lb.AcceptOKs, m.Lb.Nacks, m.Lb.MaxRecvBallot), g, i)
            same("committedUpTo", int(rep.cu[g]), x.committedUpTo, g)
            same("executed cursor", int(rep.ex[g]) + 1, x.executed, g)
            if lead:
                same("crtInstance", int(rep.pg["crt_instance"][g]), x.crtInstance, g)
                if self.mode == MIN:
                    same("peerCommits", rep.pc[g].tolist(), x.peerCommits, g)
        keys, vals = rep.be.kv_export()
        state = {}
        for g in range(self.G):
            state.update(self.model.rep[g][r].State)
        same("State", dict(zip(keys.tolist(), vals.tolist())), dict(sorted(state.items())), "all")
        self._same("the durable log so far", r, station, b"" if self.mode == CLASSIC else rep.durable,
                   b"" if self.mode == CLASSIC else self.model.store[r])


def run(sc, backends, compare=True):
    """every turn of a scenario through the backends, next to the model, until it ends or the model
    panics and the backends refuse alike (Driver.refused). Returns the Driver."""
    d = Driver(sc, backends, compare)
    d.refused = None
    for _ in range(sc["turns"]):
        if d.step() is None:
            break
    return d


def check_end(d):
    """after the last turn: all replicas of a group agree on every instance two of them hold
    COMMITTED (read from the backends' arrays, not the model), and a MIN follower's whole durable log,
    where every instance it accepted carries one command (the 29-byte records
    getDataFromStableStore reads, bareminpaxos.go:122-161), replays into its instance window"""
    N, G, ipg = d.N, d.G, d.ipg
    for i in range(G * ipg):
        held = []
        for rep in d.reps:
            st, lb = int(rep.st["status"][i]), int(rep.lb["status"][i])
            if (lb if lb != NIL else st) == R.COMMITTED:
                x = rep.inst[i]
                cmds = None
                if int(x["flags"]) & R.IC_HAS_CMDS:
                    a, n = int(x["first_cmd"]), int(x["n_cmds"])
                    cmds = (rep.arena[0][a:a + n].tobytes(), rep.arena[1][a:a + n].tobytes(),
                            rep.arena[2][a:a + n].tobytes())
                held.append((int(rep.st["ballot"][i]), cmds))
        with_cmds = [h for h in held if h[1] is not None]
        assert all(h[0] == held[0][0] for h in held), i
        assert all(h[1] == with_cmds[0][1] for h in with_cmds), i
    if d.mode != MIN:
        return
    for rep in d.reps:
        follows = [g for g in range(G) if g % N != rep.r]
        log = bytes(rep.durable)
        leads_any = any(int(rep.st["status"][i]) != NIL for g in range(G) if g % N == rep.r
                        for i in range(g * ipg, (g + 1) * ipg))
        one_each = all(int(rep.inst["n_cmds"][i]) == 1 for g in follows
                       for i in range(g * ipg, (g + 1) * ipg) if int(rep.st["status"][i]) != NIL)
        if leads_any or not one_each or not log or not hasattr(rep.be, "replay_durable"):
            continue        # a leader's decide records carry no command: the Go cannot read them back
        recs, op, key, val, last, ballot, cu = rep.be.replay_durable(
            np.frombuffer(log, np.uint8), G * ipg, default_ballot=-1)
        d.replayed = getattr(d, "replayed", 0) + 1
        for i in range(G * ipg):
            if int(rep.st["status"][i]) == NIL:
                assert last[i] == -1, i
                continue
            j, a = int(last[i]), int(rep.inst["first_cmd"][i])
            assert (int(recs["ballot"][j]), int(recs["status"][j]), int(recs["inst_no"][j])) == \
                (int(rep.st["ballot"][i]), int(rep.st["status"][i]), i), i
            assert (int(op[j]), int(key[j]), int(val[j])) == \
                (int(rep.arena[0][a]), int(rep.arena[1][a]), int(rep.arena[2][a])), i

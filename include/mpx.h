/*
 * mpx.h — C ABI of the MI355X batched-consensus engine (minpaxos_amd).
 *
 * The engine replaces, for batches of records, the per-message hot path of the
 * MinPaxos replica (arobertlin/MinPaxos, Go):
 *
 *   mpx_accept_tally      <- bareminpaxos.(*Replica).handleAcceptReply
 *                              src/bareminpaxos/bareminpaxos.go:1014-1064   (MPX_MODE_MIN)
 *                            paxos.(*Replica).handleAcceptReply
 *                              src/paxos/paxos.go:631-673 (+ updateCommittedUpTo :259-264)
 *                                                                          (MPX_MODE_CLASSIC)
 *   mpx_prepare_select    <- paxos.(*Replica).handlePrepareReply  src/paxos/paxos.go:577-629
 *   mpx_prepare_select_min<- bareminpaxos.(*Replica).handlePrepareReply
 *                              src/bareminpaxos/bareminpaxos.go:912-966 (+ PrepareBookkeeping :75-82)
 *   mpx_apply             <- (*state.Command).Execute  src/state/state.go:77-103, driven in log
 *                            order by executeCommands  src/bareminpaxos/bareminpaxos.go:1066-1098
 *                            (conf_prev output: state.Conflict  src/state/state.go:53-60)
 *   mpx_conflict_batch    <- state.ConflictBatch  src/state/state.go:62-71
 *   mpx_group_step        <- handleAcceptReply + executeCommands for many independent replicas
 *                            (Paxos groups) at once: one tally and one apply per group
 *   mpx_watermarks_allreduce <- (no reference equivalent; the one cross-shard step: an RCCL
 *                            all-reduce of per-group committedUpTo / executed watermarks)
 *   mpx_decode_peer_stream <- genericsmr.(*Replica).replicaListener
 *                              src/genericsmr/genericsmr.go:402-446 with the fixed-size
 *                            Unmarshal()s it dispatches to (minpaxosprotomarsh.go:259-270,
 *                            :568-580, :737-749; Beacon/BeaconReply): frames a peer byte stream
 *                            and decodes its AcceptReplies into mpx_accept_reply records
 *   mpx_encode_replies    <- the ProposeReplyTS fan-out of handleAcceptReply
 *                              src/bareminpaxos/bareminpaxos.go:1030-1042 and executeCommands
 *                            :1076-1084 through ReplyProposeTS (genericsmr.go:529-535): the byte
 *                            run each client connection receives for a batch of replies
 *   mpx_accept_handle     <- bareminpaxos.(*Replica).handleAccept  bareminpaxos.go:753-806 /
 *                            paxos.(*Replica).handleAccept  src/paxos/paxos.go:470-520: the
 *                            acceptor's half of Phase 2, and mpx_encode_accept_replies the
 *                            AcceptReply frames replyAccept writes to each leader's connection
 *   mpx_propose_handle    <- bareminpaxos.(*Replica).handlePropose  bareminpaxos.go:617-710 /
 *                            paxos.(*Replica).handlePropose  src/paxos/paxos.go:388-443: which
 *                            drained proposals become an instance, and mpx_encode_accepts the
 *                            Accept frames bcastAccept (:450-520 / :299-331) writes to every peer;
 *                            mpx_encode_accepts_stored the same frames with the CatchUpLog read
 *                            from the instance store (st / lb / mpx_inst_cmds and the arena)
 *   mpx_unmarshal_frames  <- Accept / Commit / PrepareReply.Unmarshal with Instance.Unmarshal and
 *                            Command.Unmarshal (minpaxosprotomarsh.go:470-507, :648-672, :352-387,
 *                            :126-153 / paxosprotomarsh.go:244-268, :403-430, :152-176;
 *                            statemarsh.go:21-39): the frames mpx_decode_stream found, as the
 *                            records mpx_accept_handle takes and the SoA commands and catch-up log
 *                            mpx_apply, mpx_encode_log and mpx_accept_batch.log_* take
 *   mpx_commit_handle     <- bareminpaxos.(*Replica).handleCommit / handleCommitShort
 *                            bareminpaxos.go:856-910 / paxos.go:522-575 with updateCommittedUpTo
 *                            (paxos.go:259-264): the follower's last station of Phase 2, and
 *                            mpx_encode_commits the CommitShort / Commit frames bcastCommit
 *                            (bareminpaxos.go:565-615 / paxos.go:336-386) writes to every peer;
 *                            mpx_gather_commit_shorts turns received CommitShort bodies into records
 *   mpx_decode_client_streams <- genericsmr.(*Replica).clientListener (genericsmr.go:448-490) with
 *                            Propose.Unmarshal (gsmrprotomarsh.go:65-80) for many client
 *                            connections at once: the proposals as SoA commands, their reply
 *                            metadata and the prop_off / send_off mpx_propose_handle_dev takes
 *   mpx_build_replies     <- the three reply loops: handlePropose's refusals (bareminpaxos.go:
 *                            622-623, :682-683 / paxos.go:390-391), handleAcceptReply with !Dreply
 *                            (bareminpaxos.go:1030-1042 / paxos.go:644-655) and executeCommands
 *                            with Dreply (bareminpaxos.go:1076-1084 / paxos.go:685-693): the
 *                            mpx_reply_recs mpx_encode_replies takes, and bcastCommit's send list
 *   mpx_execute_gather    <- executeCommands' walk (bareminpaxos.go:1066-1098 / paxos.go:675-706):
 *                            which instances run, and their commands gathered for mpx_apply
 *   mpx_store_commands    <- where handleAccept, handleCommit and handlePropose assign an
 *                            instance's Cmds (bareminpaxos.go:786-793, :861-868, :687-699): the
 *                            commands appended to a device arena, the slots' mpx_inst_cmds written;
 *                            mpx_store_compact squeezes the retired instances out of the arena
 *   mpx_record_log        <- the handlers' stable-store appends: recordInstanceMetadata (+
 *                            recordCommands) of handlePropose, handleAccept, handleCommit[Short]
 *                            and handleAcceptReply's commit branch (bareminpaxos.go:697-699,
 *                            :798-800, :881-882, :909, :1045-1046 / paxos.go:436-438, :547-548,
 *                            :574, :656-657): a batch's durable-log bytes as one run
 *   mpx_encode_log        <- minpaxosproto.(*Instance).Marshal (minpaxosprotomarsh.go:100-124) for
 *                            the CatchUpLog of bcastAccept (bareminpaxos.go:488-513), and
 *                            recordInstanceMetadata + recordCommands (bareminpaxos.go:164-188)
 *   mpx_replay_durable    <- getDataFromStableStore (bareminpaxos.go:122-161): the durable log
 *                            read back into records, watermarks and the instance slots
 *
 * Contract (every entry point):
 *   - plain C, no exceptions cross the boundary, never aborts; return 0 (MPX_OK) or a negative
 *     MPX_E_* code; mpx_last_error() explains the last failure of a handle.
 *   - records are processed with SEQUENTIAL semantics in array order: the results equal those of
 *     calling the reference handler once per record, in array order. Records must be grouped by
 *     instance (all replies for one instance contiguous) and the groups must appear in ASCENDING
 *     instance order (what the Go shim's stable sort of a drained batch produces); any other
 *     order is rejected with MPX_E_INVAL. Within a group, slot order = arrival order. MIN
 *     watermarks are "last assignment wins" in array order, which under ascending order is the
 *     highest instance that makes an assignment.
 *   - host-pointer entry points are synchronous: results are in the caller's buffers on return.
 *     *_dev entry points take device pointers and a hipStream_t (passed as void*, NULL = the
 *     engine's stream) and are asynchronous; they never allocate or synchronise, so they can be
 *     captured into a hipGraph.
 *   - alignment of *_dev pointers: arrays of 16- and 32-byte records (mpx_accept_reply,
 *     mpx_inst_state, mpx_prepare_reply, mpx_prep_state, mpx_group_prep_state, mpx_var_frame,
 *     mpx_log_rec, mpx_accept_msg, mpx_acceptor_state) 16 bytes - the kernels move them as 16-byte
 *     vectors; every other array (mpx_prepare_reply_min, mpx_prepare_effect, mpx_peer_frame,
 *     mpx_reply_rec, results, offsets, scalars, keys, values) the alignment of its C type; byte
 *     arrays (op, decided / prepared flags, encoded output) any address. The two exceptions are
 *     the decoders' input byte streams, which need 16 bytes (stated at their entry points). The
 *     host-pointer forms take any alignment C allows: they stage into aligned device memory.
 *   - a handle is not re-entrant; use one handle per replica event loop / per GPU.
 *   - the tally (mpx_accept_tally_dev), CLASSIC prepare (mpx_prepare_select_dev), apply
 *     (mpx_apply_dev), group-step and durable-log replay (mpx_replay_durable_dev) kernels keep
 *     control words or scratch in the handle between calls (tickets, maxima, the replica-batch
 *     list tags, the replay's binned-maximum scratch), each reset by the call's last workgroup,
 *     and the encoders, mpx_unmarshal_frames_dev, mpx_decode_client_streams_dev,
 *     mpx_build_replies_dev, mpx_execute_gather_dev, mpx_store_commands_dev,
 *     mpx_store_compact_dev and mpx_record_log_dev keep their offsets, maps and totals there:
 *     all *_dev calls on one handle must be issued in ONE stream order (one stream, or streams
 *     ordered by events) — two such calls in flight at once corrupt every later call.
 *   - a captured graph keeps the scratch pointers of the calls it captured: growing a handle's
 *     scratch afterwards (a larger mpx_apply_reserve / mpx_replay_durable_reserve /
 *     mpx_unmarshal_frames_reserve / mpx_decode_client_streams_reserve /
 *     mpx_build_replies_reserve / mpx_execute_gather_reserve / mpx_store_commands_reserve /
 *     mpx_store_compact_reserve / mpx_record_log_reserve, or a host-pointer mpx_apply /
 *     mpx_replay_durable / mpx_unmarshal_frames / mpx_decode_client_streams / mpx_build_replies /
 *     mpx_execute_gather / mpx_store_commands / mpx_store_compact / mpx_record_log call that
 *     needs more) frees the old buffers and
 *     invalidates such graphs; reserve the largest size before capturing.
 *   - where the reference would panic (nil instance, peer id outside peerCommits), the engine
 *     returns MPX_E_NIL_INSTANCE / MPX_E_BAD_ID and the outputs are unspecified.
 */
#ifndef MPX_H_
#define MPX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPX_ABI_VERSION 8  /* 4: + mpx_group_step_totals_dev; 5: + mpx_graph_*, mpx_apply_buffers / _staged;
                              6: + mpx_replay_durable_reserve; 7: + mpx_group_step_events;
                              8: + MPX_FLAG_STEP_ONE_LAUNCH; additive since, same number:
                              mpx_accept_handle[_dev], mpx_encode_accept_replies[_reserve|_dev],
                              mpx_propose_handle[_dev], mpx_encode_accepts[_reserve|_dev],
                              mpx_unmarshal_frames[_reserve|_dev], mpx_commit_handle[_dev],
                              mpx_encode_commits[_reserve|_dev], mpx_gather_commit_shorts[_dev],
                              mpx_order_records[_reserve|_dev],
                              mpx_decode_client_streams[_reserve|_dev],
                              mpx_build_replies[_reserve|_dev],
                              mpx_execute_gather[_reserve|_dev],
                              mpx_store_commands[_reserve|_dev], mpx_store_compact[_reserve|_dev],
                              mpx_record_log[_reserve|_dev], mpx_record_bound,
                              mpx_encode_accepts_stored[_reserve|_dev] */

/* ---- error codes ---------------------------------------------------------------------- */
#define MPX_OK 0
#define MPX_E_INVAL (-1)        /* bad argument / size / layout                            */
#define MPX_E_NOMEM (-2)        /* host or device allocation failed                        */
#define MPX_E_HIP (-3)          /* HIP runtime error                                       */
#define MPX_E_RCCL (-4)         /* RCCL error                                              */
#define MPX_E_NIL_INSTANCE (-5) /* record names an instance outside the window or nil:
                                   the reference dereferences a nil *Instance (panic)     */
#define MPX_E_BAD_ID (-6)       /* reply Id outside [0,N): reference indexes peerCommits   */
#define MPX_E_KV_FULL (-7)      /* KV table capacity exceeded                              */
#define MPX_E_NODEV (-8)        /* no GPU / HIP device unavailable                         */
#define MPX_E_UNSUPPORTED (-9)  /* input beyond the supported limits                       */

/* ---- enums (values mirror the reference) ---------------------------------------------- */
/* minpaxosproto.InstanceStatus  src/minpaxosproto/minpaxosproto.go:8-15
 * paxos.InstanceStatus          src/paxos/paxos.go:50-55                                   */
#define MPX_PREPARING 0
#define MPX_PREPARED 1
#define MPX_ACCEPTED 2
#define MPX_COMMITTED 3
#define MPX_STATUS_NIL (-1) /* instanceSpace[i] == nil                                      */

/* state.Operation  src/state/state.go:10-19 */
#define MPX_OP_NONE 0
#define MPX_OP_PUT 1
#define MPX_OP_GET 2
#define MPX_OP_DELETE 3
#define MPX_OP_RLOCK 4
#define MPX_OP_WLOCK 5

#define MPX_MODE_MIN 0     /* bareminpaxos semantics (the live protocol)                   */
#define MPX_MODE_CLASSIC 1 /* paxos semantics (classic per-instance Multi-Paxos)           */

#define MPX_MAX_REPLICAS 16 /* ballots are (round<<4)|replicaId: bareminpaxos.go:383-385   */

/* ---- packed records (no pointers: cgo-legal as unsafe.Pointer(&slice[0])) -------------- */

/* minpaxosproto.AcceptReply{Instance,OK,Ballot,Id}  src/minpaxosproto/minpaxosproto.go:75-80
 * (CLASSIC: paxosproto.AcceptReply{Instance,OK,Ballot} src/paxosproto/paxosproto.go:37-41;
 * id unused). ok follows the reference test `OK == TRUE` (TRUE = 1).                        */
typedef struct mpx_accept_reply {
    int32_t instance;
    int32_t ballot;
    int32_t id;
    uint8_t ok;
    uint8_t pad[3];
} mpx_accept_reply; /* 16 B */

/* Instance.Status + LeaderBookkeeping{MaxRecvBallot,AcceptOKs,Nacks}
 * src/minpaxosproto/minpaxosproto.go:17-29 ; src/paxos/paxos.go:57-70                      */
typedef struct mpx_inst_state {
    int32_t status;
    int32_t accept_oks;
    int32_t nacks;
    int32_t max_recv_ballot;
} mpx_inst_state; /* 16 B */

/* paxosproto.PrepareReply{Instance,OK,Ballot,Command}  src/paxosproto/paxosproto.go:23-28.
 * Command is an opaque handle the host resolves (an empty command is just another handle). */
typedef struct mpx_prepare_reply {
    int32_t instance;
    int32_t ballot;
    uint32_t ok;
    uint32_t value_id;
} mpx_prepare_reply; /* 16 B */

/* per-instance CLASSIC prepare state: paxos Instance{cmds,ballot,status,lb}
 * src/paxos/paxos.go:57-70 ; value_id = handle of inst.cmds                                */
#define MPX_PF_HAS_PROPOSALS 1u /* lb.clientProposals != nil                                */
#define MPX_PF_REQUEUED 2u      /* proposals were pushed back on ProposeChan in this call    */
#define MPX_PF_PREPARED_NOW 4u  /* instance became PREPARED in this call (host bcastAccept)  */
typedef struct mpx_prep_state {
    int32_t ballot; /* inst.ballot                                                          */
    int32_t status;
    int32_t prepare_oks;
    int32_t nacks;
    int32_t max_recv_ballot;
    uint32_t value_id;
    uint32_t flags;
    uint32_t pad;
} mpx_prep_state; /* 32 B */

/* minpaxosproto.PrepareReply{Id,Instance,OK,Ballot,LastCommitted,Command,CatchUpLog}
 * src/minpaxosproto/minpaxosproto.go:56-64 (Command -> value_id; CatchUpLog stays host-side) */
typedef struct mpx_prepare_reply_min {
    int32_t id;
    int32_t instance;
    int32_t ballot;
    int32_t last_committed;
    uint32_t ok;
    uint32_t value_id;
} mpx_prepare_reply_min; /* 24 B */

/* bareminpaxos PrepareBookkeeping src/bareminpaxos/bareminpaxos.go:75-82, plus the replica
 * scalars it reads/writes (defaultBallot, committedUpTo). peerCommits lives in a separate
 * [groups][N] int32 array.                                                                */
typedef struct mpx_group_prep_state {
    int32_t default_ballot;   /* r.defaultBallot (read only)                                */
    int32_t prepare_oks;
    int32_t nacks;
    int32_t max_recv_ballot;
    int32_t highest_instance; /* highestInstanceNumber                                      */
    uint32_t value_id;        /* handle of prepareBookkeeping.cmds                          */
    int32_t committed_upto;   /* r.committedUpTo                                            */
    uint32_t triggered;       /* number of times the accept trigger (:945) fired            */
} mpx_group_prep_state; /* 32 B */

/* per-record effect of mpx_prepare_select_min: what the host must do for that reply        */
#define MPX_EF_COUNTED 1u  /* ballot == defaultBallot: counted (:921-923)                   */
#define MPX_EF_SELECTED 2u /* became the max (instance, ballot): cmds = reply.Command (:925) */
#define MPX_EF_CATCHUP 4u  /* copy CatchUpLog[0 .. last_committed-catchup_from] into
                              instanceSpace[catchup_from ..] (:934-940)                     */
#define MPX_EF_TRIGGER 8u  /* install Instance{defaultBallot,ACCEPTED,cmds} at highest and
                              bcastAccept (:945-958)                                        */
typedef struct mpx_prepare_effect {
    uint32_t flags;
    int32_t catchup_from;
} mpx_prepare_effect; /* 8 B */

/* ---- engine ----------------------------------------------------------------------------- */
typedef struct mpx_config {
    int32_t n_replicas;     /* N, 1..16                                                     */
    int32_t mode;           /* MPX_MODE_MIN / MPX_MODE_CLASSIC                              */
    uint64_t kv_capacity;   /* key capacity of the engine's KV table (mpx_apply); 0 = 1<<20.
                               The table has the next power of two >= 2 x kv_capacity slots
                               (at least 1024), cut by key hash into buckets of 256 slots;
                               a key whose bucket is full fails the call with MPX_E_KV_FULL
                               (at the default load of <= 1/2 a practical impossibility
                               for non-adversarial keys)                                  */
    uint32_t kv_per_group;  /* max live keys per group table (mpx_group_step), <= 1024;
                               0 = 512. Also picks the fused step's fast-path variant (256:
                               the config-5 kernel); a group whose call touches more than
                               2048 distinct keys fails with MPX_E_KV_FULL                  */
    uint32_t flags;         /* MPX_FLAG_* (0: none)                                         */
    uint64_t max_groups;    /* groups per mpx_group_step_dev call (work list); 0 = 1<<20    */
    /* mpx_apply tuning, fixed for the handle's life (0 = default everywhere). Every setting
     * gives identical results; they move time and scratch only.                            */
    uint64_t apply_chunk;   /* commands per pipeline chunk (bounds the scratch of one call:
                               34 B / command partitioned, 48 B sorted); 0 = 1<<26          */
    uint32_t apply_path;    /* MPX_APPLY_AUTO: by call size (the replica-batch kernels up to
                               MPX_APPLY_SMALL_MAX commands, the partitioned pipeline past
                               it - the sort-based one only between MPX_APPLY_SMALL_MAX and
                               a raised apply_fast_min); calls past MPX_APPLY_SMALL_MAX
                               commands on tables past 2^30 slots are unsupported (the
                               partitioned pipeline stops there, the sort-based one's result
                               codes at 2^29 slots: the call fails); or
                               force one of MPX_APPLY_SMALL / _SORTED / _PARTITIONED (SMALL
                               and PARTITIONED where the call / table allow, else AUTO's
                               pick)                                                        */
    uint32_t apply_fast_min;  /* AUTO: calls of at least this many commands (and more than
                                 MPX_APPLY_SMALL_MAX) run partitioned; 0 = 16384            */
    uint32_t apply_hot_min;   /* partitioned: samples (of 64K) that make a key hot and keep
                                 its commands in place; 0 = 5; MPX_APPLY_NO_HOT = none      */
    uint32_t reserved;        /* 0                                                          */
} mpx_config; /* 56 B */

/* mpx_config.flags */
#define MPX_FLAG_STEP_ONE_LAUNCH 1u /* every mpx_group_step[_totals]_dev is ONE kernel: the
                               per-group fast kernel, which also reduces the step totals (its
                               last workgroup), with no work-list kernel behind it. The shape
                               must fit a fast variant (R = max(N-1,1) x ipg replies: ipg <= 256
                               with R <= 1024 and kv_per_group <= 1024, or R <= 2048 and
                               kv_per_group <= 256; ipg <= 512 with R <= 2048 and kv_per_group
                               <= 512; else the call returns MPX_E_INVAL) and so must every
                               group: at most R replies, 1024 commands (2048 at ipg > 256), distinct keys
                               within the variant's LDS table - a group past them fails the step
                               (MPX_E_INVAL at the next synchronising call, its outputs not
                               written). For callers that bound their batches; the default
                               two-launch step takes any group.                              */
#define MPX_FLAG_KNOWN 1u

#define MPX_APPLY_AUTO 0
#define MPX_APPLY_SORTED 1
#define MPX_APPLY_PARTITIONED 2
#define MPX_APPLY_SMALL 3
#define MPX_APPLY_NO_HOT 0xFFFFFFFFu
#define MPX_APPLY_SMALL_MAX 16384

typedef struct mpx_engine mpx_engine;

int mpx_abi_version(void);
int mpx_device_count(int* count);
int mpx_open(int device, const mpx_config* cfg, mpx_engine** out);
int mpx_close(mpx_engine* eng);
const char* mpx_last_error(mpx_engine* eng);
/* the engine's HIP stream (hipStream_t), for callers that queue their own work on it      */
void* mpx_stream(mpx_engine* eng);
int mpx_synchronize(mpx_engine* eng);

/* ---- A1/A2: accept tally (host pointers, synchronous) ----------------------------------
 * st[i] is the state of instance inst_base+i, updated in place. committed_upto and
 * peer_commits[N] are in/out (r.committedUpTo, r.prepareBookkeeping.peerCommits).
 * decided_out (optional, n_inst bytes) = 1 for instances decided in this call, else 0.   */
int mpx_accept_tally(mpx_engine* eng, const mpx_accept_reply* recs, size_t n,
                     mpx_inst_state* st, size_t n_inst, int32_t inst_base,
                     int32_t* committed_upto, int32_t* peer_commits, uint8_t* decided_out);

/* device-pointer variant. st_in/st_out may alias; st_out[i] is written for every instance
 * that has at least one record (other entries untouched). d_scalars: int32 in/out
 * [0] = committedUpTo, [1..N] = peerCommits. d_decided (optional): as decided_out, all n_inst
 * bytes written. Alignment: d_recs, d_st_in, d_st_out 16 bytes; d_scalars 4; d_decided any. */
int mpx_accept_tally_dev(mpx_engine* eng, const mpx_accept_reply* d_recs, size_t n,
                         const mpx_inst_state* d_st_in, mpx_inst_state* d_st_out,
                         size_t n_inst, int32_t inst_base, int32_t* d_scalars,
                         uint8_t* d_decided, void* stream);

/* ---- A4: CLASSIC prepare selection (max-ballot value selection) ------------------------
 * default_ballot in/out (r.defaultBallot raised to inst.ballot of newly prepared instances)
 * prepared_out (optional): 1 where the instance became PREPARED in this call.              */
int mpx_prepare_select(mpx_engine* eng, const mpx_prepare_reply* recs, size_t n,
                       mpx_prep_state* st, size_t n_inst, int32_t inst_base,
                       int32_t* default_ballot, uint8_t* prepared_out);
/* device-pointer variant, as mpx_accept_tally_dev: d_st_in / d_st_out may alias, d_st_out[i] is
 * written only for instances that have records. Alignment: d_recs, d_st_in, d_st_out 16 bytes;
 * d_default_ballot 4; d_prepared any.                                                       */
int mpx_prepare_select_dev(mpx_engine* eng, const mpx_prepare_reply* d_recs, size_t n,
                           const mpx_prep_state* d_st_in, mpx_prep_state* d_st_out,
                           size_t n_inst, int32_t inst_base, int32_t* d_default_ballot,
                           uint8_t* d_prepared, void* stream);

/* ---- A3: MIN prepare selection, one PrepareBookkeeping per group ------------------------
 * replies of group g are recs[grp_rec_off[g] .. grp_rec_off[g+1]) in arrival order.
 * peer_commits: [n_groups][N] in/out. eff (optional): one effect per record.              */
int mpx_prepare_select_min(mpx_engine* eng, const mpx_prepare_reply_min* recs, size_t n,
                           const uint64_t* grp_rec_off, mpx_group_prep_state* gst,
                           size_t n_groups, int32_t* peer_commits, mpx_prepare_effect* eff);
/* device-pointer variant; d_grp_rec_off is trusted. Alignment: d_gst 16 bytes; d_grp_rec_off 8;
 * d_recs (24-byte records), d_peer_commits, d_eff 4.                                         */
int mpx_prepare_select_min_dev(mpx_engine* eng, const mpx_prepare_reply_min* d_recs,
                               size_t n, const uint64_t* d_grp_rec_off,
                               mpx_group_prep_state* d_gst, size_t n_groups,
                               int32_t* d_peer_commits, mpx_prepare_effect* d_eff,
                               void* stream);

/* ---- A5/A6: batched KV apply on the engine's State ---------------------------------------
 * Executes the m commands in array (log) order against the engine's persistent table:
 * ret[i] = Execute's return value; conf_prev[i] (optional) = state.Conflict(previous command
 * on the same key in this call, command i), 0 if there is none. Only keys PUT at some point
 * occupy the table: GETs (and other ops) of absent keys return NIL and leave it unchanged.   */
int mpx_apply(mpx_engine* eng, const uint8_t* op, const int64_t* key, const int64_t* val,
              size_t m, int64_t* ret, uint8_t* conf_prev);
/* allocate the KV table and the apply workspace for calls of up to max_cmds commands, so
 * that mpx_apply_dev (which never allocates) can run; idempotent, grows only               */
int mpx_apply_reserve(mpx_engine* eng, size_t max_cmds);
int mpx_apply_dev(mpx_engine* eng, const uint8_t* d_op, const int64_t* d_key,
                  const int64_t* d_val, size_t m, int64_t* d_ret, uint8_t* d_conf_prev,
                  void* stream);
/* ---- replica-batch apply without copies (the cgo shim's form, ABI 5) -------------------
 * mpx_apply_buffers: the engine's pinned, GPU-mapped command and result arrays for calls of up
 * to max_m (<= MPX_APPLY_SMALL_MAX) commands; the caller writes a drained executeCommands batch
 * straight into io->op / key / val and calls mpx_apply_staged(eng, m): the results of
 * mpx_apply(eng, io->op, io->key, io->val, m, io->ret, io->conf) land in io->ret / io->conf,
 * read and written by the kernels across the link, with no copy on either side. The arrays stay
 * valid until the next mpx_apply_buffers that grows them or mpx_close; needs apply_path AUTO or
 * SMALL. Synchronous, like mpx_apply.                                                       */
typedef struct mpx_apply_io {
    uint8_t* op;
    int64_t* key;
    int64_t* val;
    int64_t* ret;
    uint8_t* conf;
    uint64_t cap;  /* commands the arrays hold                                               */
} mpx_apply_io;
int mpx_apply_buffers(mpx_engine* eng, size_t max_m, mpx_apply_io* io);
int mpx_apply_staged(mpx_engine* eng, size_t m);
/* table access: number of present keys; export (any order) / import / clear               */
int mpx_kv_size(mpx_engine* eng, size_t* n);
int mpx_kv_export(mpx_engine* eng, int64_t* keys, int64_t* vals, size_t cap, size_t* n);
int mpx_kv_import(mpx_engine* eng, const int64_t* keys, const int64_t* vals, size_t n);
int mpx_kv_clear(mpx_engine* eng);

/* state.ConflictBatch over consecutive instances: out[i] = ConflictBatch(inst i, inst i+1),
 * instance i = commands [inst_off[i], inst_off[i+1]). out has n_inst-1 entries.            */
int mpx_conflict_batch(mpx_engine* eng, const uint8_t* op, const int64_t* key,
                       const uint64_t* inst_off, size_t n_inst, uint8_t* out);
/* device form; d_inst_off is trusted (n_inst+1 non-decreasing offsets starting at 0)       */
int mpx_conflict_batch_dev(mpx_engine* eng, const uint8_t* d_op, const int64_t* d_key,
                           const uint64_t* d_inst_off, size_t n_inst, uint8_t* d_out,
                           void* stream);

/* ---- A7: CLASSIC commit watermark (updateCommittedUpTo over a status window) ------------ */
int mpx_committed_prefix(mpx_engine* eng, const mpx_inst_state* st, size_t n_inst,
                         int32_t inst_base, int32_t* committed_upto);

/* ---- fused per-group step (sharded engine, config 5) -------------------------------------
 * G independent groups (replicas), each with ipg instance slots (instances 0..ipg-1 in its
 * own instance space). Group g's accept replies: recs[grp_rec_off[g]..grp_rec_off[g+1]),
 * grouped by instance, instance numbers group-local. Instance (g,i) owns commands
 * [cmd_off[g*ipg+i], cmd_off[g*ipg+i+1]); has_cmds (optional) = 0 marks Cmds == nil.
 * Per group: tally (cfg mode), then executeCommands from executed[g]+1 while
 * i <= committed[g] and Cmds != nil, against the group's KV table.
 * KV tables: kv_cnt[g] live entries in kv_key/kv_val[g*kv_per_group ..].                    */
typedef struct mpx_group_batch {
    uint32_t n_groups;
    uint32_t ipg;
    const mpx_accept_reply* recs;
    const uint64_t* grp_rec_off;   /* n_groups+1                                            */
    const mpx_inst_state* st_in;   /* n_groups*ipg                                          */
    mpx_inst_state* st_out;        /* may alias st_in                                       */
    const int32_t* committed_in;   /* n_groups                                              */
    int32_t* committed_out;
    const int32_t* executed_in;    /* n_groups (last executed instance, -1 = none)          */
    int32_t* executed_out;
    const int32_t* peer_in;        /* n_groups*N                                            */
    int32_t* peer_out;
    const uint8_t* op;             /* commands, global arrays                               */
    const int64_t* key;
    const int64_t* val;
    const uint32_t* cmd_off;       /* n_groups*ipg+1                                        */
    const uint8_t* has_cmds;       /* optional, n_groups*ipg                                */
    int64_t* ret;                  /* written for executed commands                         */
    uint8_t* conf_prev;            /* optional                                              */
    const uint32_t* kv_cnt_in;     /* n_groups                                              */
    const int64_t* kv_key_in;      /* n_groups*kv_per_group                                 */
    const int64_t* kv_val_in;
    uint32_t* kv_cnt_out;          /* may alias the inputs                                  */
    int64_t* kv_key_out;
    int64_t* kv_val_out;
    uint8_t* decided;              /* optional, n_groups*ipg                                */
    uint32_t* n_decided;           /* optional, n_groups: instances decided in this call
                                      (status became COMMITTED at a quorum crossing)        */
} mpx_group_batch;

/* host pointers (synchronous) / device pointers (asynchronous on stream). One handle runs
 * its group steps (and step totals) one at a time in stream order: they share the handle's
 * work-list and accumulator words.                                                         */
int mpx_group_step(mpx_engine* eng, const mpx_group_batch* b);
int mpx_group_step_dev(mpx_engine* eng, const mpx_group_batch* b, void* stream);

/* per-step totals of a group batch after mpx_group_step_dev (device pointers; b->n_decided
 * required): d_totals[0] = instances decided, d_totals[1] = instances executed
 * (executeCommands iterations), d_totals[2] = commands executed (Execute calls). Written, not
 * accumulated; reduce them over ranks with mpx_step_allreduce_dev.                         */
#define MPX_STEP_TOTALS 3
int mpx_step_totals_dev(mpx_engine* eng, const mpx_group_batch* b, int64_t* d_totals,
                        void* stream);
/* mpx_group_step_dev and mpx_step_totals_dev in one (b->n_decided required): the second
 * kernel of the step (the work-list kernel) also reduces the groups' outputs to d_totals[0..2]
 * (same values), so a step is two kernel launches instead of three.                       */
int mpx_group_step_totals_dev(mpx_engine* eng, const mpx_group_batch* b, int64_t* d_totals,
                              void* stream);
/* timing hook (ABI 7): every later group step of the handle records ev_fast_start right before
 * and ev_fast_end right after the launch of its first kernel (the per-group fast kernel, or the
 * work-list fill), on the call's stream, so the pair brackets that kernel alone (the work-list
 * kernel that follows is outside). Both NULL turns it off. Events from mpx_event_create;
 * they must stay alive while registered - mpx_event_destroy of either one unregisters the
 * pair (the hook is then off, as after NULL, NULL).                                           */
int mpx_group_step_events(mpx_engine* eng, void* ev_fast_start, void* ev_fast_end);

/* ---- multi-GPU: the one collective (RCCL over xGMI) -------------------------------------
 * Each rank owns a block of groups; non-owned entries must hold -1. After the call every
 * rank holds max over ranks (= the owner's value) for every group. 128-byte unique id is
 * produced by rank 0 and broadcast by the caller (e.g. through torch.distributed).         */
int mpx_comm_unique_id(void* out128);
int mpx_comm_init(mpx_engine* eng, int nranks, int rank, const void* unique_id128);
int mpx_watermarks_allreduce(mpx_engine* eng, int32_t* committed, int32_t* executed,
                             size_t n_groups);
/* device pointers: committed/executed are one contiguous int32 buffer of 2*n_groups       */
int mpx_watermarks_allreduce_dev(mpx_engine* eng, int32_t* d_watermarks, size_t n_groups,
                                 void* stream);
/* the whole per-step exchange as one RCCL group: max over ranks of the 2*n_groups watermark
 * vector and sum over ranks of n_totals int64 counters (e.g. the mpx_step_totals_dev ones)  */
int mpx_step_allreduce_dev(mpx_engine* eng, int32_t* d_watermarks, size_t n_groups,
                           int64_t* d_totals, size_t n_totals, void* stream);
/* the same exchange out of place: d_wm_send keeps -1 on the groups other ranks own for good
 * (set once; the group step writes only the rank's own range), so a step needs no refill of
 * the foreign ranges; the max over ranks lands in d_wm_recv (2*n_groups). d_totals is reduced
 * in place.                                                                                 */
int mpx_step_allreduce_oop_dev(mpx_engine* eng, const int32_t* d_wm_send, int32_t* d_wm_recv,
                               size_t n_groups, int64_t* d_totals, size_t n_totals, void* stream);

/* ---- peer stream framing + AcceptReply decode ----------------------
 * A peer connection carries frames [code u8][body]. Codes (genericsmrproto.go:7-18 and the
 * registration order of bareminpaxos.NewReplica, bareminpaxos.go:108-113):                 */
#define MPX_PEER_BEACON 6        /* 8-byte timestamp                                         */
#define MPX_PEER_BEACON_REPLY 7  /* 8-byte timestamp                                         */
#define MPX_PEER_PREPARE 8       /* 12-byte body                                             */
#define MPX_PEER_ACCEPT 9        /* variable length (Command + CatchUpLog slices)            */
#define MPX_PEER_COMMIT 10       /* variable length (Command slice)                          */
#define MPX_PEER_COMMIT_SHORT 11 /* 16-byte body                                             */
#define MPX_PEER_PREPARE_REPLY 12/* variable length                                          */
#define MPX_PEER_ACCEPT_REPLY 13 /* 13-byte body {Instance i32, OK u8, Ballot i32, Id i32}   */
/* every other code is a 1-byte frame (replicaListener logs "unknown message type" and reads
 * the next byte as a new code, genericsmr.go:440-442)                                       */

/* a fixed-size frame other than AcceptReply: where it starts (its code byte) and its code  */
typedef struct mpx_peer_frame {
    uint32_t offset;
    uint8_t code;
    uint8_t pad[3];
} mpx_peer_frame; /* 8 B */

#define MPX_DECODE_END 0      /* the buffer ends exactly at a frame boundary                 */
#define MPX_DECODE_PARTIAL 1  /* stopped at a frame whose body runs past the buffer: keep the
                                 tail [consumed, len) and call again when more bytes arrive   */
#define MPX_DECODE_VARIABLE 2 /* stopped at a variable-length frame (Accept / Commit /
                                 PrepareReply) at `consumed`: the host unmarshals it and
                                 calls again after it                                        */
#define MPX_DECODE_MAX_BYTES 0x7FFFFFFFu /* per call                                        */

typedef struct mpx_decode_result {
    uint64_t consumed;         /* bytes framed (start of the stop frame, or len)            */
    uint64_t n_accept_replies; /* AcceptReply frames in [0, consumed)                       */
    uint64_t n_other;          /* other fixed-size frames in [0, consumed)                  */
    int32_t stop_reason;       /* MPX_DECODE_*                                              */
    int32_t stop_code;         /* code byte at `consumed`, -1 at MPX_DECODE_END             */
} mpx_decode_result; /* 32 B */

/* Frames buf[0..len) in stream order. AcceptReplies go to ar[0..min(n, ar_cap)) in arrival
 * order, other fixed-size frames to other[0..min(n, other_cap)); the counts in *res are
 * always complete, so a caller whose capacity was short sees n > cap and can call again.
 * AcceptReply is framed as the 13 bytes its Marshal writes (minpaxosprotomarsh.go:545-566);
 * the reference's io.ReadAtLeast(wire, bs, 9) (:571) can return a short body on a partial
 * TCP read and desynchronise the stream, which the engine does not reproduce.              */
int mpx_decode_peer_stream(mpx_engine* eng, const uint8_t* buf, size_t len,
                           mpx_accept_reply* ar, size_t ar_cap, mpx_peer_frame* other,
                           size_t other_cap, mpx_decode_result* res);
/* scratch for mpx_decode_peer_stream_dev on buffers of up to max_len bytes (grows only)    */
int mpx_decode_reserve(mpx_engine* eng, size_t max_len);
/* device form: needs mpx_decode_reserve(len) first. d_buf must be 16-byte aligned (the tiles are
 * loaded as 16-byte vectors; any other address is rejected with MPX_E_INVAL), d_ar 16 bytes,
 * d_res 8, d_other 4. A capacity of 0 may come with a null pointer.                          */
int mpx_decode_peer_stream_dev(mpx_engine* eng, const uint8_t* d_buf, size_t len,
                               mpx_accept_reply* d_ar, size_t ar_cap, mpx_peer_frame* d_other,
                               size_t other_cap, mpx_decode_result* d_res, void* stream);

/* ---- full peer-stream decode: fixed AND variable-length frames, MIN or CLASSIC wire ------
 * mpx_decode_stream frames one connection's bytes with the framing of the engine's protocol
 * (mpx_config.mode): bareminpaxos registers minpaxosproto messages (bareminpaxos.go:108-113),
 * paxos registers paxosproto messages (paxos.go:93-98), both as codes 8..13 in the order
 * Prepare, Accept, Commit, CommitShort, PrepareReply, AcceptReply. Body lengths:
 *                   MIN (minpaxosprotomarsh.go)            CLASSIC (paxosprotomarsh.go)
 *   6/7 Beacon      8                                        8
 *   8  Prepare      12 (:259-270)                            13 (:76-87)
 *   9  Accept       16 + V(n) + 17n + V(m) + m Instances     12 + V(n) + 17n (:244-270)
 *                   (:470-507)
 *   10 Commit       12 + V(n) + 17n (:648-672)               12 + V(n) + 17n (:403-430)
 *   11 CommitShort  16 (:737-749)                            16 (:492-503)
 *   12 PrepareReply 17 + V(n) + 17n + V(m) + m Instances     9 + V(n) + 17n (:152-176)
 *                   (:352-387)
 *   13 AcceptReply  13 (:568-580)                            9 (:324-338)
 * V(x) is a Go binary.PutVarint (zig-zag, 1..10 bytes); an Instance is 8 + V(k) + 17k bytes
 * (:126-153); 17 bytes is one state.Command (statemarsh.go:21-37). Every other code is a 1-byte
 * frame (genericsmr.go:440-442).
 * Outputs, each in stream order:
 *   AcceptReply  -> mpx_accept_reply (CLASSIC: id = -1, the wire carries no Id)
 *   PrepareReply -> mpx_prepare_reply_min (MIN) / mpx_prepare_reply (CLASSIC) with value_id =
 *                   the index of the frame's mpx_var_frame (its Command slice), AND an
 *                   mpx_var_frame
 *   Accept / Commit -> mpx_var_frame (mpx_unmarshal_frames turns the byte ranges into records)
 *   other fixed-size frames -> mpx_peer_frame                                               */
typedef struct mpx_var_frame {
    uint32_t offset;      /* the frame's code byte                                          */
    uint32_t length;      /* code byte included                                            */
    uint32_t n_cmds;      /* len(Command)                                                   */
    uint32_t cmds_off;    /* first 17-byte Command                                          */
    uint32_t n_log;       /* len(CatchUpLog) (MIN Accept / PrepareReply), else 0              */
    uint32_t log_off;     /* first Instance of the CatchUpLog (end of Command if n_log == 0)  */
    uint8_t code;
    uint8_t pad[7];
} mpx_var_frame; /* 32 B */

typedef struct mpx_decode_out {
    mpx_accept_reply* ar;     size_t ar_cap;
    void* prep;               size_t prep_cap; /* mpx_prepare_reply_min[] (MIN) or
                                                  mpx_prepare_reply[] (CLASSIC)              */
    mpx_var_frame* var;       size_t var_cap;
    mpx_peer_frame* other;    size_t other_cap;
} mpx_decode_out;

#define MPX_DECODE_MALFORMED 3 /* a varint overflows 64 bits (Unmarshal returns an error and
                                  replicaListener stops, genericsmr.go:433-437) or a slice
                                  length is negative (make panics)                          */
#define MPX_DECODE_LONG 4      /* _dev only: the frame at `consumed` ends more than
                                  MPX_DECODE_WINDOW bytes past the 128-byte chunk it starts
                                  in; it IS decoded (counted, records written) and the chain
                                  resumes at `next`: call again with start = next            */
#define MPX_DECODE_WINDOW 64

typedef struct mpx_stream_result {
    uint64_t consumed;          /* stop position (len at MPX_DECODE_END)                     */
    uint64_t next;              /* MPX_DECODE_LONG: where the next frame starts              */
    uint64_t n_accept_replies;  /* totals over the stream so far (in/out for the _dev form)  */
    uint64_t n_prepare_replies;
    uint64_t n_var;
    uint64_t n_other;
    int32_t stop_reason;        /* MPX_DECODE_END / PARTIAL / MALFORMED (/ LONG, _dev)       */
    int32_t stop_code;          /* code byte at `consumed`, -1 at MPX_DECODE_END             */
} mpx_stream_result; /* 56 B */

/* host pointers, synchronous: the whole buffer (long frames included); res out            */
int mpx_decode_stream(mpx_engine* eng, const uint8_t* buf, size_t len,
                      const mpx_decode_out* out, mpx_stream_result* res);
/* scratch for _dev calls on buffers of up to max_len bytes (grows only)                    */
int mpx_decode_stream_reserve(mpx_engine* eng, size_t max_len);
/* device form: frames d_buf[start, len) (start = 0, or a previous call's res.next) and
 * appends records at the indices the counts in *d_res (in/out: zero it for a new stream)
 * give; one call stops at the first frame that is a terminal (END / PARTIAL / MALFORMED) or
 * LONG. `out` is a host struct of device pointers. Needs mpx_decode_stream_reserve(len) first.
 * d_buf must be 16-byte aligned (whatever `start` is; any other address is rejected with
 * MPX_E_INVAL); out->ar, out->var and CLASSIC's out->prep 16 bytes; d_res 8; MIN's out->prep
 * (24-byte records) and out->other 4. A capacity of 0 may come with a null pointer.          */
int mpx_decode_stream_dev(mpx_engine* eng, const uint8_t* d_buf, size_t len, size_t start,
                          const mpx_decode_out* out, mpx_stream_result* d_res, void* stream);

/* ---- client reply fan-out -----------------------------------------
 * One reply per executed (or decided) command, in execution order: the proposing client's
 * connection index, and the ProposeReplyTS fields the leader fills from
 * inst.Lb.ClientProposals[j] (CommandId, Timestamp) and Execute's return (Value; state.NIL = 0
 * for replies sent at decide time). genericsmrproto.ProposeReplyTS  genericsmrproto.go:31-37 */
typedef struct mpx_reply_rec {
    int64_t value;
    int64_t timestamp;
    int32_t command_id;
    uint32_t client; /* 0 .. n_clients-1                                                     */
} mpx_reply_rec; /* 24 B */

#define MPX_PROPOSE_REPLY_BYTES 25 /* gsmrprotomarsh.go:702-732: OK, CommandId, Value,
                                      Timestamp, Leader (little endian)                      */

/* out (25*n bytes) receives, client by client, each client's replies in execution order,
 * encoded exactly as ProposeReplyTS.Marshal writes them with OK = ok and Leader = leader;
 * client c's run is out[client_off[c] .. client_off[c+1]) (client_off: n_clients+1 entries).
 * A record whose client >= n_clients makes the call fail with MPX_E_INVAL.                  */
int mpx_encode_replies(mpx_engine* eng, const mpx_reply_rec* recs, size_t n, uint32_t n_clients,
                       uint8_t ok, int32_t leader, uint8_t* out, uint64_t* client_off);
int mpx_encode_replies_reserve(mpx_engine* eng, size_t max_n);
int mpx_encode_replies_dev(mpx_engine* eng, const mpx_reply_rec* d_recs, size_t n,
                           uint32_t n_clients, uint8_t ok, int32_t leader, uint8_t* d_out,
                           uint64_t* d_client_off, void* stream);

/* ---- the acceptor side: batched handleAccept and its AcceptReply bytes ---------------------
 * A replica answers the Accepts of every group it does not lead. mpx_accept_handle applies
 *   bareminpaxos.(*Replica).handleAccept  src/bareminpaxos/bareminpaxos.go:753-806  (MIN)
 *   paxos.(*Replica).handleAccept         src/paxos/paxos.go:470-520               (CLASSIC)
 * to a batch of Accept headers; what it emits is what mpx_accept_tally consumes on the leader. */

/* Accept header: minpaxosproto.Accept{LeaderId,Instance,Ballot,LastCommitted,Command,CatchUpLog}
 * minpaxosproto.go:66-73 / paxosproto.Accept{LeaderId,Instance,Ballot,Command} paxosproto.go:30-35.
 * Command -> value_id (a handle the host resolves). LastCommitted and CatchUpLog are read only by
 * commented-out code in handleAccept (:767-784), so they stay on the host. */
typedef struct mpx_accept_msg {
    int32_t instance;
    int32_t ballot;
    int32_t leader_id;
    uint32_t value_id;
} mpx_accept_msg; /* 16 B */

/* acceptor view of instanceSpace[i]: status MPX_STATUS_NIL = nil. flags: MPX_PF_HAS_PROPOSALS in,
 * MPX_PF_REQUEUED out (same bits as mpx_prep_state.flags); the caller clears MPX_PF_REQUEUED
 * once it has pushed the proposals back */
typedef struct mpx_acceptor_state {
    int32_t status;
    int32_t ballot;
    uint32_t value_id;
    uint32_t flags;
} mpx_acceptor_state; /* 16 B */

/* per group: r.defaultBallot (read only: handleAccept never writes it) and r.Id */
typedef struct mpx_acceptor_group {
    int32_t default_ballot;
    int32_t self_id;
} mpx_acceptor_group; /* 8 B */

#define MPX_AH_REPLIED 1u /* replyAccept was called: replies[i] / reply_to[i] are valid         */
#define MPX_AH_STORED 2u  /* instance installed or updated: the host stores Command and does
                             recordInstanceMetadata + recordCommands + sync (MIN :793-800,
                             CLASSIC :513-517)                                                  */
#define MPX_AH_REQUEUE 4u /* CLASSIC :495-502: clientProposals were pushed back on ProposeChan  */

/* msgs[n] under the contract above (grouped by instance, ascending; slot order = arrival order).
 * Window index idx = instance - inst_base belongs to group idx / ipg; n_inst == n_groups * ipg
 * (a single log: n_groups = 1, ipg = n_inst). st[n_inst] is updated in place; a nil instance is
 * legal input (the acceptor creates it). Outputs are slot-aligned with msgs, one entry per
 * message, always written: effect[i] (MPX_AH_*); where REPLIED, replies[i] (id = the group's
 * self_id in MIN, -1 in CLASSIC, whose wire has no Id) and reply_to[i] = msgs[i].leader_id;
 * elsewhere an all-zero record and reply_to[i] = -1.
 *   MIN: an Accept for an instance that is ACCEPTED at the message's ballot is ignored; otherwise,
 *   if the ballot equals default_ballot, the instance becomes {ACCEPTED, ballot, value_id, flags 0}
 *   (whatever its status was) and the reply is {instance, OK, ballot, self_id}; otherwise nothing.
 *   CLASSIC: every message replies. nil: ballot < default_ballot -> {FALSE, default_ballot}, else
 *   install {ACCEPTED, ballot, value_id, 0} and reply {TRUE, default_ballot}; inst.ballot > ballot
 *   -> {FALSE, inst.ballot}; inst.ballot < ballot -> take value and ballot, ACCEPTED, {TRUE, ballot},
 *   proposals requeued (MPX_PF_HAS_PROPOSALS -> MPX_PF_REQUEUED, MPX_AH_REQUEUE); equal -> take the
 *   value, ACCEPTED unless COMMITTED, {TRUE, default_ballot}. OK implies MPX_AH_STORED.
 * Errors: an instance outside the window (the reference's instanceSpace index panics) ->
 * MPX_E_NIL_INSTANCE; leader_id outside [0, N) on a message that replies (SendMsg indexes
 * PeerWriters, genericsmr.go:501) -> MPX_E_BAD_ID; order -> MPX_E_INVAL.                        */
int mpx_accept_handle(mpx_engine* eng, const mpx_accept_msg* msgs, size_t n,
                      mpx_acceptor_state* st, size_t n_inst, int32_t inst_base,
                      const mpx_acceptor_group* groups, size_t n_groups, uint32_t ipg,
                      mpx_accept_reply* replies, int32_t* reply_to, uint8_t* effect);
/* device form: d_st_in / d_st_out may alias; d_st_out[i] is written only for instances that have
 * messages. One kernel, no scratch, no control words.                                          */
int mpx_accept_handle_dev(mpx_engine* eng, const mpx_accept_msg* d_msgs, size_t n,
                          const mpx_acceptor_state* d_st_in, mpx_acceptor_state* d_st_out,
                          size_t n_inst, int32_t inst_base, const mpx_acceptor_group* d_groups,
                          size_t n_groups, uint32_t ipg, mpx_accept_reply* d_replies,
                          int32_t* d_reply_to, uint8_t* d_effect, void* stream);

/* The frames replyAccept -> SendMsg (genericsmr.go:499-512) writes: the code byte
 * MPX_PEER_ACCEPT_REPLY, then AcceptReply.Marshal, little endian:
 *   MIN      14 B  [13][Instance i32][OK u8][Ballot i32][Id i32]  (minpaxosprotomarsh.go:545-566)
 *   CLASSIC  10 B  [13][Instance i32][OK u8][Ballot i32]          (paxosprotomarsh.go:306-322)
 * by mpx_config.mode. replies[i] goes to destination reply_to[i] (< 0: skipped; >= n_dest: the
 * call fails with MPX_E_INVAL); n_dest <= MPX_MAX_REPLICAS. out (frame bytes x n) receives,
 * destination by destination, each destination's frames in array order, back to back;
 * destination d's run is out[dest_off[d] .. dest_off[d+1]) (dest_off: n_dest+1 entries).       */
#define MPX_ACCEPT_REPLY_FRAME_MIN 14
#define MPX_ACCEPT_REPLY_FRAME_CLASSIC 10
int mpx_encode_accept_replies(mpx_engine* eng, const mpx_accept_reply* replies,
                              const int32_t* reply_to, size_t n, uint32_t n_dest, uint8_t* out,
                              uint64_t* dest_off);
/* scratch for _dev calls of up to max_n replies (grows only; the dev entry never allocates). The
 * scratch lives in the handle: like the other *_dev calls that keep scratch there, encodes of one
 * handle run in one stream order, and a larger reserve invalidates graphs captured before it.   */
int mpx_encode_accept_replies_reserve(mpx_engine* eng, size_t max_n);
int mpx_encode_accept_replies_dev(mpx_engine* eng, const mpx_accept_reply* d_replies,
                                  const int32_t* d_reply_to, size_t n, uint32_t n_dest,
                                  uint8_t* d_out, uint64_t* d_dest_off, void* stream);

/* ---- instance-log encoding ----------------------------------
 * A run of log records (instance metadata + commands [cmd_off[i], cmd_off[i+1]) of the SoA
 * command arrays op/key/val, the layout mpx_apply takes) encoded back to back in one of the
 * reference's two byte formats; rec_off[i] is where record i starts, rec_off[n] the total.
 *   MPX_LOG_CATCHUP  Instance.Marshal: Ballot i32, Status i32, PutVarint(len(Cmds)), Cmds (17 B
 *                    each: Op, K, V). bcastAccept sends peer q the records peerCommits[q]+1 ..
 *                    lastCommitted: the suffix out[rec_off[from] .. rec_off[n]).
 *   MPX_LOG_DURABLE  recordInstanceMetadata (Ballot u32, Status u32, instNo u32) +
 *                    recordCommands (17 B per command; an empty or nil slice writes nothing). */
#define MPX_LOG_CATCHUP 0
#define MPX_LOG_DURABLE 1
typedef struct mpx_log_rec {
    int32_t ballot;
    int32_t status;
    int32_t inst_no; /* instNo (MPX_LOG_DURABLE; unused by MPX_LOG_CATCHUP)                  */
    uint32_t pad;
} mpx_log_rec; /* 16 B */

/* bytes out must hold for n records with m commands in total                              */
size_t mpx_encode_log_bound(size_t n, size_t m);
/* cmd_off: n+1 non-decreasing offsets with cmd_off[n] <= m. The output is never larger than
 * mpx_encode_log_bound(n, m); if rec_off[n] > out_cap the call fails with MPX_E_INVAL and only
 * rec_off is written.                                                                      */
int mpx_encode_log(mpx_engine* eng, int format, const mpx_log_rec* recs, size_t n,
                   const uint64_t* cmd_off, const uint8_t* op, const int64_t* key,
                   const int64_t* val, size_t m, uint8_t* out, size_t out_cap,
                   uint64_t* rec_off);
int mpx_encode_log_reserve(mpx_engine* eng, size_t max_n, size_t max_m);
/* d_out must hold mpx_encode_log_bound(n, m) bytes, of which only [0, rec_off[n]) are written;
 * cmd_off is trusted (not validated). Needs mpx_encode_log_reserve(n, m) first. Alignment:
 * d_recs 16 bytes; d_cmd_off, d_key, d_val, d_rec_off 8; d_op and d_out any address.         */
int mpx_encode_log_dev(mpx_engine* eng, int format, const mpx_log_rec* d_recs, size_t n,
                       const uint64_t* d_cmd_off, const uint8_t* d_op, const int64_t* d_key,
                       const int64_t* d_val, size_t m, uint8_t* d_out, uint64_t* d_rec_off,
                       void* stream);

/* ---- the proposer side: batched handlePropose and the Accept bytes --------------------------
 * The first two stations of Phase 2:
 *   handlePropose  bareminpaxos.go:617-710 (MIN) / paxos.go:388-443 (CLASSIC)
 *   bcastAccept    bareminpaxos.go:450-520 / paxos.go:299-331, through SendMsg
 *                  (genericsmr.go:499-512) and Accept.Marshal (minpaxosprotomarsh.go:425-468 /
 *                  paxosprotomarsh.go:214-242)
 * Instance numbers are window numbers as in mpx_accept_handle: idx = instance - inst_base belongs
 * to group g = idx / ipg, n_inst == n_groups * ipg, first_g = inst_base + g * ipg plays the
 * reference's instance 0 of group g and "nothing committed" is first_g - 1.                     */

/* per group: r.defaultBallot, r.Id, r.Leader (CLASSIC: IsLeader is leader == self_id),
 * prepareBookkeeping.prepareOKs (MIN), r.crtInstance (in/out), r.committedUpTo                  */
typedef struct mpx_proposer_group {
    int32_t default_ballot;
    int32_t self_id;
    int32_t leader;
    int32_t prepare_oks;
    int32_t crt_instance;
    int32_t committed_upto;
    uint32_t pad[2];
} mpx_proposer_group; /* 32 B */

/* one run of handlePropose: a batch of at most MPX_PROPOSE_MAX_BATCH proposals and what became
 * of it. first_cmd / n_cmds: the batch's range of the call's proposal (= command) arrays.       */
typedef struct mpx_accept_send {
    int32_t instance;       /* instNo (ACCEPT, PREPARE, REFUSED), else -1                       */
    int32_t ballot;         /* the installed ballot (REFUSED: defaultBallot)                    */
    int32_t last_committed; /* r.committedUpTo, bcastAccept's lastcommitted                     */
    uint32_t flags;         /* MPX_PH_*                                                         */
    uint64_t first_cmd;
    uint32_t n_cmds;
    uint32_t pad;
} mpx_accept_send; /* 32 B */

#define MPX_PROPOSE_MAX_BATCH 5000 /* MAX_BATCH, bareminpaxos.go:22 / paxos.go:20               */
#define MPX_PH_ACCEPT 1u     /* instance installed PREPARED at defaultBallot: bcastAccept (after
                                recordInstanceMetadata + recordCommands + sync)                 */
#define MPX_PH_NOT_LEADER 2u /* every proposal of the slot is answered FALSE                    */
#define MPX_PH_REFUSED 4u    /* MIN :671-685: the batch is consumed, its FIRST proposal is
                                answered FALSE, the others get no reply                         */
#define MPX_PH_PREPARE 8u    /* CLASSIC :421-428: installed PREPARING at makeUniqueBallot(0) =
                                self_id; the host does bcastPrepare                             */

/* Group g's drained proposals are [prop_off[g], prop_off[g+1]) of the call's proposal arrays, in
 * arrival order (only the counts enter this call). The handler runs once per MPX_PROPOSE_MAX_BATCH
 * of them, sequentially: slot send_off[g] + b describes proposals [prop_off[g] + 5000 b, ...) and
 * send_off[g+1] - send_off[g] = ceil(n_g / 5000). Every slot is written; there is no compaction.
 *   both     not leader (MIN: also prepare_oks <= N>>1): MPX_PH_NOT_LEADER on every slot of the
 *            group, nothing else changes
 *   MIN      crt_instance advances past non-nil slots, instNo = crt; committed_upto < instNo-1 ->
 *            MPX_PH_REFUSED (crt stays advanced); else crt++, st[instNo] = {PREPARED,
 *            default_ballot, value_id = (uint32) first_cmd, MPX_PF_HAS_PROPOSALS}, MPX_PH_ACCEPT
 *            with {instNo, default_ballot, committed_upto}
 *   CLASSIC  advance, instNo = crt, crt++ (no pipeline check); default_ballot == -1 ->
 *            {PREPARING, self_id, ...} and MPX_PH_PREPARE, else {PREPARED, default_ballot, ...}
 *            and MPX_PH_ACCEPT
 * lb (optional): installed instances get {status, 0, 0, 0}, so mpx_accept_tally can run on it.
 * crt_instance leaving the group's window [first_g, first_g + ipg) is the reference's
 * instanceSpace index panic: MPX_E_NIL_INSTANCE, outputs unspecified.
 * Host form: computes send_off (n_groups+1 entries, always written once the arguments are valid);
 * MPX_E_INVAL when prop_off decreases or send_off[n_groups] > sends_cap.                        */
int mpx_propose_handle(mpx_engine* eng, mpx_proposer_group* groups, size_t n_groups,
                       const uint64_t* prop_off, mpx_acceptor_state* st, mpx_inst_state* lb,
                       size_t n_inst, int32_t inst_base, uint32_t ipg, uint64_t* send_off,
                       mpx_accept_send* sends, size_t sends_cap);
/* device form: d_send_off is an input, trusted like d_prop_off. One kernel, a lane per group, no
 * scratch, no control words beyond the error word; it captures into a graph.                   */
int mpx_propose_handle_dev(mpx_engine* eng, mpx_proposer_group* d_groups, size_t n_groups,
                           const uint64_t* d_prop_off, const uint64_t* d_send_off,
                           mpx_acceptor_state* d_st, mpx_inst_state* d_lb, size_t n_inst,
                           int32_t inst_base, uint32_t ipg, mpx_accept_send* d_sends,
                           void* stream);

#define MPX_AB_THRIFTY 1u /* r.Thrifty: N>>1 destinations instead of N-1                         */

/* one call of mpx_encode_accepts. Slots of sends without MPX_PH_ACCEPT are skipped.
 * groups: self_id is LeaderId (the other fields are not read). peer_commits[n_groups * N]:
 * prepareBookkeeping.peerCommits per group (MIN). cmd_*: the new commands, SoA, indexed by a
 * send's first_cmd / n_cmds. The log, by window index (MIN): log_recs[n_inst] (ballot, status;
 * MPX_STATUS_NIL = nil; inst_no unused) with commands [log_cmd_off[i], log_cmd_off[i+1]) of
 * log_op / log_key / log_val. alive_mask: bit q = r.Alive[q] (CLASSIC).                        */
typedef struct mpx_accept_batch {
    const mpx_accept_send* sends;
    size_t n_sends;
    int32_t inst_base;
    uint32_t ipg;
    size_t n_groups;
    const mpx_proposer_group* groups;
    const int32_t* peer_commits;
    const uint8_t* cmd_op;
    const int64_t* cmd_key;
    const int64_t* cmd_val;
    size_t n_cmds;
    const mpx_log_rec* log_recs;
    const uint64_t* log_cmd_off;
    const uint8_t* log_op;
    const int64_t* log_key;
    const int64_t* log_val;
    size_t n_log_cmds;
    uint32_t flags;      /* MPX_AB_*                                                            */
    uint32_t alive_mask;
} mpx_accept_batch;

/* Destinations of a send, in ring order q = self_id+1, ... mod N up to self_id; n = N-1, or N>>1
 * with MPX_AB_THRIFTY. MIN: the first n successors, alive or not (the reference reconnects and
 * counts the peer, :476-482). CLASSIC: the first n successors whose alive bit is set (:323-327).
 * Frames, little endian, V = binary.PutVarint:
 *   MIN      [9][LeaderId][Instance][Ballot][LastCommitted][V(n)][n x 17 B][V(m)][m Instances]
 *            peer q's CatchUpLog: instances lo .. last_committed of the group's log, lo = first_g
 *            if peer_commits[q] < first_g, else peer_commits[q] + 1 (:496-506); empty when
 *            lo > last_committed. Instance = Ballot i32, Status i32, V(k), k x 17 B.
 *   CLASSIC  [9][LeaderId][Instance][Ballot][V(n)][n x 17 B]
 * out receives, destination by destination, each destination's frames in send-array order, back
 * to back; destination q's run is out[dest_off[q] .. dest_off[q+1]) (dest_off: N+1 entries,
 * always complete). Nothing is ever written at or past out_cap.
 * Errors: a nil instance inside a catch-up range (the reference dereferences nil) ->
 * MPX_E_NIL_INSTANCE. Host form: last_committed >= instance or < first_g - 1, a send outside the
 * window, a command or log range outside its arrays, self_id outside [0, N) -> MPX_E_INVAL;
 * dest_off[N] > out_cap -> MPX_E_INVAL with dest_off written.                                  */
int mpx_encode_accepts(mpx_engine* eng, const mpx_accept_batch* b, uint8_t* out, size_t out_cap,
                       uint64_t* dest_off);
/* scratch for _dev calls of up to max_sends slots over a window of up to max_n_inst instances
 * (max_log_cmds: reserved for forms that materialise the catch-up runs; the built one keeps only
 * offsets). Grows only. The scratch lives in the handle: like the other *_dev calls that keep
 * scratch there, encodes of one handle run in one stream order, and a larger reserve invalidates
 * graphs captured before it.                                                                    */
int mpx_encode_accepts_reserve(mpx_engine* eng, size_t max_sends, size_t max_n_inst,
                               size_t max_log_cmds);
/* b: a host struct of device pointers. The offsets and ranges are trusted; a send outside the
 * window (MPX_E_NIL_INSTANCE), a bad self_id (MPX_E_BAD_ID) or last_committed (MPX_E_INVAL) is
 * reported through the error word like the other _dev calls and emits no frame. Never allocates
 * or synchronises. Alignment: sends, groups, log_recs 16 bytes; offsets, keys, values 8;
 * cmd_op, log_op and d_out any address.                                                         */
int mpx_encode_accepts_dev(mpx_engine* eng, const mpx_accept_batch* b, uint8_t* d_out,
                           size_t out_cap, uint64_t* d_dest_off, void* stream);

/* ---- Accept / Commit / PrepareReply payloads: Unmarshal in a batch ---------------------------
 * The inverse of mpx_encode_accepts: from the mpx_var_frame ranges mpx_decode_stream[_dev] left
 * (the same buf, the same offsets) to the records and arrays the rest of the engine takes, by
 * mpx_config.mode:
 *                           MIN (minpaxosprotomarsh.go)   CLASSIC (paxosprotomarsh.go)
 *   Accept.Unmarshal        :470-507                      :244-268
 *   Commit.Unmarshal        :648-672                      :403-430
 *   PrepareReply.Unmarshal  :352-387                      :152-176
 *   Instance.Unmarshal      :126-153                      -
 *   Command.Unmarshal       statemarsh.go:21-39 (Op u8, K i64, V i64)
 * Header fields sit at offset + 1, little endian: MIN Accept LeaderId, Instance, Ballot,
 * LastCommitted; CLASSIC Accept and every Commit LeaderId, Instance, Ballot. A PrepareReply's fixed
 * fields are already in mpx_decode_stream's prepare records (their value_id is the frame's var
 * index); only its Command slice and, in MIN, its CatchUpLog are unmarshalled here (its
 * LastCommitted is the i32 at offset + 14).
 * Everything is in stream order, that is, var order:
 *   accepts / commits   one slot per frame of that code (compacted), value_id = the frame's index
 *                       in var; accept_last_committed slot-aligned with accepts
 *   cmd_off             n_var+1 entries, one per var frame of any code: the exclusive prefix sums of
 *                       var[i].n_cmds; frame i's Command slice is commands [cmd_off[i], cmd_off[i+1])
 *                       of op / key / val
 *   log_inst_off        n_var+1 entries, the prefix sums of var[i].n_log: frame i's CatchUpLog is
 *                       log records [log_inst_off[i], log_inst_off[i+1]). Commit frames and every
 *                       CLASSIC frame have n_log = 0
 *   log_recs, log_cmd_off, log_op / log_key / log_val
 *                       the log instances and their commands, log_cmd_off the prefix sums of the
 *                       instances' command counts: the layout mpx_encode_log and
 *                       mpx_accept_batch.log_* take, so the output of one is a legal input of the
 *                       other
 * inst_no of a log record is the sender's numbering: both senders build ranges that end at the
 * frame's LastCommitted (bcastAccept bareminpaxos.go:496-506, handlePrepare :743), so record j of a
 * frame with m log instances is instance LastCommitted - m + 1 + j. The receivers index the log by
 * position, j = record - log_inst_off[i] (bareminpaxos.go:937 and the commented-out :778).
 * The counts in *res are always complete; an element at or past its capacity is not written (as in
 * mpx_decode_stream), and a capacity of 0 may come with null pointers. With d_n_var the entries of
 * cmd_off / log_inst_off past the processed frames repeat the totals.                          */
typedef struct mpx_unmarshal_out {
    mpx_accept_msg* accepts;         /* code 9 frames, stream order; value_id = the frame's var index */
    int32_t* accept_last_committed;  /* slot-aligned with accepts (MIN; CLASSIC writes -1)            */
    size_t accept_cap;
    mpx_accept_msg* commits;         /* code 10 frames, same record (leader_id, instance, ballot)     */
    size_t commit_cap;
    uint64_t* cmd_off;               /* n_var+1: frame i's Command slice = [cmd_off[i], cmd_off[i+1]) */
    uint8_t* op; int64_t* key; int64_t* val; size_t cmd_cap;
    uint64_t* log_inst_off;          /* n_var+1: frame i's CatchUpLog = log records [..[i], ..[i+1])  */
    mpx_log_rec* log_recs;           /* ballot, status, inst_no, pad = 0                              */
    uint64_t* log_cmd_off;           /* log_inst_cap+1                                                */
    size_t log_inst_cap;
    uint8_t* log_op; int64_t* log_key; int64_t* log_val; size_t log_cmd_cap;
} mpx_unmarshal_out;

typedef struct mpx_unmarshal_result {
    uint64_t n_accepts, n_commits, n_cmds, n_log_inst, n_log_cmds;  /* always complete */
    uint64_t n_var;                                                 /* frames processed */
} mpx_unmarshal_result; /* 48 B */

/* host pointers, synchronous; stages like the other host forms. The frames are validated before
 * anything is launched; MPX_E_INVAL for a frame outside [0, len), cmds_off + 17 * n_cmds or log_off
 * outside the frame (or a header that does not fit before cmds_off, or n_log != 0 on a frame
 * without a log), a code other than 9, 10 or 12, and frames that overlap or are not ascending by
 * offset. A CatchUpLog whose walk does not end exactly at the frame's end: MPX_E_INVAL.          */
int mpx_unmarshal_frames(mpx_engine* eng, const uint8_t* buf, size_t len, const mpx_var_frame* var,
                         size_t n_var, const mpx_unmarshal_out* out, mpx_unmarshal_result* res);
/* scratch for _dev calls of up to max_var frames that carry up to max_log_inst catch-up instances
 * in total (grows only). The scratch lives in the handle: like the other *_dev calls that keep
 * scratch there, unmarshals of one handle run in one stream order, and a larger reserve
 * invalidates graphs captured before it.                                                        */
int mpx_unmarshal_frames_reserve(mpx_engine* eng, size_t max_var, size_t max_log_inst);
/* device form: `out` is a host struct of device pointers. The frames are trusted (they come from
 * mpx_decode_stream_dev). d_n_var (optional, device): min(*d_n_var, n_var) frames are processed, so
 * the call can be captured right behind mpx_decode_stream_dev with n_var = var_cap and
 * d_n_var = &d_stream_res->n_var. A catch-up walk that does not end exactly at its frame's end, or
 * more catch-up instances than the reserve was told, is reported through the handle's error word
 * (MPX_E_INVAL at the next synchronising call); that frame's log records are unspecified. Never
 * allocates or synchronises; needs mpx_unmarshal_frames_reserve first. d_buf may be read up to len
 * rounded up to 16, never at or past it. Alignment: d_buf 16 bytes, as for the decoders (any other
 * address is rejected with MPX_E_INVAL); d_var, accepts, commits, log_recs 16; offsets, keys,
 * values, d_n_var, d_res 8; accept_last_committed 4; op and log_op any address.                  */
int mpx_unmarshal_frames_dev(mpx_engine* eng, const uint8_t* d_buf, size_t len,
                             const mpx_var_frame* d_var, size_t n_var, const uint64_t* d_n_var,
                             const mpx_unmarshal_out* out, mpx_unmarshal_result* d_res, void* stream);

/* ---- the commit side: batched handleCommit[Short] and the Commit bytes -----------------------
 * The last station of Phase 2. A leader that decided an instance calls bcastCommit
 * (bareminpaxos.go:565-615 / paxos.go:336-386); every follower runs
 *   handleCommit       bareminpaxos.go:856-883 / paxos.go:522-549
 *   handleCommitShort  bareminpaxos.go:885-910 / paxos.go:551-575
 * per message and advances committedUpTo (updateCommittedUpTo, paxos.go:259-264). The two
 * protocols' handlers are the same code and their wire formats are identical, so nothing here
 * depends on mpx_config.mode. Instance numbers are window numbers as in mpx_accept_handle:
 * idx = instance - inst_base belongs to group g = idx / ipg, n_inst == n_groups * ipg,
 * first_g = inst_base + g * ipg and "nothing committed" is first_g - 1.                        */

#define MPX_VALUE_KEEP 0xFFFFFFFFu /* value_id of a CommitShort record: the message carries no
                                      Command; on a nil instance it is the handle of Cmds == nil */

#define MPX_CH_INSTALLED 1u /* the instance was nil: a fresh Instance{ballot, COMMITTED} was made  */
#define MPX_CH_CMDS 2u      /* a Commit: the host stores Command (and recordCommands)              */
#define MPX_CH_REQUEUE 4u   /* clientProposals were pushed back on ProposeChan (:871-876 / :537-542) */

/* msgs[n]: the record mpx_unmarshal_frames writes for Commits and mpx_gather_commit_shorts for
 * CommitShorts, under the contract above (grouped by instance, ascending; slot order = arrival
 * order). A CommitShort carries value_id == MPX_VALUE_KEEP, a Commit any other handle. leader_id
 * is not read. st[n_inst] is updated in place; committed_upto[n_groups] (r.committedUpTo per
 * group) is in/out. Outputs are slot-aligned with msgs, one entry per message, always written:
 * effect[i] (MPX_CH_*) and, when log_recs is given, log_recs[i] = {ballot = msgs[i].ballot,
 * status = COMMITTED, inst_no = msgs[i].instance, pad 0}: the record mpx_encode_log(
 * MPX_LOG_DURABLE) takes for recordInstanceMetadata.
 * Per message, sequentially in array order (no ballot is compared: a lower-ballot Commit
 * overwrites, as in the Go):
 *   instance  message      state after                                 effect
 *   nil       Commit       {COMMITTED, ballot, value_id, 0}            INSTALLED | CMDS
 *   nil       CommitShort  {COMMITTED, ballot, MPX_VALUE_KEEP, 0}      INSTALLED
 *   non-nil   Commit       status COMMITTED, ballot, value_id taken    CMDS (| REQUEUE)
 *   non-nil   CommitShort  status COMMITTED, ballot; value_id kept     0 (| REQUEUE)
 * REQUEUE when flags has MPX_PF_HAS_PROPOSALS: that bit is cleared and MPX_PF_REQUEUED set (the
 * acceptor's convention; the caller clears MPX_PF_REQUEUED once it has pushed the proposals back).
 * committed_upto[g], for every group that has at least one message in the batch and only for
 * those (the reference advances inside a handler): c rises while c + 1 < first_g + ipg and
 * st[c + 1].status == COMMITTED, over the states the batch leaves. Inside a commit-only batch
 * statuses only move to COMMITTED, so this equals calling updateCommittedUpTo after every
 * message. The advance stops at the window's end, where the reference would index the next
 * slot of instanceSpace.
 * Errors: an instance outside the window -> MPX_E_NIL_INSTANCE; order -> MPX_E_INVAL; a
 * committed_upto[g] outside [first_g - 1, first_g + ipg - 1] -> MPX_E_INVAL (the host form checks
 * every group before anything runs; the _dev form reports it through the error word for the
 * groups the batch touches).                                                                    */
int mpx_commit_handle(mpx_engine* eng, const mpx_accept_msg* msgs, size_t n,
                      mpx_acceptor_state* st, size_t n_inst, int32_t inst_base,
                      int32_t* committed_upto, size_t n_groups, uint32_t ipg, uint8_t* effect,
                      mpx_log_rec* log_recs);
/* device form: d_st is in place (no in / out pair: the prefix reads the final states of instances
 * that had no message); d_st[i] is stored only for instances that have messages. Two kernels on
 * the stream, no scratch, no control words beyond the error word; it captures into a graph.
 * Alignment: d_msgs, d_st, d_log_recs 16 bytes; d_committed_upto 4; d_effect any address.        */
int mpx_commit_handle_dev(mpx_engine* eng, const mpx_accept_msg* d_msgs, size_t n,
                          mpx_acceptor_state* d_st, size_t n_inst, int32_t inst_base,
                          int32_t* d_committed_upto, size_t n_groups, uint32_t ipg,
                          uint8_t* d_effect, mpx_log_rec* d_log_recs, void* stream);

/* one decided instance whose Commit goes out: the leader fills the array from the tally's decided
 * mask (mpx_build_replies does it on the device), with MPX_CS_SEND on the decided slots (the
 * others are skipped: no compaction needed)                                                     */
typedef struct mpx_commit_send {
    int32_t instance;
    int32_t ballot;
    uint64_t first_cmd; /* the instance's commands: [first_cmd, first_cmd + n_cmds) of cmd_*      */
    uint32_t n_cmds;
    uint32_t flags;     /* MPX_CS_*                                                               */
    uint32_t pad[2];
} mpx_commit_send; /* 32 B */
#define MPX_CS_SEND 1u

/* one call of mpx_encode_commits. groups: only self_id (LeaderId) is read. cmd_*: SoA, indexed by a
 * send's first_cmd / n_cmds. flags: MPX_AB_THRIFTY. alive_mask: bit q = r.Alive[q].              */
typedef struct mpx_commit_batch {
    const mpx_commit_send* sends;
    size_t n_sends;
    int32_t inst_base;
    uint32_t ipg;
    size_t n_groups;
    const mpx_proposer_group* groups;
    const uint8_t* cmd_op;
    const int64_t* cmd_key;
    const int64_t* cmd_val;
    size_t n_cmds;
    uint32_t flags;
    uint32_t alive_mask;
} mpx_commit_batch;

/* Destinations of a send, as bcastCommit's two loops walk the ring q = self_id + 1, ... mod N:
 * the first n alive successors (n = N-1, or N>>1 with MPX_AB_THRIFTY) get a CommitShort; with
 * MPX_AB_THRIFTY, when that loop did not wrap (q != self_id), the following alive successors get a
 * full Commit until N-1 have been sent or the ring returns to self_id. N = 1 sends nothing.
 * Frames, little endian, V = binary.PutVarint:
 *   CommitShort 17 B  [11][LeaderId][Instance][Count = n_cmds][Ballot]
 *                     (minpaxosprotomarsh.go:710-735 / paxosprotomarsh.go:465-490)
 *   Commit            [10][LeaderId][Instance][Ballot][V(n)][n x 17 B]
 *                     (minpaxosprotomarsh.go:618-646 / paxosprotomarsh.go:373-401)
 * out receives, destination by destination, each destination's frames in send-array order, back
 * to back; destination q's run is out[dest_off[q] .. dest_off[q+1]) (dest_off: N+1 entries, always
 * complete). Nothing is ever written at or past out_cap.
 * Errors, host form: a send outside the window, a command range outside its arrays, self_id
 * outside [0, N) -> MPX_E_INVAL; dest_off[N] > out_cap -> MPX_E_INVAL with dest_off written.    */
#define MPX_COMMIT_SHORT_FRAME 17
int mpx_encode_commits(mpx_engine* eng, const mpx_commit_batch* b, uint8_t* out, size_t out_cap,
                       uint64_t* dest_off);
/* scratch of the family's _dev calls: mpx_encode_commits_dev of up to max_sends slots and
 * mpx_gather_commit_shorts_dev of up to max_other frames (grows only). The scratch lives in the
 * handle: like the other *_dev calls that keep scratch there, the family's calls on one handle run
 * in one stream order, and a larger reserve invalidates graphs captured before it.              */
int mpx_encode_commits_reserve(mpx_engine* eng, size_t max_sends, size_t max_other);
/* b: a host struct of device pointers. The same errors are reported through the error word
 * (MPX_E_INVAL at the next synchronising call) and such a send emits no frame. Never allocates or
 * synchronises. Alignment: sends, groups 16 bytes; keys, values, d_dest_off 8; cmd_op and d_out
 * any address.                                                                                  */
int mpx_encode_commits_dev(mpx_engine* eng, const mpx_commit_batch* b, uint8_t* d_out,
                           size_t out_cap, uint64_t* d_dest_off, void* stream);

/* CommitShort bodies to records: from the mpx_peer_frame list mpx_decode_stream[_dev] left (the
 * same buf, the same offsets), the frames of code MPX_PEER_COMMIT_SHORT, compacted and in stream
 * order: msgs[i] = {instance, ballot, leader_id, value_id = MPX_VALUE_KEEP}, count[i] = the Count
 * field, frame_index[i] = the frame's index in other (so the caller can merge with the
 * unmarshalled Commits by stream offset). Frames of other codes are skipped. *n_shorts is always
 * complete; nothing is written at or past cap (a capacity of 0 may come with null arrays).
 * Host form: a CommitShort frame outside [0, len) -> MPX_E_INVAL.                               */
int mpx_gather_commit_shorts(mpx_engine* eng, const uint8_t* buf, size_t len,
                             const mpx_peer_frame* other, size_t n_other, mpx_accept_msg* msgs,
                             int32_t* count, uint32_t* frame_index, size_t cap, uint64_t* n_shorts);
/* device form: needs mpx_encode_commits_reserve(.., n_other) first. d_n_other (optional, device):
 * min(*d_n_other, n_other) frames are processed, so the call can be captured right behind
 * mpx_decode_stream_dev with n_other = other_cap and d_n_other = &d_stream_res->n_other. A frame
 * outside [0, len) is reported through the error word and skipped. d_buf may be read up to len
 * rounded up to 16, never at or past it. Alignment: d_buf 16 bytes, as for the decoders (any other
 * address is rejected with MPX_E_INVAL); d_msgs 16; d_n_other, d_n_shorts 8; d_other, d_count,
 * d_frame_index 4.                                                                              */
int mpx_gather_commit_shorts_dev(mpx_engine* eng, const uint8_t* d_buf, size_t len,
                                 const mpx_peer_frame* d_other, size_t n_other,
                                 const uint64_t* d_n_other, mpx_accept_msg* d_msgs,
                                 int32_t* d_count, uint32_t* d_frame_index, size_t cap,
                                 uint64_t* d_n_shorts, void* stream);

/* ---- batch assembly: several connections' records as one legal handler batch ----------------
 * Every handler above takes records grouped by instance, the groups ascending, slot order =
 * arrival order (Contract). mpx_order_records produces that order from up to MPX_ORDER_MAX_SRC
 * record arrays (one per connection, or the Commit and CommitShort lists of one stream): what the
 * Go shim's sort.SliceStable by Instance over the arrival-ordered concatenation produces.
 * Output order, ascending by these keys in turn: instance; arrival (when the call gives arrival
 * keys); source index; index within the source.
 *   out[n]   the records, 16 bytes each, bit-identical to the inputs (padding bytes included)
 *   perm[n]  optional: for output slot i, the record's index in the concatenation of the sources
 *            (the shim maps payloads and per-slot effects back with it)
 *   *res     the result record below
 * n_inst / inst_base: the window, as the handlers take it (1 <= n_inst <= 2^32; every instance of
 * the window must be an int32). arrival_bits (0..32): the significant low bits of the arrival
 * keys; 0 exactly when no source gives arrival keys.
 * flags: MPX_ORDER_GENERAL takes the multi-launch radix path also for calls of at most
 * MPX_ORDER_ONE_LAUNCH_MAX records, which otherwise run as one kernel in one workgroup; the results
 * are the same (for tests and measurements).
 * Errors: a record outside the window -> MPX_E_NIL_INSTANCE (the code the handlers answer for
 * it), outputs unspecified; n_src > MPX_ORDER_MAX_SRC, n_inst outside its range, unknown flags,
 * arrival keys given for some sources with records and not for others, arrival_bits > 32,
 * arrival_bits set without keys or keys without arrival_bits, an arrival key with bits at or above
 * arrival_bits (host form only) -> MPX_E_INVAL; 2^32-1 records or more in total ->
 * MPX_E_UNSUPPORTED.                                                                              */
#define MPX_ORDER_MAX_SRC 16
#define MPX_ORDER_ONE_LAUNCH_MAX 4096
#define MPX_ORDER_GENERAL 1u   /* call flag                                                      */
#define MPX_ORD_WAS_ORDERED 1u /* result flag: the concatenated input was already in output order
                                  (perm is the identity); without arrival keys that is: it already
                                  met the handlers' contract                                     */
typedef struct mpx_order_src {      /* one connection's / one list's records, in arrival order   */
    const void* recs;               /* 16-byte records whose first field is int32 instance:
                                       mpx_accept_reply or mpx_accept_msg                        */
    const uint32_t* arrival;        /* optional per-record arrival key (e.g. the frame's stream
                                       offset); given for every source of a call or for none     */
    size_t n;
} mpx_order_src;

typedef struct mpx_order_result {
    uint64_t n;        /* records written                                                        */
    uint64_t n_runs;   /* distinct instances (= groups the handlers will see)                    */
    int32_t lo, hi;    /* smallest / largest instance; lo = 0, hi = -1 when n == 0               */
    uint32_t flags;    /* MPX_ORD_WAS_ORDERED                                                    */
    uint32_t pad;
} mpx_order_result;    /* 32 B */

int mpx_order_records(mpx_engine* eng, const mpx_order_src* src, size_t n_src, size_t n_inst,
                      int32_t inst_base, uint32_t arrival_bits, uint32_t flags, void* out,
                      uint32_t* perm, mpx_order_result* res);
/* scratch of mpx_order_records_dev calls of up to max_n records in total over windows of up to
 * max_n_inst instances with any arrival_bits (grows only). The scratch and the family's control
 * words live in the handle: the family's calls on one handle run in one stream order, and a
 * larger reserve invalidates graphs captured before it.                                         */
int mpx_order_records_reserve(mpx_engine* eng, size_t max_n, size_t max_n_inst);
/* device form: src is a HOST array whose recs / arrival are device pointers (the n are host
 * values); d_out must not overlap an input. Needs mpx_order_records_reserve first (a call of no
 * record does not). Never allocates or synchronises; it captures into a graph. An out-of-window
 * record is reported through the error word (MPX_E_NIL_INSTANCE at the next synchronising call);
 * arrival keys are masked to arrival_bits. Alignment: recs and d_out 16 bytes; d_perm, arrival 4;
 * d_res 8; any other address is rejected with MPX_E_INVAL.                                      */
int mpx_order_records_dev(mpx_engine* eng, const mpx_order_src* src, size_t n_src, size_t n_inst,
                          int32_t inst_base, uint32_t arrival_bits, uint32_t flags, void* d_out,
                          uint32_t* d_perm, mpx_order_result* d_res, void* stream);

/* ---- client bytes in: batched Propose decode over many connections ---------------------------
 * genericsmr.(*Replica).clientListener (genericsmr.go:448-490) reads one client connection as
 * little-endian frames [code u8][body], after WaitForConnections consumed the connection-type byte
 * (genericsmr.go:341-374; that byte is the caller's, never part of a connection here):
 *   0 PROPOSE            30 B  CommandId i32, Op u8, K i64, V i64, Timestamp i64
 *                              (gsmrprotomarsh.go:41-80, statemarsh.go:8-39) -> one proposal
 *   2 READ               13 B  CommandId i32, Key i64 (:327-350): unmarshalled and dropped (:475)
 *   4 PROPOSE_AND_READ   30 B  CommandId i32, Command 17 B, Key i64 (:267-292): dropped (:483)
 *   any other byte        1 B  the switch has no default: the next byte is read as a code
 * mpx_decode_client_streams frames many connections' unread bytes at once. A connection's bytes
 * are buf[offset, offset + length); a frame whose body runs past them is a partial read
 * (MPX_DECODE_PARTIAL): the caller keeps [consumed, length), as with the peer decoders. The
 * reference ignores the error of Command.Unmarshal inside Propose.Unmarshal (:73), so a stream
 * that ends inside a Propose's command can desynchronise it at EOF; the engine does not reproduce
 * that: such a Propose is a partial read like any other.
 * Outputs: the proposals connection by connection in conns order and in stream order inside a
 * connection (one of the interleavings Go's goroutines may give, and a deterministic one).
 * Proposal i is op[i], key[i], val[i] (the SoA layout of mpx_apply and mpx_accept_batch.cmd_*; the
 * Op byte passes through whatever its value) and meta[i]; a proposal at or past prop_cap is not
 * written (a capacity of 0 may come with null arrays), all counts are complete regardless.
 * conn_res[k] is written for every connection. A stop in connection k has no effect on connection
 * k + 1; bytes of buf outside every connection are never interpreted.
 * conns: ascending by offset, non-overlapping, every offset a multiple of MPX_CLIENT_ALIGN, every
 * connection inside [0, len] (a connection of length 0 is legal anywhere in the array); group
 * non-decreasing and < n_groups, so connection order is already grouped by group.
 *   prop_off[g]  (optional, n_groups + 1) the index of the first proposal of the first connection
 *                with group >= g; prop_off[n_groups] the total
 *   send_off[g]  (optional, n_groups + 1) exclusive prefix sums of ceil(n_g / MPX_PROPOSE_MAX_BATCH):
 *                with prop_off the two trusted inputs of mpx_propose_handle_dev;
 *                res->n_sends = send_off[n_groups] <= n_groups + len / 30 / 5000, the bound a
 *                caller sizes `sends` with
 * Limits: len <= MPX_DECODE_MAX_BYTES, n_conns <= MPX_CLIENT_MAX_CONNS, n_groups <=
 * MPX_CLIENT_MAX_GROUPS, else MPX_E_UNSUPPORTED.
 * Errors, host form, answered before anything is staged: null arguments; an offset not a multiple
 * of MPX_CLIENT_ALIGN; a connection outside [0, len], overlapping or out of order; a group that
 * decreases or is >= n_groups; prop_off or send_off given with n_groups == 0 -> MPX_E_INVAL.     */
#define MPX_CLIENT_PROPOSE 0
#define MPX_CLIENT_READ 2
#define MPX_CLIENT_PROPOSE_AND_READ 4
#define MPX_CLIENT_PROPOSE_FRAME 30
#define MPX_CLIENT_READ_FRAME 13
#define MPX_CLIENT_ALIGN 128          /* a connection's bytes start on a multiple of this        */
#define MPX_CLIENT_MAX_CONNS (1u << 20)
#define MPX_CLIENT_MAX_GROUPS (1u << 20)

typedef struct mpx_client_conn {      /* one connection's unread bytes                           */
    uint64_t offset;                  /* into buf, multiple of MPX_CLIENT_ALIGN                  */
    uint32_t length;
    uint32_t group;                   /* the group (Replica) it belongs to       */
} mpx_client_conn;                    /* 16 B */

typedef struct mpx_proposal {         /* bytes 8..23 of mpx_reply_rec, same field order          */
    int64_t timestamp;
    int32_t command_id;
    uint32_t client;                  /* index in conns                                          */
} mpx_proposal;                       /* 16 B */

typedef struct mpx_client_conn_result {
    uint64_t first;                   /* index of the connection's first proposal in the outputs */
    uint32_t consumed;                /* bytes framed; the caller keeps [consumed, length)       */
    uint32_t n_proposals;
    uint32_t n_dropped;               /* READ, PROPOSE_AND_READ and 1-byte frames in [0, consumed) */
    int32_t stop_reason;              /* MPX_DECODE_END / MPX_DECODE_PARTIAL                     */
    int32_t stop_code;                /* code byte at consumed, -1 at MPX_DECODE_END             */
    uint32_t pad;
} mpx_client_conn_result;             /* 32 B */

typedef struct mpx_client_result {
    uint64_t n_proposals, n_dropped;  /* over all connections                                    */
    uint64_t n_partial;               /* connections that stopped MPX_DECODE_PARTIAL             */
    uint64_t n_sends;                 /* send_off[n_groups] (computed with or without send_off)  */
} mpx_client_result;                  /* 32 B */

typedef struct mpx_client_out {
    uint8_t* op;
    int64_t* key;
    int64_t* val;
    mpx_proposal* meta;
    size_t prop_cap;
    uint64_t* prop_off;               /* optional, n_groups + 1                                  */
    uint64_t* send_off;               /* optional, n_groups + 1                                  */
} mpx_client_out;

int mpx_decode_client_streams(mpx_engine* eng, const uint8_t* buf, size_t len,
                              const mpx_client_conn* conns, size_t n_conns, size_t n_groups,
                              const mpx_client_out* out, mpx_client_conn_result* conn_res,
                              mpx_client_result* res);
/* scratch of mpx_decode_client_streams_dev calls on buffers of up to max_len bytes with up to
 * max_conns connections and max_groups groups (grows only). The scratch and the family's control
 * words live in the handle: the family's calls on one handle run in one stream order, and a
 * larger reserve invalidates graphs captured before it.                                         */
int mpx_decode_client_streams_reserve(mpx_engine* eng, size_t max_len, size_t max_conns,
                                      size_t max_groups);
/* device form: d_conns is a DEVICE array (a replayed graph sees new lengths every replay); out is a
 * host struct of device pointers. Needs mpx_decode_client_streams_reserve first (a call with
 * n_conns == 0 does not). Never allocates or synchronises; it captures into a graph. A connection
 * with a misaligned offset, outside [0, len], with a group >= n_groups, or starting before the end
 * / below the group of an earlier connection that passed the first three checks, is reported
 * through the error word (MPX_E_INVAL at the next synchronising call) and frames nothing:
 * consumed 0, counts 0, MPX_DECODE_END; the other connections are framed as if it were empty.
 * Alignment: d_buf 16 bytes (it is loaded as 16-byte vectors and may be read up to len rounded up
 * to 16, never at or past it); d_conns, out->meta, d_conn_res 16; offsets, keys, values, d_res 8;
 * out->op any address; any other address is rejected with MPX_E_INVAL.                          */
int mpx_decode_client_streams_dev(mpx_engine* eng, const uint8_t* d_buf, size_t len,
                                  const mpx_client_conn* d_conns, size_t n_conns, size_t n_groups,
                                  const mpx_client_out* out, mpx_client_conn_result* d_conn_res,
                                  mpx_client_result* d_res, void* stream);

/* ---- reply assembly: the client reply records from the sends, the masks, ret and meta ---------
 * The three loops in which the reference answers its clients, as one expansion over data the
 * other calls leave on the device (the mpx_accept_send slots of mpx_propose_handle, the tally's
 * decided bytes, mpx_apply's ret, mpx_decode_client_streams' meta); what comes out is what
 * mpx_encode_replies takes:
 *   MPX_RB_FALSE     handlePropose's refusals         bareminpaxos.go:622-623, :682-683,
 *                                                     paxos.go:390-391
 *   MPX_RB_DECIDED   handleAcceptReply with !Dreply   bareminpaxos.go:1030-1042, paxos.go:644-655
 *   MPX_RB_EXECUTED  executeCommands with Dreply      bareminpaxos.go:1076-1084, paxos.go:685-693
 * Output order: send-array order, and inside a slot j = first_cmd .. first_cmd + n_cmds - 1. For
 * sends as mpx_propose_handle writes them that is group by group with ascending instance, the
 * order in which the reference's handlers and executeCommands reach them; the stable per-client
 * fan-out of mpx_encode_replies keeps it.
 *   MPX_RB_FALSE     a MPX_PH_NOT_LEADER slot emits one record per proposal, a MPX_PH_REFUSED slot
 *                    one record, for its first proposal only: {value 0, timestamp 0, command_id -1,
 *                    client = meta[j].client} (the Go writes ProposeReplyTS{FALSE, -1, state.NIL,
 *                    0, ...}, not the proposal's own id and timestamp). mask, ret, ret_first and
 *                    commit_sends must be null.
 *   MPX_RB_DECIDED   eligible slots carry MPX_PH_ACCEPT or MPX_PH_PREPARE (an installed instance
 *                    with client proposals; the caller passes no slot whose instance has
 *                    ClientProposals == nil). A slot is selected when mask is null or
 *                    mask[instance - inst_base] != 0; every proposal of a selected slot emits
 *                    {0 (state.NIL), meta[j].timestamp, meta[j].command_id, meta[j].client}.
 *                    ret and ret_first must be null.
 *   MPX_RB_EXECUTED  the same selection; value = ret[(ret_first ? ret_first[s] : first_cmd) +
 *                    (j - first_cmd)]. ret is required.
 *   commit_sends     (optional; DECIDED and EXECUTED) every one of the n_sends entries is written,
 *                    slot-aligned: {instance, ballot, first_cmd, n_cmds, flags = MPX_CS_SEND iff the
 *                    slot is selected, pad 0}: CLASSIC's bcastCommit list, as mpx_encode_commits
 *                    takes it. recs may then be null with cap == 0.
 *   counts           res->n_replies and res->n_slots (the selected slots; MPX_RB_FALSE: the
 *                    answering ones) are always complete; a record at or past cap is not written.
 *                    With pad_client != MPX_RB_NO_PAD every slot of recs in [min(n_replies, cap),
 *                    cap) is written {0, 0, 0, pad_client}: a captured chain encodes n = cap records
 *                    with n_clients + 1 clients and pad_client = n_clients, and ignores the last
 *                    run (mpx_encode_replies_dev takes a host n).
 * flags: MPX_RB_GENERAL takes the multi-launch path also for calls of at most
 * MPX_RB_ONE_LAUNCH_SLOTS slots and a cap of at most MPX_RB_ONE_LAUNCH_REPLIES records, which
 * otherwise run as one kernel in one workgroup; the results are the same (for tests and
 * measurements).
 * Errors, host form, answered before anything is staged: null arguments, an unknown kind or flags,
 * the kind's forbidden or missing arrays, reserved != 0, an eligible slot whose command range
 * leaves [0, n_props), a selected slot whose result range leaves [0, n_ret) (a slot the mask passes
 * over reads no result: mpx_execute_gather's ret_first puts an instance that did not execute where
 * the executed ones before it end, which may be n_ret itself) -> MPX_E_INVAL; with mask given, an
 * eligible slot whose instance is outside the window -> MPX_E_NIL_INSTANCE; n_sends or the total
 * at or above 2^32-1 -> MPX_E_UNSUPPORTED.                                                        */
#define MPX_RB_FALSE 1u
#define MPX_RB_DECIDED 2u
#define MPX_RB_EXECUTED 3u
#define MPX_RB_GENERAL 1u          /* call flag                                                  */
#define MPX_RB_NO_PAD 0xFFFFFFFFu
#define MPX_RB_ONE_LAUNCH_SLOTS 1024
#define MPX_RB_ONE_LAUNCH_REPLIES 8192

typedef struct mpx_reply_batch {
    const mpx_accept_send* sends;  /* as mpx_propose_handle wrote them (or kept from earlier turns
                                      / built by hand)                                           */
    size_t n_sends;
    int32_t inst_base;             /* the window mask is indexed by                              */
    size_t n_inst;
    const mpx_proposal* meta;      /* of the proposal arrays first_cmd indexes                   */
    size_t n_props;
    const uint8_t* mask;           /* optional, n_inst bytes by window index (the tally's decided
                                      bytes, or an "executed" mask); NULL = every eligible slot  */
    const int64_t* ret;            /* MPX_RB_EXECUTED: Execute's results                         */
    size_t n_ret;
    const uint64_t* ret_first;     /* optional, n_sends: where slot s's results start in ret (an
                                      apply over gathered commands); NULL = first_cmd            */
    uint32_t kind;                 /* MPX_RB_*                                                   */
    uint32_t flags;                /* MPX_RB_GENERAL                                             */
    uint32_t pad_client;           /* MPX_RB_NO_PAD, or the client index the tail is padded with */
    uint32_t reserved;             /* 0                                                          */
} mpx_reply_batch;

typedef struct mpx_reply_result {
    uint64_t n_replies, n_slots;
} mpx_reply_result;                /* 16 B */

int mpx_build_replies(mpx_engine* eng, const mpx_reply_batch* b, mpx_reply_rec* recs, size_t cap,
                      mpx_commit_send* commit_sends, mpx_reply_result* res);
/* scratch of mpx_build_replies_dev calls of up to max_sends slots (grows only). The scratch lives
 * in the handle: the family's calls on one handle run in one stream order, and a larger reserve
 * invalidates graphs captured before it.                                                        */
int mpx_build_replies_reserve(mpx_engine* eng, size_t max_sends);
/* device form: b is a host struct of device pointers. Needs mpx_build_replies_reserve first (a
 * call with n_sends == 0 does not). Never allocates or synchronises; it captures into a graph. The
 * per-slot conditions above are reported through the error word (the code arrives at the next
 * synchronising call): such a slot emits nothing and its commit_sends flags are 0. Alignment:
 * sends, meta, d_commit_sends 16 bytes; d_recs, ret, ret_first, d_res 8; mask any address; any
 * other address is rejected with MPX_E_INVAL.                                                   */
int mpx_build_replies_dev(mpx_engine* eng, const mpx_reply_batch* b, mpx_reply_rec* d_recs,
                          size_t cap, mpx_commit_send* d_commit_sends, mpx_reply_result* d_res,
                          void* stream);

/* ---- execute assembly: executeCommands' walk and the gather of its commands --------------------
 * executeCommands (bareminpaxos.go:1066-1098 / paxos.go:675-706, the same code) walks every
 * group's instances from the last executed one up to committedUpTo, stops at the first whose
 * Cmds is nil and runs Execute on the others' commands in order. This call does the walk and
 * gathers those commands, flat and in Execute's call order, for mpx_apply[_dev]; it leaves the
 * "executed" mask and the ret_first array mpx_build_replies(MPX_RB_EXECUTED) takes. Instance
 * numbers are window numbers as in mpx_commit_handle: idx = instance - inst_base belongs to group
 * g = idx / ipg, n_inst == n_groups * ipg, first_g = inst_base + g * ipg, "none" is first_g - 1.
 * Per group g, sequentially:
 *     i = executed_in[g] + 1
 *     while i <= committed_upto[g] and inst[i - inst_base].flags & MPX_IC_HAS_CMDS:
 *         the instance executes: its commands src[first_cmd .. first_cmd + n_cmds) are appended
 *         i++
 *     executed_out[g] = i - 1
 * executed_in[g] >= committed_upto[g] is legal and does nothing (MIN assigns committedUpTo =
 * areply.Instance: it can move down). A nil instance at or below committedUpTo, where the Go
 * dereferences nil, stops the walk like Cmds == nil (flags == 0 stands for both; the group step's
 * has_cmds has the same convention). n_cmds == 0 with MPX_IC_HAS_CMDS is an empty non-nil slice: it
 * executes nothing and the walk goes on.
 * Output order: group by group, ascending instance, inside an instance first_cmd .. first_cmd +
 * n_cmds - 1.
 *   mask[n_inst]             required; every byte written, 1 exactly for the instances executed
 *                            in this call
 *   inst_first[n_inst]       optional; the exclusive sum of the executed instances' n_cmds before
 *                            window slot idx, written for every slot
 *   ret_first[n_sends]       optional, needs sends; inst_first[sends[s].instance - inst_base] for a
 *                            send whose instance is in the window, else 0: mpx_reply_batch.ret_first
 *   grp_cmd_off[n_groups+1]  optional; the offset of group g's first gathered command, entry
 *                            n_groups the total
 *   counts                   res is always complete, also past cap; a command at or past cap is
 *                            not written (executed_in / executed_out are separate so that a short
 *                            call can be repeated with a larger cap)
 *   MPX_XG_PAD               every position j in [min(n_cmds, cap), cap) is written {op 0
 *                            (state.NONE), key j, val 0}: Execute of NONE returns NIL and touches
 *                            nothing (state.go:85-102), so a captured chain calls mpx_apply_dev(m =
 *                            cap) and ignores the tail of ret; the key is j so that the pad does not
 *                            pile onto one key's list in the apply kernels
 *   MPX_XG_GENERAL           takes the multi-launch path also for calls of at most
 *                            MPX_XG_ONE_LAUNCH_INST slots and a cap of at most
 *                            MPX_XG_ONE_LAUNCH_CMDS, which otherwise run as one kernel in one
 *                            workgroup; the results are the same (for tests and measurements)
 * Errors, host form, answered before anything is staged: null required arrays, n_inst != n_groups *
 * ipg (or ipg == 0 with groups), unknown flags, reserved != 0, ret_first without sends ->
 * MPX_E_INVAL; committed_upto[g] or executed_in[g] outside [first_g - 1, first_g + ipg - 1] ->
 * MPX_E_INVAL; an instance that executes whose [first_cmd, first_cmd + n_cmds) leaves [0, n_src) ->
 * MPX_E_INVAL; n_inst or the gathered total at or above 2^32-1 -> MPX_E_UNSUPPORTED.            */
#define MPX_IC_HAS_CMDS 1u         /* mpx_inst_cmds.flags: Cmds != nil                            */
#define MPX_XG_PAD 1u              /* call flags                                                 */
#define MPX_XG_GENERAL 2u
#define MPX_XG_ONE_LAUNCH_INST 1024
#define MPX_XG_ONE_LAUNCH_CMDS 8192

/* where a window slot's Cmds live in the caller's persistent SoA command arrays */
typedef struct mpx_inst_cmds {
    uint64_t first_cmd;
    uint32_t n_cmds;
    uint32_t flags;                /* MPX_IC_HAS_CMDS; 0 = Cmds == nil, or a nil instance        */
} mpx_inst_cmds;                   /* 16 B */

typedef struct mpx_execute_batch {
    const mpx_inst_cmds* inst;     /* n_inst, one per window slot                                */
    size_t n_inst;
    int32_t inst_base;
    uint32_t ipg;
    size_t n_groups;
    const int32_t* committed_upto; /* n_groups                                                   */
    const int32_t* executed_in;    /* n_groups: last executed instance, first_g - 1 = none       */
    int32_t* executed_out;         /* n_groups; may alias executed_in                            */
    const uint8_t* src_op;         /* the source commands, n_src                                 */
    const int64_t* src_key;
    const int64_t* src_val;
    size_t n_src;
    const mpx_accept_send* sends;  /* optional: the slots ret_first is written for               */
    size_t n_sends;
    uint32_t flags;                /* MPX_XG_*                                                   */
    uint32_t reserved;             /* 0                                                          */
} mpx_execute_batch;

typedef struct mpx_execute_out {
    uint8_t* op;                   /* the gathered commands, cap each                            */
    int64_t* key;
    int64_t* val;
    size_t cap;
    uint8_t* mask;                 /* n_inst                                                     */
    uint64_t* inst_first;          /* optional, n_inst                                           */
    uint64_t* ret_first;           /* optional, n_sends                                          */
    uint64_t* grp_cmd_off;         /* optional, n_groups + 1                                     */
} mpx_execute_out;

typedef struct mpx_execute_result {
    uint64_t n_cmds;               /* commands gathered (complete, also past cap)                */
    uint64_t n_inst;               /* instances executed                                         */
    uint64_t n_groups;             /* groups whose cursor moved                                  */
    uint64_t reserved;             /* written 0                                                  */
} mpx_execute_result;              /* 32 B */

int mpx_execute_gather(mpx_engine* eng, const mpx_execute_batch* b, const mpx_execute_out* out,
                       mpx_execute_result* res);
/* scratch of mpx_execute_gather_dev calls of up to max_n_inst slots in up to max_n_groups groups
 * (grows only). The scratch lives in the handle and holds one word per group between calls, which
 * this call initialises: the family's calls on one handle run in one stream order, and a larger
 * reserve invalidates graphs captured before it.                                               */
int mpx_execute_gather_reserve(mpx_engine* eng, size_t max_n_inst, size_t max_n_groups);
/* device form: b and out are host structs of device pointers. Needs mpx_execute_gather_reserve
 * first. Never allocates or synchronises, needs no memset on the stream; it captures into a graph.
 * The per-group and per-instance conditions above are reported through the error word (the code
 * arrives at the next synchronising call): such a group does nothing (executed_out[g] =
 * executed_in[g]), such an instance executes with no commands; every store stays inside its
 * array. The total is not bounded here. Alignment: inst and sends 16 bytes; src_key, src_val, key,
 * val, inst_first, ret_first, grp_cmd_off and d_res 8; committed_upto and executed_* 4; src_op, op
 * and mask any address; any other address is rejected with MPX_E_INVAL.                        */
int mpx_execute_gather_dev(mpx_engine* eng, const mpx_execute_batch* b, const mpx_execute_out* out,
                           mpx_execute_result* d_res, void* stream);

/* ---- store assembly: instance commands into a device command arena -----------------------------
 * Where the Go assigns an instance's commands: MIN handleAccept's fresh Instance{..., accept.Command}
 * (bareminpaxos.go:786-793) and CLASSIC's cmds = accept.Command (paxos.go:479-483, :491, :506),
 * exactly the messages flagged MPX_AH_STORED; handleCommit's Instance{..., commit.Command} / Cmds =
 * commit.Command (bareminpaxos.go:861-868 / paxos.go:526-534), flagged MPX_CH_CMDS; handlePropose's
 * installed instance (bareminpaxos.go:687-699 / paxos.go:410-437), the slots flagged MPX_PH_ACCEPT
 * or MPX_PH_PREPARE. handleCommitShort (bareminpaxos.go:890-898) assigns no commands: a record with
 * value_id == MPX_VALUE_KEEP never stores. Unmarshal always makes a non-nil slice, so a stored
 * message of zero commands leaves {first_cmd, 0, MPX_IC_HAS_CMDS}.
 * mpx_store_commands appends the commands of the batch's storing items to an append-only arena
 * (the source arrays mpx_execute_gather reads) and writes the instances' mpx_inst_cmds.
 *   item -> commands   MSGS: item i is record p = perm ? perm[i] : i of the sources' concatenation;
 *                      it belongs to source s with rec_base[s] <= p < rec_base[s + 1] (rec_base =
 *                      the prefix sum of src[].n_recs) and its commands are [cmd_off[v],
 *                      cmd_off[v + 1]) of that source, v = value_id. It stores when effect[i] &
 *                      store_mask and value_id != MPX_VALUE_KEEP.
 *                      SENDS: [first_cmd, first_cmd + n_cmds) of src[0]; an item stores when
 *                      flags & (MPX_PH_ACCEPT | MPX_PH_PREPARE).
 *   winner             of the storing items of one instance the last in array order wins (the
 *                      handlers run per message in array order). Items are grouped by instance, so
 *                      a storing item loses exactly when the next storing item names its instance.
 *   effect             the winners' commands are appended at [*used, *used + n_cmds) in item order,
 *                      inside an item in source order; inst[instance - inst_base] = {first_cmd,
 *                      n_cmds, MPX_IC_HAS_CMDS} for every winner and no other slot is touched;
 *                      *used advances by n_cmds. Work and scratch scale with n and the commands
 *                      copied, never with n_inst.
 *   all or nothing     *used + n_cmds > cap: nothing is written (arena, inst, *used), res is
 *                      complete and carries MPX_SC_FULL, the call returns MPX_OK; the caller
 *                      compacts or grows and repeats.
 *   MPX_SC_GENERAL     takes the multi-launch path also for a call of at most
 *                      MPX_SC_ONE_LAUNCH_ITEMS items whose sources hold at most
 *                      MPX_SC_ONE_LAUNCH_CMDS commands in all, which otherwise runs as one kernel
 *                      in one workgroup with no scratch; the bytes are the same.
 * Errors, host form, answered before anything is staged: null required arrays, unknown kind or
 * flags, reserved != 0, d_n given, n_src outside [1, MPX_SC_MAX_SRC] (SENDS: not 1), n_src > 1
 * without perm, sum n_recs < n, a perm entry out of range, *used > cap, a storing item whose
 * value_id >= n_frames of its source or whose command range leaves [0, n_cmds), a decreasing
 * cmd_off -> MPX_E_INVAL; a storing item outside the window -> MPX_E_NIL_INSTANCE; n or the total
 * at or above 2^32-1 -> MPX_E_UNSUPPORTED. Items that do not store are not judged.              */
#define MPX_SC_MSGS 0u            /* kind: mpx_accept_msg records + slot-aligned effect bytes   */
#define MPX_SC_SENDS 1u           /* kind: mpx_accept_send slots (ACCEPT | PREPARE store)       */
#define MPX_SC_GENERAL 1u         /* call flag: force the multi-launch path                     */
#define MPX_SC_FULL 1u            /* result flag: the arena could not take the batch            */
#define MPX_SC_MAX_SRC 16         /* = MPX_ORDER_MAX_SRC                                        */
#define MPX_SC_ONE_LAUNCH_ITEMS 1024
#define MPX_SC_ONE_LAUNCH_CMDS 8192

/* one connection's unmarshal output (MSGS), or the proposal arrays (SENDS: cmd_off null,
 * n_frames 0, n_recs = n_sends) */
typedef struct mpx_store_src {
    const uint64_t* cmd_off;       /* n_frames + 1 entries                                       */
    size_t n_frames;
    const uint8_t* op;             /* the source's commands, n_cmds each                         */
    const int64_t* key;
    const int64_t* val;
    size_t n_cmds;
    size_t n_recs;                 /* records of this source in the concatenation perm indexes   */
} mpx_store_src;

typedef struct mpx_store_batch {
    uint32_t kind, flags;          /* MPX_SC_MSGS / MPX_SC_SENDS; MPX_SC_GENERAL                 */
    const void* items;             /* mpx_accept_msg[n] or mpx_accept_send[n]                    */
    const uint8_t* effect;         /* MSGS: slot-aligned; SENDS: null                            */
    size_t n;
    const uint64_t* d_n;           /* optional, _dev only: min(*d_n, n) items are read, so the call
                                      captures behind mpx_order_records_dev (&d_res->n)          */
    const uint32_t* perm;          /* MSGS with n_src > 1: mpx_order_records' perm; else optional */
    const mpx_store_src* src;
    size_t n_src;
    size_t n_inst;
    int32_t inst_base;
    uint32_t store_mask;           /* MSGS: MPX_AH_STORED and MPX_CH_CMDS are both 2             */
    uint32_t reserved;             /* 0                                                          */
} mpx_store_batch;

typedef struct mpx_store_arena {
    uint8_t* op;                   /* cap each                                                   */
    int64_t* key;
    int64_t* val;
    size_t cap;
    uint64_t* used;                /* in/out append cursor                                       */
} mpx_store_arena;

typedef struct mpx_store_result {
    uint64_t n_stored;             /* slots written (winners)                                    */
    uint64_t n_cmds;               /* their commands, complete also on MPX_SC_FULL               */
    uint64_t n_superseded;         /* storing items that lost to a later one                     */
    uint64_t flags;                /* MPX_SC_FULL                                                */
} mpx_store_result;                /* 32 B */

/* host form: stages only what the call writes (the appended range, the span of inst between the
 * first and the last storing item, the cursor and res) */
int mpx_store_commands(mpx_engine* eng, const mpx_store_batch* b, const mpx_store_arena* arena,
                       mpx_inst_cmds* inst, mpx_store_result* res);
/* scratch of mpx_store_commands_dev calls of up to max_n items (grows only; a larger reserve
 * invalidates graphs captured before it) */
int mpx_store_commands_reserve(mpx_engine* eng, size_t max_n);
/* device form: b and arena are host structs of device pointers (b->src a host array of them). Needs
 * mpx_store_commands_reserve first. Never allocates or synchronises, needs no memset on the stream;
 * it captures into a graph. The per-item conditions above and *used > cap are reported through the
 * error word (the code arrives at the next synchronising call): such an item neither stores nor
 * supersedes, *used > cap is treated as MPX_SC_FULL, and every store stays inside its array.
 * Alignment: items 16 bytes; cmd_off, key, val (sources and arena), used, d_n and d_res 8; d_inst
 * 16; perm 4; op bytes and effect any address; any other address is rejected with MPX_E_INVAL. */
int mpx_store_commands_dev(mpx_engine* eng, const mpx_store_batch* b, const mpx_store_arena* arena,
                           mpx_inst_cmds* d_inst, mpx_store_result* d_res, void* stream);

/* Compaction, out of place: every slot of inst[n_inst] with MPX_IC_HAS_CMDS, in window order, has
 * its commands copied from `from` to `to` from position 0, and its first_cmd rewritten in place;
 * to->used is written (not read), `from` is left as it was. Slots without the flag are untouched:
 * an instance is retired by clearing its flag first. A total above to->cap: nothing is written and
 * res carries MPX_SC_FULL. res: n_stored = the flagged slots, n_cmds = their commands,
 * n_superseded = 0. A flagged slot whose range leaves [0, *from->used) -> MPX_E_INVAL (host form);
 * the _dev form raises the error word and the slot is left {its new position, 0 commands}. from
 * and to must not overlap (checked by address range), *from->used <= from->cap; n_inst or the
 * total at or above 2^32-1 -> MPX_E_UNSUPPORTED. Alignment as above.                           */
int mpx_store_compact(mpx_engine* eng, mpx_inst_cmds* inst, size_t n_inst,
                      const mpx_store_arena* from, const mpx_store_arena* to, mpx_store_result* res);
int mpx_store_compact_reserve(mpx_engine* eng, size_t max_n_inst);
int mpx_store_compact_dev(mpx_engine* eng, mpx_inst_cmds* d_inst, size_t n_inst,
                          const mpx_store_arena* from, const mpx_store_arena* to,
                          mpx_store_result* d_res, void* stream);

/* ---- record assembly: a batch's durable-log bytes built on the device ---------------------------
 * Every handler of the reference ends in a write to the stable store: recordInstanceMetadata and,
 * where the message carries commands, recordCommands (bareminpaxos.go:164-188 / paxos.go:107-130).
 * mpx_record_log walks the batch's items in array order and appends, for every RECORDING item, the
 * bytes its handler writes, back to back, into out: the batch's stable-store append as one byte
 * run (the host keeps Write + Sync).
 *   kind            items                      records when                  metadata
 *   MPX_LR_ACCEPTS  mpx_accept_msg + effect    effect[i] & MPX_AH_STORED     {ballot, ACCEPTED, instance}
 *                   handleAccept, bareminpaxos.go:798-800. Commands: the message's, resolved as
 *                   mpx_store_commands MSGS resolves them (perm, up to MPX_SC_MAX_SRC sources,
 *                   cmd_off[value_id] ..). EVERY storing message records, not only the instance's
 *                   winner (a value_id of MPX_VALUE_KEEP is judged like any other handle).
 *   MPX_LR_COMMITS  mpx_accept_msg + effect    every item                    {ballot, COMMITTED, instance}
 *                   handleCommit / handleCommitShort, bareminpaxos.go:881-882, :909 / paxos.go:
 *                   547-548, :574. Commands where effect[i] & MPX_CH_CMDS and value_id !=
 *                   MPX_VALUE_KEEP, resolved as above; a CommitShort writes metadata only.
 *   MPX_LR_SENDS    mpx_accept_send            flags & MPX_PH_ACCEPT         {ballot, PREPARED, instance}
 *                   handlePropose, bareminpaxos.go:697-698 / paxos.go:436-437. Commands:
 *                   [first_cmd, first_cmd + n_cmds) of src[0]. MPX_PH_PREPARE stores but records
 *                   nothing (paxos.go:421-428); NOT_LEADER and REFUSED slots record nothing.
 *   MPX_LR_DECIDED  mpx_accept_send + mask     flags & MPX_PH_ACCEPT and     {ballot, COMMITTED, instance}
 *                                              mask[instance - inst_base]
 *                   handleAcceptReply's commit branch, bareminpaxos.go:1045 / paxos.go:656: the
 *                   ballot mpx_build_replies' mpx_commit_send takes from the same slot. No
 *                   commands; src is not read (n_src 0 .. MPX_SC_MAX_SRC).
 *   format          MPX_LOG_DURABLE: MIN's 12-byte metadata (Ballot, Status, instNo as LE u32).
 *                   MPX_LOG_DURABLE_CLASSIC: paxos.go:107-116, Ballot LE u32 and one status byte, 5
 *                   bytes, no instance number. Commands are 17 bytes each (Op, K, V) in both. The
 *                   format is a field of the call, independent of mpx_config.mode.
 *                   mpx_encode_log does not take MPX_LOG_DURABLE_CLASSIC.
 *                   MPX_LR_ACCEPTS with MPX_LOG_DURABLE_CLASSIC -> MPX_E_UNSUPPORTED: CLASSIC's
 *                   handleAccept records the instance's status at that message, which is COMMITTED
 *                   in the reordered-ACCEPT branch (paxos.go:506-509, :514); neither effect nor the
 *                   final state tells it.
 *   order           records come out in array order: the handlers' contract order, grouped by
 *                   instance, arrival order kept inside an instance. (The reference appends in
 *                   arrival order across instances too; replay keeps the last record of an
 *                   instance, so it sees no difference.)
 *   outputs         out[out_cap]; item_off[n + 1] (optional): where item i's record starts, a
 *                   non-recording item has zero length, item_off[n] = n_bytes, entries past the
 *                   items read (d_n) equal the total; always written. res: always complete.
 *   all or nothing  n_bytes > out_cap: out is left untouched, res carries MPX_LR_FULL, the call
 *                   returns MPX_OK. mpx_record_bound(n, m) = 12 n + 17 m bounds both formats.
 *   MPX_LR_GENERAL  takes the multi-launch path also for a call of at most
 *                   MPX_LR_ONE_LAUNCH_ITEMS items whose sources hold at most
 *                   MPX_LR_ONE_LAUNCH_CMDS commands in all, which otherwise runs as one kernel in
 *                   one workgroup with no scratch; the bytes are the same. Work and scratch scale
 *                   with n and the bytes written, never with n_inst.
 * Errors, host form, answered before anything is staged: null required arrays (res; items with n;
 * effect for ACCEPTS / COMMITS; mask for DECIDED with n_inst; src except for DECIDED; out with
 * out_cap; a source's arrays), unknown kind, format or flags, reserved != 0, d_n given, n_src
 * outside [1, MPX_SC_MAX_SRC] (SENDS: not 1; DECIDED: above MPX_SC_MAX_SRC), n_src > 1 without
 * perm, sum n_recs < n (not DECIDED), a perm entry out of range, a recording item whose value_id >=
 * n_frames of its source or whose command range leaves [0, n_cmds), a decreasing cmd_off ->
 * MPX_E_INVAL; MPX_LR_DECIDED with a slot flagged MPX_PH_ACCEPT whose instance lies outside the
 * window -> MPX_E_NIL_INSTANCE; n or the byte total at or above 2^32-1 -> MPX_E_UNSUPPORTED. Items
 * that do not record are not judged.                                                          */
#define MPX_LOG_DURABLE_CLASSIC 2 /* mpx_record_batch.format only                               */
#define MPX_LR_ACCEPTS 0u
#define MPX_LR_COMMITS 1u
#define MPX_LR_SENDS 2u
#define MPX_LR_DECIDED 3u
#define MPX_LR_GENERAL 1u         /* call flag: force the multi-launch path                     */
#define MPX_LR_FULL 1u            /* result flag: out could not take the run                    */
#define MPX_LR_ONE_LAUNCH_ITEMS 1024
#define MPX_LR_ONE_LAUNCH_CMDS 8192

typedef struct mpx_record_batch {
    uint32_t kind, flags;          /* MPX_LR_*; MPX_LR_GENERAL                                   */
    uint32_t format, reserved;     /* MPX_LOG_DURABLE / MPX_LOG_DURABLE_CLASSIC; 0               */
    const void* items;             /* mpx_accept_msg[n] or mpx_accept_send[n]                    */
    const uint8_t* effect;         /* ACCEPTS, COMMITS: slot-aligned; else null                  */
    const uint8_t* mask;           /* DECIDED: mask[n_inst]; else null                           */
    size_t n;
    const uint64_t* d_n;           /* optional, _dev only: min(*d_n, n) items are read, so the call
                                      captures behind mpx_order_records_dev (&d_res->n)          */
    const uint32_t* perm;          /* ACCEPTS / COMMITS with n_src > 1: mpx_order_records' perm  */
    const mpx_store_src* src;      /* as mpx_store_batch.src                                     */
    size_t n_src;
    size_t n_inst;                 /* DECIDED: the window of mask                                */
    int32_t inst_base;
    uint32_t pad;                  /* not read                                                   */
} mpx_record_batch;

typedef struct mpx_record_result {
    uint64_t n_recs;               /* recording items                                            */
    uint64_t n_cmds;               /* their commands                                             */
    uint64_t n_bytes;              /* the run, complete also on MPX_LR_FULL                      */
    uint64_t flags;                /* MPX_LR_FULL                                                */
} mpx_record_result;               /* 32 B */

/* 12 n + 17 m: the most bytes n items carrying m commands in all can record, either format */
size_t mpx_record_bound(size_t n, size_t m);
int mpx_record_log(mpx_engine* eng, const mpx_record_batch* b, uint8_t* out, size_t out_cap,
                   uint64_t* item_off, mpx_record_result* res);
/* scratch of mpx_record_log_dev calls of up to max_n items (grows only; a larger reserve
 * invalidates graphs captured before it) */
int mpx_record_log_reserve(mpx_engine* eng, size_t max_n);
/* device form: b is a host struct of device pointers (b->src a host array of them). Needs
 * mpx_record_log_reserve first. Never allocates or synchronises, needs no memset on the stream;
 * it captures into a graph. The per-item conditions above are reported through the error word
 * (the code arrives at the next synchronising call): such an item records nothing, and every
 * store stays inside its array. Alignment: items 16 bytes; cmd_off, key, val, d_item_off, d_n and
 * d_res 8; perm 4; op, effect, mask and d_out any address; any other address is rejected with
 * MPX_E_INVAL.                                                                                 */
int mpx_record_log_dev(mpx_engine* eng, const mpx_record_batch* b, uint8_t* d_out, size_t out_cap,
                       uint64_t* d_item_off, mpx_record_result* d_res, void* stream);

/* ---- Accept frames with the catch-up log read from the instance store ---------------------------
 * A second form of mpx_encode_accepts for a leader that keeps its instances on the device: the
 * CatchUpLog of a MIN frame is not a dense window-ordered copy (log_recs / log_cmd_off / log_*)
 * but the state the handlers and mpx_store_commands already maintain. Every field mpx_accept_batch
 * shares with this struct means what it means there; frames, destinations, dest_off, the out_cap
 * rule, the rules about last_committed and the CLASSIC wire are mpx_encode_accepts' word for word,
 * and so are the bytes whenever the dense log describes the same instances.
 * Log record i (window index), Instance.Marshal (minpaxosprotomarsh.go:100-124):
 *   nil      exactly when st[i].status == MPX_STATUS_NIL
 *   Ballot   st[i].ballot
 *   Status   lb[i].status where lb is given and lb[i].status != MPX_STATUS_NIL, else st[i].status
 *            (the Go keeps one Status per instance; here mpx_propose_handle writes PREPARED into
 *            both windows, mpx_accept_tally moves only lb to COMMITTED, and the acceptor and commit
 *            handlers write only st)
 *   Cmds     with inst[i].flags & MPX_IC_HAS_CMDS: src[first_cmd .. first_cmd + n_cmds); without
 *            it Cmds == nil, which marshals as V(0) (:117-123) - an instance a CommitShort made
 *            is this case, and it is legal
 * The arena is named and bounded as mpx_execute_batch names it (n_src = its capacity). CLASSIC
 * frames carry no log: st / lb / inst / src_* are not read and may be null.
 * Errors, host form, answered before anything is staged: everything mpx_encode_accepts answers,
 * with the same codes; reserved != 0, or null st / inst with MIN sends -> MPX_E_INVAL; a nil
 * instance inside some destination's catch-up range -> MPX_E_NIL_INSTANCE; a flagged slot inside a
 * range whose [first_cmd, first_cmd + n_cmds) leaves [0, n_src) -> MPX_E_INVAL. Slots outside
 * every range are not judged. The host form stages the span of st / lb / inst between the lowest
 * and the highest window index any range touches and, of the arena, only the commands of the
 * instances inside some range, gathered into a compact copy (never the arena itself).            */
typedef struct mpx_accept_store_batch {
    const mpx_accept_send* sends;
    size_t n_sends;
    int32_t inst_base;
    uint32_t ipg;
    size_t n_groups;
    const mpx_proposer_group* groups;
    const int32_t* peer_commits;
    const uint8_t* cmd_op;         /* the sends' new commands, as mpx_accept_batch.cmd_*         */
    const int64_t* cmd_key;
    const int64_t* cmd_val;
    size_t n_cmds;
    const mpx_acceptor_state* st;  /* n_inst: ballot and status of instanceSpace[i]              */
    const mpx_inst_state* lb;      /* n_inst, optional: the leader bookkeeping window            */
    const mpx_inst_cmds* inst;     /* n_inst: where the slot's Cmds live                         */
    const uint8_t* src_op;         /* the command arena, n_src                                   */
    const int64_t* src_key;
    const int64_t* src_val;
    size_t n_src;
    uint32_t flags;                /* MPX_AB_*                                                   */
    uint32_t alive_mask;
    uint32_t reserved;             /* 0                                                          */
} mpx_accept_store_batch;

int mpx_encode_accepts_stored(mpx_engine* eng, const mpx_accept_store_batch* b, uint8_t* out,
                              size_t out_cap, uint64_t* dest_off);
/* scratch for _dev calls of up to max_sends slots over a window of up to max_n_inst instances
 * (grows only). It is the scratch of mpx_encode_accepts_dev, sized for this form's one more array:
 * both forms of one handle run in one stream order, and a larger reserve of either invalidates
 * graphs captured before it.                                                                    */
int mpx_encode_accepts_stored_reserve(mpx_engine* eng, size_t max_sends, size_t max_n_inst);
/* device form: b is a host struct of device pointers. Needs mpx_encode_accepts_stored_reserve
 * first. Never allocates or synchronises, needs no memset on the stream; it captures into a graph.
 * What mpx_encode_accepts_dev reports through the error word it reports alike; a nil instance
 * inside a catch-up range (MPX_E_NIL_INSTANCE) and a flagged slot inside one whose range leaves
 * the arena (MPX_E_INVAL) arrive the same way, and such an instance is sized and encoded as having
 * no commands: frame sizes and bytes agree and no load leaves [0, n_src). Alignment: sends,
 * groups, st, lb, inst 16 bytes; cmd_key, cmd_val, src_key, src_val and d_dest_off 8; peer_commits
 * 4; cmd_op, src_op and d_out any address; any other address is rejected with MPX_E_INVAL.     */
int mpx_encode_accepts_stored_dev(mpx_engine* eng, const mpx_accept_store_batch* b, uint8_t* d_out,
                                  size_t out_cap, uint64_t* d_dest_off, void* stream);

/* ---- the prepare side: batched handlePrepare and the PrepareReply bytes ----------------------
 * The follower's half of Phase 1:
 *   handlePrepare  bareminpaxos.go:712-751 (MIN) / paxos.go:445-468 (CLASSIC)
 *   replyPrepare   through SendMsg (genericsmr.go:499-512) and PrepareReply.Marshal
 *                  (minpaxosprotomarsh.go:308-350 / paxosprotomarsh.go:126-150)
 * Prepare bytes in (mpx_gather_prepares behind mpx_decode_stream), PrepareReply bytes out
 * (mpx_encode_prepare_replies), both on device buffers; what goes out is what mpx_decode_stream,
 * mpx_unmarshal_frames and mpx_prepare_select[_min] consume on the leader. The leader's
 * bcastPrepare and its prepareBookkeeping setup stay on the host. Instance numbers are window
 * numbers as in mpx_accept_handle: idx = instance - inst_base belongs to group g = idx / ipg,
 * n_inst == n_groups * ipg, first_g = inst_base + g * ipg plays the reference's instance 0 of
 * group g and "nothing committed" is first_g - 1.                                               */

/* one Prepare, either mode. minpaxosproto.Prepare{LeaderId,Ballot,LastCommitted}
 * (minpaxosproto.go) / paxosproto.Prepare{LeaderId,Instance,Ballot,ToInfinity}.                */
typedef struct mpx_prepare_msg {
    int32_t key;       /* CLASSIC: Instance (window number). MIN: the group the connection
                          belongs to, in [0, n_groups)                                          */
    int32_t ballot;
    int32_t leader_id;
    int32_t arg;       /* CLASSIC: ToInfinity (the wire byte, 0..255). MIN: LastCommitted
                          (window number)                                                        */
} mpx_prepare_msg; /* 16 B */

#define MPX_PRH_OK 1u     /* the reply's OK is TRUE                                              */
#define MPX_PRH_RAISED 2u /* this message changed default_ballot                                 */
#define MPX_PRH_LOG 4u    /* MIN: the catch-up branch (:732-748): the reply carries Command and
                             the CatchUpLog log_from[i] .. last_committed                        */

/* Prepare bodies to records: from the mpx_peer_frame list mpx_decode_stream[_dev] left (the same
 * buf, the same offsets), the frames of code MPX_PEER_PREPARE, compacted and in stream order.
 * The body is 12 bytes in MIN (msgs[i] = {group, Ballot, LeaderId, LastCommitted}) and 13 in
 * CLASSIC ({Instance, Ballot, LeaderId, ToInfinity}), by mpx_config.mode. group: the Replica the
 * peer connection belongs to (as mpx_client_conn.group for clients); it fills key in MIN and is
 * not read in CLASSIC. frame_index[i] = the frame's index in other. Frames of other codes are
 * skipped. *n_prepares is always complete; nothing is written at or past cap (a capacity of 0 may
 * come with null arrays). Host form: a Prepare frame outside [0, len) -> MPX_E_INVAL.           */
int mpx_gather_prepares(mpx_engine* eng, const uint8_t* buf, size_t len,
                        const mpx_peer_frame* other, size_t n_other, int32_t group,
                        mpx_prepare_msg* msgs, uint32_t* frame_index, size_t cap,
                        uint64_t* n_prepares);
/* device form: its scratch is the PrepareReply encoder's: it needs
 * mpx_encode_prepare_replies_reserve(n_other, 0, 1) (or any larger reserve) first. d_n_other
 * (optional, device): min(*d_n_other, n_other) frames are processed, so the call can be captured
 * right behind mpx_decode_stream_dev. A frame outside [0, len) is reported through the error word
 * and skipped. d_buf may be read up to len rounded up to 16, never at or past it. Alignment: d_buf
 * and d_msgs 16 bytes (any other address is rejected with MPX_E_INVAL); d_n_other, d_n_prepares 8;
 * d_other, d_frame_index 4.                                                                     */
int mpx_gather_prepares_dev(mpx_engine* eng, const uint8_t* d_buf, size_t len,
                            const mpx_peer_frame* d_other, size_t n_other,
                            const uint64_t* d_n_other, int32_t group, mpx_prepare_msg* d_msgs,
                            uint32_t* d_frame_index, size_t cap, uint64_t* d_n_prepares,
                            void* stream);

/* handlePrepare for a batch. msgs[n] in contract order: grouped by key ascending, slot order =
 * arrival order inside a key (mpx_order_records keyed on key gives it; in MIN with inst_base = 0
 * and n_inst = n_groups). st[n_inst] is read only; groups[n_groups] is in/out. replies:
 * mpx_prepare_reply[n] in CLASSIC, mpx_prepare_reply_min[n] in MIN, by mpx_config.mode. They mean
 * what mpx_decode_stream makes them mean, except value_id: the window index of the slot whose Cmds
 * the reply's Command carries, or MPX_VALUE_KEEP where the reply carries none. Outputs are
 * slot-aligned with msgs, one entry per message, always written: replies[i], reply_to[i] =
 * msgs[i].leader_id, effect[i] (MPX_PRH_*) and, in MIN, log_from[i] (null in CLASSIC).
 *   CLASSIC  D = the group's running default_ballot. st[idx] nil: ok = !(D > ballot), the reply is
 *            {Instance, ok, D, no commands}; else ok = !(ballot < inst.ballot), {Instance, ok,
 *            inst.ballot, value_id = idx}. Then, if arg == 1 (TRUE is uint8(1): a byte of 2 raises
 *            nothing) and ballot > D, D = ballot. Only groups[g].default_ballot is written.
 *            D moves over the instances of a group in BATCH order (instance ascending), not in
 *            arrival order: the on-purpose difference INTEGRATION documents for the watermarks.
 *   MIN      per group, sequentially in batch order: if default_ballot < ballot: ok, default_ballot
 *            = ballot, leader = leader_id, prepare_oks = 0 and, where gps and peer_commits are
 *            given, gps[g] = {ballot, 0, 0, ballot, first_g, MPX_VALUE_KEEP; committed_upto and
 *            triggered untouched} and peer_commits[g * N ..] = first_g (the reference's literal 0).
 *            crt_instance advances past non-nil slots. committed_upto <= arg: the reply is
 *            {self_id, crt - 1, ok, default_ballot, committed_upto}, no commands, no log, log_from
 *            = committed_upto + 1. Otherwise MPX_PRH_LOG: Command is the Cmds of slot committed_upto
 *            + 1 when crt > committed_upto (value_id = its window index), and the CatchUpLog is the
 *            instances arg + 1 .. committed_upto: log_from = arg + 1.
 *            The reference indexes a nil culog at :744 and would panic; the engine builds the range
 *            that indexing names, the range handlePrepareReply (:936-938) consumes.
 * Errors: a CLASSIC key outside the window, a MIN crt_instance leaving the group's window, a nil
 * or out-of-window slot committed_upto + 1 where Command reads it, a catch-up range that leaves
 * the group's window or holds a nil slot -> MPX_E_NIL_INSTANCE; a MIN key outside [0, n_groups)
 * -> MPX_E_INVAL; leader_id outside [0, N) -> MPX_E_BAD_ID; order -> MPX_E_INVAL. A message that
 * raised an error still leaves a reply that encodes safely: no commands, an empty log.
 * Host form: stages only the span of st the batch touches.                                      */
int mpx_prepare_handle(mpx_engine* eng, const mpx_prepare_msg* msgs, size_t n,
                       const mpx_acceptor_state* st, size_t n_inst, int32_t inst_base,
                       mpx_proposer_group* groups, size_t n_groups, uint32_t ipg,
                       mpx_group_prep_state* gps, int32_t* peer_commits, void* replies,
                       int32_t* reply_to, uint8_t* effect, int32_t* log_from);
/* device form: d_groups (and d_gps, d_peer_commits) updated in place. One kernel, no scratch, no
 * control words beyond the error word; it captures into a graph. A thread per message; the thread
 * of a group's first message walks the group's run, so the work is the messages' (plus MIN's crt
 * advance and the slots of the ranges it names), never the window's. Alignment: d_msgs, d_st,
 * d_groups, d_gps 16 bytes; d_replies 8 (MIN) / 16 (CLASSIC); d_peer_commits, d_reply_to,
 * d_log_from 4; d_effect any address.                                                           */
int mpx_prepare_handle_dev(mpx_engine* eng, const mpx_prepare_msg* d_msgs, size_t n,
                           const mpx_acceptor_state* d_st, size_t n_inst, int32_t inst_base,
                           mpx_proposer_group* d_groups, size_t n_groups, uint32_t ipg,
                           mpx_group_prep_state* d_gps, int32_t* d_peer_commits, void* d_replies,
                           int32_t* d_reply_to, uint8_t* d_effect, int32_t* d_log_from,
                           void* stream);

/* one call of mpx_encode_prepare_replies: the handler's outputs and the instance store, named as
 * mpx_accept_store_batch names it                                                                */
typedef struct mpx_prepare_reply_batch {
    const void* replies;           /* mpx_prepare_reply_min[n] (MIN) / mpx_prepare_reply[n]      */
    const int32_t* reply_to;       /* n: the destination (< 0: skipped)                          */
    const int32_t* log_from;       /* n, MIN: the log is log_from[i] .. replies[i].last_committed */
    size_t n;
    uint32_t n_dest;               /* 1 .. MPX_MAX_REPLICAS                                       */
    int32_t inst_base;
    size_t n_inst;
    const mpx_acceptor_state* st;  /* n_inst (MIN)                                                */
    const mpx_inst_state* lb;      /* n_inst, optional                                            */
    const mpx_inst_cmds* inst;     /* n_inst                                                      */
    const uint8_t* src_op;         /* the command arena, n_src                                    */
    const int64_t* src_key;
    const int64_t* src_val;
    size_t n_src;
    uint32_t reserved;             /* 0                                                           */
} mpx_prepare_reply_batch;

/* The frames replyPrepare -> SendMsg writes, little endian, V = binary.PutVarint:
 *   MIN      [12][Id][Instance][OK u8][Ballot][LastCommitted][V(n)][n x 17 B][V(m)][m Instances]
 *   CLASSIC  [12][Instance][OK u8][Ballot][V(n)][n x 17 B]
 * Command is inst[value_id]'s range of the arena; a slot without MPX_IC_HAS_CMDS, or a value_id of
 * MPX_VALUE_KEEP, marshals as V(0). A log Instance is mpx_encode_accepts_stored's, word for word:
 * nil exactly when st is nil, Ballot from st, Status from lb where it has one, else from st, Cmds
 * through inst. m = last_committed - log_from[i] + 1 where that is positive, else 0.
 * replies[i] goes to destination reply_to[i] (< 0: skipped; >= n_dest: MPX_E_INVAL). out receives,
 * destination by destination, each destination's frames in array order, back to back: destination
 * d's run is out[dest_off[d] .. dest_off[d+1]) (dest_off: n_dest + 1 entries, always complete).
 * Nothing is ever written at or past out_cap; dest_off[n_dest] > out_cap -> MPX_E_INVAL with
 * dest_off written.
 * Errors, host form, answered before anything is staged: a value_id other than MPX_VALUE_KEEP
 * outside [0, n_inst), a log range that leaves the window, a flagged slot a frame reads whose
 * [first_cmd, first_cmd + n_cmds) leaves [0, n_src) -> MPX_E_INVAL; a nil instance inside a log
 * range -> MPX_E_NIL_INSTANCE. The host form stages the span of st / lb / inst the frames touch
 * and, of the arena, only the referenced commands, gathered into a compact copy.                */
int mpx_encode_prepare_replies(mpx_engine* eng, const mpx_prepare_reply_batch* b, uint8_t* out,
                               size_t out_cap, uint64_t* dest_off);
/* scratch for _dev calls of up to max_n replies to up to n_dest destinations over a window of up
 * to max_n_inst instances, and for mpx_gather_prepares_dev over up to max_n frames (grows only).
 * The scratch lives in the handle: the family's calls on one handle run in one stream order, and a
 * larger reserve invalidates graphs captured before it.                                         */
int mpx_encode_prepare_replies_reserve(mpx_engine* eng, size_t max_n, size_t max_n_inst,
                                       uint32_t n_dest);
/* device form: b is a host struct of device pointers. Never allocates or synchronises, needs no
 * memset on the stream; it captures into a graph. The errors above arrive through the error word;
 * the instance, command range or log range at fault is sized and encoded as empty, so sizes and
 * bytes agree and no load leaves the window or the arena. Alignment: replies 8 (MIN) / 16
 * (CLASSIC); st, lb, inst 16 bytes; src_key, src_val and d_dest_off 8; reply_to, log_from 4;
 * src_op and d_out any address; any other address is rejected with MPX_E_INVAL.                 */
int mpx_encode_prepare_replies_dev(mpx_engine* eng, const mpx_prepare_reply_batch* b,
                                   uint8_t* d_out, size_t out_cap, uint64_t* d_dest_off,
                                   void* stream);

/* ---- durable-log replay (read side) ----------------------------------
 * bareminpaxos.(*Replica).getDataFromStableStore  src/bareminpaxos/bareminpaxos.go:122-161:
 * the stable store as back-to-back MPX_DURABLE_REC_BYTES records (metadata Ballot, Status,
 * instNo as LE u32, then exactly ONE state.Command: Op u8, K i64, V i64). Per record, as the
 * sequential loop leaves it:
 *   recs[i] / op[i] / key[i] / val[i]  the decoded record (recs[i].pad = 0)
 *   scalars[0] (in/out) defaultBallot  = max(defaultBallot, every ballot)          (:145-147)
 *   scalars[1] (in/out) committedUpTo  = max(committedUpTo, instNo of COMMITTED)    (:149-151)
 *   last_rec[instNo]  = index of the LAST record naming instNo (-1: none)            (:153-157)
 * len must be a whole number of records (a trailing partial record, which the reference decodes
 * as a zero-padded garbage instance, is rejected with MPX_E_INVAL) and len / 29 < 2^31.
 * instNo outside [0, inst_cap) is where the reference's instanceSpace index panics:
 * MPX_E_NIL_INSTANCE, outputs unspecified.                                                   */
#define MPX_DURABLE_REC_BYTES 29
/* rec_base: the file index of this call's first record (0 for a whole file; the running record
 * count when a long store is replayed in chunks): last_rec holds rec_base + i, so a later
 * chunk's records win over an earlier chunk's. rec_base + len / 29 must stay below 2^31.
 * last_rec[inst_cap] is in/out: the caller initialises it to -1 before the first chunk.      */
int mpx_replay_durable(mpx_engine* eng, const uint8_t* log, size_t len, int32_t inst_cap,
                       int32_t rec_base, mpx_log_rec* recs, uint8_t* op, int64_t* key,
                       int64_t* val, int32_t* last_rec, int32_t* scalars);
/* device form: d_log 16-byte aligned; d_last_rec[inst_cap] and d_scalars[2] in/out.
 * The slot maxima are binned in LDS (no device atomic per record) when the engine holds the
 * scratch for the call: mpx_replay_durable_reserve(max_len, inst_cap) once beforehand (the dev
 * entry never allocates; instance spaces up to 2^25 slots); without it the call takes one
 * device-scope atomicMax per record. Same results either way.                              */
int mpx_replay_durable_reserve(mpx_engine* eng, size_t max_len, int32_t inst_cap);
int mpx_replay_durable_dev(mpx_engine* eng, const uint8_t* d_log, size_t len, int32_t inst_cap,
                           int32_t rec_base, mpx_log_rec* d_recs, uint8_t* d_op,
                           int64_t* d_key, int64_t* d_val, int32_t* d_last_rec,
                           int32_t* d_scalars, void* stream);

/* ---- device memory, streams and events of the engine's HIP runtime -----------------------
 * For hosts with no HIP binding of their own (a cgo shim, the Python bench and tests): every
 * buffer the *_dev entry points take can come from here, so caller and engine share one HIP
 * runtime and one device. Asynchronous calls take a stream (NULL = the engine's).           */
#define MPX_COPY_H2D 1
#define MPX_COPY_D2H 2
#define MPX_COPY_D2D 3
int mpx_dev_alloc(mpx_engine* eng, size_t bytes, void** d_out);
int mpx_dev_free(mpx_engine* eng, void* d);
int mpx_memcpy_async(mpx_engine* eng, void* dst, const void* src, size_t bytes, int kind,
                     void* stream);
int mpx_memset_async(mpx_engine* eng, void* d, int byte_value, size_t bytes, void* stream);
int mpx_stream_create(mpx_engine* eng, void** stream_out);
int mpx_stream_destroy(mpx_engine* eng, void* stream);
int mpx_stream_synchronize(mpx_engine* eng, void* stream);
int mpx_event_create(mpx_engine* eng, int timing, void** event_out);
int mpx_event_destroy(mpx_engine* eng, void* event);
int mpx_event_record(mpx_engine* eng, void* event, void* stream);
int mpx_stream_wait_event(mpx_engine* eng, void* stream, void* event);
/* milliseconds between two recorded (and completed) timing events                          */
int mpx_event_elapsed_ms(mpx_engine* eng, void* ev_start, void* ev_end, float* ms);

/* ---- hipGraph capture of *_dev sequences (ABI 5) -----------------------------------------
 * mpx_graph_begin puts `stream` into capture (relaxed mode): every *_dev call, copy, memset,
 * event record and stream wait issued on it - and on other streams that join it through an
 * event it records - until mpx_graph_end is recorded into a graph, not run. Every stream that
 * joined must be joined back (an event recorded on it, waited on by `stream`) before the end.
 * mpx_graph_end ends the capture and instantiates the graph (*exec_out); mpx_graph_launch
 * replays it on a stream as one submission; mpx_graph_destroy frees it. Captured calls keep
 * the argument values (pointers, sizes) they were issued with. Used by bench.py to replay the
 * whole per-step sequence of the sharded engine (group step, step totals, the RCCL group on a
 * second stream) with one host call per step group.                                         */
int mpx_graph_begin(mpx_engine* eng, void* stream);
int mpx_graph_end(mpx_engine* eng, void* stream, void** exec_out);
int mpx_graph_launch(mpx_engine* eng, void* exec, void* stream);
int mpx_graph_destroy(mpx_engine* eng, void* exec);

/* the HIP and RCCL runtimes this library is bound to, as one JSON object (NUL-terminated,
 * truncated to cap): {"hip_runtime": v, "hip_driver": v, "rccl": v, "hip_path": "...",
 * "rccl_path": "..."}. Returns the full length (excluding the NUL) or a negative error.    */
int mpx_runtime_info(char* buf, size_t cap);

/* ---- diagnostics: TEST-ONLY entry points (the product path never calls them) -----------
 * mpx_debug_kv_set_epoch: set the KV table's call epoch (1 <= epoch < 2^30) without touching
 * its slots, so a test can drive calls across the epoch wrap on a table whose slots carry
 * older tags. mpx_debug_kv_state: copy the table's per-slot state words (bit 0 present, bit 1
 * last command of the tagged call was a PUT, bits 2.. the tag); *n = slots (cap + 1).
 * mpx_debug_kv_set_small_tag: set the tag of the last replica-batch call (0 <= tag < 2^18 - 1;
 * the next call uses tag + 1, and the call with tag 2^18 - 1 clears the per-slot list heads and
 * restarts the tags at 1), so a test can drive calls across the tag wrap.                                                       */
int mpx_debug_kv_set_epoch(mpx_engine* eng, uint32_t epoch);
int mpx_debug_kv_set_small_tag(mpx_engine* eng, uint32_t tag);
int mpx_debug_kv_state(mpx_engine* eng, uint32_t* state, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif /* MPX_H_ */

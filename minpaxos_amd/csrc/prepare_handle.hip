// prepare_handle.hip — the follower's half of Phase 1: Prepare bytes in, PrepareReply bytes out.
//
// mpx_gather_prepares: one scan (scan.hpp) of the code-8 flags of mpx_decode_stream's `other`
// list whose output step is the gather, as commit.hip's CommitShort gather: the 12-byte (MIN) or
// 13-byte (CLASSIC) body is taken from the two aligned 16-byte vectors that enclose it.
//
// k_prepare_handle<MODE>: handlePrepare (bareminpaxos.go:712-751 / paxos.go:445-468) for a batch
// in contract order. A thread per message; the thread whose message is the first of its group in
// the batch walks the group's run, the reference's sequential handler with the group's scalars in
// registers (CLASSIC: the running defaultBallot; MIN: defaultBallot, Leader, prepareOKs,
// crtInstance). A Phase 1 storm is one Prepare for each of many groups, so the runs are short
// and the groups run side by side; work is the messages', plus MIN's crtInstance advance and the
// slots of the ranges a reply names (their nil check), never the window's. One launch, no
// scratch, no control words beyond the error word.
//
// mpx_encode_prepare_replies: what replyPrepare -> SendMsg (genericsmr.go:499-512) writes, the
// code byte 12 then PrepareReply.Marshal
//   MIN      minpaxosprotomarsh.go:308-350  Id, Instance, OK, Ballot, LastCommitted, V(n), n
//            Commands, V(m), m Instances (:100-124: Ballot, Status, V(k), k Commands)
//   CLASSIC  paxosprotomarsh.go:126-150     Instance, OK, Ballot, V(n), n Commands
// with Command and the CatchUpLog read from the instance store as accepts_stored.hip reads its
// log (st / lb / mpx_inst_cmds / the command arena: catchup.hpp's StoreLog):
//   1. MIN: two window scans: lcoff (the commands a slot marshals: none when unflagged, nil or
//      out of the arena, so sizes and bytes agree and no load leaves [0, n_src)) and log_off (the
//      slots' Instance.Marshal sizes). A log range's bytes are a difference of two prefix sums.
//   2. k_pr_sizes, a thread per (destination q, reply s): the frame's size, 0 where reply_to[s]
//      != q; a destination-major scan in place: frame_off[] and dest_off[] (the stable partition
//      by reply_to falls out of the item order).
//   3. k_pr_emit: a workgroup per 8 KB output window: the holder search, then per 256 items the
//      pieces that overlap the window (the header, Command's commands, log headers, log commands),
//      dealt over the threads by a workgroup scan, ORed into the LDS image, stored as 16-byte
//      vectors.
// Nothing is materialised per frame. The scans, the window loop and the scratch are catchup.hpp's;
// here: the gather, the handler, the PrepareReply frame (pr_frame) and its head (PrPolicy).
#include "common.hpp"
#include "catchup.hpp"
#include "kernels.hpp"
#include "scan.hpp"

namespace mpx {

// ---- Prepare bodies to records ---------------------------------------------------------------------
namespace {
struct GpIn {  // 1 for a Prepare frame among the first min(*d_n, n)
    const mpx_peer_frame* oth;
    const uint64_t* d_n;
    uint64_t n;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        const uint64_t lim = d_n ? (*d_n < n ? *d_n : n) : n;
        return i < lim && oth[i].code == MPX_PEER_PREPARE ? 1u : 0u;
    }
};
struct GpOut {  // the scan's output step is the gather: ex is the frame's slot
    const uint8_t* buf;
    uint64_t len;
    const mpx_peer_frame* oth;
    mpx_prepare_msg* msgs;
    uint32_t* fidx;
    uint64_t cap, n;
    uint64_t* n_prepares;
    uint32_t* err;
    int32_t group;
    uint32_t body;  // 12 (MIN: LeaderId, Ballot, LastCommitted) / 13 (CLASSIC: LeaderId, Instance,
                    // Ballot, ToInfinity u8)
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t ex, uint32_t item) const {
        if (i == n - 1) *n_prepares = (uint64_t)ex + item;
        if (!item || ex >= cap) return;
        const uint64_t p = (uint64_t)oth[i].offset + 1;
        if (p + body > len) {
            raise_err(err, kErrInval);
            return;
        }
        // the two aligned vectors that enclose [p, p + body); the second only where the body
        // reaches into it (it then starts below len)
        const uint4* v = reinterpret_cast<const uint4*>(buf + (p & ~15ull));
        const uint4 x = ld_stream(v);
        const uint4 y = (p & 15u) + body > 16u ? ld_stream(v + 1) : make_uint4(0, 0, 0, 0);
        const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        const uint32_t k = (uint32_t)(p & 15u) >> 2, b = (uint32_t)(p & 3u);
        uint32_t u[5];
#pragma unroll
        for (int j = 0; j < 5; ++j)
            u[j] = k == 0 ? w[j] : k == 1 ? w[j + 1] : k == 2 ? w[j + 2] : w[j + 3];
        uint32_t f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = b ? __builtin_amdgcn_alignbyte(u[j + 1], u[j], b) : u[j];
        const int4 m = body == 12u
                           ? make_int4(group, (int32_t)f[1], (int32_t)f[0], (int32_t)f[2])
                           : make_int4((int32_t)f[1], (int32_t)f[2], (int32_t)f[0],
                                       (int32_t)(f[3] & 0xFFu));
        st_stream(reinterpret_cast<int4*>(msgs) + ex, m);
        fidx[ex] = (uint32_t)i;
    }
};
}  // namespace

// ---- handlePrepare ---------------------------------------------------------------------------------
namespace {
constexpr int kPhBlock = 256;
constexpr int64_t kNoGroup = -1;

struct PhArgs {
    const mpx_prepare_msg* msgs;
    uint64_t n;
    const mpx_acceptor_state* st;
    uint64_t n_inst;
    int32_t base;
    uint32_t ipg;
    mpx_proposer_group* groups;
    uint64_t n_groups;
    int32_t nrep;
    mpx_group_prep_state* gps;
    int32_t* pc;
    void* replies;
    int32_t* reply_to;
    uint8_t* effect;
    int32_t* log_from;
    uint32_t* err;
};

// the group a message belongs to, kNoGroup where its key names none
template <int MODE>
__device__ __forceinline__ int64_t ph_group(const PhArgs& a, int32_t key) {
    if (MODE == MPX_MODE_MIN) return key >= 0 && (uint64_t)key < a.n_groups ? (int64_t)key : kNoGroup;
    const int64_t idx = (int64_t)key - a.base;
    return idx >= 0 && (uint64_t)idx < a.n_inst ? idx / a.ipg : kNoGroup;
}
__device__ __forceinline__ void ph_put_classic(const PhArgs& a, uint64_t i, int32_t inst,
                                               int32_t ballot, uint32_t ok, uint32_t vid) {
    reinterpret_cast<int4*>(a.replies)[i] = make_int4(inst, ballot, (int32_t)ok, (int32_t)vid);
}
__device__ __forceinline__ void ph_put_min(const PhArgs& a, uint64_t i, int32_t id, int32_t inst,
                                           int32_t ballot, int32_t lc, uint32_t ok, uint32_t vid,
                                           int32_t log_from) {
    int2* r = reinterpret_cast<int2*>(a.replies) + 3 * i;  // 24-byte records, 8-byte aligned
    r[0] = make_int2(id, inst);
    r[1] = make_int2(ballot, lc);
    r[2] = make_int2((int32_t)ok, (int32_t)vid);
    a.log_from[i] = log_from;
}
}  // namespace

template <int MODE>
__global__ __launch_bounds__(kPhBlock) void k_prepare_handle(PhArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kPhBlock + threadIdx.x;
    if (i >= a.n) return;
    const int4* m4 = reinterpret_cast<const int4*>(a.msgs);
    const int4* st4 = reinterpret_cast<const int4*>(a.st);
    const int4 me = m4[i];  // key, ballot, leader_id, arg
    const int64_t g = ph_group<MODE>(a, me.x);
    int64_t gprev = kNoGroup;
    if (i) {
        const int32_t pk = m4[i - 1].x;
        if (pk > me.x) raise_err(a.err, kErrOrder);
        gprev = ph_group<MODE>(a, pk);
    }
    if (g == kNoGroup) {  // no group's run holds it: an all-zero reply that encodes as empty
        raise_err(a.err, MODE == MPX_MODE_MIN ? kErrInval : kErrNil);
        if (me.z < 0 || me.z >= a.nrep) raise_err(a.err, kErrBadId);
        a.reply_to[i] = me.z;
        a.effect[i] = 0;
        if (MODE == MPX_MODE_MIN) ph_put_min(a, i, 0, 0, 0, 0, 0u, MPX_VALUE_KEEP, 1);
        else ph_put_classic(a, i, me.x, 0, 0u, MPX_VALUE_KEEP);
        return;
    }
    if (gprev == g) return;  // the run's first thread handles it
    const int4 ga = reinterpret_cast<const int4*>(a.groups + g)[0];  // D, self, leader, prepareOKs
    int32_t D = ga.x, leader = ga.z, poks = ga.w;
    if (MODE != MPX_MODE_MIN) {
        for (uint64_t j = i; j < a.n; ++j) {
            const int4 m = j == i ? me : m4[j];
            if (j != i && ph_group<MODE>(a, m.x) != g) break;
            if (m.z < 0 || m.z >= a.nrep) raise_err(a.err, kErrBadId);
            const int64_t idx = (int64_t)m.x - a.base;
            const int4 s = st4[idx];  // status, ballot
            uint32_t ok, vid;
            int32_t rb;
            if (s.x == MPX_STATUS_NIL) {  // :449-454
                ok = D > m.y ? 0u : 1u;
                rb = D;
                vid = MPX_VALUE_KEEP;  // make([]state.Command, 0)
            } else {  // :455-461
                ok = m.y < s.y ? 0u : 1u;
                rb = s.y;
                vid = (uint32_t)idx;
            }
            const bool raised = m.w == 1 && m.y > D;  // :465-467, TRUE = uint8(1)
            if (raised) D = m.y;
            ph_put_classic(a, j, m.x, rb, ok, vid);
            a.reply_to[j] = m.z;
            a.effect[j] = (uint8_t)((ok ? MPX_PRH_OK : 0u) | (raised ? MPX_PRH_RAISED : 0u));
        }
        if (D != ga.x) a.groups[g].default_ballot = D;
        return;
    }
    const int2 gb = reinterpret_cast<const int2*>(a.groups + g)[2];  // crt, committedUpTo
    const int32_t self = ga.y, cu = gb.y;
    const int64_t first = (int64_t)a.base + g * (int64_t)a.ipg, endw = first + a.ipg;
    int64_t crt = gb.x;
    bool dead = false;  // crtInstance left the window: the reference has panicked
    for (uint64_t j = i; j < a.n; ++j) {
        const int4 m = j == i ? me : m4[j];
        if (j != i && ph_group<MODE>(a, m.x) != g) break;
        if (m.z < 0 || m.z >= a.nrep) raise_err(a.err, kErrBadId);
        uint32_t eff = 0;
        if (D < m.y) {  // :718-723
            eff = MPX_PRH_OK | MPX_PRH_RAISED;
            D = m.y;
            leader = m.z;
            poks = 0;
            if (a.gps) {  // PrepareBookkeeping{ballot, 0, 0, peerCommits, 0, nil}
                int32_t* p = reinterpret_cast<int32_t*>(a.gps + g);
                reinterpret_cast<int4*>(p)[0] = make_int4(m.y, 0, 0, m.y);
                reinterpret_cast<int2*>(p)[2] = make_int2((int32_t)first, (int32_t)MPX_VALUE_KEEP);
            }
            if (a.pc)
                for (int32_t q = 0; q < a.nrep; ++q) a.pc[g * a.nrep + q] = (int32_t)first;
        }
        while (!dead) {  // :725-727
            if (crt < first || crt >= endw) {
                dead = true;
                break;
            }
            if (st4[crt - a.base].x == MPX_STATUS_NIL) break;
            ++crt;
        }
        uint32_t vid = MPX_VALUE_KEEP;
        int32_t lf = cu + 1;  // an empty log
        if (dead) {
            raise_err(a.err, kErrNil);
        } else if (cu > m.w) {  // :733-748
            bool bad = false;
            if (crt > cu) {  // :737-740: temp := *r.instanceSpace[r.committedUpTo+1]
                const int64_t s = (int64_t)cu + 1;
                if (s < first || s >= endw || st4[s - a.base].x == MPX_STATUS_NIL) bad = true;
                else vid = (uint32_t)(s - a.base);
            }
            const int64_t lo = (int64_t)m.w + 1;  // :743-745, the range the indexing names
            if (lo < first || cu >= endw) bad = true;
            for (int64_t r = lo; !bad && r <= cu; ++r)
                if (st4[r - a.base].x == MPX_STATUS_NIL) bad = true;
            if (bad) {
                raise_err(a.err, kErrNil);
                vid = MPX_VALUE_KEEP;
            } else {
                eff |= MPX_PRH_LOG;
                lf = (int32_t)lo;
            }
        }
        ph_put_min(a, j, self, (int32_t)(crt - 1), D, cu, eff & MPX_PRH_OK, vid, lf);
        a.reply_to[j] = m.z;
        a.effect[j] = (uint8_t)eff;
    }
    reinterpret_cast<int4*>(a.groups + g)[0] = make_int4(D, self, leader, poks);
    a.groups[g].crt_instance = (int32_t)crt;
}

hipError_t launch_prepare_handle(int mode, const mpx_prepare_msg* msgs, uint64_t n,
                                 const mpx_acceptor_state* st, uint64_t n_inst, int32_t base,
                                 mpx_proposer_group* groups, uint64_t n_groups, uint32_t ipg,
                                 int32_t nrep, mpx_group_prep_state* gps, int32_t* peer_commits,
                                 void* replies, int32_t* reply_to, uint8_t* effect,
                                 int32_t* log_from, uint32_t* err, hipStream_t stream) {
    if (n >= (1ull << 32) || n_inst > (1ull << 32)) return hipErrorInvalidValue;
    if (!n) return hipSuccess;
    const PhArgs a{msgs, n,   st,           n_inst,  base,     ipg,    groups,   n_groups,
                   nrep, gps, peer_commits, replies, reply_to, effect, log_from, err};
    const unsigned grid = (unsigned)((n + kPhBlock - 1) / kPhBlock);
    if (mode == MPX_MODE_MIN) k_prepare_handle<MPX_MODE_MIN><<<grid, kPhBlock, 0, stream>>>(a);
    else k_prepare_handle<MPX_MODE_CLASSIC><<<grid, kPhBlock, 0, stream>>>(a);
    return hipGetLastError();
}

// ---- PrepareReply frames ---------------------------------------------------------------------------
namespace {
constexpr uint32_t kPrHeadMin = 18u;      // the code byte, Id, Instance, OK, Ballot, LastCommitted
constexpr uint32_t kPrHeadClassic = 10u;  // the code byte, Instance, OK, Ballot

// the device's view of a call
struct PrArgs {
    const void* replies;
    const int32_t* reply_to;
    const int32_t* log_from;
    uint64_t n;
    uint32_t n_dest;
    int32_t base;
    uint64_t n_inst;
    const mpx_acceptor_state* st;
    const mpx_inst_state* lb;
    const mpx_inst_cmds* inst;
    const uint8_t* sop;
    const int64_t* skey;
    const int64_t* sval;
    uint64_t n_src;
    const uint64_t* lcoff;    // scratch (MIN): lcoff[i] = commands marshalled for window slots [0, i)
    const uint64_t* log_off;  // scratch (MIN): log_off[i] = log bytes of window slots [0, i)
    uint32_t min, head;
};
struct PrHead {
    int32_t id, inst, ballot, lc;
    uint32_t ok;
};

// frame of reply s to destination q (bytes == 0: none)
__device__ __forceinline__ CuFrame<PrHead> pr_frame(const PrArgs& a, uint64_t item, uint32_t* err) {
    CuFrame<PrHead> f;
    f.bytes = 0;
    const uint64_t q = item / a.n, s = item - q * a.n;
    const int32_t to = a.reply_to[s];
    if (to < 0 || (uint32_t)to != (uint32_t)q) {
        if (q == 0 && to >= 0 && (uint32_t)to >= a.n_dest) raise_err(err, kErrInval);  // (once)
        return f;
    }
    uint32_t vid;
    int64_t lc = 0;
    if (a.min) {
        const int2* r = reinterpret_cast<const int2*>(a.replies) + 3 * s;
        const int2 r0 = r[0], r1 = r[1], r2 = r[2];
        f.head.id = r0.x;
        f.head.inst = r0.y;
        f.head.ballot = r1.x;
        f.head.lc = r1.y;
        f.head.ok = (uint32_t)r2.x;
        vid = (uint32_t)r2.y;
        lc = (int64_t)r1.y - a.base;
    } else {
        const int4 r = reinterpret_cast<const int4*>(a.replies)[s];
        f.head.id = 0;
        f.head.inst = r.x;
        f.head.ballot = r.y;
        f.head.lc = 0;
        f.head.ok = (uint32_t)r.z;
        vid = (uint32_t)r.w;
    }
    f.n = f.m = 0;
    f.first_cmd = f.lo = f.L0 = 0;
    if (vid != MPX_VALUE_KEEP) {
        if ((uint64_t)vid >= a.n_inst || !a.inst) {
            raise_err(err, kErrInval);
        } else {
            const StoreCmds c = store_cmds(a.inst, vid);
            if (c.flags & MPX_IC_HAS_CMDS) {
                if (c.in_arena(a.n_src)) {
                    f.n = c.n;
                    f.first_cmd = c.first;
                } else {
                    raise_err(err, kErrInval);
                }
            }
        }
    }
    uint64_t logb = 0;
    if (a.min) {
        const int64_t lf = (int64_t)a.log_from[s] - a.base;
        if (lf <= lc) {
            if (lf < 0 || (uint64_t)lc >= a.n_inst) {
                raise_err(err, kErrInval);  // the range leaves the window: an empty log
            } else {
                f.m = (uint32_t)(lc - lf + 1);
                f.lo = (uint64_t)lf;
                f.L0 = a.log_off[lf];
                logb = a.log_off[lc + 1] - f.L0;
            }
        }
    }
    f.bytes = (uint64_t)a.head + varint_len(f.n) + 17ull * f.n + (a.min ? varint_len(f.m) + logb : 0);
    return f;
}

// catchup.hpp's policy: Command's commands come from the arena, as the log's do; the frame was
// sized with Command's whole range inside the arena
template <bool MIN>
struct PrPolicy {
    static constexpr bool kLog = MIN;
    static constexpr uint32_t kHead = MIN ? kPrHeadMin : kPrHeadClassic;
    using Head = PrHead;
    const PrArgs& a;
    __device__ __forceinline__ const uint64_t* log_off() const { return a.log_off; }
    __device__ __forceinline__ StoreLog log() const {
        return {a.st, a.lb, a.inst, a.sop, a.skey, a.sval, a.n_src, a.lcoff};
    }
    __device__ __forceinline__ CuFrame<Head> frame(uint64_t item, uint32_t* err) const {
        return pr_frame(a, item, err);
    }
    __device__ __forceinline__ void put_head(uint32_t (&h)[6], const Head& F) const {
        h[0] = MPX_PEER_PREPARE_REPLY;
        if (MIN) {
            put32(h, 1, (uint32_t)F.id);
            put32(h, 5, (uint32_t)F.inst);
            h[2] |= (F.ok & 0xFFu) << 8;  // byte 9
            put32(h, 10, (uint32_t)F.ballot);
            put32(h, 14, (uint32_t)F.lc);
        } else {
            put32(h, 1, (uint32_t)F.inst);
            h[1] |= (F.ok & 0xFFu) << 8;  // byte 5
            put32(h, 6, (uint32_t)F.ballot);
        }
    }
    __device__ __forceinline__ Cmd3 cmd(uint64_t j) const {
        return {a.sop[j], (uint64_t)a.skey[j], (uint64_t)a.sval[j]};
    }
};
}  // namespace

__global__ __launch_bounds__(kFrBlock) void k_pr_sizes(PrArgs a, uint64_t n_items,
                                                       uint64_t* __restrict__ size, uint32_t* err) {
    catchup_sizes(PrPolicy<true>{a}, n_items, size, err);  // (pr_frame reads the mode from a)
}

// (a kernel per mode: the head's length is then a constant, and the header words stay in
// registers; as one kernel with a run-time head they went to 32 bytes of scratch per lane)
template <bool MIN>
__global__ __launch_bounds__(kFrBlock) void k_pr_emit(PrArgs a, const uint64_t* __restrict__ frame_off,
                                                      uint64_t n_items, uint8_t* __restrict__ out,
                                                      uint64_t out_cap, uint32_t* err) {
    catchup_emit(PrPolicy<MIN>{a}, frame_off, n_items, out, out_cap, err);
}

uint64_t prepare_replies_work_bytes(uint32_t n_dest, uint64_t n, uint64_t n_inst, Carver&& c) {
    return CatchupWork(c, n_dest, n, n_inst, true), c.bytes();
}

hipError_t launch_encode_prepare_replies(int mode, const mpx_prepare_reply_batch* b, uint8_t* out,
                                         uint64_t out_cap, uint64_t* dest_off, void* work,
                                         uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    if (b->n_dest < 1 || b->n_dest > MPX_MAX_REPLICAS) return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)b->n_dest * b->n;
    if (b->n >= (1ull << 32) || b->n_inst > (1ull << 32)) return hipErrorInvalidValue;
    if (items == 0) {
        k_zero_u64<<<1, 64, 0, stream>>>(dest_off, b->n_dest + 1);
        return hipGetLastError();
    }
    const bool min = mode == MPX_MODE_MIN;
    Carver c(work);
    const CatchupWork w(c, b->n_dest, b->n, b->n_inst, true);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const PrArgs a{b->replies,
                   b->reply_to,
                   b->log_from,
                   b->n,
                   b->n_dest,
                   b->inst_base,
                   b->n_inst,
                   b->st,
                   b->lb,
                   b->inst,
                   b->src_op,
                   b->src_key,
                   b->src_val,
                   b->n_src,
                   w.lcoff,
                   w.log_off,
                   min ? 1u : 0u,
                   min ? kPrHeadMin : kPrHeadClassic};
    if (min && b->n_inst) {  // (CLASSIC frames carry no log)
        const hipError_t r = store_log_offsets(b->st, b->inst, b->n_src, b->n_inst, w, stream);
        if (r != hipSuccess) return r;
    }
    return catchup_run(k_pr_sizes, min ? k_pr_emit<true> : k_pr_emit<false>, a, w, b->n, items, out,
                       out_cap, dest_off, err, stream);
}

hipError_t launch_gather_prepares(int mode, const uint8_t* buf, uint64_t len,
                                  const mpx_peer_frame* other, uint64_t n_other,
                                  const uint64_t* d_n_other, int32_t group, mpx_prepare_msg* msgs,
                                  uint32_t* frame_index, uint64_t cap, uint64_t* n_prepares,
                                  void* work, uint64_t work_bytes, uint32_t* err,
                                  hipStream_t stream) {
    if (n_other >= (1ull << 32) || len > MPX_DECODE_MAX_BYTES) return hipErrorInvalidValue;
    if (!n_other) {
        k_zero_u64<<<1, 1, 0, stream>>>(n_prepares, 1);
        return hipGetLastError();
    }
    Carver c(work);
    const CatchupWork w(c, 1, n_other, 0, true);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    return device_scan(GpIn{other, d_n_other, n_other},
                       GpOut{buf, len, other, msgs, frame_index, cap, n_other, n_prepares, err,
                             group, mode == MPX_MODE_MIN ? 12u : 13u},
                       n_other, ScanSum32{}, 0u, reinterpret_cast<uint32_t*>(w.scan_tmp), stream);
}

}  // namespace mpx

// proposer.hip — the proposer's half of Phase 2: batched handlePropose and the Accept bytes.
//
// k_propose_handle<MODE>: a lane per group runs the reference handler once per batch of at most
// MPX_PROPOSE_MAX_BATCH drained proposals, sequentially (a later batch sees what the earlier one
// did to crtInstance and the instance window):
//   MIN      bareminpaxos.go:617-710: not leader or prepareOKs <= N>>1 -> every proposal is
//            answered FALSE (:618-625); else crtInstance advances past non-nil slots (:627-630);
//            committedUpTo < instNo-1 -> the batch is consumed and refused (:671-685); else the
//            instance is installed PREPARED at defaultBallot and bcastAccept runs (:687-704)
//   CLASSIC  paxos.go:388-443: !IsLeader -> FALSE (:389-393); else advance, instNo, crt++
//            (:395-400); defaultBallot == -1 -> PREPARING at makeUniqueBallot(0), bcastPrepare
//            (:421-428); else PREPARED at defaultBallot, bcastAccept (:429-441)
// One launch, no scratch, no control words beyond the error word: latency-bound like
// k_prepare_min.
//
// mpx_encode_accepts: what bcastAccept -> SendMsg (genericsmr.go:499-512) writes to every peer
// connection for a batch of mpx_accept_send slots, the code byte 9 then Accept.Marshal
//   MIN      minpaxosprotomarsh.go:425-468  LeaderId, Instance, Ballot, LastCommitted, V(n),
//            n Commands, V(m), m Instances (:100-124: Ballot, Status, V(k), k Commands); peer q's
//            CatchUpLog is the group's instances lo .. LastCommitted (bareminpaxos.go:496-506)
//   CLASSIC  paxosprotomarsh.go:214-242     LeaderId, Instance, Ballot, V(n), n Commands
// Nothing is materialised per frame or per group:
//   1. a scan (scan.hpp) of the window's log records' encoded sizes: log_off[], so a catch-up
//      range's bytes are a difference of two prefix sums (sizes computed from cmd_off by the
//      scan's input functor, as in logenc.hip)
//   2. k_ab_sizes, a thread per (destination q, send s): the frame's size (0 where q is not a
//      destination of s or the slot is skipped), and a destination-major scan of the sizes in
//      place: frame_off[] and dest_off[]
//   3. k_ab_emit: a workgroup per 8 KB output window finds the window's first frame by a 256-ary
//      search of frame_off, then walks the items 256 at a time: a thread per item works out which
//      of its frame's pieces (the header, new commands, catch-up instance headers, catch-up
//      commands) overlap the window; a workgroup scan of the piece counts spreads the pieces over
//      the threads, whatever the mix (one 85 KB frame over many windows, or a hundred small
//      frames in one); each piece is ORed into the LDS image as dwords and the image leaves as
//      16-byte stores.
// Steps 2 and 3, the Accept frame (accept_frame, AcceptPolicy) and the scratch are catchup.hpp's,
// shared with accepts_stored.hip and prepare_handle.hip; the log source here is DenseLog
// (log_recs, log_cmd_off, log_op / log_key / log_val). Here: the handler, the kernels by name, the
// launcher.
#include "common.hpp"
#include "catchup.hpp"
#include "kernels.hpp"
#include "scan.hpp"

namespace mpx {

// ---- handlePropose -------------------------------------------------------------------------------
namespace {
constexpr int kPhBlock = 256;

__device__ __forceinline__ void put_send(mpx_accept_send* p, int32_t inst, int32_t ballot,
                                         int32_t lc, uint32_t flags, uint64_t first,
                                         uint32_t n) {
    int4* q = reinterpret_cast<int4*>(p);
    q[0] = make_int4(inst, ballot, lc, (int32_t)flags);
    q[1] = make_int4((int32_t)(uint32_t)first, (int32_t)(uint32_t)(first >> 32), (int32_t)n, 0);
}
}  // namespace

template <int MODE>
__global__ __launch_bounds__(kPhBlock) void k_propose_handle(
    mpx_proposer_group* groups, uint64_t n_groups, const uint64_t* __restrict__ prop_off,
    const uint64_t* __restrict__ send_off, mpx_acceptor_state* st, mpx_inst_state* lb,
    int32_t base, uint32_t ipg, int32_t nrep, mpx_accept_send* sends, uint32_t* err) {
    const uint64_t g = (uint64_t)blockIdx.x * kPhBlock + threadIdx.x;
    if (g >= n_groups) return;
    const int4 ga = reinterpret_cast<const int4*>(groups + g)[0];  // D, self, leader, prepareOKs
    const int2 gb = reinterpret_cast<const int2*>(groups + g)[2];  // crt, committedUpTo
    const int32_t D = ga.x, self = ga.y, committed = gb.y;
    const bool leads = ga.z == self && (MODE != MPX_MODE_MIN || ga.w > (nrep >> 1));
    const uint64_t p0 = prop_off[g], p1 = prop_off[g + 1], so = send_off[g];
    const int64_t first = (int64_t)base + (int64_t)g * ipg, endw = first + ipg;
    int64_t crt = gb.x;
    bool dead = false;  // crtInstance left the window: the reference has panicked
    int4* st4 = reinterpret_cast<int4*>(st);
    for (uint64_t fc = p0, b = 0; fc < p1; fc += MPX_PROPOSE_MAX_BATCH, ++b) {
        const uint32_t nc =
            (uint32_t)(p1 - fc < MPX_PROPOSE_MAX_BATCH ? p1 - fc : MPX_PROPOSE_MAX_BATCH);
        mpx_accept_send* out = sends + so + b;
        if (!leads) {
            put_send(out, -1, 0, 0, MPX_PH_NOT_LEADER, fc, nc);
            continue;
        }
        while (!dead) {  // :627-630 / :395-397
            if (crt < first || crt >= endw) {
                dead = true;
                break;
            }
            if (st[crt - base].status == MPX_STATUS_NIL) break;
            ++crt;
        }
        if (dead) {
            put_send(out, -1, 0, 0, 0u, fc, nc);
            continue;
        }
        const int32_t inst = (int32_t)crt;
        const int64_t idx = crt - base;
        if (MODE == MPX_MODE_MIN) {
            if (committed < inst - 1) {  // :671-685
                put_send(out, inst, D, committed, MPX_PH_REFUSED, fc, nc);
                continue;
            }
            ++crt;  // :688
            st4[idx] = make_int4(MPX_PREPARED, D, (int32_t)(uint32_t)fc, MPX_PF_HAS_PROPOSALS);
            if (lb) reinterpret_cast<int4*>(lb)[idx] = make_int4(MPX_PREPARED, 0, 0, 0);
            put_send(out, inst, D, committed, MPX_PH_ACCEPT, fc, nc);
        } else {
            ++crt;  // :400
            const bool prep = D == -1;  // :421
            const int32_t bal = prep ? self : D;  // makeUniqueBallot(0) = (0 << 4) | r.Id
            const int32_t status = prep ? MPX_PREPARING : MPX_PREPARED;
            st4[idx] = make_int4(status, bal, (int32_t)(uint32_t)fc, MPX_PF_HAS_PROPOSALS);
            if (lb) reinterpret_cast<int4*>(lb)[idx] = make_int4(status, 0, 0, 0);
            put_send(out, inst, bal, committed, prep ? MPX_PH_PREPARE : MPX_PH_ACCEPT, fc, nc);
        }
    }
    if (dead) raise_err(err, kErrNil);
    if (leads) groups[g].crt_instance = (int32_t)crt;
}

hipError_t launch_propose_handle(int mode, mpx_proposer_group* groups, uint64_t n_groups,
                                 const uint64_t* prop_off, const uint64_t* send_off,
                                 mpx_acceptor_state* st, mpx_inst_state* lb, uint64_t n_inst,
                                 int32_t base, uint32_t ipg, int32_t nrep, mpx_accept_send* sends,
                                 uint32_t* err, hipStream_t stream) {
    if (n_groups == 0) return hipSuccess;
    if (!ipg || n_groups * (uint64_t)ipg != n_inst || n_inst > (1ull << 32))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n_groups + kPhBlock - 1) / kPhBlock);
    if (mode == MPX_MODE_MIN)
        k_propose_handle<MPX_MODE_MIN><<<grid, kPhBlock, 0, stream>>>(
            groups, n_groups, prop_off, send_off, st, lb, base, ipg, nrep, sends, err);
    else
        k_propose_handle<MPX_MODE_CLASSIC><<<grid, kPhBlock, 0, stream>>>(
            groups, n_groups, prop_off, send_off, st, lb, base, ipg, nrep, sends, err);
    return hipGetLastError();
}

// ---- the Accept bytes ----------------------------------------------------------------------------
namespace {
using AbArgs = AcceptArgs<DenseLog>;  // the log: log_recs, log_cmd_off, log_op / log_key / log_val
}  // namespace

// frame bytes of item (q, s), destination-major, left in frame_off (the chain send -> group ->
// peer commit -> log_off runs in every lane at once; as the scan's input functor it took 56 us for
// 327,680 items), scanned in place by SizeIn / FrameOffOut (frames.hpp)
template <int MODE>
__global__ __launch_bounds__(kFrBlock) void k_ab_sizes(AbArgs a, uint64_t n_items,
                                                       uint64_t* __restrict__ size, uint32_t* err) {
    catchup_sizes(AcceptPolicy<MODE, DenseLog>{a}, n_items, size, err);
}
template <int MODE>
__global__ __launch_bounds__(kFrBlock) void k_ab_emit(AbArgs a, const uint64_t* __restrict__ frame_off,
                                                      uint64_t n_items, uint8_t* __restrict__ out,
                                                      uint64_t out_cap, uint32_t* err) {
    catchup_emit(AcceptPolicy<MODE, DenseLog>{a}, frame_off, n_items, out, out_cap, err);
}

uint64_t accepts_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_inst, Carver&& c) {
    return CatchupWork(c, nrep, n_sends, n_inst, false), c.bytes();
}

hipError_t launch_encode_accepts(int mode, int32_t nrep, const mpx_accept_batch* b, uint8_t* out,
                                 uint64_t out_cap, uint64_t* dest_off, void* work,
                                 uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    if (nrep < 1 || nrep > MPX_MAX_REPLICAS) return hipErrorInvalidValue;
    const uint64_t n_inst = (uint64_t)b->n_groups * b->ipg;
    const uint64_t items = (uint64_t)nrep * b->n_sends;
    if (b->n_sends >= (1ull << 32) || n_inst > (1ull << 32)) return hipErrorInvalidValue;
    if (items == 0) {
        k_zero_u64<<<1, 64, 0, stream>>>(dest_off, (uint32_t)nrep + 1);
        return hipGetLastError();
    }
    Carver c(work);
    const CatchupWork w(c, (uint32_t)nrep, b->n_sends, n_inst, false);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const AbArgs a{{b->sends, b->n_sends, b->inst_base, b->ipg, n_inst, b->groups, b->peer_commits,
                    b->cmd_op, b->cmd_key, b->cmd_val},
                   {b->log_recs, b->log_cmd_off, b->log_op, b->log_key, b->log_val},
                   w.log_off,
                   (uint32_t)nrep,
                   (b->flags & MPX_AB_THRIFTY) ? 1u : 0u,
                   b->alive_mask};
    if (mode != MPX_MODE_MIN)
        return catchup_run(k_ab_sizes<MPX_MODE_CLASSIC>, k_ab_emit<MPX_MODE_CLASSIC>, a, w,
                           b->n_sends, items, out, out_cap, dest_off, err, stream);
    // log_off[]: a scan of the window's log records' encoded sizes, from log_cmd_off
    const hipError_t r = device_scan(LogRecBytes{b->log_cmd_off}, OffsetsOut{w.log_off}, n_inst,
                                     ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    return catchup_run(k_ab_sizes<MPX_MODE_MIN>, k_ab_emit<MPX_MODE_MIN>, a, w, b->n_sends, items,
                       out, out_cap, dest_off, err, stream);
}

}  // namespace mpx

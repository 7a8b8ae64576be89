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
// The steps are frames.hpp's, shared with commit.hip and logenc.hip: varint_len/_byte, ring_pos,
// SizeIn / FrameOffOut, holder, cmd_span, piece_scan / piece_item, image_or / image_or_cmd,
// window_store, k_zero_u64. Here: the handler, the frame layout (ab_frame, AbPiece), the loop.
#include "common.hpp"
#include "frames.hpp"
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
constexpr int kAbBlock = kFrBlock;
constexpr int kAbWaves = kAbBlock / kWave;
constexpr int kAbWindowVec = 2;  // 16-byte vectors per thread in one output window
constexpr int kAbWindow = kAbBlock * 16 * kAbWindowVec;  // bytes of one output window
constexpr int kAbWords = kAbWindow / 4;               // ... as the dwords of its LDS image
constexpr int kAbGrid = 8192;             // workgroups at most (windows are walked grid-stride)

// the device's view of a call
struct AbArgs {
    const mpx_accept_send* sends;
    uint64_t n_sends;
    int32_t base;
    uint32_t ipg;
    uint64_t n_inst;
    const mpx_proposer_group* groups;
    const int32_t* peer_commits;
    const uint8_t* op;
    const int64_t* key;
    const int64_t* val;
    const mpx_log_rec* lrec;
    const uint64_t* lcoff;
    const uint8_t* lop;
    const int64_t* lkey;
    const int64_t* lval;
    const uint64_t* log_off;  // scratch: log_off[i] = catch-up bytes of window records [0, i)
    uint32_t nrep, thrifty, alive;
};

// frame of send s to destination q (bytes == 0: none)
struct AbFrame {
    uint64_t bytes;
    uint64_t first_cmd;
    uint64_t lo, L0;  // MIN: first catch-up record (window index), its log_off
    uint32_t n, m;    // len(Command), len(CatchUpLog)
    int32_t leader, inst, ballot, lc;
};

// is q one of the group's destinations (bcastAccept's ring walk from self)?
template <int MODE>
__device__ __forceinline__ bool ab_is_dest(uint32_t q, uint32_t self, uint32_t N, uint32_t thrifty,
                                           uint32_t alive) {
    if (q == self) return false;
    const uint32_t want = thrifty ? N >> 1 : N - 1;
    uint32_t before;
    const uint32_t p = ring_pos(q, self, N, alive, before);
    if (MODE == MPX_MODE_MIN) return p < want;  // a dead peer is reconnected and counted (:476-482)
    return before != kRingDead && before < want;  // CLASSIC (:323-327): dead peers are passed over
}

template <int MODE>
__device__ __forceinline__ AbFrame ab_frame(const AbArgs& a, uint64_t item, uint32_t* err) {
    AbFrame f;
    f.bytes = 0;
    const uint64_t q = item / a.n_sends, s = item - q * a.n_sends;
    const int4 s0 = reinterpret_cast<const int4*>(a.sends + s)[0];
    if (!((uint32_t)s0.w & MPX_PH_ACCEPT)) return f;
    const int4 s1 = reinterpret_cast<const int4*>(a.sends + s)[1];
    const int64_t idx = (int64_t)s0.x - a.base;
    if (idx < 0 || (uint64_t)idx >= a.n_inst) {
        raise_err(err, kErrNil);
        return f;
    }
    const uint64_t g = (uint64_t)idx / a.ipg;
    const int32_t self = a.groups[g].self_id;
    if (self < 0 || (uint32_t)self >= a.nrep) {
        raise_err(err, kErrBadId);
        return f;
    }
    if (!ab_is_dest<MODE>((uint32_t)q, (uint32_t)self, a.nrep, a.thrifty, a.alive)) return f;
    f.n = (uint32_t)s1.z;
    f.m = 0;
    f.first_cmd = (uint64_t)(uint32_t)s1.x | ((uint64_t)(uint32_t)s1.y << 32);
    f.leader = self;
    f.inst = s0.x;
    f.ballot = s0.y;
    f.lc = s0.z;
    f.lo = 0;
    f.L0 = 0;
    const uint32_t vn = varint_len(f.n);
    if (MODE != MPX_MODE_MIN) {
        f.bytes = 13ull + vn + 17ull * f.n;
        return f;
    }
    const int64_t first = (int64_t)(g * a.ipg), lc = (int64_t)s0.z - a.base;
    if (lc < first - 1 || lc >= idx) {
        raise_err(err, kErrInval);
        return f;
    }
    const int64_t pc = (int64_t)a.peer_commits[g * a.nrep + q] - a.base;
    const int64_t lo = pc < first ? first : pc + 1;  // :496-506
    uint64_t logb = 0;
    if (lo <= lc) {
        f.m = (uint32_t)(lc - lo + 1);
        f.lo = (uint64_t)lo;
        f.L0 = a.log_off[lo];
        logb = a.log_off[lc + 1] - f.L0;
    }
    f.bytes = 17ull + vn + 17ull * f.n + varint_len(f.m) + logb;
    return f;
}

// scan 1: catch-up bytes of window record i (Instance.Marshal)
struct AbRecBytes {
    const uint64_t* coff;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const uint64_t nc = coff[i + 1] - coff[i];
        return 8u + varint_len(nc) + 17 * nc;
    }
};
struct AbRecOut {
    uint64_t* log_off;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t s, uint64_t b) const {
        log_off[i + 1] = s + b;
    }
};
// scan 2: frame bytes of item (q, s), destination-major: k_ab_sizes leaves them in frame_off (the
// chain send -> group -> peer commit -> log_off runs in every lane at once; as the scan's input
// functor it took 56 us for 327,680 items), scanned in place by SizeIn / FrameOffOut (frames.hpp)

// what a window needs of one frame, left in LDS by the item's thread for the piece threads
struct AbPiece {
    int64_t start;       // frame start - window start
    uint64_t cmd0;       // first new command overlapping the window (global index)
    uint64_t lcmd0;      // first catch-up command overlapping the window (log command index)
    uint64_t L0;         // log_off of the frame's first catch-up record
    uint64_t i0;         // first catch-up record overlapping the window (window index)
    uint32_t j0;         // cmd0's position in the frame's Command slice
    uint32_t n, m;
    uint32_t c_new, c_inst, c_log;  // pieces: new commands, catch-up headers, catch-up commands
    int32_t leader, inst, ballot, lc;
};
}  // namespace

template <int MODE>
__global__ __launch_bounds__(kAbBlock) void k_ab_sizes(AbArgs a, uint64_t n_items,
                                                       uint64_t* __restrict__ size, uint32_t* err) {
    const uint64_t i = (uint64_t)blockIdx.x * kAbBlock + threadIdx.x;
    if (i < n_items) size[i] = ab_frame<MODE>(a, i, err).bytes;
}
template <int MODE>
__global__ __launch_bounds__(kAbBlock) void k_ab_emit(AbArgs a, const uint64_t* __restrict__ frame_off,
                                                      uint64_t n_items, uint8_t* __restrict__ out,
                                                      uint64_t out_cap, uint32_t* err) {
    __shared__ AbPiece fi[kAbBlock];
    __shared__ uint32_t poff[kAbBlock + 1];
    __shared__ uint32_t wtot[kAbWaves];
    __shared__ __attribute__((aligned(16))) uint32_t W[kAbWindow / 4];
    constexpr uint32_t kHead = MODE == MPX_MODE_MIN ? 17u : 13u;
    const int t = threadIdx.x;
    const uint64_t total = frame_off[n_items];
    const uint64_t lim = total < out_cap ? total : out_cap;  // nothing at or past out_cap
    for (uint64_t b0 = (uint64_t)blockIdx.x * kAbWindow; b0 < lim;
         b0 += (uint64_t)gridDim.x * kAbWindow) {
        const uint64_t b1 = b0 + kAbWindow < lim ? b0 + kAbWindow : lim;
#pragma unroll
        for (int v = 0; v < kAbWindowVec; ++v)
            reinterpret_cast<uint4*>(W)[t + v * kAbBlock] = make_uint4(0, 0, 0, 0);
        const uint64_t lo = holder(frame_off, n_items, 0, b0, t);  // the item holding byte b0
        for (uint64_t c0 = lo;; c0 += kAbBlock) {
            const uint64_t i = c0 + t;
            uint32_t np = 0;
            uint64_t fs = 0, fe = 0;
            if (i < n_items) {
                fs = frame_off[i];
                fe = frame_off[i + 1];
            }
            if (fe > fs && fs < b1 && fe > b0) {
                const AbFrame f = ab_frame<MODE>(a, i, nullptr);  // (k_ab_sizes raised the errors)
                AbPiece p;
                p.start = (int64_t)fs - (int64_t)b0;
                p.n = f.n;
                p.m = f.m;
                p.leader = f.leader;
                p.inst = f.inst;
                p.ballot = f.ballot;
                p.lc = f.lc;
                p.L0 = f.L0;
                const uint64_t cs = fs + kHead + varint_len(f.n);  // the Command slice
                const CmdSpan sp = cmd_span(cs, b0, b1);
                const uint64_t jl = sp.lo, jh = sp.hi < f.n ? sp.hi : f.n;
                p.j0 = (uint32_t)jl;
                p.cmd0 = f.first_cmd + jl;
                p.c_new = jh > jl ? (uint32_t)(jh - jl) : 0u;
                p.c_inst = p.c_log = 0;
                p.i0 = 0;
                p.lcmd0 = 0;
                if (MODE == MPX_MODE_MIN && f.m) {
                    // the window in the log's byte coordinates: [x0, x1) of [L0, L1)
                    const uint64_t ls = cs + 17ull * f.n + varint_len(f.m);
                    const uint64_t L1 = f.L0 + (fe - ls);
                    const uint64_t x0 = b0 > ls ? f.L0 + (b0 - ls) : f.L0;
                    const uint64_t x1 = b1 > ls ? (f.L0 + (b1 - ls) < L1 ? f.L0 + (b1 - ls) : L1)
                                                : f.L0;
                    if (x0 < x1) {
                        // i0 = last record with log_off <= x0, i1 = last with log_off < x1
                        uint64_t ra = f.lo, rb = f.lo + f.m;
                        while (rb - ra > 1) {
                            const uint64_t mid = (ra + rb) >> 1;
                            if (a.log_off[mid] <= x0) ra = mid; else rb = mid;
                        }
                        const uint64_t i0 = ra;
                        rb = f.lo + f.m;
                        while (rb - ra > 1) {
                            const uint64_t mid = (ra + rb) >> 1;
                            if (a.log_off[mid] < x1) ra = mid; else rb = mid;
                        }
                        const uint64_t i1 = ra;
                        p.i0 = i0;
                        p.c_inst = (uint32_t)(i1 - i0 + 1);
                        const uint64_t ca0 = a.lcoff[i0], ca1 = a.lcoff[i0 + 1];
                        const uint64_t cb0 = a.lcoff[i1], cb1 = a.lcoff[i1 + 1];
                        const uint64_t cs0 = a.log_off[i0 + 1] - 17 * (ca1 - ca0);
                        const uint64_t cs1 = a.log_off[i1 + 1] - 17 * (cb1 - cb0);
                        const uint64_t la = ca0 + cmd_span(cs0, x0, x1).lo;
                        uint64_t lh = cb0 + cmd_span(cs1, x0, x1).hi;
                        lh = lh < cb1 ? lh : cb1;
                        p.lcmd0 = la;
                        p.c_log = lh > la ? (uint32_t)(lh - la) : 0u;
                    }
                }
                fi[t] = p;
                np = 1u + p.c_new + p.c_inst + p.c_log;
            }
            const uint32_t pieces = piece_scan(np, poff, wtot, t);
            for (uint32_t p = t; p < pieces; p += kAbBlock) {
                const uint32_t fa = piece_item(poff, p);
                const AbPiece& F = fi[fa];
                uint32_t k = p - poff[fa];
                const uint32_t vn = varint_len(F.n);
                const int64_t cs = F.start + kHead + vn;
                if (k == 0) {  // the header and V(n); MIN: V(m) behind the commands
                    const uint32_t ld = (uint32_t)F.leader, in = (uint32_t)F.inst;
                    const uint32_t bl = (uint32_t)F.ballot, lc = (uint32_t)F.lc;
                    uint32_t h[6] = {MPX_PEER_ACCEPT | (ld << 8), (ld >> 24) | (in << 8),
                                     (in >> 24) | (bl << 8), bl >> 24, 0u, 0u};
                    if (MODE == MPX_MODE_MIN) {
                        h[3] |= lc << 8;
                        h[4] = lc >> 24;
                    }
                    for (uint32_t x = 0; x < vn; ++x) {
                        const uint32_t at = kHead + x;
                        h[at >> 2] |= varint_byte(F.n, x) << (8 * (at & 3));
                    }
                    image_or<kAbWords>(W, F.start, h, kHead + vn);
                    if (MODE == MPX_MODE_MIN) {
                        const uint32_t vm = varint_len(F.m);
                        uint32_t v[2] = {0u, 0u};
                        for (uint32_t x = 0; x < vm; ++x)
                            v[x >> 2] |= varint_byte(F.m, x) << (8 * (x & 3));
                        image_or<kAbWords>(W, cs + 17ll * F.n, v, vm);
                    }
                    continue;
                }
                --k;
                if (k < F.c_new) {  // a new command
                    const uint64_t j = F.cmd0 + k;
                    image_or_cmd<kAbWords>(W, cs + 17ll * (F.j0 + k), a.op[j], (uint64_t)a.key[j],
                              (uint64_t)a.val[j]);
                    continue;
                }
                k -= F.c_new;
                // the CatchUpLog starts at ls; a record's bytes sit at ls + log_off[i] - L0
                const int64_t ls = cs + 17ll * F.n + varint_len(F.m);
                if (k < F.c_inst) {  // a catch-up record's header
                    const uint64_t r = F.i0 + k;
                    const mpx_log_rec m = a.lrec[r];
                    if (m.status == MPX_STATUS_NIL) raise_err(err, kErrNil);
                    const uint64_t nc = a.lcoff[r + 1] - a.lcoff[r];
                    const uint32_t vk = varint_len(nc);
                    uint32_t h[5] = {(uint32_t)m.ballot, (uint32_t)m.status, 0u, 0u, 0u};
                    for (uint32_t x = 0; x < vk; ++x)
                        h[2 + (x >> 2)] |= varint_byte(nc, x) << (8 * (x & 3));
                    image_or<kAbWords>(W, ls + (int64_t)(a.log_off[r] - F.L0), h, 8 + vk);
                    continue;
                }
                k -= F.c_inst;
                {  // a catch-up command: its record is the last of the window's with lcoff <= j
                    const uint64_t j = F.lcmd0 + k;
                    uint64_t ra = F.i0, rb = F.i0 + F.c_inst;
                    while (rb - ra > 1) {
                        const uint64_t mid = (ra + rb) >> 1;
                        if (a.lcoff[mid] <= j) ra = mid; else rb = mid;
                    }
                    const uint64_t c0r = a.lcoff[ra], c1r = a.lcoff[ra + 1];
                    const uint64_t csr = a.log_off[ra + 1] - 17 * (c1r - c0r);
                    image_or_cmd<kAbWords>(W, ls + (int64_t)(csr - F.L0) + 17ll * (int64_t)(j - c0r), a.lop[j],
                              (uint64_t)a.lkey[j], (uint64_t)a.lval[j]);
                }
            }
            const uint64_t nx = c0 + kAbBlock;
            if (nx >= n_items || frame_off[nx] >= b1) break;  // (uniform)
            __syncthreads();  // fi and poff are rewritten by the next chunk
        }
        __syncthreads();
        window_store(W, (uint32_t)(b1 - b0), out + b0, t);
        __syncthreads();  // the next window zeroes W
    }
}

namespace {
struct AbWork {
    uint64_t* log_off;    // n_inst + 1
    uint64_t* frame_off;  // nrep * n_sends + 1
    uint64_t* scan_tmp;   // for the larger of the two scans
    AbWork(Carver& c, uint32_t nrep, uint64_t n_sends, uint64_t n_inst) {
        const uint64_t items = (uint64_t)nrep * n_sends;
        log_off = c.take<uint64_t>(n_inst + 1);
        frame_off = c.take<uint64_t>(items + 1);
        const uint64_t big = items > n_inst ? items : n_inst;
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(big ? big : 1));
    }
};

template <int MODE>
hipError_t ab_run(const AbArgs& a, const AbWork& w, uint64_t items, uint8_t* out, uint64_t out_cap,
                  uint64_t* dest_off, uint32_t* err, hipStream_t stream) {
    k_ab_sizes<MODE><<<(unsigned)((items + kAbBlock - 1) / kAbBlock), kAbBlock, 0, stream>>>(
        a, items, w.frame_off, err);
    const hipError_t r = device_scan(SizeIn{w.frame_off},
                                     FrameOffOut{w.frame_off, dest_off, a.n_sends, items}, items,
                                     ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    const uint64_t windows = (out_cap + kAbWindow - 1) / kAbWindow;
    if (!windows) return hipSuccess;
    const unsigned grid = (unsigned)(windows < (uint64_t)kAbGrid ? windows : (uint64_t)kAbGrid);
    k_ab_emit<MODE><<<grid, kAbBlock, 0, stream>>>(a, w.frame_off, items, out, out_cap, err);
    return hipGetLastError();
}
}  // namespace

uint64_t accepts_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_inst, Carver&& c) {
    return AbWork(c, nrep, n_sends, n_inst), c.bytes();
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
    const AbWork w(c, (uint32_t)nrep, b->n_sends, n_inst);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    AbArgs a;
    a.sends = b->sends;
    a.n_sends = b->n_sends;
    a.base = b->inst_base;
    a.ipg = b->ipg;
    a.n_inst = n_inst;
    a.groups = b->groups;
    a.peer_commits = b->peer_commits;
    a.op = b->cmd_op;
    a.key = b->cmd_key;
    a.val = b->cmd_val;
    a.lrec = b->log_recs;
    a.lcoff = b->log_cmd_off;
    a.lop = b->log_op;
    a.lkey = b->log_key;
    a.lval = b->log_val;
    a.log_off = w.log_off;
    a.nrep = (uint32_t)nrep;
    a.thrifty = (b->flags & MPX_AB_THRIFTY) ? 1u : 0u;
    a.alive = b->alive_mask;
    if (mode != MPX_MODE_MIN) return ab_run<MPX_MODE_CLASSIC>(a, w, items, out, out_cap, dest_off, err, stream);
    k_zero_u64<<<1, 1, 0, stream>>>(w.log_off, 1);
    const hipError_t r = device_scan(AbRecBytes{b->log_cmd_off}, AbRecOut{w.log_off}, n_inst,
                                     ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    return ab_run<MPX_MODE_MIN>(a, w, items, out, out_cap, dest_off, err, stream);
}

}  // namespace mpx

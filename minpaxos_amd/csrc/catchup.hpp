// catchup.hpp — the windowed emitter of frames that carry a catch-up log, shared by the three
// encoders of that family: proposer.hip (Accept frames, the log in dense arrays),
// accepts_stored.hip (the same frames, the log read from the instance store) and
// prepare_handle.hip (PrepareReply frames, Command and log read from the instance store).
// A frame of the family is
//   head (P::kHead bytes), V(n), n Commands, and where P::kLog: V(m), m Instances
//   (Instance.Marshal, minpaxosprotomarsh.go:100-124: Ballot, Status, V(k), k Commands)
// and its log is a range of window records whose bytes are differences of the prefix sums
// log_off[] (bytes) and lcoff[] (commands). Here, once: the instance store's view and the scans'
// functors, the two log sources, the window's view of a frame's log, the emit loop, the scratch
// carve-up, the Accept frame and the launcher tail. A unit keeps what is its own: its argument
// struct, its frame function where it has one, its head writer, and its __global__ kernels, whose
// bodies are catchup_sizes / catchup_emit with the unit's policy P:
//   kHead, kLog            the head's length and whether frames carry a log (compile time: the
//                          header words stay in registers, and without a log its pieces are
//                          compiled away)
//   Head                   the head's fields, carried in the LDS piece record
//   frame(item, err)       CuFrame<Head> of item (destination q, slot s); bytes == 0: none
//   put_head(h, head)      the head's kHead bytes into the zeroed words h
//   cmd(j)                 Command j of the frames' own commands
//   log_off(), log()       the log's byte offsets and its source (DenseLog / StoreLog)
// The steps are frames.hpp's (holder, cmd_span, piece_scan / piece_item, image_or, window_store).
#pragma once
#include "frames.hpp"
#include "scratch.hpp"

namespace mpx {

constexpr int kCuWaves = kFrBlock / kWave;
constexpr int kCuWindowVec = 2;  // 16-byte vectors per thread in one output window
constexpr int kCuWindow = kFrBlock * 16 * kCuWindowVec;  // bytes of one output window
constexpr int kCuWords = kCuWindow / 4;                  // ... as the dwords of its LDS image
constexpr int kCuGrid = 8192;  // workgroups at most (windows are walked grid-stride)

// ---- bytes -----------------------------------------------------------------------------------------
// the len bytes of V(n) (len <= 8) as one little-endian word
__device__ __forceinline__ uint64_t varint_word(uint64_t n, uint32_t len) {
    uint64_t w = 0;
    for (uint32_t x = 0; x < len; ++x) w |= (uint64_t)varint_byte(n, x) << (8 * x);
    return w;
}
// v's four bytes into the header words h at byte offset at (a constant where h is to stay in
// registers: an indexed store into h sends it to scratch)
template <int ND>
__device__ __forceinline__ void put32(uint32_t (&h)[ND], uint32_t at, uint32_t v) {
    const uint32_t sh = 8u * (at & 3u);
    h[at >> 2] |= v << sh;
    if (sh) h[(at >> 2) + 1] |= v >> (32u - sh);
}

struct Cmd3 {  // state.Command
    uint32_t op;
    uint64_t key, val;
};

// ---- the instance store's view ---------------------------------------------------------------------
// a slot's Cmds as the store names them
struct StoreCmds {
    uint64_t first;
    uint32_t n, flags;
    __device__ __forceinline__ bool in_arena(uint64_t n_src) const {
        return first <= n_src && n <= n_src - first;
    }
};
__device__ __forceinline__ StoreCmds store_cmds(const mpx_inst_cmds* inst, uint64_t i) {
    const int4 x = reinterpret_cast<const int4*>(inst)[i];
    return {(uint64_t)(uint32_t)x.x | ((uint64_t)(uint32_t)x.y << 32), (uint32_t)x.z, (uint32_t)x.w};
}

// scan: the commands window slot i marshals inside a log (the synthetic lcoff): none when it is
// unflagged (Cmds == nil marshals as V(0), :117-123), nil, or its range leaves the arena
struct StoreCmdCount {
    const mpx_acceptor_state* st;
    const mpx_inst_cmds* inst;
    uint64_t n_src;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const StoreCmds c = store_cmds(inst, i);
        const int32_t status = st[i].status;
        const bool has = (c.flags & MPX_IC_HAS_CMDS) && status != MPX_STATUS_NIL && c.in_arena(n_src);
        return has ? c.n : 0u;
    }
};
// scan: log bytes of window slot i (Instance.Marshal) from the commands' offsets
struct LogRecBytes {
    const uint64_t* coff;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const uint64_t nc = coff[i + 1] - coff[i];
        return 8u + varint_len(nc) + 17 * nc;
    }
};
// both leave n + 1 offsets, the leading zero included (no launch for it)
struct OffsetsOut {
    uint64_t* off;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t s, uint64_t b) const {
        if (i == 0) off[0] = 0;
        off[i + 1] = s + b;
    }
};

// ---- log sources -----------------------------------------------------------------------------------
// record(r, err): window record r's (ballot, status), raising what the record's state raises;
// cmd(ra, x, j): command x of record ra, the log's j-th (lcoff[ra] + x == j)
struct LogRec {
    int32_t ballot, status;
};
// a dense, window-ordered copy
struct DenseLog {
    const mpx_log_rec* rec;
    const uint64_t* lcoff;
    const uint8_t* op;
    const int64_t* key;
    const int64_t* val;
    __device__ __forceinline__ LogRec record(uint64_t r, uint32_t* err) const {
        const mpx_log_rec m = rec[r];
        if (m.status == MPX_STATUS_NIL) raise_err(err, kErrNil);
        return {m.ballot, m.status};
    }
    __device__ __forceinline__ Cmd3 cmd(uint64_t, uint64_t, uint64_t j) const {
        return {op[j], (uint64_t)key[j], (uint64_t)val[j]};
    }
};
// the state a turn keeps on the device: the acceptor window st (ballot, status), the leader
// bookkeeping window lb (status once the tally has committed; optional) and mpx_inst_cmds per slot
// pointing into the command arena; lcoff is scratch (StoreCmdCount's scan)
struct StoreLog {
    const mpx_acceptor_state* st;
    const mpx_inst_state* lb;
    const mpx_inst_cmds* inst;
    const uint8_t* op;
    const int64_t* key;
    const int64_t* val;
    uint64_t n_src;
    const uint64_t* lcoff;
    __device__ __forceinline__ LogRec record(uint64_t r, uint32_t* err) const {
        const int4 s = reinterpret_cast<const int4*>(st)[r];  // status, ballot
        const StoreCmds c = store_cmds(inst, r);
        int32_t status = s.x;
        if (lb) {  // the tally commits in lb alone
            const int32_t ls = lb[r].status;
            status = ls != MPX_STATUS_NIL ? ls : status;
        }
        // what the host form answers before it stages; the record is then emitted with no
        // commands, as it was sized
        if (s.x == MPX_STATUS_NIL) raise_err(err, kErrNil);
        else if ((c.flags & MPX_IC_HAS_CMDS) && !c.in_arena(n_src)) raise_err(err, kErrInval);
        return {s.y, status};
    }
    __device__ __forceinline__ Cmd3 cmd(uint64_t ra, uint64_t x, uint64_t) const {
        // lcoff counts a record's commands only where its whole range is in the arena, so
        // first_cmd + x < n_src
        const uint64_t at = inst[ra].first_cmd + x;
        return {op[at], (uint64_t)key[at], (uint64_t)val[at]};
    }
};

// ---- frames ----------------------------------------------------------------------------------------
// frame of slot s to destination q (bytes == 0: none)
template <class Head>
struct CuFrame {
    uint64_t bytes;
    uint64_t first_cmd;
    uint64_t lo, L0;  // first log record (window index), its log_off
    uint32_t n, m;    // len(Command), len(CatchUpLog)
    Head head;
};
// what a window needs of one frame, left in LDS by the item's thread for the piece threads
template <class Head>
struct CuPiece {
    int64_t start;   // frame start - window start
    uint64_t cmd0;   // first of the frame's own commands overlapping the window (the source's index)
    uint64_t lcmd0;  // first log command overlapping the window (lcoff's index)
    uint64_t L0;     // log_off of the frame's first log record
    uint64_t i0;     // first log record overlapping the window (window index)
    uint32_t j0;     // cmd0's position in the frame's Command slice
    uint32_t n, m;
    uint32_t c_new, c_inst, c_log;  // pieces: own commands, log headers, log commands
    Head head;
};

// The window [b0, b1) seen from the log of a frame that ends at fe and whose log starts at byte
// ls with record lo of m at log_off L0: the records [i0, i0 + c_inst) and the log commands
// [lcmd0, lcmd0 + c_log) that overlap it, a partial one at either end included
struct LogView {
    uint64_t i0, lcmd0;
    uint32_t c_inst, c_log;
};
__device__ __forceinline__ LogView log_view(const uint64_t* log_off, const uint64_t* lcoff,
                                            uint64_t lo, uint32_t m, uint64_t L0, uint64_t ls,
                                            uint64_t fe, uint64_t b0, uint64_t b1) {
    LogView v{0, 0, 0u, 0u};
    // the window in the log's byte coordinates: [x0, x1) of [L0, L1)
    const uint64_t L1 = L0 + (fe - ls);
    const uint64_t x0 = b0 > ls ? L0 + (b0 - ls) : L0;
    const uint64_t x1 = b1 > ls ? (L0 + (b1 - ls) < L1 ? L0 + (b1 - ls) : L1) : L0;
    if (x0 < x1) {
        // i0 = last record with log_off <= x0, i1 = last with log_off < x1
        uint64_t ra = lo, rb = lo + m;
        while (rb - ra > 1) {
            const uint64_t mid = (ra + rb) >> 1;
            if (log_off[mid] <= x0) ra = mid; else rb = mid;
        }
        const uint64_t i0 = ra;
        rb = lo + m;
        while (rb - ra > 1) {
            const uint64_t mid = (ra + rb) >> 1;
            if (log_off[mid] < x1) ra = mid; else rb = mid;
        }
        const uint64_t i1 = ra;
        v.i0 = i0;
        v.c_inst = (uint32_t)(i1 - i0 + 1);
        const uint64_t ca0 = lcoff[i0], ca1 = lcoff[i0 + 1];
        const uint64_t cb0 = lcoff[i1], cb1 = lcoff[i1 + 1];
        const uint64_t cs0 = log_off[i0 + 1] - 17 * (ca1 - ca0);
        const uint64_t cs1 = log_off[i1 + 1] - 17 * (cb1 - cb0);
        const uint64_t la = ca0 + cmd_span(cs0, x0, x1).lo;
        uint64_t lh = cb0 + cmd_span(cs1, x0, x1).hi;
        lh = lh < cb1 ? lh : cb1;
        v.lcmd0 = la;
        v.c_log = lh > la ? (uint32_t)(lh - la) : 0u;
    }
    return v;
}

// ---- the kernels' bodies ---------------------------------------------------------------------------
// (their pointers carry no __restrict__: the kernels' parameters do, and repeated here it changed
// how the sizes kernels' argument loads were scheduled)
// a thread per item (destination q, slot s): the frame's size, and the errors its frame raises
template <class P>
__device__ __forceinline__ void catchup_sizes(const P& pol, uint64_t n_items, uint64_t* size,
                                              uint32_t* err) {
    const uint64_t i = (uint64_t)blockIdx.x * kFrBlock + threadIdx.x;
    if (i < n_items) size[i] = pol.frame(i, err).bytes;
}

// a workgroup per output window, grid-stride: the holder search, then per kFrBlock items the
// pieces that overlap the window (the head with V(n) and V(m), the frame's own commands, log
// headers, log commands), dealt over the threads by a workgroup scan, ORed into the LDS image,
// stored as 16-byte vectors
template <class P>
__device__ __forceinline__ void catchup_emit(const P& pol, const uint64_t* frame_off,
                                             uint64_t n_items, uint8_t* out, uint64_t out_cap,
                                             uint32_t* err) {
    using Piece = CuPiece<typename P::Head>;
    constexpr uint32_t kHead = P::kHead;
    static_assert(kHead + 5u <= 24u, "the head and V(n) fill six words at most");
    __shared__ Piece fi[kFrBlock];
    __shared__ uint32_t poff[kFrBlock + 1];
    __shared__ uint32_t wtot[kCuWaves];
    __shared__ __attribute__((aligned(16))) uint32_t W[kCuWords];
    const int t = threadIdx.x;
    const uint64_t total = frame_off[n_items];
    const uint64_t lim = total < out_cap ? total : out_cap;  // nothing at or past out_cap
    for (uint64_t b0 = (uint64_t)blockIdx.x * kCuWindow; b0 < lim;
         b0 += (uint64_t)gridDim.x * kCuWindow) {
        const uint64_t b1 = b0 + kCuWindow < lim ? b0 + kCuWindow : lim;
#pragma unroll
        for (int v = 0; v < kCuWindowVec; ++v)
            reinterpret_cast<uint4*>(W)[t + v * kFrBlock] = make_uint4(0, 0, 0, 0);
        const uint64_t lo = holder(frame_off, n_items, 0, b0, t);  // the item holding byte b0
        for (uint64_t c0 = lo;; c0 += kFrBlock) {
            const uint64_t i = c0 + t;
            uint32_t np = 0;
            uint64_t fs = 0, fe = 0;
            if (i < n_items) {
                fs = frame_off[i];
                fe = frame_off[i + 1];
            }
            if (fe > fs && fs < b1 && fe > b0) {
                const auto f = pol.frame(i, nullptr);  // (the sizes kernel raised the errors)
                Piece p;
                p.start = (int64_t)fs - (int64_t)b0;
                p.n = f.n;
                p.m = f.m;
                p.head = f.head;
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
                if (P::kLog && f.m) {
                    const LogView v = log_view(pol.log_off(), pol.log().lcoff, f.lo, f.m, f.L0,
                                               cs + 17ull * f.n + varint_len(f.m), fe, b0, b1);
                    p.i0 = v.i0;
                    p.lcmd0 = v.lcmd0;
                    p.c_inst = v.c_inst;
                    p.c_log = v.c_log;
                }
                fi[t] = p;
                np = 1u + p.c_new + p.c_inst + p.c_log;
            }
            const uint32_t pieces = piece_scan(np, poff, wtot, t);
            for (uint32_t p = t; p < pieces; p += kFrBlock) {
                const uint32_t fa = piece_item(poff, p);
                const Piece& F = fi[fa];
                uint32_t k = p - poff[fa];
                const uint32_t vn = varint_len(F.n);
                const int64_t cs = F.start + kHead + vn;
                if (k == 0) {  // the head and V(n); with a log, V(m) behind the commands
                    uint32_t h[6] = {0u, 0u, 0u, 0u, 0u, 0u};
                    pol.put_head(h, F.head);
                    // V(n) behind the head: at most 5 bytes, shifted as one 64-bit word (no
                    // indexed store into h: it stays in registers)
                    const uint64_t vw = varint_word(F.n, vn) << (8 * (kHead & 3));
                    h[kHead >> 2] |= (uint32_t)vw;
                    h[(kHead >> 2) + 1] |= (uint32_t)(vw >> 32);
                    image_or<kCuWords>(W, F.start, h, kHead + vn);
                    if (P::kLog) {
                        const uint32_t vm = varint_len(F.m);
                        const uint64_t mw = varint_word(F.m, vm);
                        const uint32_t v[2] = {(uint32_t)mw, (uint32_t)(mw >> 32)};
                        image_or<kCuWords>(W, cs + 17ll * F.n, v, vm);
                    }
                    continue;
                }
                --k;
                if (k < F.c_new) {  // one of the frame's own commands
                    const Cmd3 c = pol.cmd(F.cmd0 + k);
                    image_or_cmd<kCuWords>(W, cs + 17ll * (F.j0 + k), c.op, c.key, c.val);
                    continue;
                }
                if (!P::kLog) continue;
                k -= F.c_new;
                // the CatchUpLog starts at ls; a record's bytes sit at ls + log_off[i] - L0
                const int64_t ls = cs + 17ll * F.n + varint_len(F.m);
                const uint64_t* const lcoff = pol.log().lcoff;
                if (k < F.c_inst) {  // a log record's header: Ballot, Status, V(len(Cmds))
                    const uint64_t r = F.i0 + k;
                    const LogRec m = pol.log().record(r, err);
                    const uint64_t nc = lcoff[r + 1] - lcoff[r];
                    const uint32_t vk = varint_len(nc);
                    const uint64_t kw = varint_word(nc, vk);
                    const uint32_t h[5] = {(uint32_t)m.ballot, (uint32_t)m.status, (uint32_t)kw,
                                           (uint32_t)(kw >> 32), 0u};
                    image_or<kCuWords>(W, ls + (int64_t)(pol.log_off()[r] - F.L0), h, 8 + vk);
                    continue;
                }
                k -= F.c_inst;
                {  // a log command: its record is the last of the window's with lcoff <= j
                    const uint64_t j = F.lcmd0 + k;
                    uint64_t ra = F.i0, rb = F.i0 + F.c_inst;
                    while (rb - ra > 1) {
                        const uint64_t mid = (ra + rb) >> 1;
                        if (lcoff[mid] <= j) ra = mid; else rb = mid;
                    }
                    const uint64_t c0r = lcoff[ra], c1r = lcoff[ra + 1];
                    const uint64_t csr = pol.log_off()[ra + 1] - 17 * (c1r - c0r);
                    const Cmd3 c = pol.log().cmd(ra, j - c0r, j);
                    image_or_cmd<kCuWords>(W, ls + (int64_t)(csr - F.L0) + 17ll * (int64_t)(j - c0r),
                                           c.op, c.key, c.val);
                }
            }
            const uint64_t nx = c0 + kFrBlock;
            if (nx >= n_items || frame_off[nx] >= b1) break;  // (uniform)
            __syncthreads();  // fi and poff are rewritten by the next chunk
        }
        __syncthreads();
        window_store(W, (uint32_t)(b1 - b0), out + b0, t);
        __syncthreads();  // the next window zeroes W
    }
}

// ---- Accept frames ---------------------------------------------------------------------------------
// the device's view of an Accept call: the sends and their commands, then the log and its offsets
struct AcceptSends {
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
};
template <class Log>
struct AcceptArgs {
    AcceptSends s;
    Log log;
    const uint64_t* log_off;  // scratch: log_off[i] = catch-up bytes of window records [0, i)
    uint32_t nrep, thrifty, alive;
};
struct AcceptHead {
    int32_t leader, inst, ballot, lc;
};

// is q one of the group's destinations (bcastAccept's ring walk from self)?
template <int MODE>
__device__ __forceinline__ bool accept_is_dest(uint32_t q, uint32_t self, uint32_t N,
                                               uint32_t thrifty, uint32_t alive) {
    if (q == self) return false;
    const uint32_t want = thrifty ? N >> 1 : N - 1;
    uint32_t before;
    const uint32_t p = ring_pos(q, self, N, alive, before);
    if (MODE == MPX_MODE_MIN) return p < want;  // a dead peer is reconnected and counted (:476-482)
    return before != kRingDead && before < want;  // CLASSIC (:323-327): dead peers are passed over
}

// frame of send s to destination q: MIN minpaxosprotomarsh.go:425-468 with peer q's CatchUpLog the
// group's instances lo .. LastCommitted (bareminpaxos.go:496-506); CLASSIC paxosprotomarsh.go:214-242
template <int MODE, class Log>
__device__ __forceinline__ CuFrame<AcceptHead> accept_frame(const AcceptArgs<Log>& a, uint64_t item,
                                                            uint32_t* err) {
    const AcceptSends& c = a.s;
    CuFrame<AcceptHead> f;
    f.bytes = 0;
    const uint64_t q = item / c.n_sends, s = item - q * c.n_sends;
    const int4 s0 = reinterpret_cast<const int4*>(c.sends + s)[0];
    if (!((uint32_t)s0.w & MPX_PH_ACCEPT)) return f;
    const int4 s1 = reinterpret_cast<const int4*>(c.sends + s)[1];
    const int64_t idx = (int64_t)s0.x - c.base;
    if (idx < 0 || (uint64_t)idx >= c.n_inst) {
        raise_err(err, kErrNil);
        return f;
    }
    const uint64_t g = (uint64_t)idx / c.ipg;
    const int32_t self = c.groups[g].self_id;
    if (self < 0 || (uint32_t)self >= a.nrep) {
        raise_err(err, kErrBadId);
        return f;
    }
    if (!accept_is_dest<MODE>((uint32_t)q, (uint32_t)self, a.nrep, a.thrifty, a.alive)) return f;
    f.n = (uint32_t)s1.z;
    f.m = 0;
    f.first_cmd = (uint64_t)(uint32_t)s1.x | ((uint64_t)(uint32_t)s1.y << 32);
    f.head.leader = self;
    f.head.inst = s0.x;
    f.head.ballot = s0.y;
    f.head.lc = s0.z;
    f.lo = 0;
    f.L0 = 0;
    const uint32_t vn = varint_len(f.n);
    if (MODE != MPX_MODE_MIN) {
        f.bytes = 13ull + vn + 17ull * f.n;
        return f;
    }
    const int64_t first = (int64_t)(g * c.ipg), lc = (int64_t)s0.z - c.base;
    if (lc < first - 1 || lc >= idx) {
        raise_err(err, kErrInval);
        return f;
    }
    const int64_t pc = (int64_t)c.peer_commits[g * a.nrep + q] - c.base;
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

// the Accept encoders' policy: the code byte 9, LeaderId, Instance, Ballot, MIN: LastCommitted
template <int MODE, class Log>
struct AcceptPolicy {
    static constexpr bool kLog = MODE == MPX_MODE_MIN;
    static constexpr uint32_t kHead = kLog ? 17u : 13u;
    using Head = AcceptHead;
    const AcceptArgs<Log>& a;
    __device__ __forceinline__ const uint64_t* log_off() const { return a.log_off; }
    __device__ __forceinline__ const Log& log() const { return a.log; }
    __device__ __forceinline__ CuFrame<Head> frame(uint64_t item, uint32_t* err) const {
        return accept_frame<MODE>(a, item, err);
    }
    __device__ __forceinline__ void put_head(uint32_t (&h)[6], const Head& F) const {
        h[0] = MPX_PEER_ACCEPT;
        put32(h, 1, (uint32_t)F.leader);
        put32(h, 5, (uint32_t)F.inst);
        put32(h, 9, (uint32_t)F.ballot);
        if (kLog) put32(h, 13, (uint32_t)F.lc);
    }
    __device__ __forceinline__ Cmd3 cmd(uint64_t j) const {
        return {a.s.op[j], (uint64_t)a.s.key[j], (uint64_t)a.s.val[j]};
    }
};

// ---- scratch and launches --------------------------------------------------------------------------
struct CatchupWork {
    uint64_t* log_off;    // n_inst + 1
    uint64_t* lcoff;      // n_inst + 1 where the log is the store's (no region otherwise)
    uint64_t* frame_off;  // n_dest * n + 1
    uint64_t* scan_tmp;   // for the largest of the scans
    CatchupWork(Carver& c, uint32_t n_dest, uint64_t n, uint64_t n_inst, bool store_log) {
        const uint64_t items = (uint64_t)n_dest * n;
        log_off = c.take<uint64_t>(n_inst + 1);
        lcoff = store_log ? c.take<uint64_t>(n_inst + 1) : nullptr;
        frame_off = c.take<uint64_t>(items + 1);
        const uint64_t big = items > n_inst ? items : n_inst;
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(big ? big : 1));
    }
};

// the store's two scans: lcoff (the commands a slot marshals), then log_off (the slots'
// Instance.Marshal sizes): two scans, not one over a 16-byte pair: scan.hpp's lanes exchange items
// as one 64-bit shuffle and its sum tiles keep 4 x 1088 items in LDS, 68 KB for a pair
// (a template, so that only the units that call it instantiate its scans)
template <class St>
hipError_t store_log_offsets(const St* st, const mpx_inst_cmds* inst,
                                    uint64_t n_src, uint64_t n_inst, const CatchupWork& w,
                                    hipStream_t stream) {
    const hipError_t r = device_scan(StoreCmdCount{st, inst, n_src}, OffsetsOut{w.lcoff}, n_inst,
                                     ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    return device_scan(LogRecBytes{w.lcoff}, OffsetsOut{w.log_off}, n_inst, ScanSum64{}, (uint64_t)0,
                       w.scan_tmp, stream);
}

// the launches behind the log's offsets: the sizes kernel (they land in frame_off), the
// destination-major scan in place (frame_off[] and dest_off[] of n slots per destination), then a
// workgroup per output window, kCuGrid at most
template <class Args>
hipError_t catchup_run(void (*sizes)(Args, uint64_t, uint64_t*, uint32_t*),
                       void (*emit)(Args, const uint64_t*, uint64_t, uint8_t*, uint64_t, uint32_t*),
                       const Args& a, const CatchupWork& w, uint64_t n, uint64_t items, uint8_t* out,
                       uint64_t out_cap, uint64_t* dest_off, uint32_t* err, hipStream_t stream) {
    sizes<<<(unsigned)((items + kFrBlock - 1) / kFrBlock), kFrBlock, 0, stream>>>(a, items,
                                                                                   w.frame_off, err);
    const hipError_t r = device_scan(SizeIn{w.frame_off}, FrameOffOut{w.frame_off, dest_off, n, items},
                                     items, ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    const uint64_t windows = (out_cap + kCuWindow - 1) / kCuWindow;
    if (!windows) return hipSuccess;
    const unsigned grid = (unsigned)(windows < (uint64_t)kCuGrid ? windows : (uint64_t)kCuGrid);
    emit<<<grid, kFrBlock, 0, stream>>>(a, w.frame_off, items, out, out_cap, err);
    return hipGetLastError();
}

}  // namespace mpx

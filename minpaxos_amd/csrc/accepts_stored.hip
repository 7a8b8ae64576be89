// accepts_stored.hip — MIN's Accept bytes with the CatchUpLog read from the instance store.
//
// mpx_encode_accepts_stored: the frames of proposer.hip's mpx_encode_accepts (bcastAccept ->
// SendMsg -> Accept.Marshal, minpaxosprotomarsh.go:425-468), byte for byte, where the catch-up
// log is not a dense window-ordered copy but the state the turn already keeps on the device: the
// acceptor window st (ballot, status), the leader bookkeeping window lb (status once the tally has
// committed) and mpx_inst_cmds {first_cmd, n_cmds, flags} per slot pointing into the append-only
// command arena, where ranges lie in batch order, may be dead, and may be shared by two slots.
// The dense encoder's prefix sums stay, as scratch:
//   1. a scan (scan.hpp) of every window slot's command count: the synthetic lcoff[]. A slot counts
//      no commands when it is unflagged (Cmds == nil marshals as V(0), :117-123), nil, or its range
//      leaves the arena, so the sizes and the emitted bytes agree and no load leaves [0, n_src)
//   2. a scan of the slots' encoded sizes 8 + V(nc) + 17 nc from lcoff: log_off[]
//      (two scans, not one over a 16-byte pair: scan.hpp's lanes exchange items as one 64-bit
//      shuffle and its sum tiles keep 4 x 1088 items in LDS, 68 KB for a pair)
//   3. k_as_sizes / the frame scan / k_as_emit: proposer.hip's sizing, window search and piece
//      dealing over those two arrays. Only the last step differs: a catch-up command piece
//      (record ra, position x) is loaded from src[inst[ra].first_cmd + x], and a record's header
//      takes its ballot from st and its status from lb where lb has one, else from st.
// Nothing is materialised: no gathered copy of a catch-up run exists at any point.
// CLASSIC frames carry no log: the launcher hands them to launch_encode_accepts.
// The steps are frames.hpp's, as in proposer.hip; here: the store's frame layout and the loop.
#include "common.hpp"
#include "frames.hpp"
#include "kernels.hpp"
#include "scan.hpp"

namespace mpx {

namespace {
constexpr int kAsBlock = kFrBlock;
constexpr int kAsWaves = kAsBlock / kWave;
constexpr int kAsWindowVec = 2;  // 16-byte vectors per thread in one output window
constexpr int kAsWindow = kAsBlock * 16 * kAsWindowVec;  // bytes of one output window
constexpr int kAsWords = kAsWindow / 4;               // ... as the dwords of its LDS image
constexpr int kAsGrid = 8192;             // workgroups at most (windows are walked grid-stride)
constexpr uint32_t kAsHead = 17u;         // the code byte, LeaderId, Instance, Ballot, LastCommitted

// the device's view of a call
struct AsArgs {
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
    const mpx_acceptor_state* st;
    const mpx_inst_state* lb;
    const mpx_inst_cmds* inst;
    const uint8_t* sop;
    const int64_t* skey;
    const int64_t* sval;
    uint64_t n_src;
    const uint64_t* lcoff;    // scratch: lcoff[i] = commands marshalled for window records [0, i)
    const uint64_t* log_off;  // scratch: log_off[i] = catch-up bytes of window records [0, i)
    uint32_t nrep, thrifty, alive;
};

// a slot's Cmds as the store names them
struct AsCmds {
    uint64_t first;
    uint32_t n, flags;
    __device__ __forceinline__ bool in_arena(uint64_t n_src) const {
        return first <= n_src && n <= n_src - first;
    }
};
__device__ __forceinline__ AsCmds as_cmds(const mpx_inst_cmds* inst, uint64_t i) {
    const int4 x = reinterpret_cast<const int4*>(inst)[i];
    return {(uint64_t)(uint32_t)x.x | ((uint64_t)(uint32_t)x.y << 32), (uint32_t)x.z, (uint32_t)x.w};
}

// scan 1: the commands window record i marshals (the synthetic lcoff)
struct AsCmdCount {
    const mpx_acceptor_state* st;
    const mpx_inst_cmds* inst;
    uint64_t n_src;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const AsCmds c = as_cmds(inst, i);
        const int32_t status = st[i].status;
        const bool has = (c.flags & MPX_IC_HAS_CMDS) && status != MPX_STATUS_NIL && c.in_arena(n_src);
        return has ? c.n : 0u;
    }
};
// scan 2: catch-up bytes of window record i (Instance.Marshal)
struct AsRecBytes {
    const uint64_t* coff;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const uint64_t nc = coff[i + 1] - coff[i];
        return 8u + varint_len(nc) + 17 * nc;
    }
};
// both leave n + 1 offsets, the leading zero included (no launch for it)
struct AsOffOut {
    uint64_t* off;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t s, uint64_t b) const {
        if (i == 0) off[0] = 0;
        off[i + 1] = s + b;
    }
};

// frame of send s to destination q (bytes == 0: none)
struct AsFrame {
    uint64_t bytes;
    uint64_t first_cmd;
    uint64_t lo, L0;  // first catch-up record (window index), its log_off
    uint32_t n, m;    // len(Command), len(CatchUpLog)
    int32_t leader, inst, ballot, lc;
};

__device__ __forceinline__ AsFrame as_frame(const AsArgs& a, uint64_t item, uint32_t* err) {
    AsFrame f;
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
    // bcastAccept's ring walk from self: a dead peer is reconnected and counted (:476-482)
    if ((uint32_t)q == (uint32_t)self) return f;
    uint32_t before;
    if (ring_pos((uint32_t)q, (uint32_t)self, a.nrep, a.alive, before) >=
        (a.thrifty ? a.nrep >> 1 : a.nrep - 1))
        return f;
    f.n = (uint32_t)s1.z;
    f.m = 0;
    f.first_cmd = (uint64_t)(uint32_t)s1.x | ((uint64_t)(uint32_t)s1.y << 32);
    f.leader = self;
    f.inst = s0.x;
    f.ballot = s0.y;
    f.lc = s0.z;
    f.lo = 0;
    f.L0 = 0;
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
    f.bytes = (uint64_t)kAsHead + varint_len(f.n) + 17ull * f.n + varint_len(f.m) + logb;
    return f;
}

// what a window needs of one frame, left in LDS by the item's thread for the piece threads
struct AsPiece {
    int64_t start;       // frame start - window start
    uint64_t cmd0;       // first new command overlapping the window (global index)
    uint64_t lcmd0;      // first catch-up command overlapping the window (lcoff's index)
    uint64_t L0;         // log_off of the frame's first catch-up record
    uint64_t i0;         // first catch-up record overlapping the window (window index)
    uint32_t j0;         // cmd0's position in the frame's Command slice
    uint32_t n, m;
    uint32_t c_new, c_inst, c_log;  // pieces: new commands, catch-up headers, catch-up commands
    int32_t leader, inst, ballot, lc;
};
}  // namespace

__global__ __launch_bounds__(kAsBlock) void k_as_sizes(AsArgs a, uint64_t n_items,
                                                       uint64_t* __restrict__ size, uint32_t* err) {
    const uint64_t i = (uint64_t)blockIdx.x * kAsBlock + threadIdx.x;
    if (i < n_items) size[i] = as_frame(a, i, err).bytes;
}

__global__ __launch_bounds__(kAsBlock) void k_as_emit(AsArgs a, const uint64_t* __restrict__ frame_off,
                                                      uint64_t n_items, uint8_t* __restrict__ out,
                                                      uint64_t out_cap, uint32_t* err) {
    __shared__ AsPiece fi[kAsBlock];
    __shared__ uint32_t poff[kAsBlock + 1];
    __shared__ uint32_t wtot[kAsWaves];
    __shared__ __attribute__((aligned(16))) uint32_t W[kAsWindow / 4];
    const int t = threadIdx.x;
    const uint64_t total = frame_off[n_items];
    const uint64_t lim = total < out_cap ? total : out_cap;  // nothing at or past out_cap
    for (uint64_t b0 = (uint64_t)blockIdx.x * kAsWindow; b0 < lim;
         b0 += (uint64_t)gridDim.x * kAsWindow) {
        const uint64_t b1 = b0 + kAsWindow < lim ? b0 + kAsWindow : lim;
#pragma unroll
        for (int v = 0; v < kAsWindowVec; ++v)
            reinterpret_cast<uint4*>(W)[t + v * kAsBlock] = make_uint4(0, 0, 0, 0);
        const uint64_t lo = holder(frame_off, n_items, 0, b0, t);  // the item holding byte b0
        for (uint64_t c0 = lo;; c0 += kAsBlock) {
            const uint64_t i = c0 + t;
            uint32_t np = 0;
            uint64_t fs = 0, fe = 0;
            if (i < n_items) {
                fs = frame_off[i];
                fe = frame_off[i + 1];
            }
            if (fe > fs && fs < b1 && fe > b0) {
                const AsFrame f = as_frame(a, i, nullptr);  // (k_as_sizes raised the errors)
                AsPiece p;
                p.start = (int64_t)fs - (int64_t)b0;
                p.n = f.n;
                p.m = f.m;
                p.leader = f.leader;
                p.inst = f.inst;
                p.ballot = f.ballot;
                p.lc = f.lc;
                p.L0 = f.L0;
                const uint64_t cs = fs + kAsHead + varint_len(f.n);  // the Command slice
                const CmdSpan sp = cmd_span(cs, b0, b1);
                const uint64_t jl = sp.lo, jh = sp.hi < f.n ? sp.hi : f.n;
                p.j0 = (uint32_t)jl;
                p.cmd0 = f.first_cmd + jl;
                p.c_new = jh > jl ? (uint32_t)(jh - jl) : 0u;
                p.c_inst = p.c_log = 0;
                p.i0 = 0;
                p.lcmd0 = 0;
                if (f.m) {
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
            for (uint32_t p = t; p < pieces; p += kAsBlock) {
                const uint32_t fa = piece_item(poff, p);
                const AsPiece& F = fi[fa];
                uint32_t k = p - poff[fa];
                const uint32_t vn = varint_len(F.n);
                const int64_t cs = F.start + kAsHead + vn;
                if (k == 0) {  // the header and V(n); V(m) behind the commands
                    const uint32_t ld = (uint32_t)F.leader, in = (uint32_t)F.inst;
                    const uint32_t bl = (uint32_t)F.ballot, lc = (uint32_t)F.lc;
                    uint32_t h[6] = {MPX_PEER_ACCEPT | (ld << 8), (ld >> 24) | (in << 8),
                                     (in >> 24) | (bl << 8), (bl >> 24) | (lc << 8), lc >> 24, 0u};
                    for (uint32_t x = 0; x < vn; ++x) {
                        const uint32_t at = kAsHead + x;
                        h[at >> 2] |= varint_byte(F.n, x) << (8 * (at & 3));
                    }
                    image_or<kAsWords>(W, F.start, h, kAsHead + vn);
                    const uint32_t vm = varint_len(F.m);
                    uint32_t v[2] = {0u, 0u};
                    for (uint32_t x = 0; x < vm; ++x)
                        v[x >> 2] |= varint_byte(F.m, x) << (8 * (x & 3));
                    image_or<kAsWords>(W, cs + 17ll * F.n, v, vm);
                    continue;
                }
                --k;
                if (k < F.c_new) {  // a new command
                    const uint64_t j = F.cmd0 + k;
                    image_or_cmd<kAsWords>(W, cs + 17ll * (F.j0 + k), a.op[j], (uint64_t)a.key[j],
                              (uint64_t)a.val[j]);
                    continue;
                }
                k -= F.c_new;
                // the CatchUpLog starts at ls; a record's bytes sit at ls + log_off[i] - L0
                const int64_t ls = cs + 17ll * F.n + varint_len(F.m);
                if (k < F.c_inst) {  // a catch-up record's header: Ballot, Status, V(len(Cmds))
                    const uint64_t r = F.i0 + k;
                    const int4 s = reinterpret_cast<const int4*>(a.st)[r];  // status, ballot
                    const AsCmds c = as_cmds(a.inst, r);
                    int32_t status = s.x;
                    if (a.lb) {  // the tally commits in lb alone
                        const int32_t ls_ = a.lb[r].status;
                        status = ls_ != MPX_STATUS_NIL ? ls_ : status;
                    }
                    // what the host form answers before it stages; the record is then emitted
                    // with no commands, as it was sized
                    if (s.x == MPX_STATUS_NIL) raise_err(err, kErrNil);
                    else if ((c.flags & MPX_IC_HAS_CMDS) && !c.in_arena(a.n_src))
                        raise_err(err, kErrInval);
                    const uint64_t nc = a.lcoff[r + 1] - a.lcoff[r];
                    const uint32_t vk = varint_len(nc);
                    uint32_t h[5] = {(uint32_t)s.y, (uint32_t)status, 0u, 0u, 0u};
                    for (uint32_t x = 0; x < vk; ++x)
                        h[2 + (x >> 2)] |= varint_byte(nc, x) << (8 * (x & 3));
                    image_or<kAsWords>(W, ls + (int64_t)(a.log_off[r] - F.L0), h, 8 + vk);
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
                    // lcoff counts a record's commands only where its whole range is in the
                    // arena, so first_cmd + (j - c0r) < n_src
                    const uint64_t at = a.inst[ra].first_cmd + (j - c0r);
                    image_or_cmd<kAsWords>(W, ls + (int64_t)(csr - F.L0) + 17ll * (int64_t)(j - c0r),
                              a.sop[at], (uint64_t)a.skey[at], (uint64_t)a.sval[at]);
                }
            }
            const uint64_t nx = c0 + kAsBlock;
            if (nx >= n_items || frame_off[nx] >= b1) break;  // (uniform)
            __syncthreads();  // fi and poff are rewritten by the next chunk
        }
        __syncthreads();
        window_store(W, (uint32_t)(b1 - b0), out + b0, t);
        __syncthreads();  // the next window zeroes W
    }
}

namespace {
struct AsWork {
    uint64_t* log_off;    // n_inst + 1
    uint64_t* lcoff;      // n_inst + 1
    uint64_t* frame_off;  // nrep * n_sends + 1
    uint64_t* scan_tmp;   // for the largest of the three scans
    AsWork(Carver& c, uint32_t nrep, uint64_t n_sends, uint64_t n_inst) {
        const uint64_t items = (uint64_t)nrep * n_sends;
        log_off = c.take<uint64_t>(n_inst + 1);
        lcoff = c.take<uint64_t>(n_inst + 1);
        frame_off = c.take<uint64_t>(items + 1);
        const uint64_t big = items > n_inst ? items : n_inst;
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(big ? big : 1));
    }
};
}  // namespace

uint64_t accepts_stored_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_inst, Carver&& c) {
    // (the dense encoder's regions and lcoff: a CLASSIC call runs as launch_encode_accepts in it)
    return AsWork(c, nrep, n_sends, n_inst), c.bytes();
}

hipError_t launch_encode_accepts_stored(int mode, int32_t nrep, const mpx_accept_store_batch* b,
                                        uint8_t* out, uint64_t out_cap, uint64_t* dest_off,
                                        void* work, uint64_t work_bytes, uint32_t* err,
                                        hipStream_t stream) {
    if (nrep < 1 || nrep > MPX_MAX_REPLICAS) return hipErrorInvalidValue;
    if (mode != MPX_MODE_MIN) {  // no log on CLASSIC's wire: the dense encoder's frames
        mpx_accept_batch d{};
        d.sends = b->sends;
        d.n_sends = b->n_sends;
        d.inst_base = b->inst_base;
        d.ipg = b->ipg;
        d.n_groups = b->n_groups;
        d.groups = b->groups;
        d.peer_commits = b->peer_commits;
        d.cmd_op = b->cmd_op;
        d.cmd_key = b->cmd_key;
        d.cmd_val = b->cmd_val;
        d.n_cmds = b->n_cmds;
        d.flags = b->flags;
        d.alive_mask = b->alive_mask;
        return launch_encode_accepts(mode, nrep, &d, out, out_cap, dest_off, work, work_bytes, err,
                                     stream);
    }
    const uint64_t n_inst = (uint64_t)b->n_groups * b->ipg;
    const uint64_t items = (uint64_t)nrep * b->n_sends;
    if (b->n_sends >= (1ull << 32) || n_inst > (1ull << 32)) return hipErrorInvalidValue;
    if (items == 0) {
        k_zero_u64<<<1, 64, 0, stream>>>(dest_off, (uint32_t)nrep + 1);
        return hipGetLastError();
    }
    Carver c(work);
    const AsWork w(c, (uint32_t)nrep, b->n_sends, n_inst);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    AsArgs a;
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
    a.st = b->st;
    a.lb = b->lb;
    a.inst = b->inst;
    a.sop = b->src_op;
    a.skey = b->src_key;
    a.sval = b->src_val;
    a.n_src = b->n_src;
    a.lcoff = w.lcoff;
    a.log_off = w.log_off;
    a.nrep = (uint32_t)nrep;
    a.thrifty = (b->flags & MPX_AB_THRIFTY) ? 1u : 0u;
    a.alive = b->alive_mask;
    hipError_t r = device_scan(AsCmdCount{b->st, b->inst, b->n_src}, AsOffOut{w.lcoff}, n_inst,
                               ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    r = device_scan(AsRecBytes{w.lcoff}, AsOffOut{w.log_off}, n_inst, ScanSum64{}, (uint64_t)0,
                    w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    k_as_sizes<<<(unsigned)((items + kAsBlock - 1) / kAsBlock), kAsBlock, 0, stream>>>(
        a, items, w.frame_off, err);
    r = device_scan(SizeIn{w.frame_off}, FrameOffOut{w.frame_off, dest_off, a.n_sends, items}, items,
                    ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    const uint64_t windows = (out_cap + kAsWindow - 1) / kAsWindow;
    if (!windows) return hipSuccess;
    const unsigned grid = (unsigned)(windows < (uint64_t)kAsGrid ? windows : (uint64_t)kAsGrid);
    k_as_emit<<<grid, kAsBlock, 0, stream>>>(a, w.frame_off, items, out, out_cap, err);
    return hipGetLastError();
}

}  // namespace mpx

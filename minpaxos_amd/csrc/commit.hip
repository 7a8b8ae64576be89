// commit.hip — the commit side of Phase 2: batched handleCommit / handleCommitShort with
// committedUpTo, the CommitShort / Commit bytes of bcastCommit, and received CommitShort bodies
// as records. The two protocols share the handlers and the wire formats: no mode template.
//
// k_commit_handle: tile_walk (tile.hpp) hands every lane one instance and its messages in arrival
// order, with the speculative state preload and the round counter of tile.hpp (TileState) that
// k_accept_handle uses; the lane applies
//   handleCommit       bareminpaxos.go:856-883 / paxos.go:522-549
//   handleCommitShort  bareminpaxos.go:885-910 / paxos.go:551-575
// to each with the instance in registers: a nil instance is installed COMMITTED at the message's
// ballot (a CommitShort leaves Cmds nil: MPX_VALUE_KEEP), a non-nil one takes status and ballot
// (a Commit also the value) and hands back its clientProposals. No ballot is compared. The
// per-message outputs (effect, and the durable-log record when asked for) take the records' places
// in the LDS tile and leave as coalesced stores; the owner of an overhang answers it straight to
// global memory. The state is stored only for instances that have messages.
//
// k_commit_prefix, behind it on the stream: updateCommittedUpTo (paxos.go:259-264) once per group
// over the states the batch left. Inside a commit-only batch statuses only move to COMMITTED, so
// the watermark after the last message equals one advance over the final statuses. A wave per
// group: a 64-ary search of the sorted msgs decides whether the group has a message (no scratch,
// no touched flags, no memset), then the statuses from c + 1 in chunks of 64, one ballot and a
// find-first per chunk.
//
// mpx_encode_commits: what bcastCommit -> SendMsg writes to every peer connection, built from the
// steps of frames.hpp that the proposer encoder uses (ring_pos, SizeIn / FrameOffOut, holder,
// cmd_span, piece_scan / piece_item, image_or / image_or_cmd):
//   1. k_ce_sizes, a thread per (destination q, send s): the frame's size (0 where q gets nothing)
//   2. a destination-major scan of the sizes in place: frame_off[] and dest_off[]
//   3. k_ce_emit: a workgroup per 8 KB output window deals out the pieces (a header, a command) of
//      the frames that overlap it; the LDS image is laid out at the output's 16-byte phase, so the
//      inside leaves as 16-byte stores whatever the output's address, the two ends bytewise
//      (its own store-out: window_store of frames.hpp is the aligned-or-bytewise form).
// Not thrifty, every frame is a 17-byte CommitShort and the call takes a send-major path of its
// own (k_cs_count, a scan of the per-tile counts, k_cs_emit: frames.hpp's partition steps, as in
// the AcceptReply encoder), which keeps no per-(destination, send) array.
//
// mpx_gather_commit_shorts: one scan (scan.hpp) of the code-11 flags of mpx_decode_stream's
// mpx_peer_frame list whose output step is the gather: the 16 body bytes at offset + 1 from the
// two enclosing aligned vectors.
#include "common.hpp"
#include "frames.hpp"
#include "kernels.hpp"
#include "scan.hpp"
#include "tile.hpp"

namespace mpx {

// ---- the handlers ---------------------------------------------------------------------------------
// handleCommit / handleCommitShort on the instance st = {status, ballot, value_id, flags} with
// message m = {instance, ballot, leader_id, value_id}; returns MPX_CH_*
__device__ __forceinline__ uint32_t ch_step(int4& st, int4 m) {
    const bool full = (uint32_t)m.w != MPX_VALUE_KEEP;
    uint32_t eff = full ? MPX_CH_CMDS : 0u;
    if (st.x == MPX_STATUS_NIL) {  // :861-866 / :890-895 (a CommitShort's Cmds are nil: KEEP)
        st = make_int4(MPX_COMMITTED, m.y, m.w, 0);
        return eff | MPX_CH_INSTALLED;
    }
    st.x = MPX_COMMITTED;  // :868-870 / :897-898
    st.y = m.y;
    if (full) st.z = m.w;
    if ((uint32_t)st.w & MPX_PF_HAS_PROPOSALS) {  // :871-876 / :899-904
        st.w = (int32_t)(((uint32_t)st.w & ~MPX_PF_HAS_PROPOSALS) | MPX_PF_REQUEUED);
        eff |= MPX_CH_REQUEUE;
    }
    return eff;
}

__global__ __launch_bounds__(kTileBlock) void k_commit_handle(
    const mpx_accept_msg* __restrict__ msgs, uint64_t n, mpx_acceptor_state* st, uint64_t n_inst,
    int32_t base, uint8_t* __restrict__ effect, mpx_log_rec* __restrict__ log_recs, uint32_t* err) {
    __shared__ TileLds S;
    __shared__ __attribute__((aligned(4))) uint8_t s_eff[kTileRecs];
    const int t = threadIdx.x;
    uint32_t ebits = 0;
    const int4* m4 = reinterpret_cast<const int4*>(msgs);
    int4* s4 = reinterpret_cast<int4*>(st);
    int4* log4 = reinterpret_cast<int4*>(log_recs);
    TileState ts;
    auto pre = [&](int32_t inst0) { ts.preload(s4, inst0, base, n_inst, t); };
    tile_walk(S, m4, n, err, pre, [&](uint32_t a, uint32_t cnt, uint64_t after, uint64_t oend,
                                      bool own, int64_t, bool) {
        const int32_t inst = own ? S.rec[a].x : 0;
        const int64_t idx = (int64_t)inst - base;
        const bool inwin = own && idx >= 0 && (uint64_t)idx < n_inst;
        ebits |= (own && !inwin) ? kErrNil : 0u;  // outside instanceSpace
        int4 cur = ts.take(s4, inwin, idx);
        // the tile part: the durable-log record takes the message's place in the LDS tile
        for (uint32_t j = 0; j < cnt; ++j) {
            const int4 m = S.rec[a + j];
            const uint32_t eff = inwin ? ch_step(cur, m) : 0u;
            S.rec[a + j] = make_int4(m.y, MPX_COMMITTED, m.x, 0);
            s_eff[a + j] = (uint8_t)eff;
        }
        // the overhang of the tile's last instance (one lane per tile): past the tile, so the
        // lane stores these itself
        for (uint64_t q = after; own && q < oend; ++q) {
            const int4 m = over_rec(S, m4, after, q);
            const uint32_t eff = inwin ? ch_step(cur, m) : 0u;
            if (log4) st_stream(log4 + q, make_int4(m.y, MPX_COMMITTED, m.x, 0));
            effect[q] = (uint8_t)eff;
        }
        if (inwin) st_stream(s4 + idx, cur);
        // after the tile's last round: the tile's outputs [first head, end), coalesced
        if (!ts.last_round(S)) return;
        __syncthreads();
        const uint64_t p0 = ((after - 1) / kTileRecs) * kTileRecs;
        const uint32_t end = (uint32_t)(after - p0), h0 = S.hpos[0];
        if (log4) {
#pragma unroll
            for (int k = 0; k < kTilePer; ++k) {
                const uint32_t p = t + k * kTileBlock;
                if (p >= h0 && p < end) st_stream(log4 + p0 + p, S.rec[p]);
            }
        }
        // effect bytes: whole dwords where the destination is dword aligned, else bytes
        const uint32_t p = 4u * t;
        if ((((uintptr_t)(effect + p0)) & 3u) == 0 && p >= h0 && p + 4 <= end) {
            *reinterpret_cast<uint32_t*>(effect + p0 + p) =
                *reinterpret_cast<const uint32_t*>(s_eff + p);
        } else {
#pragma unroll
            for (uint32_t q = p; q < p + 4; ++q)
                if (q >= h0 && q < end) effect[p0 + q] = s_eff[q];
        }
    });
    if (ebits) raise_err(err, ebits);
}

namespace {
constexpr int kCpBlock = 256;
constexpr int kCpWaves = kCpBlock / kWave;  // groups per workgroup
}  // namespace

// updateCommittedUpTo for the groups that have a message: a wave per group
__global__ __launch_bounds__(kCpBlock) void k_commit_prefix(
    const mpx_accept_msg* __restrict__ msgs, uint64_t n, const mpx_acceptor_state* __restrict__ st,
    int32_t base, uint32_t ipg, uint64_t n_groups, int32_t* __restrict__ committed, uint32_t* err) {
    const int l = lane_id();
    const uint64_t g = (uint64_t)blockIdx.x * kCpWaves + threadIdx.x / kWave;
    if (g >= n_groups) return;  // (wave-uniform)
    const int64_t first = (int64_t)base + (int64_t)(g * ipg), end = first + ipg;
    // the first message at or after first_g: 64 evenly spaced probes per round; the answer stays in
    // [L, R], every value below is wave-uniform
    uint64_t L = 0, R = n;
    while (L < R) {
        const uint64_t step = (R - L + kWave - 1) / kWave;
        const uint64_t p = L + (uint64_t)l * step;
        const bool below = p < R && (int64_t)msgs[p].instance < first;
        const uint64_t c = (uint64_t)popc(ballot(below));
        if (!c) break;  // msgs[L] is it
        const uint64_t nr = L + c * step;
        L += (c - 1) * step + 1;
        R = nr < R ? nr : R;
    }
    if (L >= n || (int64_t)msgs[L].instance >= end) return;  // no message: the group keeps its value
    int64_t c = committed[g];
    if (c < first - 1 || c > end - 1) {
        if (l == 0) raise_err(err, kErrInval);
        return;
    }
    for (;;) {
        const int64_t i = c + 1 + l;
        const bool ok = i < end && st[i - base].status == MPX_COMMITTED;
        const uint64_t stop = ballot(!ok);
        if (stop) {
            c += lo_bit(stop);
            break;
        }
        c += kWave;
    }
    if (l == 0) committed[g] = (int32_t)c;
}

hipError_t launch_commit_handle(const mpx_accept_msg* msgs, uint64_t n, mpx_acceptor_state* st,
                                uint64_t n_inst, int32_t base, int32_t* committed_upto,
                                uint64_t n_groups, uint32_t ipg, uint8_t* effect,
                                mpx_log_rec* log_recs, uint32_t* err, hipStream_t stream) {
    if (n == 0) return hipSuccess;  // no message: no output slot, no instance or group touched
    if (!ipg || n_groups * (uint64_t)ipg != n_inst || n_inst > (1ull << 32))
        return hipErrorInvalidValue;
    const uint64_t tiles = (n + kTileRecs - 1) / kTileRecs;
    const uint32_t grid = resident_grid((const void*)k_commit_handle, kTileBlock, tiles);
    k_commit_handle<<<grid, kTileBlock, 0, stream>>>(msgs, n, st, n_inst, base, effect, log_recs,
                                                     err);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    k_commit_prefix<<<(unsigned)((n_groups + kCpWaves - 1) / kCpWaves), kCpBlock, 0, stream>>>(
        msgs, n, st, base, ipg, n_groups, committed_upto, err);
    return hipGetLastError();
}

// ---- the Commit bytes -----------------------------------------------------------------------------
namespace {
constexpr int kCeBlock = kFrBlock;
constexpr int kCeWaves = kCeBlock / kWave;
constexpr int kCeWindow = 8192;            // bytes of one output window
constexpr int kCeImage = kCeWindow + 16;   // ... at the output's 16-byte phase
constexpr int kCeWords = kCeImage / 4;
constexpr int kCeGrid = 8192;              // workgroups at most (windows are walked grid-stride)
constexpr uint32_t kCeNone = 0, kCeShort = 1, kCeFull = 2;

// the device's view of a call
struct CeArgs {
    const mpx_commit_send* sends;
    uint64_t n_sends;
    int32_t base;
    uint32_t ipg;
    uint64_t n_inst;
    const mpx_proposer_group* groups;
    const uint8_t* op;
    const int64_t* key;
    const int64_t* val;
    uint64_t n_cmds;
    uint32_t nrep, thrifty, alive;
};

// frame of send s to destination q (bytes == 0: none)
struct CeFrame {
    uint64_t bytes;
    uint64_t first_cmd;
    uint32_t n, kind;
    int32_t leader, inst, ballot;
};

// what q receives from bcastCommit's two ring walks from self (:584-614 / :355-385): the first n1
// alive successors a CommitShort; thrifty, the alive successors after them a Commit (the second
// loop runs when the first did not wrap, which is when such a successor exists)
__device__ __forceinline__ uint32_t ce_kind(uint32_t q, uint32_t self, uint32_t N, uint32_t thrifty,
                                            uint32_t alive) {
    if (q == self) return kCeNone;
    const uint32_t n1 = thrifty ? N >> 1 : N - 1;
    uint32_t before;
    ring_pos(q, self, N, alive, before);
    if (before == kRingDead) return kCeNone;
    if (before < n1) return kCeShort;
    return thrifty ? kCeFull : kCeNone;
}

// send s of the call, validated (ok = false: past the end, a skipped slot, or in error - raised)
struct CeSend {
    bool ok;
    uint64_t first_cmd;
    uint32_t n;
    int32_t self, inst, ballot;
};
__device__ __forceinline__ CeSend ce_send(const CeArgs& a, uint64_t s, uint32_t* err) {
    CeSend x;
    x.ok = false;
    x.first_cmd = 0;
    x.n = 0;
    x.self = x.inst = x.ballot = 0;
    if (s >= a.n_sends) return x;
    const int4 s1 = reinterpret_cast<const int4*>(a.sends + s)[1];  // n_cmds, flags, pad
    if (!((uint32_t)s1.y & MPX_CS_SEND)) return x;
    const int4 s0 = reinterpret_cast<const int4*>(a.sends + s)[0];  // instance, ballot, first_cmd
    const int64_t idx = (int64_t)s0.x - a.base;
    x.n = (uint32_t)s1.x;
    x.first_cmd = (uint64_t)(uint32_t)s0.z | ((uint64_t)(uint32_t)s0.w << 32);
    if (idx < 0 || (uint64_t)idx >= a.n_inst || x.first_cmd > a.n_cmds ||
        x.n > a.n_cmds - x.first_cmd) {
        raise_err(err, kErrInval);
        return x;
    }
    x.self = a.groups[(uint64_t)idx / a.ipg].self_id;
    if (x.self < 0 || (uint32_t)x.self >= a.nrep) {
        raise_err(err, kErrInval);
        return x;
    }
    x.inst = s0.x;
    x.ballot = s0.y;
    x.ok = true;
    return x;
}

__device__ __forceinline__ CeFrame ce_frame(const CeArgs& a, uint64_t item, uint32_t* err) {
    CeFrame f;
    f.bytes = 0;
    f.kind = kCeNone;
    const uint64_t q = item / a.n_sends, s = item - q * a.n_sends;
    const CeSend x = ce_send(a, s, err);
    f.n = x.n;
    f.first_cmd = x.first_cmd;
    if (!x.ok) return f;
    f.kind = ce_kind((uint32_t)q, (uint32_t)x.self, a.nrep, a.thrifty, a.alive);
    f.leader = x.self;
    f.inst = x.inst;
    f.ballot = x.ballot;
    if (f.kind == kCeShort) f.bytes = MPX_COMMIT_SHORT_FRAME;
    if (f.kind == kCeFull) f.bytes = 13ull + varint_len(f.n) + 17ull * f.n;
    return f;
}

// ---- the not-thrifty case: every frame is a CommitShort ------------------------------------------
// Every alive peer but the leader gets the 17 bytes, so the call is a stable partition of the
// sends over the destinations fused with the encoding, on the partition steps of frames.hpp that
// mpx_encode_accept_replies (acceptor.hip) uses, with no per-(destination, send) array:
//   k_cs_count   a workgroup counts its tile's frames per destination into hist[dest][tile]
//   exclusive scan of hist (scan.hpp): the first frame of every (destination, tile), and dest_off
//   k_cs_emit    per destination, the tile ranks its sends (ballots: stable), encodes their frames
//                into an LDS image and copies it to its place with 16-byte stores at 16-byte
//                aligned addresses, the two ends bytewise, nothing at or past out_cap
constexpr int kCsBlock = kFrBlock;
constexpr int kCsWaves = kCsBlock / kWave;
constexpr int kCsPer = kFrPer;                // sends per lane per tile
constexpr int kCsTile = kFrTile;              // 1024 sends per tile
constexpr int kCsDest = kFrDest;
constexpr int kCsFrame = MPX_COMMIT_SHORT_FRAME;

// bit q: q receives send x's CommitShort
__device__ __forceinline__ uint32_t cs_mask(const CeArgs& a, const CeSend& x) {
    if (!x.ok) return 0u;
    return a.alive & ((1u << a.nrep) - 1u) & ~(1u << x.self);
}

struct CsHistIn {
    const uint32_t* h;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return h[i]; }
};
struct CsFirstOut {
    uint64_t* first;
    uint64_t* dest_off;
    uint64_t tiles, n;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t c) const {
        first[i] = ex;
        if (i % tiles == 0) dest_off[i / tiles] = ex * kCsFrame;
        if (i == n - 1) dest_off[n / tiles] = (ex + c) * kCsFrame;
    }
};

// what a window needs of one frame, left in LDS by the item's thread for the piece threads
struct CePiece {
    int64_t start;   // frame start - window start
    uint64_t cmd0;   // first command overlapping the window (global index)
    uint32_t j0;     // cmd0's position in the frame's Command slice
    uint32_t n, kind;
    int32_t leader, inst, ballot;
};
}  // namespace

__global__ __launch_bounds__(kCeBlock) void k_ce_sizes(CeArgs a, uint64_t n_items,
                                                       uint64_t* __restrict__ size, uint32_t* err) {
    const uint64_t i = (uint64_t)blockIdx.x * kCeBlock + threadIdx.x;
    if (i < n_items) size[i] = ce_frame(a, i, err).bytes;
}
__global__ __launch_bounds__(kCeBlock) void k_ce_emit(CeArgs a, const uint64_t* __restrict__ frame_off,
                                                      uint64_t n_items, uint8_t* __restrict__ out,
                                                      uint64_t out_cap) {
    __shared__ CePiece fi[kCeBlock];
    __shared__ uint32_t poff[kCeBlock + 1];
    __shared__ uint32_t wtot[kCeWaves];
    __shared__ __attribute__((aligned(16))) uint32_t W[kCeImage / 4];
    const int t = threadIdx.x;
    const uint64_t total = frame_off[n_items];
    const uint64_t lim = total < out_cap ? total : out_cap;  // nothing at or past out_cap
    const uint32_t ph = (uint32_t)((uintptr_t)out & 15u);    // image byte 0 is 16-byte aligned
    for (uint64_t b0 = (uint64_t)blockIdx.x * kCeWindow; b0 < lim;
         b0 += (uint64_t)gridDim.x * kCeWindow) {
        const uint64_t b1 = b0 + kCeWindow < lim ? b0 + kCeWindow : lim;
        for (int i = t; i < kCeImage / 16; i += kCeBlock)
            reinterpret_cast<uint4*>(W)[i] = make_uint4(0, 0, 0, 0);
        uint64_t c0 = holder(frame_off, n_items, 0, b0, t);
        for (;;) {
            const uint64_t i = c0 + t;
            uint32_t np = 0;
            uint64_t fs = 0, fe = 0;
            if (i < n_items) {
                fs = frame_off[i];
                fe = frame_off[i + 1];
            }
            if (fe > fs && fs < b1 && fe > b0) {
                const CeFrame f = ce_frame(a, i, nullptr);  // (k_ce_sizes raised the errors)
                CePiece p;
                p.start = (int64_t)fs - (int64_t)b0;
                p.n = f.n;
                p.kind = f.kind;
                p.leader = f.leader;
                p.inst = f.inst;
                p.ballot = f.ballot;
                p.j0 = 0;
                p.cmd0 = 0;
                uint32_t c_new = 0;
                if (f.kind == kCeFull) {
                    const uint64_t cs = fs + 13 + varint_len(f.n);  // the Command slice
                    const CmdSpan sp = cmd_span(cs, b0, b1);
                    const uint64_t jl = sp.lo, jh = sp.hi < f.n ? sp.hi : f.n;
                    p.j0 = (uint32_t)jl;
                    p.cmd0 = f.first_cmd + jl;
                    c_new = jh > jl ? (uint32_t)(jh - jl) : 0u;
                }
                fi[t] = p;
                np = 1u + c_new;
            }
            const uint32_t pieces = piece_scan(np, poff, wtot, t);
            for (uint32_t p = t; p < pieces; p += kCeBlock) {
                const uint32_t fa = piece_item(poff, p);
                const CePiece& F = fi[fa];
                const uint32_t k = p - poff[fa];
                const uint32_t ld = (uint32_t)F.leader, in = (uint32_t)F.inst;
                const uint32_t bl = (uint32_t)F.ballot;
                const int64_t at = F.start + ph;
                if (k == 0 && F.kind == kCeShort) {  // [11][LeaderId][Instance][Count][Ballot]
                    const uint32_t h[5] = {MPX_PEER_COMMIT_SHORT | (ld << 8), (ld >> 24) | (in << 8),
                                           (in >> 24) | (F.n << 8), (F.n >> 24) | (bl << 8), bl >> 24};
                    image_or<kCeWords>(W, at, h, MPX_COMMIT_SHORT_FRAME);
                } else if (k == 0) {  // [10][LeaderId][Instance][Ballot][V(n)]
                    const uint32_t vn = varint_len(F.n);
                    uint32_t h[5] = {MPX_PEER_COMMIT | (ld << 8), (ld >> 24) | (in << 8),
                                     (in >> 24) | (bl << 8), bl >> 24, 0u};
                    for (uint32_t x = 0; x < vn; ++x) {
                        const uint32_t b = 13 + x;
                        h[b >> 2] |= varint_byte(F.n, x) << (8 * (b & 3));
                    }
                    image_or<kCeWords>(W, at, h, 13 + vn);
                } else {  // a command: Op u8, K i64, V i64
                    const uint64_t j = F.cmd0 + (k - 1);
                    const uint64_t k8 = (uint64_t)a.key[j], v8 = (uint64_t)a.val[j];
                    image_or_cmd<kCeWords>(W, at + 13 + varint_len(F.n) + 17ll * (F.j0 + (k - 1)),
                                           a.op[j], k8, v8);
                }
            }
            const uint64_t nx = c0 + kCeBlock;
            if (nx >= n_items || frame_off[nx] >= b1) break;  // (uniform)
            __syncthreads();  // fi and poff are rewritten by the next chunk
            // a chunk without a byte (a destination that receives nothing is n_sends such items
            // in a row): on to the item that holds the next byte
            c0 = pieces ? nx : holder(frame_off, n_items, nx, frame_off[nx], t);
        }
        __syncthreads();
        // image bytes [lo, hi) go to out + b0 - ph + [lo, hi): whole aligned vectors inside
        const uint32_t lo = ph, hi = ph + (uint32_t)(b1 - b0);
        const uint32_t m0 = ((lo + 15u) & ~15u) < hi ? ((lo + 15u) & ~15u) : hi;
        const uint32_t m1 = (hi & ~15u) > m0 ? (hi & ~15u) : m0;
        uint8_t* dst = out + b0 - ph;
        const uint8_t* Sb = reinterpret_cast<const uint8_t*>(W);
        for (uint32_t i = m0 / 16 + t; i < m1 / 16; i += kCeBlock)
            st_stream(reinterpret_cast<uint4*>(dst) + i, reinterpret_cast<const uint4*>(W)[i]);
        if (lo + t < m0) dst[lo + t] = Sb[lo + t];
        if (t >= 32 && m1 + (t - 32) < hi) dst[m1 + (t - 32)] = Sb[m1 + (t - 32)];
        __syncthreads();  // the next window zeroes W
    }
}

__global__ __launch_bounds__(kCsBlock) void k_cs_count(CeArgs a, uint64_t tiles,
                                                       uint32_t* __restrict__ hist, uint32_t* err) {
    __shared__ uint32_t cnt[kCsDest];
    const int t = threadIdx.x, l = lane_id();
    dest_count_begin(cnt, t);
    const uint64_t p0 = (uint64_t)blockIdx.x * kCsTile;
    uint32_t mine = 0;  // lane q < N: frames of the wave to destination q
#pragma unroll
    for (int k = 0; k < kCsPer; ++k)
        mine = dest_count_wave<kDestMask>(
            mine, cs_mask(a, ce_send(a, p0 + k * kCsBlock + t, err)), a.nrep, l);
    dest_count_end(cnt, mine, a.nrep, tiles, hist, t, l);
}

__global__ __launch_bounds__(kCsBlock) void k_cs_emit(CeArgs a, uint64_t tiles,
                                                      const uint64_t* __restrict__ first,
                                                      uint8_t* __restrict__ out, uint64_t out_cap) {
    // one destination's frames of the tile; 16 spare bytes for the last chunk's shifted reads
    __shared__ __attribute__((aligned(16))) uint8_t img[kCsTile * kCsFrame + 16];
    __shared__ uint16_t wc[kFrUnits][kCsDest];  // per (k, wave) unit: count, then exclusive prefix
    __shared__ uint32_t tot[kCsDest];           // the tile's frames per destination
    const int t = threadIdx.x, l = lane_id(), w = t / kWave;
    const uint64_t p0 = (uint64_t)blockIdx.x * kCsTile;
    uint32_t m[kCsPer];
    CeSend x[kCsPer];
#pragma unroll
    for (int k = 0; k < kCsPer; ++k) {
        x[k] = ce_send(a, p0 + k * kCsBlock + t, nullptr);  // (k_cs_count raised the errors)
        m[k] = cs_mask(a, x[k]);
        unit_count<kDestMask>(wc[k * kCsWaves + w], m[k], a.nrep, l);
    }
    __syncthreads();
    if ((uint32_t)t < a.nrep) tot[t] = unit_prefix(wc, t);
    if (t < 4) reinterpret_cast<uint32_t*>(img + kCsTile * kCsFrame)[t] = 0;
    __syncthreads();
    for (uint32_t q = 0; q < a.nrep; ++q) {
#pragma unroll
        for (int k = 0; k < kCsPer; ++k) {
            const bool on = dest_is<kDestMask>(m[k], q);
            const uint64_t mq = ballot(on);
            if (!on) continue;
            const uint32_t pos = wc[k * kCsWaves + w][q] + (uint32_t)popc(mq & lanes_below(l));
            uint8_t* h = img + pos * kCsFrame;  // [11][LeaderId][Instance][Count][Ballot]
            const uint32_t f[4] = {(uint32_t)x[k].self, (uint32_t)x[k].inst, x[k].n,
                                   (uint32_t)x[k].ballot};
            h[0] = MPX_PEER_COMMIT_SHORT;
#pragma unroll
            for (int j = 0; j < 16; ++j) h[1 + j] = (uint8_t)(f[j >> 2] >> (8 * (j & 3)));
        }
        __syncthreads();
        const uint64_t start = first[(uint64_t)q * tiles + blockIdx.x] * kCsFrame;
        uint32_t bytes = tot[q] * kCsFrame;
        if (start < out_cap && out_cap - start < bytes) bytes = (uint32_t)(out_cap - start);
        if (bytes && start < out_cap) copy_run_shifted(img, 0, bytes, out + start, t);
        __syncthreads();  // the next destination rewrites the image
    }
}

// ---- CommitShort bodies to records ----------------------------------------------------------------
namespace {
struct GsIn {  // 1 for a CommitShort frame among the first min(*d_n, n)
    const mpx_peer_frame* oth;
    const uint64_t* d_n;
    uint64_t n;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const {
        const uint64_t lim = d_n ? (*d_n < n ? *d_n : n) : n;
        return i < lim && oth[i].code == MPX_PEER_COMMIT_SHORT ? 1u : 0u;
    }
};
struct GsOut {  // the scan's output step is the gather: ex is the frame's slot
    const uint8_t* buf;
    uint64_t len;
    const mpx_peer_frame* oth;
    mpx_accept_msg* msgs;
    int32_t* count;
    uint32_t* fidx;
    uint64_t cap, n;
    uint64_t* n_shorts;
    uint32_t* err;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t ex, uint32_t item) const {
        if (i == n - 1) *n_shorts = (uint64_t)ex + item;
        if (!item || ex >= cap) return;
        const uint64_t p = (uint64_t)oth[i].offset + 1;  // LeaderId, Instance, Count, Ballot
        if (p + 16 > len) {
            raise_err(err, kErrInval);
            return;
        }
        // the two aligned vectors that enclose [p, p + 16); the second only where the body
        // reaches into it (it then starts below len)
        const uint4* v = reinterpret_cast<const uint4*>(buf + (p & ~15ull));
        const uint4 x = ld_stream(v);
        const uint4 y = (p & 15u) ? ld_stream(v + 1) : make_uint4(0, 0, 0, 0);
        const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        const uint32_t k = (uint32_t)(p & 15u) >> 2, b = (uint32_t)(p & 3u);
        uint32_t u[5];
#pragma unroll
        for (int j = 0; j < 5; ++j)
            u[j] = k == 0 ? w[j] : k == 1 ? w[j + 1] : k == 2 ? w[j + 2] : w[j + 3];
        uint32_t f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = b ? __builtin_amdgcn_alignbyte(u[j + 1], u[j], b) : u[j];
        st_stream(reinterpret_cast<int4*>(msgs) + ex,
                  make_int4((int32_t)f[1], (int32_t)f[3], (int32_t)f[0], (int32_t)MPX_VALUE_KEEP));
        count[ex] = (int32_t)f[2];
        fidx[ex] = (uint32_t)i;
    }
};

// the family's scratch
struct CmWork {
    uint64_t* frame_off;  // nrep * n_sends + 1
    uint64_t* scan_tmp;   // the encoder's scan
    uint32_t* gs_tmp;     // the gather's scan
    uint32_t* hist;       // not thrifty: frames per (destination, tile of sends)
    uint64_t* first;      // ... and the first frame of each
    CmWork(Carver& c, uint32_t nrep, uint64_t n_sends, uint64_t n_other) {
        const uint64_t items = (uint64_t)nrep * n_sends;
        const uint64_t tiles = (n_sends + kCsTile - 1) / kCsTile;
        frame_off = c.take<uint64_t>(items + 1);
        hist = c.take<uint32_t>((uint64_t)nrep * (tiles ? tiles : 1));
        first = c.take<uint64_t>((uint64_t)nrep * (tiles ? tiles : 1));
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(items ? items : 1));
        gs_tmp = (uint32_t*)c.take<char>(scan_scratch_bytes<uint32_t>(n_other ? n_other : 1));
    }
};
}  // namespace

uint64_t commits_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_other, Carver&& c) {
    return CmWork(c, nrep, n_sends, n_other), c.bytes();
}

hipError_t launch_encode_commits(int32_t nrep, const mpx_commit_batch* b, uint8_t* out,
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
    const CmWork w(c, (uint32_t)nrep, b->n_sends, 0);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    CeArgs a;
    a.sends = b->sends;
    a.n_sends = b->n_sends;
    a.base = b->inst_base;
    a.ipg = b->ipg;
    a.n_inst = n_inst;
    a.groups = b->groups;
    a.op = b->cmd_op;
    a.key = b->cmd_key;
    a.val = b->cmd_val;
    a.n_cmds = b->n_cmds;
    a.nrep = (uint32_t)nrep;
    a.thrifty = (b->flags & MPX_AB_THRIFTY) ? 1u : 0u;
    a.alive = b->alive_mask;
    if (!a.thrifty) {  // every frame is a CommitShort: send-major, no per-item array
        const uint64_t tiles = (b->n_sends + kCsTile - 1) / kCsTile;
        k_cs_count<<<(unsigned)tiles, kCsBlock, 0, stream>>>(a, tiles, w.hist, err);
        const uint64_t h = (uint64_t)nrep * tiles;
        const hipError_t r = device_scan(CsHistIn{w.hist}, CsFirstOut{w.first, dest_off, tiles, h},
                                         h, ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
        if (r != hipSuccess) return r;
        if (!out_cap) return hipSuccess;
        k_cs_emit<<<(unsigned)tiles, kCsBlock, 0, stream>>>(a, tiles, w.first, out, out_cap);
        return hipGetLastError();
    }
    k_ce_sizes<<<(unsigned)((items + kCeBlock - 1) / kCeBlock), kCeBlock, 0, stream>>>(
        a, items, w.frame_off, err);
    const hipError_t r = device_scan(SizeIn{w.frame_off},
                                     FrameOffOut{w.frame_off, dest_off, a.n_sends, items}, items,
                                     ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    const uint64_t windows = (out_cap + kCeWindow - 1) / kCeWindow;
    if (!windows) return hipSuccess;
    const unsigned grid = (unsigned)(windows < (uint64_t)kCeGrid ? windows : (uint64_t)kCeGrid);
    k_ce_emit<<<grid, kCeBlock, 0, stream>>>(a, w.frame_off, items, out, out_cap);
    return hipGetLastError();
}

hipError_t launch_gather_commit_shorts(const uint8_t* buf, uint64_t len, const mpx_peer_frame* other,
                                       uint64_t n_other, const uint64_t* d_n_other,
                                       mpx_accept_msg* msgs, int32_t* count, uint32_t* frame_index,
                                       uint64_t cap, uint64_t* n_shorts, void* work,
                                       uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    if (n_other >= (1ull << 32) || len > MPX_DECODE_MAX_BYTES) return hipErrorInvalidValue;
    if (!n_other) {
        k_zero_u64<<<1, 1, 0, stream>>>(n_shorts, 1);
        return hipGetLastError();
    }
    Carver c(work);
    const CmWork w(c, 1, 0, n_other);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    return device_scan(GsIn{other, d_n_other, n_other},
                       GsOut{buf, len, other, msgs, count, frame_index, cap, n_other, n_shorts, err},
                       n_other, ScanSum32{}, 0u, w.gs_tmp, stream);
}

}  // namespace mpx

// acceptor.hip — the acceptor's half of Phase 2: batched handleAccept and the AcceptReply bytes.
//
// k_accept_handle<MODE>: tile_walk (tile.hpp) hands every lane one instance and its Accepts in
// arrival order; the lane applies handleAccept to each with the instance in registers:
//   MIN      bareminpaxos.go:753-806: a resent Accept (ACCEPTED at the same ballot) is ignored
//            (:757-762); an Accept at r.defaultBallot installs a fresh Instance and replies
//            (:786-801); any other ballot does nothing
//   CLASSIC  paxos.go:470-520: every Accept is answered, by the five branches of :474-511
// The per-message outputs (the reply, its destination, the effect flags) are slot-aligned with
// the input. A lane puts them where its records were: the reply over the record in the LDS tile
// (each tile position belongs to exactly one lane's run, and the lane has read the record by
// then), destination and effect beside it; after the tile's last round the workgroup writes the
// tile's outputs as coalesced stores. Records at the head of a tile that continue an instance of
// an earlier tile (the overhang) are answered by the lane that owns that instance, straight to
// global memory, so a tile writes [first head, end). One launch, no scalars, no control words.
// The speculative state preload and the round counter are tile.hpp's TileState, shared with
// k_commit_handle; the wave-uniform trip count, s_to and the tile epilogue are its own.
//
// mpx_encode_accept_replies: a stable partition of the replies over at most MPX_MAX_REPLICAS
// destinations fused with the encoding of the frames replyAccept -> SendMsg writes
// (genericsmr.go:499-512): the code byte 13, then AcceptReply.Marshal
//   MIN      minpaxosprotomarsh.go:545-566  Instance i32, OK u8, Ballot i32, Id i32   (14 B)
//   CLASSIC  paxosprotomarsh.go:306-322     Instance i32, OK u8, Ballot i32          (10 B)
//   k_ar_count    a workgroup counts the destinations of its tile by wave ballots into
//                 hist[dest][tile] (destination-major)
//   exclusive scan of hist (scan.hpp): the first output frame of every (destination, tile)
//   k_ar_emit     the tile ranks its replies per destination (ballots: stable), encodes the
//                 frames into an LDS image grouped by destination, and copies every destination's
//                 run to its place with 16-byte stores at 16-byte aligned addresses (the run's two
//                 ends bytewise)
// The partition's steps (dest_count_*, unit_count, unit_prefix, copy_run_shifted) are
// frames.hpp's, shared with the CommitShort path of commit.hip; the frame encoding and the
// dest_off rule are here.
#include "common.hpp"
#include "frames.hpp"
#include "kernels.hpp"
#include "scan.hpp"
#include "tile.hpp"

namespace mpx {

// ---- the acceptor step ---------------------------------------------------------------------------
struct AhOut {              // what one Accept produced
    int4 reply;             // mpx_accept_reply, all zero when nothing was sent
    int32_t to;             // leader_id, -1 when nothing was sent
    uint32_t eff;           // MPX_AH_*
};

// handleAccept on the instance st = {status, ballot, value_id, flags} with message m =
// {instance, ballot, leader_id, value_id}; D = r.defaultBallot, self = r.Id
template <int MODE>
__device__ __forceinline__ AhOut ah_step(int4& st, int4 m, int32_t D, int32_t self) {
    AhOut o{make_int4(0, 0, 0, 0), -1, 0u};
    const int32_t b = m.y;
    if (MODE == MPX_MODE_MIN) {
        if (st.x == MPX_ACCEPTED && st.y == b) return o;  // :757-762 (nil is never ACCEPTED)
        if (D != b) return o;                             // :786
        st = make_int4(MPX_ACCEPTED, b, m.w, 0);          // :787-793
        o.reply = make_int4(m.x, b, self, 1);             // :794
        o.to = m.z;
        o.eff = MPX_AH_REPLIED | MPX_AH_STORED;
        return o;
    }
    int32_t ok, rb;
    uint32_t eff = MPX_AH_REPLIED;
    if (st.x == MPX_STATUS_NIL) {                         // :474
        ok = b < D ? 0 : 1;
        rb = D;                                           // :477 / :484
        if (ok) st = make_int4(MPX_ACCEPTED, b, m.w, 0);  // :479-483
    } else if (st.y > b) {                                // :486
        ok = 0;
        rb = st.y;
    } else if (st.y < b) {                                // :489
        st.z = m.w;
        st.y = b;
        st.x = MPX_ACCEPTED;
        ok = 1;
        rb = b;
        if ((uint32_t)st.w & MPX_PF_HAS_PROPOSALS) {      // :495-502
            st.w = (int32_t)(((uint32_t)st.w & ~MPX_PF_HAS_PROPOSALS) | MPX_PF_REQUEUED);
            eff |= MPX_AH_REQUEUE;
        }
    } else {                                              // :503 reordered ACCEPT
        st.z = m.w;
        st.x = st.x != MPX_COMMITTED ? MPX_ACCEPTED : st.x;
        ok = 1;
        rb = D;
    }
    o.reply = make_int4(m.x, rb, -1, ok);                 // the CLASSIC wire has no Id
    o.to = m.z;
    o.eff = eff | (ok ? MPX_AH_STORED : 0u);              // :513-517
    return o;
}

// 4 waves per SIMD (at most 128 VGPRs): left to itself the compiler takes 139 / 141 and runs 3.
// Same-box A/B, alternating, 2^24 single-Accept instances: 0.246-0.248 -> 0.223-0.225 ms MIN,
// 0.250 -> 0.232-0.233 ms CLASSIC (whose 8 bytes of scratch per lane cost less than the wave).
constexpr int kAcceptWpe = 4;
template <int MODE>
__global__ __attribute__((amdgpu_waves_per_eu(kAcceptWpe, kAcceptWpe)))
__launch_bounds__(kTileBlock) void k_accept_handle(
    const mpx_accept_msg* __restrict__ msgs, uint64_t n, const mpx_acceptor_state* __restrict__ st_in,
    mpx_acceptor_state* __restrict__ st_out, uint64_t n_inst, int32_t base,
    const mpx_acceptor_group* __restrict__ groups, uint32_t one_group, uint32_t ipg, int32_t nrep,
    mpx_accept_reply* __restrict__ replies, int32_t* __restrict__ reply_to,
    uint8_t* __restrict__ effect, uint32_t* err) {
    __shared__ TileLds S;
    __shared__ int32_t s_to[kTileRecs];
    __shared__ __attribute__((aligned(4))) uint8_t s_eff[kTileRecs];
    const int t = threadIdx.x;
    uint32_t ebits = 0;
    const int4* m4 = reinterpret_cast<const int4*>(msgs);
    const int4* s4 = reinterpret_cast<const int4*>(st_in);
    int4* out4 = reinterpret_cast<int4*>(replies);
    TileState ts;
    auto pre = [&](int32_t inst0) { ts.preload(s4, inst0, base, n_inst, t); };
    tile_walk(S, m4, n, err, pre, [&](uint32_t a, uint32_t cnt, uint64_t after, uint64_t oend,
                                      bool own, int64_t, bool) {
        const int32_t inst = own ? S.rec[a].x : 0;
        const int64_t idx = (int64_t)inst - base;
        const bool inwin = own && idx >= 0 && (uint64_t)idx < n_inst;
        ebits |= (own && !inwin) ? kErrNil : 0u;  // outside instanceSpace
        int2 grp = make_int2(0, 0);
        if (inwin)
            grp = *reinterpret_cast<const int2*>(groups + (one_group ? 0u : (uint32_t)idx / ipg));
        int4 st = ts.take(s4, inwin, idx);
        auto answer = [&](int4 m) {
            AhOut o{make_int4(0, 0, 0, 0), -1, 0u};
            if (inwin) o = ah_step<MODE>(st, m, grp.x, grp.y);
            // SendMsg indexes PeerWriters[LeaderId] (genericsmr.go:501)
            ebits |= ((o.eff & MPX_AH_REPLIED) && (m.z < 0 || m.z >= nrep)) ? kErrBadId : 0u;
            return o;
        };
        // the tile part: uniform trip count (wave maximum), predicated body. The reply takes the
        // record's place in the LDS tile (tile_walk's next_inst, read from a neighbour's head
        // record that may already hold a reply, is not used here).
        uint32_t rmax = cnt;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t x = (uint32_t)__shfl_xor((int)rmax, d);
            rmax = rmax > x ? rmax : x;
        }
        rmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)rmax);
        for (uint32_t j = 0; j < rmax; ++j) {
            if (j < cnt) {
                const AhOut o = answer(S.rec[a + j]);
                S.rec[a + j] = o.reply;
                s_to[a + j] = o.to;
                s_eff[a + j] = (uint8_t)o.eff;
            }
        }
        // the overhang of the tile's last instance (one lane per tile): past the tile, so the
        // lane stores these itself
        for (uint64_t q = after; own && q < oend; ++q) {
            const AhOut o = answer(over_rec(S, m4, after, q));
            st_stream(out4 + q, o.reply);
            reply_to[q] = o.to;
            effect[q] = (uint8_t)o.eff;
        }
        if (inwin) st_stream(reinterpret_cast<int4*>(st_out) + idx, st);
        // after the tile's last round: the tile's outputs [first head, end), coalesced
        if (!ts.last_round(S)) return;
        __syncthreads();
        const uint64_t p0 = ((after - 1) / kTileRecs) * kTileRecs;
        const uint32_t end = (uint32_t)(after - p0), h0 = S.hpos[0];
#pragma unroll
        for (int k = 0; k < kTilePer; ++k) {
            const uint32_t p = t + k * kTileBlock;
            if (p >= h0 && p < end) {
                st_stream(out4 + p0 + p, S.rec[p]);
                st_stream(reply_to + p0 + p, s_to[p]);
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

hipError_t launch_accept_handle(int mode, const mpx_accept_msg* msgs, uint64_t n,
                                const mpx_acceptor_state* st_in, mpx_acceptor_state* st_out,
                                uint64_t n_inst, int32_t base, const mpx_acceptor_group* groups,
                                uint64_t n_groups, uint32_t ipg, int32_t nrep,
                                mpx_accept_reply* replies, int32_t* reply_to, uint8_t* effect,
                                uint32_t* err, hipStream_t stream) {
    if (n == 0) return hipSuccess;  // no message: no output slot, no instance touched
    if (!ipg || n_groups * (uint64_t)ipg != n_inst || n_inst > (1ull << 32))
        return hipErrorInvalidValue;
    const uint64_t tiles = (n + kTileRecs - 1) / kTileRecs;
    const uint32_t one = n_groups == 1 ? 1u : 0u;
    if (mode == MPX_MODE_MIN) {
        const uint32_t grid =
            resident_grid((const void*)k_accept_handle<MPX_MODE_MIN>, kTileBlock, tiles);
        k_accept_handle<MPX_MODE_MIN><<<grid, kTileBlock, 0, stream>>>(
            msgs, n, st_in, st_out, n_inst, base, groups, one, ipg, nrep, replies, reply_to,
            effect, err);
    } else {
        const uint32_t grid =
            resident_grid((const void*)k_accept_handle<MPX_MODE_CLASSIC>, kTileBlock, tiles);
        k_accept_handle<MPX_MODE_CLASSIC><<<grid, kTileBlock, 0, stream>>>(
            msgs, n, st_in, st_out, n_inst, base, groups, one, ipg, nrep, replies, reply_to,
            effect, err);
    }
    return hipGetLastError();
}

// ---- the reply bytes -----------------------------------------------------------------------------
namespace {
constexpr int kArBlock = kFrBlock;
constexpr int kArWaves = kArBlock / kWave;           // 4
constexpr int kArPer = kFrPer;                       // replies per lane per tile
constexpr int kArTile = kFrTile;                     // 1024 replies per tile
constexpr int kArDest = kFrDest;

struct ArHistIn {
    const uint32_t* h;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return h[i]; }
};
struct ArFirstOut {
    uint32_t* first;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t ex, uint32_t) const {
        first[i] = ex;
    }
};
}  // namespace

// destination of reply p of the call: 0 .. n_dest-1, or kArDest (skipped: reply_to < 0, past the
// end, or - the call fails - >= n_dest)
__device__ __forceinline__ uint32_t ar_dest(const int32_t* __restrict__ reply_to, uint64_t n,
                                            uint64_t p, uint32_t n_dest, uint32_t* err) {
    if (p >= n) return kArDest;
    const int32_t d = ld_stream(reply_to + p);
    if (d < 0) return kArDest;
    if ((uint32_t)d >= n_dest) {
        raise_err(err, kErrInval);
        return kArDest;
    }
    return (uint32_t)d;
}

__global__ __launch_bounds__(kArBlock) void k_ar_count(const int32_t* __restrict__ reply_to,
                                                       uint64_t n, uint32_t n_dest, uint64_t tiles,
                                                       uint32_t* __restrict__ hist, uint32_t* err) {
    __shared__ uint32_t cnt[kArDest];
    const int t = threadIdx.x, l = lane_id();
    dest_count_begin(cnt, t);
    const uint64_t p0 = (uint64_t)blockIdx.x * kArTile;
    uint32_t mine = 0;  // lane d < n_dest: replies of the wave to destination d
#pragma unroll
    for (int k = 0; k < kArPer; ++k)
        mine = dest_count_wave<kDestIndex>(
            mine, ar_dest(reply_to, n, p0 + k * kArBlock + t, n_dest, err), n_dest, l);
    dest_count_end(cnt, mine, n_dest, tiles, hist, t, l);
}

template <int FRAME>
__global__ __launch_bounds__(kArBlock) void k_ar_emit(
    const mpx_accept_reply* __restrict__ replies, const int32_t* __restrict__ reply_to, uint64_t n,
    uint32_t n_dest, uint64_t tiles, const uint32_t* __restrict__ first, uint8_t* __restrict__ out,
    uint64_t* __restrict__ dest_off, uint32_t* err) {
    // the tile's frames grouped by destination; 16 spare bytes for the last run's shifted reads
    __shared__ __attribute__((aligned(16))) uint8_t img[kArTile * FRAME + 16];
    __shared__ uint16_t wc[kFrUnits][kArDest];  // per (k, wave) unit: count, then exclusive prefix
    __shared__ uint32_t tstart[kArDest + 1];    // destination's first frame in the image
    const int t = threadIdx.x, l = lane_id(), w = t / kWave;
    const uint64_t p0 = (uint64_t)blockIdx.x * kArTile;
    uint32_t dst[kArPer], lr[kArPer];
    int4 rec[kArPer];
    const int4* r4 = reinterpret_cast<const int4*>(replies);
#pragma unroll
    for (int k = 0; k < kArPer; ++k) {
        const uint64_t p = p0 + k * kArBlock + t;
        dst[k] = ar_dest(reply_to, n, p, n_dest, nullptr);  // (k_ar_count raised the error)
        rec[k] = dst[k] < kArDest ? ld_stream(r4 + p) : make_int4(0, 0, 0, 0);
    }
    // stable rank inside the (k, wave) unit, and the unit's counts
#pragma unroll
    for (int k = 0; k < kArPer; ++k) {
        const uint64_t own = unit_count<kDestIndex>(wc[k * kArWaves + w], dst[k], n_dest, l);
        lr[k] = (uint32_t)popc(own & lanes_below(l));
    }
    __syncthreads();
    if ((uint32_t)t < n_dest) tstart[t + 1] = unit_prefix(wc, t);  // the count for now
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        tstart[0] = 0;
        for (uint32_t x = 0; x < n_dest; ++x) {
            run += tstart[x + 1];
            tstart[x + 1] = run;
        }
    }
    __syncthreads();
    // encode at the frame's place in the image (frames are even-sized: 2-byte stores)
#pragma unroll
    for (int k = 0; k < kArPer; ++k) {
        if (dst[k] >= kArDest) continue;
        const uint32_t pos = tstart[dst[k]] + wc[k * kArWaves + w][dst[k]] + lr[k];
        uint16_t* h = reinterpret_cast<uint16_t*>(img + pos * FRAME);
        const uint32_t in = (uint32_t)rec[k].x, bl = (uint32_t)rec[k].y, id = (uint32_t)rec[k].z;
        const uint32_t ok = (uint32_t)rec[k].w & 0xffu;
        h[0] = (uint16_t)(MPX_PEER_ACCEPT_REPLY | (in << 8));
        h[1] = (uint16_t)(in >> 8);
        h[2] = (uint16_t)((in >> 24) | (ok << 8));
        h[3] = (uint16_t)bl;
        h[4] = (uint16_t)(bl >> 16);
        if (FRAME == MPX_ACCEPT_REPLY_FRAME_MIN) {
            h[5] = (uint16_t)id;
            h[6] = (uint16_t)(id >> 16);
        }
    }
    if (t < 4) reinterpret_cast<uint32_t*>(img + kArTile * FRAME)[t] = 0;
    __syncthreads();
    // every destination's run of the image to its place in that destination's output run
    for (uint32_t x = 0; x < n_dest; ++x) {
        const uint64_t g = first[(uint64_t)x * tiles + blockIdx.x];  // frames before the run
        const uint32_t s0 = tstart[x] * FRAME, bytes = (tstart[x + 1] - tstart[x]) * FRAME;
        if (blockIdx.x == 0 && t == 0) dest_off[x] = g * FRAME;
        if (blockIdx.x == tiles - 1 && x == n_dest - 1 && t == 0)
            dest_off[n_dest] = g * FRAME + bytes;
        if (!bytes) continue;
        copy_run_shifted(img, s0, bytes, out + g * FRAME, t);
    }
}

namespace {
struct ArWork {
    uint32_t *hist, *first, *scan_tmp;
    // (rows of kArDest whatever the call's n_dest, and a tile for an empty call)
    ArWork(Carver& c, uint64_t n) {
        const uint64_t tiles = (n + kArTile - 1) / kArTile;
        const uint64_t h = (uint64_t)kArDest * (tiles ? tiles : 1);
        hist = c.take<uint32_t>(h);
        first = c.take<uint32_t>(h);
        scan_tmp = (uint32_t*)c.take<char>(scan_scratch_bytes<uint32_t>(h));
    }
};
}  // namespace

uint64_t accept_replies_work_bytes(uint64_t n, Carver&& c) { return ArWork(c, n), c.bytes(); }

hipError_t launch_encode_accept_replies(int mode, const mpx_accept_reply* replies,
                                        const int32_t* reply_to, uint64_t n, uint32_t n_dest,
                                        uint8_t* out, uint64_t* dest_off, void* work,
                                        uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    if (!n_dest || n_dest > (uint32_t)kArDest || n >= (1ull << 32)) return hipErrorInvalidValue;
    if (n == 0) {
        k_zero_u64<<<1, 64, 0, stream>>>(dest_off, n_dest + 1);
        return hipGetLastError();
    }
    Carver c(work);
    const ArWork w(c, n);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const uint64_t tiles = (n + kArTile - 1) / kArTile;
    const uint64_t h = (uint64_t)n_dest * tiles;
    k_ar_count<<<(unsigned)tiles, kArBlock, 0, stream>>>(reply_to, n, n_dest, tiles, w.hist, err);
    const hipError_t r = device_scan(ArHistIn{w.hist}, ArFirstOut{w.first}, h, ScanSum32{}, 0u,
                                     w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    if (mode == MPX_MODE_MIN)
        k_ar_emit<MPX_ACCEPT_REPLY_FRAME_MIN><<<(unsigned)tiles, kArBlock, 0, stream>>>(
            replies, reply_to, n, n_dest, tiles, w.first, out, dest_off, err);
    else
        k_ar_emit<MPX_ACCEPT_REPLY_FRAME_CLASSIC><<<(unsigned)tiles, kArBlock, 0, stream>>>(
            replies, reply_to, n, n_dest, tiles, w.first, out, dest_off, err);
    return hipGetLastError();
}

}  // namespace mpx

// client.hip — batched client-stream framing + Propose decode over many connections.
//
// Reference: genericsmr.(*Replica).clientListener  src/genericsmr/genericsmr.go:448-490 reads one
// client connection as frames [code u8][body]: PROPOSE (0, 30 bytes with the code:
// gsmrprotomarsh.go:65-80 and statemarsh.go:21-39) is handed to ProposeChan; READ (2, 13 bytes,
// :341-350) and PROPOSE_AND_READ (4, 30 bytes, :280-292) are unmarshalled and dropped; the switch
// has no default, so any other byte is a 1-byte frame. A frame that runs past the connection's
// bytes is a partial read: the host keeps the tail.
//
// The payload bytes are mostly 0x00, which is the PROPOSE code, so nothing resynchronises by
// pattern: framing is the entry-map scheme of decode.hip, re-cut for this wire. A frame that
// starts in a 128-byte chunk ends at most 29 bytes into the next, so a chunk is a function from
// its entry state (entry offset 0..29, or DEAD: no live chain) to (exit state, proposals and
// dropped frames passed). A connection starts on a chunk boundary (MPX_CLIENT_ALIGN), so every
// chunk has at most one owner (a binary search over the ascending offsets), and a connection's
// first chunk is a constant function: it enters at 0 whatever came before, DEAD included. A chunk
// outside every connection maps everything to DEAD. With that, composition across connections
// needs no special case: a chain that stopped (a partial frame, or the connection's end) is DEAD
// until the next head, and the counts keep adding across heads, which is what gives every
// connection its `first`. Maps compose associatively: 128 chunk maps reduce to a tile map (tree
// in LDS), 128 tile maps to a group map, one block walks the group maps, the down-sweeps hand
// every tile and chunk its entry state and counts, and the chunks emit. Where a connection
// stops is found by the one chunk whose walk meets the stop. Launches: 11, whatever the connections.
#include "common.hpp"
#include "kernels.hpp"

namespace mpx {

namespace {

constexpr int kChunk = 128;                 // bytes per lane
constexpr int kTileLanes = 128;             // lanes per tile workgroup
constexpr int kTileBytes = kChunk * kTileLanes;
constexpr int kLook = 30;                   // live entry offsets 0..29
constexpr uint32_t kDeadSt = 30;            // the state of no live chain
constexpr int kStates = 31;
constexpr int kGroupTiles = 128;            // tile maps per group
constexpr uint32_t kNoConn = 0xFFFFFFFFu;
static_assert(MPX_CLIENT_ALIGN == kChunk, "a chunk has at most one owner");
static_assert(MPX_CLIENT_PROPOSE_FRAME == kLook && MPX_CLIENT_READ_FRAME == 13 &&
                  MPX_CLIENT_PROPOSE == 0 && MPX_CLIENT_READ == 2 && MPX_CLIENT_PROPOSE_AND_READ == 4,
              "the DP's look-back distances");

__device__ __forceinline__ uint32_t frame_len(uint32_t code) {
    return (code & ~4u) == 0 ? 30u : code == 2u ? 13u : 1u;
}

// a connection as the kernels use it: key = its offset, or for a faulty connection the largest
// end before it (ascending either way, so the owner search stays a binary search); len = 0 for a
// faulty one; gkey = its group, or the largest group before it
struct CConn {
    uint64_t key;
    uint32_t len, gkey;
};

// chunk-map entry (u32): [0..4] exit state, [8..10] proposals (<= 5), [16..23] dropped (<= 128)
constexpr uint32_t kCProp = 1u << 8, kCDrop = 1u << 16;
// tile-level entry (u32): [0..4] state, [5..14] proposals (<= 547), [15..29] dropped (<= 16384)
__device__ __forceinline__ uint32_t t_from_chunk(uint32_t x) {
    return (x & 31u) | (((x >> 8) & 7u) << 5) | (((x >> 16) & 0xFFu) << 15);
}
__device__ __forceinline__ uint32_t t_compose(uint32_t a, const uint32_t* b) {
    const uint32_t y = b[a & 31u];
    return (y & 31u) | (((a >> 5) + (y >> 5)) << 5);
}
// across tiles
struct GEntry {
    uint32_t st, pr, dr;
};

// the owner of the chunk at c0: the last connection with key <= c0, if c0 is inside it
__device__ __forceinline__ uint32_t find_owner(const CConn* __restrict__ sc, uint32_t n, uint64_t c0) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sc[mid].key <= c0) lo = mid + 1;
        else hi = mid;
    }
    if (!lo) return kNoConn;
    const CConn c = sc[lo - 1];
    return c0 < c.key + c.len ? lo - 1 : kNoConn;
}

// The lane's chunk -> its 30 live map entries (w[k] = entry k) by a backward DP over the chunk's
// positions: dp[p] = dp[p + len(p)] + frame p (past the chunk: the exit state). Before
// step p the window holds w[k] = dp[p+1+k]. rem: the connection's bytes from the chunk's start
// (clamped): a frame running past them is DEAD, with no count, and so is a position past them.
__device__ __forceinline__ void chunk_map_dp(const uint32_t (&wd)[kChunk / 4], uint32_t rem,
                                             uint32_t (&w)[kLook]) {
    // dp[128 + k], a frame's end k bytes into the next chunk, is the exit state k
#pragma unroll
    for (int k = 0; k < kLook; ++k) w[k] = (uint32_t)k;
#pragma unroll
    for (int p = kChunk - 1; p >= 0; --p) {
        const uint32_t code = (wd[p >> 2] >> ((p & 3) * 8)) & 0xFFu;
        const bool l30 = (code & ~4u) == 0, l13 = code == 2u;
        const uint32_t fl = l30 ? 30u : l13 ? 13u : 1u;
        // masks, not selects: a select between window slots becomes an indexed private array
        const uint32_t m30 = 0u - (uint32_t)l30, m13 = 0u - (uint32_t)l13;
        const uint32_t nx = (w[29] & m30) | (w[12] & m13) | (w[0] & ~(m30 | m13));
        uint32_t d = nx + (code == 0 ? kCProp : kCDrop);
        if ((uint32_t)p + fl > rem) d = kDeadSt;
#pragma unroll
        for (int k = kLook - 1; k > 0; --k) w[k] = w[k - 1];
        w[0] = d;
    }
}

// 31 states of 5 bits in three u64 (12 each)
__device__ __forceinline__ void pack_states(const uint32_t (&m)[kStates], uint64_t (&x)[3]) {
    x[0] = x[1] = x[2] = 0;
#pragma unroll
    for (int e = 0; e < kStates; ++e) x[e / 12] |= (uint64_t)(m[e] & 31u) << (5 * (e % 12));
}

constexpr int kLevels = 7;  // log2(kTileLanes)
constexpr int kTStride = 33;
__device__ __forceinline__ int level_base(int k) { return 2 * kTileLanes - (2 * kTileLanes >> k); }

// The reduction of a tile's 128 chunk maps to the tile map, in place (decode.hip tile_reduce)
__device__ void tile_reduce(uint32_t (*T)[kTStride]) {
    const int l = threadIdx.x;
    constexpr int kMaxTasks = (kTileLanes / 2 * kStates + kTileLanes - 1) / kTileLanes;
#pragma unroll
    for (int k = 1; k <= kLevels; ++k) {
        const int total = (kTileLanes >> k) * kStates;
        uint32_t r[kMaxTasks];
#pragma unroll
        for (int i = 0; i < kMaxTasks; ++i) {
            const int t = l + i * kTileLanes;
            if (t < total) {
                const int j = t / kStates;
                r[i] = t_compose(T[2 * j][t % kStates], T[2 * j + 1]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kMaxTasks; ++i) {
            const int t = l + i * kTileLanes;
            if (t < total) T[t / kStates][t % kStates] = r[i];
        }
        __syncthreads();
    }
}

constexpr int kPrepT = 1024;

}  // namespace

// ---- pass P: the connections checked and made searchable. A connection is judged against the
// largest end and the largest group of the earlier connections that pass the per-connection
// checks: exclusive running maxima, scanned in three launches (per block of 1024 connections in
// LDS, the block totals in one block, then every connection's verdict) -----------------------
__device__ __forceinline__ bool cl_self_ok(const mpx_client_conn& c, uint64_t len, uint32_t n_groups) {
    return !(c.offset & (MPX_CLIENT_ALIGN - 1)) && c.offset <= len &&
           (uint64_t)c.length <= len - c.offset && c.group < n_groups;
}
// inclusive maxima over the block's threads, in place in LDS
__device__ __forceinline__ void cl_block_max_scan(uint64_t* s_end, uint32_t* s_grp) {
    const uint32_t t = threadIdx.x;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)kPrepT; d <<= 1) {
        const uint64_t a = t >= d ? s_end[t - d] : 0;
        const uint32_t b = t >= d ? s_grp[t - d] : 0;
        __syncthreads();
        s_end[t] = max(s_end[t], a);
        s_grp[t] = max(s_grp[t], b);
        __syncthreads();
    }
}
// sc[k] = {maximum end, -, maximum group} of the block's connections before k; bt_*[block] = the
// block's maxima
__global__ __launch_bounds__(kPrepT) void k_cl_prep_scan(const mpx_client_conn* __restrict__ conns,
                                                         uint32_t n, uint64_t len, uint32_t n_groups,
                                                         CConn* __restrict__ sc,
                                                         uint64_t* __restrict__ bt_end,
                                                         uint32_t* __restrict__ bt_grp) {
    __shared__ uint64_t s_end[kPrepT];
    __shared__ uint32_t s_grp[kPrepT];
    const uint32_t t = threadIdx.x, k = blockIdx.x * kPrepT + t;
    uint64_t me = 0;
    uint32_t mg = 0;
    if (k < n) {
        const mpx_client_conn c = conns[k];
        if (cl_self_ok(c, len, n_groups)) {
            me = c.offset + c.length;
            mg = c.group;
        }
    }
    s_end[t] = me;
    s_grp[t] = mg;
    cl_block_max_scan(s_end, s_grp);
    if (k < n) sc[k] = CConn{t ? s_end[t - 1] : 0, 0u, t ? s_grp[t - 1] : 0u};
    if (t == kPrepT - 1) {
        bt_end[blockIdx.x] = s_end[t];
        bt_grp[blockIdx.x] = s_grp[t];
    }
}
// the block maxima -> the maxima before each block (at most kPrepT blocks: MPX_CLIENT_MAX_CONNS)
__global__ __launch_bounds__(kPrepT) void k_cl_prep_totals(uint64_t* __restrict__ bt_end,
                                                           uint32_t* __restrict__ bt_grp, uint32_t nb,
                                                           uint32_t n_chunks, uint32_t* __restrict__ P,
                                                           uint32_t* __restrict__ D) {
    __shared__ uint64_t s_end[kPrepT];
    __shared__ uint32_t s_grp[kPrepT];
    const uint32_t t = threadIdx.x;
    s_end[t] = t < nb ? bt_end[t] : 0;
    s_grp[t] = t < nb ? bt_grp[t] : 0;
    cl_block_max_scan(s_end, s_grp);
    if (t < nb) {
        bt_end[t] = t ? s_end[t - 1] : 0;
        bt_grp[t] = t ? s_grp[t - 1] : 0;
    }
    if (t == 0 && n_chunks == 0) P[0] = D[0] = 0;  // (no walk runs on an empty buffer)
}
static_assert(MPX_CLIENT_MAX_CONNS <= kPrepT * kPrepT, "one block scans the block maxima");
// every connection's verdict and its searchable form
__global__ __launch_bounds__(kPrepT) void k_cl_prep_conns(const mpx_client_conn* __restrict__ conns,
                                                          uint32_t n, uint64_t len, uint32_t n_groups,
                                                          const uint64_t* __restrict__ bt_end,
                                                          const uint32_t* __restrict__ bt_grp,
                                                          CConn* __restrict__ sc, uint32_t* err) {
    const uint32_t k = blockIdx.x * kPrepT + threadIdx.x;
    bool bad = false;
    if (k < n) {
        const mpx_client_conn c = conns[k];
        const CConn pre = sc[k];
        const uint64_t pe = max(bt_end[blockIdx.x], pre.key);
        const uint32_t pg = max(bt_grp[blockIdx.x], pre.gkey);
        const bool valid = cl_self_ok(c, len, n_groups) && c.offset >= pe && c.group >= pg;
        sc[k] = CConn{valid ? c.offset : pe, valid ? c.length : 0u, valid ? c.group : pg};
        bad = !valid;
    }
    if (ballot(bad) && lane_id() == 0) raise_err(err, kErrInval);
}

// ---- pass A: chunk maps and tile maps ----------------------------------------------------------
__global__ __launch_bounds__(kTileLanes) void k_cl_tile_maps(
    const uint8_t* __restrict__ buf, const CConn* __restrict__ sc, uint32_t n_conns,
    uint32_t* __restrict__ own, uint64_t* __restrict__ xmap, GEntry* __restrict__ tmap) {
    __shared__ uint32_t T[kTileLanes][kTStride];
    const uint32_t l = threadIdx.x;
    const uint64_t ci = (uint64_t)blockIdx.x * kTileLanes + l;
    const uint64_t c0 = ci * kChunk;
    const uint32_t k = find_owner(sc, n_conns, c0);
    uint32_t w[kLook];
    bool head = false;
    if (k == kNoConn) {
#pragma unroll
        for (int e = 0; e < kLook; ++e) w[e] = kDeadSt;
    } else {
        const CConn c = sc[k];
        const uint64_t cend = c.key + c.len;
        uint32_t wd[kChunk / 4];
        const uint4* s = reinterpret_cast<const uint4*>(buf + c0);
#pragma unroll
        for (int i = 0; i < kChunk / 16; ++i) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (c0 + 16 * i < cend) v = s[i];  // default policy: the emit pass reads it again
            wd[4 * i] = v.x;
            wd[4 * i + 1] = v.y;
            wd[4 * i + 2] = v.z;
            wd[4 * i + 3] = v.w;
        }
        chunk_map_dp(wd, (uint32_t)min(cend - c0, (uint64_t)(2 * kChunk)), w);
        head = c0 == c.key;
    }
    // a head enters at 0 whatever state the chain before it is in, DEAD included
    uint32_t m[kStates];
#pragma unroll
    for (int e = 0; e < kLook; ++e) m[e] = head ? w[0] : w[e];
    m[kDeadSt] = head ? w[0] : kDeadSt;
    own[ci] = k;
    uint64_t x[3];
    pack_states(m, x);
    xmap[ci * 3] = x[0];
    xmap[ci * 3 + 1] = x[1];
    xmap[ci * 3 + 2] = x[2];
#pragma unroll
    for (int e = 0; e < kStates; ++e) T[l][e] = t_from_chunk(m[e]);
    __syncthreads();
    tile_reduce(T);
    if (l < (uint32_t)kStates) {
        const uint32_t r = T[0][l];
        tmap[(uint64_t)blockIdx.x * kStates + l] = GEntry{r & 31u, (r >> 5) & 0x3FFu, r >> 15};
    }
}

// The map walks of passes B1-B3 follow up to 128 maps in kDParts parts side by side (decode.hip):
// thread (q, e) takes state e through part q, one thread chains the part maps from the run's
// entry, and kDParts threads then walk their parts where every map's entry is wanted.
constexpr int kDParts = 8;
constexpr uint32_t kDPer = kGroupTiles / kDParts;
__device__ __forceinline__ GEntry g_compose(GEntry a, const GEntry* b) {
    const GEntry y = b[a.st];
    return GEntry{y.st, a.pr + y.pr, a.dr + y.dr};
}
__device__ __forceinline__ void cl_part_maps(const GEntry (*S)[kStates], uint32_t n,
                                             GEntry (*Q)[kStates]) {
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)(kDParts * kStates)) {
        const uint32_t q = t / kStates, e = t % kStates;
        const uint32_t t0 = q * kDPer, t1 = min(t0 + kDPer, n);
        GEntry a{e, 0, 0};
        for (uint32_t k = t0; k < t1; ++k) a = g_compose(a, S[k]);
        Q[q][e] = a;
    }
}
// thread 0: the parts' entries from the run's entry r; returns the state after the run
__device__ __forceinline__ GEntry cl_part_entries(const GEntry (*Q)[kStates], GEntry r, GEntry* PE) {
    for (int q = 0; q < kDParts; ++q) {
        PE[q] = r;
        r = g_compose(r, Q[q]);
    }
    return r;
}
// threads q < kDParts: out[k] = {entry state of map k, proposals, dropped before it}
__device__ __forceinline__ void cl_part_walk(const GEntry (*S)[kStates], uint32_t n,
                                             const GEntry* PE, GEntry* out) {
    const uint32_t q = threadIdx.x;
    if (q >= (uint32_t)kDParts) return;
    const uint32_t t0 = q * kDPer, t1 = min(t0 + kDPer, n);
    GEntry a = PE[q];
    for (uint32_t k = t0; k < t1; ++k) {
        out[k] = a;
        a = g_compose(a, S[k]);
    }
}

// ---- pass B1: group maps (a group = 128 consecutive tiles) ----------------------------------
__global__ __launch_bounds__(256) void k_cl_group_maps(const GEntry* __restrict__ tmap,
                                                       uint32_t n_tiles, GEntry* __restrict__ gmap) {
    __shared__ GEntry S[kGroupTiles][kStates];
    __shared__ GEntry Q[kDParts][kStates];
    const uint32_t g = blockIdx.x, first = g * kGroupTiles;
    const uint32_t nt = min((uint32_t)kGroupTiles, n_tiles - first);
    for (uint32_t i = threadIdx.x; i < nt * kStates; i += blockDim.x)
        (&S[0][0])[i] = tmap[(uint64_t)first * kStates + i];
    __syncthreads();
    cl_part_maps(S, nt, Q);
    __syncthreads();
    if (threadIdx.x < (uint32_t)kStates) {
        GEntry a{threadIdx.x, 0, 0};
#pragma unroll
        for (int q = 0; q < kDParts; ++q) a = g_compose(a, Q[q]);
        gmap[(uint64_t)g * kStates + threadIdx.x] = a;
    }
}

// ---- pass B2: the true chain through the group maps from DEAD (one block, 128 groups at a
// time); the totals close the per-chunk count arrays -------------------------------------------
__global__ __launch_bounds__(256) void k_cl_walk(const GEntry* __restrict__ gmap, uint32_t n_groups,
                                                 GEntry* __restrict__ gres, uint32_t* __restrict__ Pn,
                                                 uint32_t* __restrict__ Dn) {
    __shared__ GEntry S[kGroupTiles][kStates];
    __shared__ GEntry Q[kDParts][kStates];
    __shared__ GEntry PE[kDParts];
    __shared__ GEntry cur;
    if (threadIdx.x == 0) cur = GEntry{kDeadSt, 0, 0};
    for (uint32_t b0 = 0; b0 < n_groups; b0 += kGroupTiles) {
        const uint32_t nb = min((uint32_t)kGroupTiles, n_groups - b0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb * kStates; i += blockDim.x)
            (&S[0][0])[i] = gmap[(uint64_t)b0 * kStates + i];
        __syncthreads();
        cl_part_maps(S, nb, Q);
        __syncthreads();
        if (threadIdx.x == 0) cur = cl_part_entries(Q, cur, PE);
        __syncthreads();
        cl_part_walk(S, nb, PE, gres + b0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *Pn = cur.pr;
        *Dn = cur.dr;
    }
}

// ---- pass B3: tile entries inside each group ---------------------------------------------------
__global__ __launch_bounds__(256) void k_cl_tile_entries(const GEntry* __restrict__ tmap,
                                                         uint32_t n_tiles,
                                                         const GEntry* __restrict__ gres,
                                                         GEntry* __restrict__ tres) {
    __shared__ GEntry S[kGroupTiles][kStates];
    __shared__ GEntry Q[kDParts][kStates];
    __shared__ GEntry PE[kDParts];
    const uint32_t g = blockIdx.x, first = g * kGroupTiles;
    const uint32_t nt = min((uint32_t)kGroupTiles, n_tiles - first);
    for (uint32_t i = threadIdx.x; i < nt * kStates; i += blockDim.x)
        (&S[0][0])[i] = tmap[(uint64_t)first * kStates + i];
    __syncthreads();
    cl_part_maps(S, nt, Q);
    __syncthreads();
    if (threadIdx.x == 0) (void)cl_part_entries(Q, gres[g], PE);
    __syncthreads();
    cl_part_walk(S, nt, PE, tres + first);
}

// ---- pass C: chunk entries (tree over the stored exit states) and emission ----------------------
// The tile's bytes are staged in LDS; the true chain is walked per chunk twice (count, then emit
// at the offsets of a block-wide exclusive scan of the counts).
constexpr int kXPad = 32;  // bytes per exit map in LDS (31 used)
// the staged tile image: 4 pad bytes after every 128-byte chunk, so the lanes - one per chunk, at
// similar offsets - read 64 LDS banks instead of two (decode.hip)
__device__ __forceinline__ uint32_t cpofs(uint32_t o) { return o + ((o >> 7) << 2); }
constexpr int kClImg = kTileBytes + 32 + 4 * (kTileLanes + 1) + 16;
__device__ __forceinline__ void cimg_put(uint8_t* B, int i, const uint4 v) {
    uint32_t* w = reinterpret_cast<uint32_t*>(B) + 4 * i + (i >> 3);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
}
// 4 bytes at tile offset o from two aligned dword reads, each at its image position
__device__ __forceinline__ uint32_t cl_le32(const uint8_t* B, uint32_t o) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(B);
    const uint32_t d = o >> 2, sh = o & 3u;
    const uint32_t d0 = d + (d >> 5), d1 = d + 1 + ((d + 1) >> 5);
    const uint64_t x = ((uint64_t)w[d1] << 32) | w[d0];
    return (uint32_t)(x >> (8 * sh));
}
__device__ __forceinline__ uint64_t cl_le64(const uint8_t* B, uint32_t o) {
    return (uint64_t)cl_le32(B, o) | ((uint64_t)cl_le32(B, o + 4) << 32);
}

__global__ __launch_bounds__(kTileLanes) void k_cl_emit(
    const uint8_t* __restrict__ buf, uint64_t len, const CConn* __restrict__ sc,
    const uint32_t* __restrict__ own, const uint64_t* __restrict__ xmap,
    const GEntry* __restrict__ tres, uint32_t n_chunks, uint8_t* __restrict__ op_out,
    int64_t* __restrict__ key_out, int64_t* __restrict__ val_out, mpx_proposal* __restrict__ meta_out,
    uint64_t prop_cap, mpx_client_conn_result* __restrict__ conn_res, uint32_t* __restrict__ P,
    uint32_t* __restrict__ D) {
    __shared__ uint8_t E[2 * kTileLanes - 1];  // entry state per tree node
    // the exit-map tree is dead once every chunk has its entry: the tile's bytes (loaded into
    // registers meanwhile) take its LDS
    constexpr int kVecs = (kTileBytes + 32) / 16;
    constexpr int kVec = (kVecs + kTileLanes - 1) / kTileLanes;
    static_assert((2 * kTileLanes - 1) * kXPad <= kTileBytes + 32, "the tree fits the tile image");
    __shared__ __attribute__((aligned(16))) uint8_t B[kClImg];
    uint8_t(*const X)[kXPad] = reinterpret_cast<uint8_t(*)[kXPad]>(B);
    __shared__ uint32_t wsum[kTileLanes / kWave];
    const GEntry r = tres[blockIdx.x];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTileBytes;
    const int l = threadIdx.x;
    const uint64_t ci = (uint64_t)blockIdx.x * kTileLanes + l;
    uint4 tv[kVec];
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const int i = l + k * kTileLanes;
        const uint64_t a = t0 + (uint64_t)i * 16;
        tv[k] = make_uint4(0, 0, 0, 0);
        // (a is a multiple of 16: a < len reads below len rounded up to 16)
        if (i < kVecs && a < len) tv[k] = *reinterpret_cast<const uint4*>(buf + a);
    }
    const uint32_t k_own = own[ci];
    CConn c{0, 0, 0};
    if (k_own != kNoConn) c = sc[k_own];
    {
        const uint64_t x0 = xmap[ci * 3], x1 = xmap[ci * 3 + 1], x2 = xmap[ci * 3 + 2];
#pragma unroll
        for (int e = 0; e < kStates; ++e) {
            const uint64_t x = e < 12 ? x0 : e < 24 ? x1 : x2;
            X[l][e] = (uint8_t)((x >> (5 * (e % 12))) & 31u);
        }
    }
    __syncthreads();
    for (int k = 1; k <= kLevels; ++k) {
        const int nodes = kTileLanes >> k;
        const int src = level_base(k - 1), dst = level_base(k);
        for (int t = l; t < nodes * kStates; t += kTileLanes) {
            const int j = t / kStates, e = t % kStates;
            X[dst + j][e] = X[src + 2 * j + 1][X[src + 2 * j][e]];
        }
        __syncthreads();
    }
    if (l == 0) E[level_base(kLevels)] = (uint8_t)r.st;
    __syncthreads();
    for (int k = kLevels; k >= 1; --k) {
        const int nodes = kTileLanes >> k;
        const int src = level_base(k), dst = level_base(k - 1);
        if (l < nodes) {
            const uint8_t e = E[src + l];
            E[dst + 2 * l] = e;
            E[dst + 2 * l + 1] = X[dst + 2 * l][e];
        }
        __syncthreads();
    }
    // a head enters at 0 whatever the chain before it did; a chunk of no connection frames nothing
    const uint64_t c0 = t0 + (uint64_t)l * kChunk;
    uint32_t e = E[l];
    if (k_own == kNoConn) e = kDeadSt;
    else if (c0 == c.key) e = 0;
    __syncthreads();  // every lane has read its tree nodes: the tile's bytes take the tree's LDS
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
        const int i = l + k * kTileLanes;
        if (i < kVecs) cimg_put(B, i, tv[k]);
    }
    __syncthreads();
    // walk 1: frames starting in this chunk on the true chain
    const uint32_t base = (uint32_t)l * kChunk;  // chunk start within the tile
    // the connection's end from the tile start (a live chunk lies inside its connection)
    const uint64_t lim = e != kDeadSt ? c.key + c.len - t0 : 0;
    uint32_t n_pr = 0, n_dr = 0;
    if (e != kDeadSt) {
        for (uint32_t p = base + e; p < base + kChunk;) {
            const uint32_t code = B[cpofs(p)];
            const uint32_t fl = frame_len(code);
            if ((uint64_t)p + fl > lim) break;  // (at or past the end, or a partial frame)
            if (code == 0) ++n_pr;
            else ++n_dr;
            p += fl;
        }
    }
    // block exclusive scan of (n_pr | n_dr << 16): a tile starts at most 547 proposals and 16384
    // dropped frames
    const uint32_t v = n_pr | (n_dr << 16);
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane_id() >= d) inc += t;
    }
    if (lane_id() == kWave - 1) wsum[l / kWave] = inc;
    __syncthreads();
    uint32_t pre = inc - v;
    for (int w2 = 0; w2 < l / kWave; ++w2) pre += wsum[w2];
    const uint32_t p_before = r.pr + (pre & 0xFFFFu), d_before = r.dr + (pre >> 16);
    if (ci < n_chunks) {
        P[ci] = p_before;
        D[ci] = d_before;
    }
    if (e == kDeadSt) return;
    // walk 2: the proposals, and the connection's stop if this chunk meets it
    uint64_t pi = p_before;
    uint32_t p = base + e;
    bool stopped = false;
    int32_t why = MPX_DECODE_END, scode = -1;
    while (p < base + kChunk) {
        if ((uint64_t)p >= lim) {
            stopped = true;
            break;
        }
        const uint32_t code = B[cpofs(p)];
        const uint32_t fl = frame_len(code);
        if ((uint64_t)p + fl > lim) {
            stopped = true;
            why = MPX_DECODE_PARTIAL;
            scode = (int32_t)code;
            break;
        }
        if (code == 0) {  // CommandId i32, Op u8, K i64, V i64, Timestamp i64 (little endian)
            if (pi < prop_cap) {
                op_out[pi] = B[cpofs(p + 5)];
                key_out[pi] = (int64_t)cl_le64(B, p + 6);
                val_out[pi] = (int64_t)cl_le64(B, p + 14);
                const uint64_t ts = cl_le64(B, p + 22);
                *reinterpret_cast<uint4*>(meta_out + pi) =
                    make_uint4((uint32_t)ts, (uint32_t)(ts >> 32), cl_le32(B, p + 1), k_own);
            }
            ++pi;
        }
        p += fl;
    }
    // the chain left the chunk exactly at the connection's end, which is also the chunk's: the
    // next chunk is not this connection's
    if (!stopped && (uint64_t)p == lim && p == base + kChunk) stopped = true;
    if (stopped) {
        mpx_client_conn_result* cr = conn_res + k_own;
        cr->consumed = (uint32_t)(t0 + p - c.key);
        cr->stop_reason = why;
        cr->stop_code = scode;
    }
}

// ---- pass R: the rest of every connection's record --------------------------------------------
constexpr int kResT = 256;
__global__ __launch_bounds__(kResT) void k_cl_conn_res(const CConn* __restrict__ sc, uint32_t n,
                                                       const uint32_t* __restrict__ P,
                                                       const uint32_t* __restrict__ D,
                                                       mpx_client_conn_result* __restrict__ conn_res,
                                                       uint32_t* __restrict__ bpart) {
    __shared__ uint32_t ws[kResT / kWave];
    const uint32_t k = blockIdx.x * kResT + threadIdx.x;
    bool partial = false;
    if (k < n) {
        const CConn c = sc[k];
        const uint64_t lo = (c.key + kChunk - 1) / kChunk, hi = (c.key + c.len + kChunk - 1) / kChunk;
        mpx_client_conn_result* cr = conn_res + k;
        cr->first = P[lo];
        cr->n_proposals = P[hi] - P[lo];
        cr->n_dropped = D[hi] - D[lo];
        cr->pad = 0;
        if (!c.len) {
            cr->consumed = 0;
            cr->stop_reason = MPX_DECODE_END;
            cr->stop_code = -1;
        } else {
            partial = cr->stop_reason == MPX_DECODE_PARTIAL;  // (the emit pass wrote it)
        }
    }
    const uint32_t cnt = (uint32_t)popc(ballot(partial));
    if (lane_id() == 0) ws[threadIdx.x / kWave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kResT / kWave; ++w) s += ws[w];
        bpart[blockIdx.x] = s;
    }
}

// ---- pass G1: prop_off (a thread per group: the first connection with gkey >= g) -------------
__global__ __launch_bounds__(256) void k_cl_prop_off(const CConn* __restrict__ sc, uint32_t n,
                                                     const uint32_t* __restrict__ P, uint32_t n_chunks,
                                                     uint32_t n_groups, uint32_t* __restrict__ po,
                                                     uint64_t* __restrict__ prop_off) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_groups) return;
    uint32_t lo = 0, hi = n;
    if (g == n_groups) lo = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sc[mid].gkey < g) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t x = lo < n ? P[(sc[lo].key + kChunk - 1) / kChunk] : P[n_chunks];
    po[g] = x;
    if (prop_off) prop_off[g] = x;
}

// ---- pass G2: send_off and the call's totals (one block; thread t takes a contiguous run of
// groups) -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPrepT) void k_cl_finish(const uint32_t* __restrict__ po,
                                                      uint32_t n_groups, uint64_t* __restrict__ send_off,
                                                      const uint32_t* __restrict__ bpart,
                                                      uint32_t n_bpart, const uint32_t* __restrict__ P,
                                                      const uint32_t* __restrict__ D, uint32_t n_chunks,
                                                      mpx_client_result* __restrict__ res) {
    __shared__ uint64_t s_sum[kPrepT];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_groups + kPrepT - 1) / kPrepT;
    const uint32_t lo = min(n_groups, t * per), hi = min(n_groups, lo + per);
    auto sends = [&](uint32_t g) {
        return (uint64_t)((po[g + 1] - po[g] + (MPX_PROPOSE_MAX_BATCH - 1)) / MPX_PROPOSE_MAX_BATCH);
    };
    uint64_t mine = 0;
    for (uint32_t g = lo; g < hi; ++g) mine += sends(g);
    uint64_t parts = 0;
    for (uint32_t i = t; i < n_bpart; i += kPrepT) parts += bpart[i];
    // inclusive scans of both in LDS, one after the other
    auto scan = [&](uint64_t x) {
        s_sum[t] = x;
        __syncthreads();
        for (uint32_t d = 1; d < (uint32_t)kPrepT; d <<= 1) {
            const uint64_t a = t >= d ? s_sum[t - d] : 0;
            __syncthreads();
            s_sum[t] += a;
            __syncthreads();
        }
    };
    scan(parts);
    const uint64_t n_partial = s_sum[kPrepT - 1];
    __syncthreads();
    scan(mine);
    uint64_t run = s_sum[t] - mine;
    const uint64_t total = s_sum[kPrepT - 1];
    if (send_off) {
        for (uint32_t g = lo; g < hi; ++g) {
            send_off[g] = run;
            run += sends(g);
        }
        if (t == 0) send_off[n_groups] = total;
    }
    if (t == 0) {
        res->n_proposals = P[n_chunks];
        res->n_dropped = D[n_chunks];
        res->n_partial = n_partial;
        res->n_sends = total;
    }
}

// a call of no connection: no scratch
__global__ void k_cl_empty(uint32_t n_groups, uint64_t* prop_off, uint64_t* send_off,
                           mpx_client_result* res) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= n_groups) {
        if (prop_off) prop_off[g] = 0;
        if (send_off) send_off[g] = 0;
    }
    if (g == 0) {
        res->n_proposals = 0;
        res->n_dropped = 0;
        res->n_partial = 0;
        res->n_sends = 0;
    }
}

namespace {
struct ClWork {
    CConn* sc;
    uint32_t *own, *P, *D, *bpart, *po, *bt_grp;
    uint64_t *xmap, *bt_end;
    GEntry *tmap, *tres, *gmap, *gres;
    uint64_t chunks, tiles, groups, rblocks;
    ClWork(Carver& c, uint64_t len, uint64_t n_conns, uint64_t n_groups) {
        chunks = (len + kChunk - 1) / kChunk;
        tiles = (chunks + kTileLanes - 1) / kTileLanes;
        groups = (tiles + kGroupTiles - 1) / kGroupTiles;
        rblocks = (n_conns + kResT - 1) / kResT;
        sc = c.take<CConn>(n_conns);
        bt_end = c.take<uint64_t>(kPrepT);
        bt_grp = c.take<uint32_t>(kPrepT);
        own = c.take<uint32_t>(tiles * kTileLanes);
        xmap = c.take<uint64_t>(tiles * kTileLanes * 3);
        tmap = c.take<GEntry>(tiles * kStates);
        tres = c.take<GEntry>(tiles);
        gmap = c.take<GEntry>(groups * kStates);
        gres = c.take<GEntry>(groups);
        P = c.take<uint32_t>(chunks + 1);
        D = c.take<uint32_t>(chunks + 1);
        bpart = c.take<uint32_t>(rblocks);
        po = c.take<uint32_t>(n_groups + 1);
    }
};
}  // namespace

uint64_t client_work_bytes(uint64_t len, uint64_t n_conns, uint64_t n_groups, Carver&& c) {
    return ClWork(c, len, n_conns, n_groups), c.bytes();
}

hipError_t launch_decode_client_streams(const uint8_t* buf, uint64_t len,
                                        const mpx_client_conn* conns, uint64_t n_conns,
                                        uint64_t n_groups, const mpx_client_out* out,
                                        mpx_client_conn_result* conn_res, mpx_client_result* res,
                                        void* work, uint64_t work_bytes, uint32_t* err,
                                        hipStream_t stream) {
    if (len > (uint64_t)MPX_DECODE_MAX_BYTES || n_conns > MPX_CLIENT_MAX_CONNS ||
        n_groups > MPX_CLIENT_MAX_GROUPS)
        return hipErrorInvalidValue;
    const uint32_t ng = (uint32_t)n_groups, nc = (uint32_t)n_conns;
    if (!nc) {
        k_cl_empty<<<(ng + 1 + 255) / 256, 256, 0, stream>>>(ng, out->prop_off, out->send_off, res);
        return hipGetLastError();
    }
    Carver c(work);
    const ClWork w(c, len, n_conns, n_groups);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const uint32_t chunks = (uint32_t)w.chunks, tiles = (uint32_t)w.tiles, groups = (uint32_t)w.groups;
    const uint32_t pblocks = (nc + kPrepT - 1) / kPrepT;
    k_cl_prep_scan<<<pblocks, kPrepT, 0, stream>>>(conns, nc, len, ng, w.sc, w.bt_end, w.bt_grp);
    k_cl_prep_totals<<<1, kPrepT, 0, stream>>>(w.bt_end, w.bt_grp, pblocks, chunks, w.P, w.D);
    k_cl_prep_conns<<<pblocks, kPrepT, 0, stream>>>(conns, nc, len, ng, w.bt_end, w.bt_grp, w.sc, err);
    if (tiles) {
        k_cl_tile_maps<<<tiles, kTileLanes, 0, stream>>>(buf, w.sc, nc, w.own, w.xmap, w.tmap);
        k_cl_group_maps<<<groups, 256, 0, stream>>>(w.tmap, tiles, w.gmap);
        k_cl_walk<<<1, 256, 0, stream>>>(w.gmap, groups, w.gres, w.P + chunks, w.D + chunks);
        k_cl_tile_entries<<<groups, 256, 0, stream>>>(w.tmap, tiles, w.gres, w.tres);
        k_cl_emit<<<tiles, kTileLanes, 0, stream>>>(buf, len, w.sc, w.own, w.xmap, w.tres, chunks,
                                                    out->op, out->key, out->val, out->meta,
                                                    out->prop_cap, conn_res, w.P, w.D);
    }
    k_cl_conn_res<<<(uint32_t)w.rblocks, kResT, 0, stream>>>(w.sc, nc, w.P, w.D, conn_res, w.bpart);
    k_cl_prop_off<<<(ng + 1 + 255) / 256, 256, 0, stream>>>(w.sc, nc, w.P, chunks, ng, w.po,
                                                            out->prop_off);
    k_cl_finish<<<1, kPrepT, 0, stream>>>(w.po, ng, out->send_off, w.bpart, (uint32_t)w.rblocks, w.P,
                                          w.D, chunks, res);
    return hipGetLastError();
}

}  // namespace mpx

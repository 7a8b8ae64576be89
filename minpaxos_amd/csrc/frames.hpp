// frames.hpp — the building blocks the frame encoders share (logenc.hip, acceptor.hip,
// proposer.hip, commit.hip): wire bytes into an LDS image, the offset scans' functors, the
// window emitters' piece bookkeeping, bcast's ring walk, and the send-major partition's steps.
// Plain inlined functions: every caller keeps its own frame layout, loops and launchers (the three
// encoders of frames with a catch-up log share theirs one level up, in catchup.hpp).
// All workgroup-wide helpers are for kFrBlock threads and are called by every thread, with its
// index t: the caller has it in a register.
#pragma once
#include "common.hpp"
#include "scan.hpp"

namespace mpx {

constexpr int kFrBlock = 256;

// ---- bytes -----------------------------------------------------------------------------------------
// binary.PutUvarint of u: its length and its k-th byte
__host__ __device__ __forceinline__ uint32_t uvarint_len(uint64_t u) {
    uint32_t l = 1;
    while (u >= 0x80) {
        u >>= 7;
        ++l;
    }
    return l;
}
__device__ __forceinline__ uint32_t uvarint_byte(uint64_t u, uint32_t k) {
    u >>= 7 * k;
    return (uint32_t)(u & 0x7F) | (u >= 0x80 ? 0x80u : 0u);
}
// binary.PutVarint of n >= 0 (the zigzag of a non-negative n is n << 1)
__host__ __device__ __forceinline__ uint32_t varint_len(uint64_t n) { return uvarint_len(n << 1); }
__device__ __forceinline__ uint32_t varint_byte(uint64_t n, uint32_t k) {
    return uvarint_byte(n << 1, k);
}

// OR the n bytes of w (little-endian dwords, bytes past n zero) into the zeroed LDS image W of
// WORDS dwords at byte offset s (may be negative: the part before the image is dropped, as is
// anything past it): one ds_or_b32 per touched dword, so two writers of one dword (a frame
// boundary inside it) meet in the OR
template <int WORDS, int ND>
__device__ __forceinline__ void image_or(uint32_t* W, int64_t s, const uint32_t (&w)[ND],
                                         uint32_t n) {
    const int64_t d0 = s >> 2;  // floor
    const uint32_t sh = (uint32_t)(s & 3) * 8u;
    const uint32_t nout = (uint32_t)(((s & 3) + n + 3) >> 2);
#pragma unroll
    for (int i = 0; i <= ND; ++i) {
        if ((uint32_t)i >= nout) break;
        const int64_t d = d0 + i;
        if (d < 0 || d >= WORDS) continue;
        const uint64_t pair = ((uint64_t)(i < ND ? w[i] : 0u) << 32) | (i ? w[i - 1] : 0u);
        const uint32_t v = (uint32_t)(pair >> (32 - sh));
        if (v) atomicOr(&W[d], v);
    }
}
// state.(*Command).Marshal (Op u8, K i64, V i64): 17 bytes = 5 dwords shifted into at most 6
template <int WORDS>
__device__ __forceinline__ void image_or_cmd(uint32_t* W, int64_t s, uint32_t o8, uint64_t k8,
                                             uint64_t v8) {
    const uint32_t kl = (uint32_t)k8, kh = (uint32_t)(k8 >> 32);
    const uint32_t vl = (uint32_t)v8, vh = (uint32_t)(v8 >> 32);
    const uint32_t c[5] = {o8 | (kl << 8), (kl >> 24) | (kh << 8), (kh >> 24) | (vl << 8),
                           (vl >> 24) | (vh << 8), vh >> 24};
    image_or<WORDS>(W, s, c, 17);
}

// the Commands of a slice starting at byte cs that the window [b0, b1) overlaps: [lo, hi), a
// partial one at either end included; hi is not clamped to the slice's length
struct CmdSpan {
    uint64_t lo, hi;
};
__device__ __forceinline__ CmdSpan cmd_span(uint64_t cs, uint64_t b0, uint64_t b1) {
    return {b0 > cs ? (b0 - cs) / 17 : 0, b1 > cs ? (b1 - cs + 16) / 17 : 0};
}

// ---- offsets ---------------------------------------------------------------------------------------
// Frame bytes of item (q, s), destination-major: a sizes kernel leaves them in frame_off (a thread
// per item, so the chain behind a size runs in every lane at once: as the scan's own input
// functor it ran 16 dependent rounds per lane) and the scan runs in place: a tile reads its sizes
// before it writes its offsets, and no tile reads another's.
struct SizeIn {
    const uint64_t* size;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return size[i]; }
};
struct FrameOffOut {
    uint64_t* frame_off;
    uint64_t* dest_off;
    uint64_t n_sends, n_items;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t s, uint64_t b) const {
        frame_off[i] = s;
        if (i % n_sends == 0) dest_off[i / n_sends] = s;
        if (i == n_items - 1) {
            frame_off[n_items] = s + b;
            dest_off[n_items / n_sends] = s + b;
        }
    }
};

namespace {
// p[0 .. n) = 0: an empty call's dest_off, or the leading zero of an offsets array. A plain kernel
// defined in a header: the units are built without relocatable device code, so each gets its own
// copy, and the anonymous namespace keeps the four host stubs from colliding at link time (every
// unit that includes this header launches it).
__global__ void k_zero_u64(uint64_t* p, uint32_t n) {
    for (uint32_t x = threadIdx.x; x < n; x += blockDim.x) p[x] = 0;
}
}  // namespace

// the item holding byte pos: the last i >= lo with frame_off[i] <= pos (256-ary search; invariant
// frame_off[lo] <= pos < frame_off[n_items])
__device__ __forceinline__ uint64_t holder(const uint64_t* __restrict__ frame_off, uint64_t n_items,
                                           uint64_t lo, uint64_t pos, int t) {
    uint64_t hi = n_items;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + kFrBlock - 1) / kFrBlock;
        const uint64_t i = lo + (uint64_t)t * step;
        const int c = __syncthreads_count(i < hi && frame_off[i] <= pos);
        const uint64_t nh = lo + (uint64_t)c * step;
        lo += (uint64_t)(c - 1) * step;
        hi = nh < hi ? nh : hi;
    }
    return lo;
}

// ---- window emit -----------------------------------------------------------------------------------
// exclusive scan of the threads' piece counts over the workgroup: poff[0 .. kFrBlock], wtot one
// word per wave; returns the total
__device__ __forceinline__ uint32_t piece_scan(uint32_t np, uint32_t* poff, uint32_t* wtot,
                                               int t) {
    const int l = lane_id(), w = t / kWave;
    const uint32_t inc = wave_incl_scan(np, ScanSum32{});
    if (l == kWave - 1) wtot[w] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int x = 0; x < w; ++x) before += wtot[x];
    poff[t] = before + inc - np;
    if (t == kFrBlock - 1) poff[kFrBlock] = before + inc;
    __syncthreads();
    return poff[kFrBlock];
}
// the item of piece p: the last one with poff <= p
__device__ __forceinline__ uint32_t piece_item(const uint32_t* poff, uint32_t p) {
    uint32_t fa = 0, fb = kFrBlock;
    while (fb - fa > 1) {
        const uint32_t mid = (fa + fb) >> 1;
        if (poff[mid] <= p) fa = mid; else fb = mid;
    }
    return fa;
}
// the first `bytes` of the window image W to dst: 16-byte stores where dst is 16-byte aligned
// (no partial lines except at the output's two ends), else bytewise
__device__ __forceinline__ void window_store(const uint32_t* W, uint32_t bytes, uint8_t* dst,
                                             int t) {
    const uint8_t* S = reinterpret_cast<const uint8_t*>(W);
    if (((uintptr_t)dst & 15) == 0) {
        const uint32_t nv = bytes / 16;
        for (uint32_t i = t; i < nv; i += kFrBlock)
            st_stream(reinterpret_cast<uint4*>(dst) + i, reinterpret_cast<const uint4*>(W)[i]);
        for (uint32_t i = nv * 16 + t; i < bytes; i += kFrBlock) dst[i] = S[i];
    } else {
        for (uint32_t i = t; i < bytes; i += kFrBlock) dst[i] = S[i];
    }
}

// ---- destinations ----------------------------------------------------------------------------------
// q's place in bcast's ring walk from self over N replicas: returns its position (0 = self + 1);
// before = the alive replicas the walk meets ahead of q, or kRingDead where q itself is not alive
constexpr uint32_t kRingDead = ~0u;
__device__ __forceinline__ uint32_t ring_pos(uint32_t q, uint32_t self, uint32_t N, uint32_t alive,
                                             uint32_t& before) {
    const uint32_t p = (q + N - self - 1) % N;
    // rot bit k = Alive[(self + 1 + k) % N]
    const uint32_t full = N >= 32 ? ~0u : (1u << N) - 1u;
    const uint32_t am = alive & full, sh = (self + 1) % N;
    const uint32_t rot = sh ? ((am >> sh) | (am << (N - sh))) & full : am;
    before = (rot >> p) & 1u ? (uint32_t)__popc(rot & ((1u << p) - 1u)) : kRingDead;
    return p;
}

// ---- send-major partition --------------------------------------------------------------------------
// A stable partition of a call's slots over at most kFrDest destinations, fused with the
// encoding: a workgroup takes a tile of kFrPer slots per thread, slot p0 + k * kFrBlock + t in
// register k, so the (register k, wave) units are in array order.
constexpr int kFrDest = MPX_MAX_REPLICAS;
constexpr int kFrPer = 4;
constexpr int kFrTile = kFrBlock * kFrPer;               // 1024 slots per tile
constexpr int kFrUnits = kFrPer * (kFrBlock / kWave);    // (register k, wave) units

// how a lane says where its slot goes: one destination's index (kFrDest: none), or a mask of them
enum DestAs { kDestIndex, kDestMask };
template <DestAs AS>
__device__ __forceinline__ bool dest_is(uint32_t d, uint32_t x) {
    return AS == kDestMask ? (d >> x) & 1u : d == x;
}

// The tile's frames per destination into hist[dest][tile], in three steps around the caller's
// loop over its kFrPer slots: cnt (kFrDest words of LDS) zeroed; per slot, lane x < n_dest counts
// the wave's frames to destination x from every lane's index or mask d, added to its running
// count `mine` (passed through: a count started inside the step costs a register); the waves'
// counts meet in cnt and leave for hist.
__device__ __forceinline__ void dest_count_begin(uint32_t* cnt, int t) {
    if (t < kFrDest) cnt[t] = 0;
    __syncthreads();
}
template <DestAs AS>
__device__ __forceinline__ uint32_t dest_count_wave(uint32_t mine, uint32_t d, uint32_t n_dest,
                                                    int l) {
    for (uint32_t x = 0; x < n_dest; ++x) {
        const uint32_t c = (uint32_t)popc(ballot(dest_is<AS>(d, x)));
        mine += (uint32_t)l == x ? c : 0u;
    }
    return mine;
}
__device__ __forceinline__ void dest_count_end(uint32_t* cnt, uint32_t mine, uint32_t n_dest,
                                               uint64_t tiles, uint32_t* __restrict__ hist, int t,
                                               int l) {
    if ((uint32_t)l < n_dest && mine) atomicAdd(&cnt[l], mine);
    __syncthreads();
    if ((uint32_t)t < n_dest) hist[(uint64_t)t * tiles + blockIdx.x] = cnt[t];
}

// One (register k, wave) unit's counts: lane x < n_dest leaves the wave's frames to destination x
// in wc_u[x]. Returns the ballot of the last destination the lane's own slot goes to: for an index,
// the lanes that go where this one goes (its stable rank is the count of those below it).
template <DestAs AS>
__device__ __forceinline__ uint64_t unit_count(uint16_t* wc_u, uint32_t d, uint32_t n_dest, int l) {
    uint64_t own = 0;
    for (uint32_t x = 0; x < n_dest; ++x) {
        const uint64_t m = ballot(dest_is<AS>(d, x));
        own = dest_is<AS>(d, x) ? m : own;
        if ((uint32_t)l == x) wc_u[x] = (uint16_t)popc(m);
    }
    return own;
}
// destination x's per-unit counts wc[u][x] to their exclusive prefixes, in array order; returns
// the tile's frames to x
__device__ __forceinline__ uint32_t unit_prefix(uint16_t (*wc)[kFrDest], uint32_t x) {
    uint32_t run = 0;
#pragma unroll
    for (int u = 0; u < kFrUnits; ++u) {
        const uint32_t c = wc[u][x];
        wc[u][x] = (uint16_t)run;
        run += c;
    }
    return run;
}

// img[s0, s0 + bytes) to d, whatever the two alignments: [0, head) bytewise up to the first
// 16-byte aligned address, then whole 16-byte vectors read at the image's byte shift, then the
// tail bytewise. The last vector's shifted read takes up to 16 bytes past the run: the image
// keeps 16 spare bytes, zeroed.
__device__ __forceinline__ void copy_run_shifted(const uint8_t* img, uint32_t s0, uint32_t bytes,
                                                 uint8_t* d, int t) {
    const uint32_t* img32 = reinterpret_cast<const uint32_t*>(img);
    uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
    head = head < bytes ? head : bytes;
    const uint32_t nv = (bytes - head) / 16;
    const uint32_t tail0 = head + nv * 16;
    for (uint32_t i = t; i < nv; i += kFrBlock) {
        const uint32_t so = s0 + head + i * 16;  // image byte offset of the chunk
        const uint32_t sh = so & 3u;
        const uint32_t* q = img32 + (so >> 2);
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4];
        uint4 v;
        v.x = __builtin_amdgcn_alignbyte(a1, a0, sh);
        v.y = __builtin_amdgcn_alignbyte(a2, a1, sh);
        v.z = __builtin_amdgcn_alignbyte(a3, a2, sh);
        v.w = __builtin_amdgcn_alignbyte(a4, a3, sh);
        st_stream(reinterpret_cast<uint4*>(d + head) + i, v);
    }
    if ((uint32_t)t < head) d[t] = img[s0 + t];
    if ((uint32_t)t >= 32u && (uint32_t)t - 32u < bytes - tail0)
        d[tail0 + t - 32] = img[s0 + tail0 + t - 32];
}

}  // namespace mpx

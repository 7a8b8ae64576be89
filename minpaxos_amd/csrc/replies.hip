// replies.hip — reply assembly: the client reply records of a batch of handlePropose slots.
//
// Reference: the three loops in which a replica answers its clients,
//   handlePropose's refusals        bareminpaxos.go:622-623, :682-683, paxos.go:390-391
//   handleAcceptReply with !Dreply  bareminpaxos.go:1030-1042, paxos.go:644-655
//   executeCommands with Dreply     bareminpaxos.go:1076-1084, paxos.go:685-693
// each a plain expansion: a slot (one run of handlePropose, mpx_accept_send) answers none, one or
// all of its proposals, in slot order. That is a segmented expansion: a pass over the slots
// (count, errors, the slot-aligned mpx_commit_send), an exclusive scan of the counts (scan.hpp),
// and an emit pass balanced over OUTPUT records: a workgroup owns a tile of kRbTile output indices,
// finds the slots that cover it by searching the scanned offsets, gathers meta (16-byte vectors)
// and ret, lays the 24-byte records out in LDS and stores the image as whole 16-byte vectors over
// contiguous lines; the pad tail is part of the same image. A small finish kernel writes the
// result record (no ticket, no atomics: the family keeps no control words). Launches: 6.
// A call of at most MPX_RB_ONE_LAUNCH_SLOTS slots and MPX_RB_ONE_LAUNCH_REPLIES records of
// capacity is one kernel in one workgroup: a slot per thread, the scan in LDS, the same tiles.
// The pieces shared with the other assembly families are assemble.hpp's.
#include "assemble.hpp"
#include "common.hpp"
#include "kernels.hpp"
#include "scan.hpp"

namespace mpx {

namespace {

constexpr int kRbT = 256;        // threads of the count and emit workgroups (pass 1: a slot each)
constexpr int kRbTile = 1024;    // output records per emit tile
constexpr int kRbOneT = 1024;    // threads of the one-launch workgroup: a slot each
constexpr int kRbFinT = 1024;    // threads of the finish kernel
// the tile image: the records from byte 0 or 8 (the tile's first byte as it falls in its 16-byte
// line of the output), rounded up to whole vectors
constexpr int kRbImgVecs = (8 + kRbTile * (int)sizeof(mpx_reply_rec) + 15) / 16;
static_assert(MPX_RB_ONE_LAUNCH_SLOTS == kRbOneT, "the one-launch kernel takes a slot per thread");
static_assert(MPX_RB_ONE_LAUNCH_REPLIES >= MPX_PROPOSE_MAX_BATCH, "a full slot fits one launch");
static_assert(sizeof(mpx_reply_rec) == 24 && sizeof(mpx_proposal) == 16 &&
                  sizeof(mpx_accept_send) == 32 && sizeof(mpx_commit_send) == 32,
              "the vector moves below");

// the call, by value to every kernel
struct RbArgs {
    const mpx_accept_send* sends;
    const mpx_proposal* meta;
    const uint8_t* mask;
    const int64_t* ret;
    const uint64_t* ret_first;
    uint64_t n_sends, n_inst, n_props, n_ret, cap;
    int32_t inst_base;
    uint32_t kind, pad_client;
    mpx_reply_rec* recs;
    mpx_commit_send* csends;
    mpx_reply_result* res;
    uint32_t* err;
};

struct RbSlot {
    uint32_t cnt;  // records the slot emits
    bool sel;      // eligible, faultless and selected
    uint32_t err;  // kErr* bits
};

// Slot s judged: eligibility by kind, the command range, the window, the mask, a selected slot's
// result range; its mpx_commit_send
// written when the call asks for them.
__device__ __forceinline__ RbSlot rb_slot(const RbArgs& a, uint64_t s) {
    const uint4* p = reinterpret_cast<const uint4*>(a.sends + s);
    const uint4 h0 = p[0], h1 = p[1];  // {instance, ballot, last_committed, flags}, {first_cmd, n_cmds, pad}
    const uint32_t flags = h0.w, n = h1.z;
    const uint64_t first = (uint64_t)h1.x | ((uint64_t)h1.y << 32);
    const bool refusals = a.kind == MPX_RB_FALSE;
    const bool eligible =
        (flags & (refusals ? MPX_PH_NOT_LEADER | MPX_PH_REFUSED : MPX_PH_ACCEPT | MPX_PH_PREPARE)) != 0;
    RbSlot r{0, false, 0};
    if (eligible) {
        if (first > a.n_props || n > a.n_props - first) r.err |= kErrInval;
        r.sel = true;
        if (a.mask) {
            const int64_t rel = (int64_t)(int32_t)h0.x - a.inst_base;
            if (rel < 0 || (uint64_t)rel >= a.n_inst) r.err |= kErrNil;
            else r.sel = a.mask[rel] != 0;
        }
        if (r.sel && a.kind == MPX_RB_EXECUTED) {  // only a selected slot reads results
            const uint64_t rf = a.ret_first ? a.ret_first[s] : first;
            if (rf > a.n_ret || n > a.n_ret - rf) r.err |= kErrInval;
        }
        if (r.err) r.sel = false;
        if (r.sel) r.cnt = refusals && !(flags & MPX_PH_NOT_LEADER) ? min(n, 1u) : n;
    }
    if (a.csends) {  // {instance, ballot, first_cmd}, {n_cmds, flags, pad[2]}
        uint4* q = reinterpret_cast<uint4*>(a.csends + s);
        q[0] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        q[1] = make_uint4(n, r.sel ? MPX_CS_SEND : 0u, 0u, 0u);
    }
    return r;
}

// the scanned offsets, in global memory (general path) or in LDS (one launch)
struct RbOff {
    const uint64_t* off;
    __device__ __forceinline__ uint64_t operator()(uint32_t s) const { return off[s]; }
};

// One tile: output indices [lo, min(lo + kRbTile, cap)), of which those below `total` are replies
// and, with padding, the others pad records. All threads of the workgroup call (T of them); img
// and rng are the workgroup's, free again on return.
template <int T>
__device__ __forceinline__ void rb_emit_tile(const RbArgs& a, uint64_t lo, uint64_t total,
                                             const RbOff off, uint4* img, uint32_t* rng) {
    const uint32_t t = threadIdx.x;
    const uint32_t n_cap = (uint32_t)min((uint64_t)kRbTile, a.cap - lo);
    const uint32_t n_real = total > lo ? (uint32_t)min(total - lo, (uint64_t)n_cap) : 0u;
    const uint32_t n_out = a.pad_client != MPX_RB_NO_PAD ? n_cap : n_real;
    if (!n_out) return;  // (the same in every thread)
    // the first and the last slot under the tile's replies
    if (n_real) {
        if (t == 0) rng[0] = last_at_or_before(off, lo, 0u, (uint32_t)a.n_sends);
        if (t == kWave) rng[1] = last_at_or_before(off, lo + n_real - 1, 0u, (uint32_t)a.n_sends);
    }
    __syncthreads();
    const uintptr_t dst = (uintptr_t)a.recs + lo * sizeof(mpx_reply_rec);
    const uint32_t head = (uint32_t)(dst & 15);  // 0 or 8: recs is 8-byte aligned
    uint2* img2 = reinterpret_cast<uint2*>(img) + (head >> 3);
    const uint32_t s_lo = n_real ? rng[0] : 0u, s_hi = n_real ? rng[1] : 0u;
#pragma unroll
    for (int k = 0; k < kRbTile / T; ++k) {
        const uint32_t r = t + (uint32_t)k * T;
        if (r >= n_out) continue;
        uint2 value = make_uint2(0u, 0u), ts = make_uint2(0u, 0u), tail = make_uint2(0u, a.pad_client);
        if (r < n_real) {
            const uint64_t i = lo + r;
            const uint32_t s = last_at_or_before(off, i, s_lo, s_hi + 1);
            const uint64_t k_in = i - off(s);
            const uint4 h1 = reinterpret_cast<const uint4*>(a.sends + s)[1];
            const uint64_t first = (uint64_t)h1.x | ((uint64_t)h1.y << 32);
            const uint4 m = *reinterpret_cast<const uint4*>(a.meta + first + k_in);
            if (a.kind == MPX_RB_FALSE) {
                tail = make_uint2(0xFFFFFFFFu, m.w);  // command_id -1, the proposal's client
            } else {
                ts = make_uint2(m.x, m.y);
                tail = make_uint2(m.z, m.w);
                if (a.kind == MPX_RB_EXECUTED) {
                    const uint64_t v =
                        (uint64_t)a.ret[(a.ret_first ? a.ret_first[s] : first) + k_in];
                    value = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
                }
            }
        }
        img2[3 * r] = value;
        img2[3 * r + 1] = ts;
        img2[3 * r + 2] = tail;
    }
    __syncthreads();
    // the image leaves as whole 16-byte vectors; an 8-byte half at either end where the tile
    // starts or ends in the middle of a line
    const uint32_t span = head + n_out * (uint32_t)sizeof(mpx_reply_rec);
    const uint32_t n_vec = (span + 15) >> 4;
    char* const line0 = reinterpret_cast<char*>(dst - head);
    const uint2* half = reinterpret_cast<const uint2*>(img);
    for (uint32_t v = t; v < n_vec; v += T) {
        const bool lo_ok = 16 * v >= head, hi_ok = 16 * v + 16 <= span;
        if (lo_ok && hi_ok) *reinterpret_cast<uint4*>(line0 + 16 * v) = img[v];
        else if (lo_ok) *reinterpret_cast<uint2*>(line0 + 16 * v) = half[2 * v];
        else if (hi_ok) *reinterpret_cast<uint2*>(line0 + 16 * v + 8) = half[2 * v + 1];
    }
    __syncthreads();
}

// the scan's ends: item i is slot i's count (one more item, 0, so that off[n_sends] is the total)
struct RbCntIn {
    const uint32_t* cnt;
    uint64_t n;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i < n ? cnt[i] : 0; }
};
struct RbOffOut {
    uint64_t* off;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t) const { off[i] = ex; }
};

}  // namespace

// ---- pass 1: a slot per thread ------------------------------------------------------------------
__global__ __launch_bounds__(kRbT) void k_rb_count(RbArgs a, uint32_t* __restrict__ cnt,
                                                   uint32_t* __restrict__ bsel) {
    const uint64_t s = (uint64_t)blockIdx.x * kRbT + threadIdx.x;
    RbSlot r{0, false, 0};
    if (s < a.n_sends) {
        r = rb_slot(a, s);
        cnt[s] = r.cnt;
    }
    raise_bits(a.err, r.err, kErrInval | kErrNil);
    const uint32_t n_sel = (uint32_t)__syncthreads_count(r.sel);
    if (threadIdx.x == 0) bsel[blockIdx.x] = n_sel;
}

// ---- pass 3: a tile of output records per workgroup -----------------------------------------------
__global__ __launch_bounds__(kRbT) void k_rb_emit(RbArgs a, const uint64_t* __restrict__ off) {
    __shared__ uint4 img[kRbImgVecs];
    __shared__ uint32_t rng[2];
    const uint64_t total = a.n_sends ? off[a.n_sends] : 0;
    rb_emit_tile<kRbT>(a, (uint64_t)blockIdx.x * kRbTile, total, RbOff{off}, img, rng);
}

// ---- the result record (one workgroup) -----------------------------------------------------------
__global__ __launch_bounds__(kRbFinT) void k_rb_finish(const uint64_t* __restrict__ off,
                                                       uint64_t n_sends,
                                                       const uint32_t* __restrict__ bsel, uint32_t nb,
                                                       mpx_reply_result* __restrict__ res) {
    __shared__ uint64_t ws[kRbFinT / kWave];
    uint64_t mine = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += kRbFinT) mine += bsel[i];
    const uint64_t n_slots = block_sum<uint64_t, kRbFinT>(mine, ws);
    if (threadIdx.x == 0) {
        res->n_replies = n_sends ? off[n_sends] : 0;
        res->n_slots = n_slots;
    }
}

// ---- one launch: a replica-sized call in one workgroup, no scratch ------------------------------
__global__ __launch_bounds__(kRbOneT) void k_rb_one(RbArgs a) {
    __shared__ uint4 img[kRbImgVecs];
    __shared__ uint64_t s_off[kRbOneT + 1];
    __shared__ uint64_t ws[kRbOneT / kWave];
    __shared__ uint32_t rng[2];
    const uint32_t t = threadIdx.x;
    RbSlot r{0, false, 0};
    if (t < a.n_sends) r = rb_slot(a, t);
    raise_bits(a.err, r.err, kErrInval | kErrNil);
    const uint32_t n_sel = (uint32_t)__syncthreads_count(r.sel);
    s_off[t + 1] = block_excl_scan<uint64_t, kRbOneT>((uint64_t)r.cnt, ws) + r.cnt;
    if (t == 0) s_off[0] = 0;
    __syncthreads();
    const uint64_t total = s_off[a.n_sends];
    if (t == 0) {
        a.res->n_replies = total;
        a.res->n_slots = n_sel;
    }
    for (uint64_t lo = 0; lo < a.cap; lo += kRbTile)
        rb_emit_tile<kRbOneT>(a, lo, total, RbOff{s_off}, img, rng);
}

namespace {
struct RbWork {
    uint32_t *cnt, *bsel;
    uint64_t *off, *scan_tmp;
    uint64_t blocks;
    RbWork(Carver& c, uint64_t n_sends) {
        blocks = (n_sends + kRbT - 1) / kRbT;
        cnt = c.take<uint32_t>(n_sends);
        off = c.take<uint64_t>(n_sends + 1);
        bsel = c.take<uint32_t>(blocks);
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(n_sends + 1));
    }
};
}  // namespace

uint64_t reply_work_bytes(uint64_t n_sends, Carver&& c) { return RbWork(c, n_sends), c.bytes(); }

hipError_t launch_build_replies(const mpx_reply_batch* b, mpx_reply_rec* recs, uint64_t cap,
                                mpx_commit_send* commit_sends, mpx_reply_result* res, void* work,
                                uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    const uint64_t n = b->n_sends, tiles = (cap + kRbTile - 1) / kRbTile;
    if (n >= 0xFFFFFFFFull || tiles >= (1ull << 31)) return hipErrorInvalidValue;
    const RbArgs a{b->sends, b->meta, b->mask, b->ret, b->ret_first, n, b->n_inst, b->n_props,
                   b->n_ret, cap, b->inst_base, b->kind, b->pad_client, recs, commit_sends, res,
                   err};
    if (!n) {  // no slot: the pad tail and the result record, no scratch
        if (tiles && b->pad_client != MPX_RB_NO_PAD)
            k_rb_emit<<<(unsigned)tiles, kRbT, 0, stream>>>(a, nullptr);
        k_rb_finish<<<1, kRbFinT, 0, stream>>>(nullptr, 0, nullptr, 0, res);
        return hipGetLastError();
    }
    if (!(b->flags & MPX_RB_GENERAL) && n <= MPX_RB_ONE_LAUNCH_SLOTS &&
        cap <= MPX_RB_ONE_LAUNCH_REPLIES) {
        k_rb_one<<<1, kRbOneT, 0, stream>>>(a);
        return hipGetLastError();
    }
    Carver c(work);
    const RbWork w(c, n);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    k_rb_count<<<(unsigned)w.blocks, kRbT, 0, stream>>>(a, w.cnt, w.bsel);
    const hipError_t r = device_scan(RbCntIn{w.cnt, n}, RbOffOut{w.off}, n + 1, ScanSum64{},
                                     (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    if (tiles) k_rb_emit<<<(unsigned)tiles, kRbT, 0, stream>>>(a, w.off);
    k_rb_finish<<<1, kRbFinT, 0, stream>>>(w.off, n, w.bsel, (uint32_t)w.blocks, res);
    return hipGetLastError();
}

}  // namespace mpx

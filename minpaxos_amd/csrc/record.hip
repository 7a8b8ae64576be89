// record.hip — record assembly: a batch's durable-log bytes, built on the device.
//
// Reference: the handlers' stable-store appends. recordInstanceMetadata (bareminpaxos.go:164-174:
// Ballot, Status, instNo as LE u32, 12 bytes; paxos.go:107-116: Ballot LE u32 and a status byte, 5
// bytes) followed, where the message carries commands, by recordCommands (bareminpaxos.go:177-188 /
// paxos.go:119-130: state.(*Command).Marshal each, 17 bytes), at handlePropose (bareminpaxos.go:
// 697-699 / paxos.go:436-438), handleAccept (bareminpaxos.go:798-800), handleCommit (:881-882 /
// paxos.go:547-548), handleCommitShort (:909 / :574) and handleAcceptReply's commit branch (:1045 /
// :656). The handlers run per message in array order, so the batch's append is the recording
// items' records back to back in array order. Nothing here is per window slot: the passes run over
// the n items and the bytes written.
//   k_lr_mark   an item per thread: whether it records, its record's bytes (0: it does not), and
//               where its commands start in its source (assemble.hpp's msg_cmds / send_cmds, as
//               store.hip resolves them)
//   scan.hpp    the sizes' exclusive scan, in place: where every item's record starts (item_off
//               beside it when the caller asked)
//   k_lr_emit   balanced over OUTPUT bytes: an 8 KB window of the run per workgroup (a grid of at
//               most kLrGrid walks the windows), cut at multiples of 8 KB of the ADDRESS, so that
//               a window's stores are 16-byte vectors whichever way out lies mod 16. The window's
//               first item by frames.hpp's holder; the items from it in turns of 256, one per
//               thread, until a turn starts past the window: its header ORed into the LDS image, its commands inside the window counted;
//               then a thread per command (piece_scan / piece_item), read straight from its source
//               and ORed in. The image goes out once. Then the result record. Nothing reaches out
//               when the run does not fit.
// Launches: 5. A call of at most MPX_LR_ONE_LAUNCH_ITEMS items whose sources hold at most
// MPX_LR_ONE_LAUNCH_CMDS commands is one kernel in one workgroup: four items per thread, the offsets
// and positions in LDS, the same window loop.
#include <algorithm>

#include "assemble.hpp"
#include "common.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // k_zero_u64: this unit launches no copy of it
#include "frames.hpp"
#pragma clang diagnostic pop
#include "kernels.hpp"
#include "scan.hpp"
#include "scratch.hpp"

namespace mpx {

namespace {

constexpr int kLrT = kFrBlock;               // threads of every workgroup here
constexpr int kLrWinBytes = kLrT * 16 * 2;   // 8 KB of output per window (logenc.hip's measured size)
constexpr int kLrWinWords = kLrWinBytes / 4;
constexpr int kLrGrid = 2048;                // workgroups of k_lr_emit at most (six resident per CU)
constexpr int kLrOnePer = MPX_LR_ONE_LAUNCH_ITEMS / kLrT;  // items per thread of the one-launch kernel
static_assert(MPX_LR_ONE_LAUNCH_ITEMS % kLrT == 0, "the one-launch kernel takes whole items per thread");
static_assert(sizeof(mpx_accept_msg) == 16 && sizeof(mpx_accept_send) == 32, "vector loads per record");
static_assert(sizeof(mpx_record_result) == 32, "the result record");

// the call, by value to every kernel
struct LrArgs {
    const void* items;
    const uint8_t *effect, *mask;
    const uint32_t* perm;
    const uint64_t* d_n;
    uint64_t n, n_inst, n_recs, out_cap;
    uint8_t* out;
    uint64_t* item_off;
    mpx_record_result* res;
    uint32_t* err;
    int32_t inst_base;
    uint32_t kind, format, n_src;
    CmdSrc src[MPX_SC_MAX_SRC];
};

__device__ __forceinline__ uint32_t lr_hdr(const LrArgs& a) { return a.format == MPX_LOG_DURABLE ? 12u : 5u; }
__device__ __forceinline__ uint32_t lr_status(const LrArgs& a) {
    return a.kind == MPX_LR_ACCEPTS ? (uint32_t)MPX_ACCEPTED
                                    : a.kind == MPX_LR_SENDS ? (uint32_t)MPX_PREPARED : (uint32_t)MPX_COMMITTED;
}

// What item i records: bytes == 0 when it does not (also a faulty one: its bit is raised).
// pos: assemble.hpp's cmd_pos of its first command.
struct LrItem {
    uint64_t bytes, pos;
};
__device__ __forceinline__ LrItem lr_item(const LrArgs& a, const CmdSrc* S, uint64_t i, uint64_t n_eff,
                                          uint32_t& ebits) {
    LrItem r{0, 0};
    if (i >= n_eff) return r;
    CmdRange c{0, 0, 0, true};  // (metadata only: no commands)
    if (a.kind <= MPX_LR_COMMITS) {
        const uint4 m = *(reinterpret_cast<const uint4*>(a.items) + i);  // {instance, ballot, leader, value}
        const uint32_t eff = a.effect[i];
        bool cmds = true;
        if (a.kind == MPX_LR_ACCEPTS) {
            if (!(eff & MPX_AH_STORED)) return r;
        } else {
            cmds = (eff & MPX_CH_CMDS) && m.w != MPX_VALUE_KEEP;  // a CommitShort: metadata only
        }
        if (cmds) {
            c = msg_cmds(S, a.n_src, a.n_recs, a.perm, i, m.w, ebits);
            if (!c.ok) return r;
        }
    } else {
        const uint4* x = reinterpret_cast<const uint4*>(a.items) + 2 * i;
        const uint4 h = x[0];  // {instance, ballot, last_committed, flags}
        if (!(h.w & MPX_PH_ACCEPT)) return r;
        if (a.kind == MPX_LR_SENDS) {
            const uint4 f = x[1];  // {first_cmd, n_cmds, pad}
            c = send_cmds(S[0], (uint64_t)f.x | ((uint64_t)f.y << 32), f.z, ebits);
            if (!c.ok) return r;
        } else {
            const int64_t rel = (int64_t)(int32_t)h.x - a.inst_base;
            if (rel < 0 || (uint64_t)rel >= a.n_inst) {
                ebits |= kErrNil;
                return r;
            }
            if (!a.mask[rel]) return r;
        }
    }
    r.bytes = lr_hdr(a) + 17 * c.len, r.pos = cmd_pos(c.src, c.lo);
    return r;
}

// the items' offsets and source positions: in global memory (general path) or in LDS (one launch).
// find(q, t): the item holding output byte q, the last i with off(i) <= q (the empty ones before
// it start there too and are passed over); every thread calls, q < off(n).
struct LrAccGlobal {
    const uint64_t *o, *p;
    uint64_t n;
    __device__ __forceinline__ uint64_t off(uint64_t i) const { return o[i]; }
    __device__ __forceinline__ uint64_t pos(uint64_t i) const { return p[i]; }
    __device__ __forceinline__ uint64_t find(uint64_t q, int t) const { return holder(o, n, 0, q, t); }
};
struct LrAccLds {
    const uint64_t *o, *p;
    static constexpr uint64_t n = MPX_LR_ONE_LAUNCH_ITEMS;  // (the entries past the call's items are empty)
    __device__ __forceinline__ uint64_t off(uint64_t i) const { return o[i]; }
    __device__ __forceinline__ uint64_t pos(uint64_t i) const { return p[i]; }
    __device__ __forceinline__ uint64_t find(uint64_t q, int) const {
        return last_at_or_before([this](uint64_t i) { return o[i]; }, q, (uint64_t)0, n);
    }
};

// a workgroup's LDS for the window loop
struct LrLds {
    __attribute__((aligned(16))) uint32_t W[kLrWinWords];
    uint64_t i_pos[kLrT];  // the turn's items: source position of the item's first command,
    int64_t i_cs[kLrT];    // image byte of it (may lie before the image),
    uint32_t i_lo[kLrT];   // the first of its commands that the window overlaps
    uint32_t poff[kLrT + 1], wtot[kLrT / kWave];
};

// The windows of the run that this workgroup takes: window w is the 8 KB of ADDRESS space from
// base + w * 8 KB (base = out rounded down to 16 bytes, `head` bytes before out), and image byte x
// of it is output byte w * 8 KB + x - head. Every thread calls.
template <typename Acc>
__device__ __forceinline__ void lr_windows(const LrArgs& a, const CmdSrc* S, const Acc& acc, uint64_t total,
                                           uint64_t w0, uint64_t w_step, LrLds& L) {
    const int t = (int)threadIdx.x;
    const uint32_t hdr = lr_hdr(a), status = lr_status(a);
    const size_t stride = a.kind <= MPX_LR_COMMITS ? sizeof(mpx_accept_msg) : sizeof(mpx_accept_send);
    const uint64_t head = (uintptr_t)a.out & 15u;
    uint8_t* const base = a.out - head;
    const uint64_t span = total ? head + total : 0;
    for (uint64_t A0 = w0 * kLrWinBytes; A0 < span; A0 += w_step * kLrWinBytes) {
        const uint64_t A1 = A0 + kLrWinBytes < span ? A0 + kLrWinBytes : span;
        const uint64_t b0 = (A0 > head ? A0 : head) - head, b1 = A1 - head;  // the window's output bytes
#pragma unroll
        for (int i = 0; i < kLrWinBytes / 16 / kLrT; ++i)
            reinterpret_cast<uint4*>(L.W)[t + i * kLrT] = make_uint4(0, 0, 0, 0);
        const uint64_t first = acc.find(b0, t);
        __syncthreads();
        const int64_t shift = (int64_t)head - (int64_t)A0;  // output byte -> image byte
        // turns of kLrT items from the window's first, until a turn starts at or past the window's end
        for (uint64_t c0 = first; c0 < acc.n && acc.off(c0) < b1; c0 += kLrT) {
            const uint64_t i = c0 + t;
            uint32_t np = 0;
            if (i < acc.n) {
                const uint64_t rs = acc.off(i), re = acc.off(i + 1);
                if (re > rs && re > b0 && rs < b1) {  // it records, inside the window
                    const uint64_t nc = (re - rs - hdr) / 17, cs = rs + hdr;
                    if (cs > b0) {
                        const uint2 x = *reinterpret_cast<const uint2*>((const char*)a.items + i * stride);
                        uint32_t h[3] = {x.y, status, x.x};  // {instance, ballot} -> Ballot, Status, instNo
                        if (hdr == 5u) h[1] &= 0xFFu, h[2] = 0u;
                        image_or<kLrWinWords>(L.W, (int64_t)rs + shift, h, hdr);
                    }
                    const CmdSpan sp = cmd_span(cs, b0, b1);
                    const uint64_t hi = sp.hi < nc ? sp.hi : nc;
                    if (hi > sp.lo) {
                        np = (uint32_t)(hi - sp.lo);
                        L.i_pos[t] = acc.pos(i), L.i_cs[t] = (int64_t)cs + shift, L.i_lo[t] = (uint32_t)sp.lo;
                    }
                }
            }
            const uint32_t pieces = piece_scan(np, L.poff, L.wtot, t);
            // two commands per thread and round: both rounds' loads are in flight before the first OR
            for (uint32_t p0 = t; p0 < pieces; p0 += 2 * kLrT) {
                uint32_t o[2] = {0, 0};
                uint64_t k[2] = {0, 0}, v[2] = {0, 0};
                int64_t at[2] = {0, 0};
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t p = p0 + u * kLrT;
                    if (p >= pieces) continue;
                    const uint32_t x = piece_item(L.poff, p);
                    const uint64_t j = (uint64_t)L.i_lo[x] + (p - L.poff[x]), pos = L.i_pos[x];
                    const CmdSrc& s = S[cmd_pos_src(pos)];
                    const uint64_t c = cmd_pos_lo(pos) + j;
                    o[u] = s.op[c], k[u] = (uint64_t)s.key[c], v[u] = (uint64_t)s.val[c];
                    at[u] = L.i_cs[x] + 17 * (int64_t)j;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (p0 + u * kLrT < pieces) image_or_cmd<kLrWinWords>(L.W, at[u], o[u], k[u], v[u]);
            }
            __syncthreads();  // the turn's arrays are rewritten by the next
        }
        // image bytes [lo, hi) to base + A0: whole 16-byte vectors, the two ends bytewise
        const uint32_t lo = (uint32_t)(b0 + head - A0), hi = (uint32_t)(A1 - A0);
        const uint32_t v0 = (lo + 15u) / 16u, v1 = hi / 16u;
        uint8_t* const dst = base + A0;
        const uint8_t* const img = reinterpret_cast<const uint8_t*>(L.W);
        if (v0 < v1) {
            for (uint32_t v = v0 + t; v < v1; v += kLrT)
                st_stream(reinterpret_cast<uint4*>(dst) + v, reinterpret_cast<const uint4*>(L.W)[v]);
            for (uint32_t x = lo + t; x < v0 * 16u; x += kLrT) dst[x] = img[x];
            for (uint32_t x = v1 * 16u + t; x < hi; x += kLrT) dst[x] = img[x];
        } else {
            for (uint32_t x = lo + t; x < hi; x += kLrT) dst[x] = img[x];
        }
        __syncthreads();  // the image is zeroed by the next window
    }
}

__device__ __forceinline__ void lr_result(const LrArgs& a, uint64_t recs, uint64_t total, bool full) {
    a.res->n_recs = recs;
    a.res->n_cmds = (total - recs * lr_hdr(a)) / 17;
    a.res->n_bytes = total;
    a.res->flags = full ? MPX_LR_FULL : 0;
}

// the scan's ends: the sizes where k_lr_mark left them, the offsets over them (a tile reads its
// sizes before it writes its offsets, and no tile reads another's)
struct LrOffOut {
    uint64_t *off, *item_off;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t) const {
        off[i] = ex;
        if (item_off) item_off[i] = ex;
    }
};

}  // namespace

// ---- pass 1: what every item records -------------------------------------------------------------
// (n + 1 entries: the last, of size 0, becomes the total)
__global__ __launch_bounds__(kLrT) void k_lr_mark(LrArgs a, uint64_t* __restrict__ size,
                                                  uint64_t* __restrict__ pos, uint32_t* __restrict__ part) {
    __shared__ CmdSrc S[MPX_SC_MAX_SRC];
    cmd_sources(a.src, a.n_src, S);
    const uint64_t i = (uint64_t)blockIdx.x * kLrT + threadIdx.x;
    uint32_t ebits = 0;
    const LrItem x = lr_item(a, S, i, n_eff(a.d_n, a.n), ebits);
    if (i <= a.n) size[i] = x.bytes, pos[i] = x.pos;
    raise_bits(a.err, ebits, kErrInval | kErrNil);
    const uint32_t c = (uint32_t)__syncthreads_count(x.bytes != 0);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
}

// ---- pass 3: the bytes, the result ---------------------------------------------------------------
__global__ __launch_bounds__(kLrT) void k_lr_emit(LrArgs a, const uint64_t* __restrict__ off,
                                                  const uint64_t* __restrict__ pos,
                                                  const uint32_t* __restrict__ part, uint32_t n_part) {
    __shared__ CmdSrc S[MPX_SC_MAX_SRC];
    __shared__ LrLds L;
    __shared__ uint64_t ws[kLrT / kWave];
    cmd_sources(a.src, a.n_src, S);
    const uint32_t t = threadIdx.x;
    const uint64_t total = off[a.n];
    const bool full = total > a.out_cap;
    if (!full) lr_windows(a, S, LrAccGlobal{off, pos, a.n}, total, blockIdx.x, gridDim.x, L);
    if (blockIdx.x) return;
    uint64_t recs = 0;
    for (uint32_t x = t; x < n_part; x += kLrT) recs += part[x];
    recs = block_sum<uint64_t, kLrT>(recs, ws);
    if (t == 0) lr_result(a, recs, total, full);
}

// ---- one launch: a replica-sized batch in one workgroup, no scratch ------------------------------
__global__ __launch_bounds__(kLrT) void k_lr_one(LrArgs a) {
    __shared__ CmdSrc S[MPX_SC_MAX_SRC];
    __shared__ LrLds L;
    __shared__ uint64_t s_off[MPX_LR_ONE_LAUNCH_ITEMS + 1], s_pos[MPX_LR_ONE_LAUNCH_ITEMS];
    __shared__ uint64_t ws[kLrT / kWave];
    __shared__ uint32_t s_recs;
    cmd_sources(a.src, a.n_src, S);
    const uint32_t t = threadIdx.x;
    if (t == 0) s_recs = 0;
    const uint64_t n_items = n_eff(a.d_n, a.n);
    // items kLrOnePer * t ..: their sizes, scanned
    uint32_t ebits = 0, recs = 0;
    uint64_t bytes[kLrOnePer], sum = 0;
#pragma unroll
    for (int k = 0; k < kLrOnePer; ++k) {
        const LrItem x = lr_item(a, S, (uint64_t)t * kLrOnePer + k, n_items, ebits);
        bytes[k] = x.bytes, s_pos[t * kLrOnePer + k] = x.pos;
        sum += x.bytes, recs += x.bytes != 0;
    }
    raise_bits(a.err, ebits, kErrInval | kErrNil);
    uint64_t run = block_excl_scan<uint64_t, kLrT>(sum, ws);
    if (recs) atomicAdd(&s_recs, recs);
#pragma unroll
    for (int k = 0; k < kLrOnePer; ++k) {
        s_off[t * kLrOnePer + k] = run;
        run += bytes[k];
    }
    if (t == kLrT - 1) s_off[MPX_LR_ONE_LAUNCH_ITEMS] = run;
    __syncthreads();
    const uint64_t total = s_off[MPX_LR_ONE_LAUNCH_ITEMS];
    const bool full = total > a.out_cap;
    if (t == 0) lr_result(a, s_recs, total, full);
    if (a.item_off)
        for (uint64_t i = t; i <= a.n; i += kLrT) a.item_off[i] = s_off[i];
    if (full) return;
    lr_windows(a, S, LrAccLds{s_off, s_pos}, total, 0, 1, L);
}

namespace {
struct LrWork {
    uint64_t *off, *pos, *scan_tmp;
    uint32_t* part;
    LrWork(Carver& c, uint64_t n) {
        off = c.take<uint64_t>(n + 1);
        pos = c.take<uint64_t>(n + 1);
        part = c.take<uint32_t>(n / kLrT + 2);
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(n + 1));
    }
};
}  // namespace

uint64_t record_work_bytes(uint64_t n, Carver&& c) { return LrWork(c, n), c.bytes(); }

hipError_t launch_record_log(const mpx_record_batch* b, uint8_t* out, uint64_t out_cap, uint64_t* item_off,
                             mpx_record_result* res, void* work, uint64_t work_bytes, uint32_t* err,
                             hipStream_t stream) {
    const uint64_t n = b->n;
    if (n >= 0xFFFFFFFFull || b->n_src > MPX_SC_MAX_SRC || b->kind > MPX_LR_DECIDED ||
        (b->format != MPX_LOG_DURABLE && b->format != MPX_LOG_DURABLE_CLASSIC))
        return hipErrorInvalidValue;
    LrArgs a{};
    a.items = b->items, a.effect = b->effect, a.mask = b->mask, a.perm = b->perm, a.d_n = b->d_n;
    a.n = n, a.n_inst = b->n_inst, a.out_cap = out_cap;
    a.out = out, a.item_off = item_off, a.res = res, a.err = err;
    a.inst_base = b->inst_base, a.kind = b->kind, a.format = b->format;
    a.n_src = b->kind == MPX_LR_DECIDED ? 0u : (uint32_t)b->n_src;
    uint64_t cmds;
    fill_cmd_sources(b->src, a.n_src, a.src, a.n_recs, cmds);
    if (!n || (!(b->flags & MPX_LR_GENERAL) && n <= MPX_LR_ONE_LAUNCH_ITEMS && cmds <= MPX_LR_ONE_LAUNCH_CMDS)) {
        k_lr_one<<<1, kLrT, 0, stream>>>(a);  // (also a call of no item: the kernel writes the result)
        return hipGetLastError();
    }
    Carver c(work);
    const LrWork w(c, n);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(n / kLrT + 1);  // n + 1 entries
    k_lr_mark<<<blocks, kLrT, 0, stream>>>(a, w.off, w.pos, w.part);
    const hipError_t r = device_scan(SizeIn{w.off}, LrOffOut{w.off, item_off}, n + 1, ScanSum64{}, (uint64_t)0,
                                     w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    const uint64_t windows = out_cap / kLrWinBytes + 2;
    k_lr_emit<<<(unsigned)std::min<uint64_t>(windows, kLrGrid), kLrT, 0, stream>>>(a, w.off, w.pos, w.part, blocks);
    return hipGetLastError();
}

}  // namespace mpx

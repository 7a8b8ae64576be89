// store.hip — store assembly: the batch's instance commands into the device command arena, and
// the arena's compaction.
//
// Reference: where the Go assigns an instance's commands. MIN handleAccept's fresh Instance{...,
// accept.Command} (bareminpaxos.go:786-793), CLASSIC's cmds = accept.Command (paxos.go:479-483,
// :491, :506), handleCommit's Instance{..., commit.Command} / Cmds = commit.Command
// (bareminpaxos.go:861-868 / paxos.go:526-534), handlePropose's installed instance
// (bareminpaxos.go:687-699 / paxos.go:410-437). The handlers run per message in array order and
// the batch is grouped by instance, so of one instance's storing items the last wins: a storing
// item loses exactly when the NEXT STORING item of the array names its instance. Nothing here is
// per window slot: the passes run over the n items and the commands copied.
// The pieces shared with the other assembly families are assemble.hpp's.
//   k_st_mark   an item per thread: whether it stores, how many commands, and where they start in
//               its source (assemble.hpp's msg_cmds / send_cmds)
//   scan.hpp    the storing items compacted into a list (their count beside it)
//   k_st_win    a list entry per thread: it wins unless the next entry names its instance; the
//               winners' lengths, the workgroups' winner counts, the cursor as the call found it
//   scan.hpp    the lengths' exclusive scan: where each winner's commands go
//   k_st_copy   balanced over OUTPUT positions: a tile of kStTile arena positions per workgroup (a
//               grid of at most kStGrid walks the tiles), four consecutive ones per thread, cut at
//               multiples of four of the ARENA index, so that a thread's key / val stores are
//               16-byte ones whichever way the arrays lie mod 16 and its op bytes one dword; the
//               tile's first and last entry by frames.hpp's holder. Then a winner per thread: its
//               mpx_inst_cmds; then the result record and the cursor. Nothing is written when the
//               arena cannot take the batch.
// Launches: 9. A call of at most MPX_SC_ONE_LAUNCH_ITEMS items whose sources hold at most
// MPX_SC_ONE_LAUNCH_CMDS commands is one kernel in one workgroup: an item per thread, the list and
// the offsets in LDS. Compaction is the same mark / scan / copy over window slots as the items, every
// flagged slot a winner (5 launches).
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

constexpr int kStT = 256;                 // threads of the item and tile workgroups
constexpr int kStPer = 4;                 // arena positions per thread
constexpr int kStTile = kStT * kStPer;    // 1024
constexpr int kStOneT = 1024;             // threads of the one-launch workgroup: an item each
constexpr int kStGrid = 1024;             // workgroups of k_st_copy at most
constexpr uint32_t kStNone = 0xFFFFFFFFu; // a length: the item does not store / the entry lost
constexpr uint32_t kStCompact = 2u;       // StArgs.kind of a compaction (beside MPX_SC_MSGS / _SENDS)
constexpr int kStWords = 4;               // the call's words: [0] storing items, [1] the cursor found
static_assert(kStT == kFrBlock, "holder() is for kFrBlock threads");
static_assert(MPX_SC_ONE_LAUNCH_ITEMS == kStOneT, "the one-launch kernel takes an item per thread");
static_assert(MPX_SC_MAX_SRC == MPX_ORDER_MAX_SRC, "a source per ordered connection");
static_assert(sizeof(mpx_accept_msg) == 16 && sizeof(mpx_accept_send) == 32 && sizeof(mpx_inst_cmds) == 16,
              "vector loads and stores per record");

// the call, by value to every kernel
struct StArgs {
    const void* items;
    const uint8_t* effect;
    const uint32_t* perm;
    const uint64_t* d_n;
    const uint64_t* from_used;  // compaction: the source arena's cursor
    uint64_t n, n_inst, n_recs, cap;
    uint8_t* a_op;
    int64_t *a_key, *a_val;
    uint64_t* used;
    mpx_inst_cmds* inst;
    mpx_store_result* res;
    uint32_t* err;
    int32_t inst_base;
    uint32_t kind, n_src, store_mask;
    CmdSrc src[MPX_SC_MAX_SRC];
};

__device__ __forceinline__ int32_t st_instance(const StArgs& a, uint64_t i) {
    const char* p = (const char*)a.items + i * (a.kind == MPX_SC_SENDS ? sizeof(mpx_accept_send)
                                                                       : sizeof(mpx_accept_msg));
    return *reinterpret_cast<const int32_t*>(p);
}

// What item i stores: len == kStNone when it does not (also a faulty one: its bit is raised).
// pos: assemble.hpp's cmd_pos of its first command.
struct StItem {
    uint32_t len;
    int32_t instance;
    uint64_t pos;
};
__device__ __forceinline__ StItem st_item(const StArgs& a, const CmdSrc* S, uint64_t i, uint64_t n_eff,
                                          uint32_t& ebits) {
    StItem r{kStNone, 0, 0};
    if (i >= n_eff) return r;
    CmdRange c{0, 0, 0, true};
    if (a.kind == kStCompact) {
        const uint4 h = *reinterpret_cast<const uint4*>(a.inst + i);  // {first_cmd, n_cmds, flags}
        if (!(h.w & MPX_IC_HAS_CMDS)) return r;
        uint64_t lo = (uint64_t)h.x | ((uint64_t)h.y << 32), len = h.z;
        uint64_t bound = *a.from_used;
        bound = bound < S[0].n_cmds ? bound : S[0].n_cmds;
        if (lo > bound || len > bound - lo || len == kStNone) ebits |= kErrInval, lo = 0, len = 0;
        r.len = (uint32_t)len, r.pos = lo;
        return r;
    }
    if (a.kind == MPX_SC_MSGS) {
        const uint4 m = *(reinterpret_cast<const uint4*>(a.items) + i);  // {instance, ballot, leader, value}
        if (!(a.effect[i] & a.store_mask) || m.w == MPX_VALUE_KEEP) return r;
        r.instance = (int32_t)m.x;
        c = msg_cmds(S, a.n_src, a.n_recs, a.perm, i, m.w, ebits);
    } else {
        const uint4* x = reinterpret_cast<const uint4*>(a.items) + 2 * i;
        const uint4 h = x[0], f = x[1];  // {instance, ballot, last_committed, flags} {first_cmd, n_cmds, pad}
        if (!(h.w & (MPX_PH_ACCEPT | MPX_PH_PREPARE))) return r;
        r.instance = (int32_t)h.x;
        c = send_cmds(S[0], (uint64_t)f.x | ((uint64_t)f.y << 32), f.z, ebits);
    }
    if (!c.ok) return r;
    const int64_t rel = (int64_t)r.instance - a.inst_base;
    if (rel < 0 || (uint64_t)rel >= a.n_inst) {
        ebits |= kErrNil;
        return r;
    }
    r.len = (uint32_t)c.len, r.pos = cmd_pos(c.src, c.lo);
    return r;
}

// Arena positions q0 .. q0 + 3 (q0 a multiple of 4): those inside [first, first + total) take the
// call's output positions q - first, whose entries lie in [e_lo, e_hi].
template <typename Acc>
__device__ __forceinline__ void st_emit4(const StArgs& a, const CmdSrc* S, const Acc& acc, uint64_t q0,
                                         uint64_t first, uint64_t total, uint32_t e_lo, uint32_t e_hi) {
    uint32_t o[kStPer];
    uint64_t k[kStPer], v[kStPer];
    bool in[kStPer];
    uint32_t e = e_lo;
    uint64_t begin = 0, end = 0, from = 0;
    const uint8_t* s_op = nullptr;
    const int64_t *s_key = nullptr, *s_val = nullptr;
    bool any = false, started = false;
#pragma unroll
    for (int j = 0; j < kStPer; ++j) {
        const uint64_t q = q0 + j;
        in[j] = q >= first && q - first < total;
        o[j] = 0, k[j] = 0, v[j] = 0;
        if (in[j]) {
            const uint64_t p = q - first;
            if (!started || p >= end) {
                e = last_at_or_before([&](uint32_t x) { return acc.off(x); }, p, started ? e + 1 : e_lo, e_hi + 1);
                begin = acc.off(e), end = acc.off(e + 1);
                const uint64_t pos = acc.pos(e);
                const CmdSrc& s = S[cmd_pos_src(pos)];
                s_op = s.op, s_key = s.key, s_val = s.val;
                from = cmd_pos_lo(pos);
                started = true;
            }
            const uint64_t src = from + (p - begin);
            o[j] = s_op[src];
            k[j] = (uint64_t)s_key[src];
            v[j] = (uint64_t)s_val[src];
            any = true;
        }
    }
    if (any) store4_cmds(a.a_op + q0, a.a_key + q0, a.a_val + q0, o, k, v, in);
}

// whether the arena takes `total` more commands after `used0` (a cursor past cap is an error)
__device__ __forceinline__ bool st_full(const StArgs& a, uint64_t used0, uint64_t total, bool& bad) {
    bad = used0 > a.cap;
    return bad || total > a.cap - used0;
}

// the record of a winner whose commands went to `first`
__device__ __forceinline__ void st_put_slot(const StArgs& a, uint64_t idx, uint64_t first, uint32_t len) {
    *reinterpret_cast<uint4*>(a.inst + idx) =
        make_uint4((uint32_t)first, (uint32_t)(first >> 32), len, MPX_IC_HAS_CMDS);
}

// the scans' ends
struct StFlagIn {
    const uint32_t* st;
    uint64_t n;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return st[i] != kStNone; }
};
struct StListOut {
    uint32_t* list;
    uint64_t* words;
    uint64_t n;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t ex, uint32_t item) const {
        if (item) list[ex] = (uint32_t)i;
        if (i == n - 1) words[0] = (uint64_t)ex + item;
    }
};
struct StLenIn {
    const uint32_t* wl;
    uint64_t n;
    __device__ __forceinline__ uint64_t operator()(uint64_t k) const {
        const uint32_t x = k < n ? wl[k] : kStNone;
        return x != kStNone ? x : 0;
    }
};
struct StOffOut {
    uint64_t* off;
    __device__ __forceinline__ void operator()(uint64_t k, uint64_t ex, uint64_t) const { off[k] = ex; }
};

// the entries' offsets and source positions: in global memory (general path) or in LDS (one launch)
struct StAccGlobal {
    const uint64_t* o;
    const uint32_t* list;  // null: entry k is item k (compaction)
    const uint64_t* p;
    __device__ __forceinline__ uint64_t off(uint32_t k) const { return o[k]; }
    __device__ __forceinline__ uint64_t pos(uint32_t k) const { return p[list ? list[k] : k]; }
};
struct StAccLds {
    const uint64_t *o, *p;
    __device__ __forceinline__ uint64_t off(uint32_t k) const { return o[k]; }
    __device__ __forceinline__ uint64_t pos(uint32_t k) const { return p[k]; }
};

}  // namespace

// ---- pass 1: what every item stores --------------------------------------------------------------
__global__ __launch_bounds__(kStT) void k_st_mark(StArgs a, uint32_t* __restrict__ st,
                                                  uint64_t* __restrict__ pos, uint64_t* __restrict__ words,
                                                  uint32_t* __restrict__ part) {
    __shared__ CmdSrc S[MPX_SC_MAX_SRC];
    cmd_sources(a.src, a.n_src, S);
    const uint64_t i = (uint64_t)blockIdx.x * kStT + threadIdx.x;
    uint32_t ebits = 0;
    const StItem x = st_item(a, S, i, n_eff(a.d_n, a.n), ebits);
    if (i < a.n) st[i] = x.len, pos[i] = x.pos;
    raise_bits(a.err, ebits, kErrInval | kErrNil);
    if (a.kind != kStCompact) return;  // (the same in every thread)
    // compaction: every flagged slot is a winner, entry k is slot k, the target starts at 0
    const uint32_t c = (uint32_t)__syncthreads_count(x.len != kStNone);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
    if (i == 0) words[0] = a.n, words[1] = 0;
}

// ---- pass 3: the winners among the storing items -------------------------------------------------
__global__ __launch_bounds__(kStT) void k_st_win(StArgs a, const uint32_t* __restrict__ st,
                                                 const uint32_t* __restrict__ list,
                                                 uint32_t* __restrict__ wl, uint64_t* __restrict__ words,
                                                 uint32_t* __restrict__ part) {
    const uint64_t k = (uint64_t)blockIdx.x * kStT + threadIdx.x;
    const uint64_t ns = words[0];
    bool win = false;
    uint32_t len = kStNone;
    if (k < ns) {
        const uint32_t i = list[k];
        win = k + 1 >= ns || st_instance(a, list[k + 1]) != st_instance(a, i);
        if (win) len = st[i];
    }
    if (k < a.n) wl[k] = len;
    const uint32_t c = (uint32_t)__syncthreads_count(win);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
    if (k == 0) words[1] = *a.used;
}

// ---- pass 5: the commands, the slots, the result -------------------------------------------------
__global__ __launch_bounds__(kStT) void k_st_copy(StArgs a, const uint32_t* __restrict__ list,
                                                  const uint32_t* __restrict__ wl,
                                                  const uint64_t* __restrict__ pos,
                                                  const uint64_t* __restrict__ off,
                                                  const uint64_t* __restrict__ words,
                                                  const uint32_t* __restrict__ part, uint32_t n_part) {
    __shared__ CmdSrc S[MPX_SC_MAX_SRC];
    __shared__ uint64_t ws[kStT / kWave];
    cmd_sources(a.src, a.n_src, S);
    const uint32_t t = threadIdx.x;
    const uint64_t total = off[a.n], ns = words[0], used0 = words[1];
    bool bad;
    const bool full = st_full(a, used0, total, bad);
    if (!full) {
        const StAccGlobal acc{off, list, pos};
        const uint64_t base = used0 & ~3ull, head = used0 & 3ull, span = total ? head + total : 0;
        for (uint64_t lo = (uint64_t)blockIdx.x * kStTile; lo < span; lo += (uint64_t)gridDim.x * kStTile) {
            const uint64_t hi = lo + kStTile < span ? lo + kStTile : span;
            const uint64_t p_lo = (lo > head ? lo : head) - head, p_hi = hi - head - 1;
            const uint32_t e_lo = (uint32_t)holder(off, a.n, 0, p_lo, (int)t);
            const uint32_t e_hi = (uint32_t)holder(off, a.n, e_lo, p_hi, (int)t);
            st_emit4(a, S, acc, base + lo + (uint64_t)t * kStPer, used0, total, e_lo, e_hi);
        }
        for (uint64_t k = (uint64_t)blockIdx.x * kStT + t; k < ns; k += (uint64_t)gridDim.x * kStT) {
            const uint32_t len = wl[k];
            if (len == kStNone) continue;
            if (a.kind == kStCompact) st_put_slot(a, k, off[k], len);
            else st_put_slot(a, (uint64_t)((int64_t)st_instance(a, list[k]) - a.inst_base), used0 + off[k], len);
        }
    }
    if (blockIdx.x) return;
    uint64_t won = 0;
    for (uint32_t x = t; x < n_part; x += kStT) won += part[x];
    won = block_sum<uint64_t, kStT>(won, ws);
    if (t == 0) {
        a.res->n_stored = won;
        a.res->n_cmds = total;
        a.res->n_superseded = a.kind == kStCompact ? 0 : ns - won;
        a.res->flags = full ? MPX_SC_FULL : 0;
        if (!full) *a.used = used0 + total;
        if (bad) raise_err(a.err, kErrInval);
    }
}

// ---- one launch: a replica-sized batch in one workgroup, no scratch ------------------------------
__global__ __launch_bounds__(kStOneT) void k_st_one(StArgs a) {
    __shared__ CmdSrc S[MPX_SC_MAX_SRC];
    __shared__ uint32_t c_len[kStOneT];
    __shared__ int32_t c_inst[kStOneT];
    __shared__ uint64_t c_pos[kStOneT], s_off[kStOneT + 1];
    __shared__ uint64_t ws[kStOneT / kWave];
    cmd_sources(a.src, a.n_src, S);
    const uint32_t t = threadIdx.x;
    const uint64_t used0 = *a.used;
    uint32_t ebits = 0;
    const StItem x = st_item(a, S, t, n_eff(a.d_n, a.n), ebits);
    raise_bits(a.err, ebits, kErrInval | kErrNil);
    // the storing items' list
    const uint32_t flag = x.len != kStNone;
    // (not assemble.hpp's block_excl_scan: one fixed-trip select gives the prefix and the total from
    // four 16-byte LDS reads; the helper's loop to the thread's own wave read 0.2 us slower here)
    const uint32_t incl = wave_incl_scan(flag, ScanSum32{});
    if (lane_id() == kWave - 1) ws[t / kWave] = incl;
    __syncthreads();
    uint32_t before = 0, ns = 0;
    for (uint32_t w = 0; w < kStOneT / kWave; ++w) {
        before += w < t / kWave ? (uint32_t)ws[w] : 0u;
        ns += (uint32_t)ws[w];
    }
    if (flag) {
        const uint32_t k = before + incl - 1;
        c_len[k] = x.len, c_inst[k] = x.instance, c_pos[k] = x.pos;
    }
    __syncthreads();
    // the winners and their offsets
    const bool win = t < ns && (t + 1 >= ns || c_inst[t + 1] != c_inst[t]);
    const uint32_t len = win ? c_len[t] : 0u;
    s_off[t + 1] = block_excl_scan<uint64_t, kStOneT>((uint64_t)len, ws) + len;
    if (t == 0) s_off[0] = 0;
    const uint32_t won = (uint32_t)__syncthreads_count(win);
    const uint64_t total = s_off[kStOneT];
    bool bad;
    const bool full = st_full(a, used0, total, bad);
    if (t == 0) {
        a.res->n_stored = won;
        a.res->n_cmds = total;
        a.res->n_superseded = ns - won;
        a.res->flags = full ? MPX_SC_FULL : 0;
        if (!full) *a.used = used0 + total;
        if (bad) raise_err(a.err, kErrInval);
    }
    if (full) return;
    if (win) st_put_slot(a, (uint64_t)((int64_t)c_inst[t] - a.inst_base), used0 + s_off[t], len);
    const StAccLds acc{s_off, c_pos};
    const uint64_t base = used0 & ~3ull, span = total ? (used0 & 3ull) + total : 0;
    for (uint64_t lo = 0; lo < span; lo += kStOneT * kStPer)
        st_emit4(a, S, acc, base + lo + (uint64_t)t * kStPer, used0, total, 0u, ns - 1);
}

// an empty compaction: the result and the target's cursor
__global__ void k_st_empty(mpx_store_result* res, uint64_t* used) {
    if (threadIdx.x == 0) {
        res->n_stored = res->n_cmds = res->n_superseded = res->flags = 0;
        *used = 0;
    }
}

namespace {
struct StWork {
    uint64_t *words, *pos, *off, *scan_tmp;
    uint32_t *st, *list, *wl, *part;
    StWork(Carver& c, uint64_t n) {
        words = c.take<uint64_t>(kStWords);
        st = c.take<uint32_t>(n);
        pos = c.take<uint64_t>(n);
        list = c.take<uint32_t>(n + 1);
        wl = c.take<uint32_t>(n + 1);
        off = c.take<uint64_t>(n + 1);
        part = c.take<uint32_t>((n + kStT - 1) / kStT + 1);
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(n + 1));
    }
};

// the tiles and winners k_st_copy's grid walks: at most kStGrid workgroups
unsigned st_copy_grid(uint64_t cap, uint64_t n) {
    const uint64_t tiles = (cap + 3) / kStTile + 1, blocks = (n + kStT - 1) / kStT;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(std::max(tiles, blocks), 1), kStGrid);
}
}  // namespace

uint64_t store_work_bytes(uint64_t n, Carver&& c) { return StWork(c, n), c.bytes(); }

hipError_t launch_store_commands(const mpx_store_batch* b, const mpx_store_arena* arena,
                                 mpx_inst_cmds* inst, mpx_store_result* res, void* work,
                                 uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    const uint64_t n = b->n;
    if (n >= 0xFFFFFFFFull || !b->n_src || b->n_src > MPX_SC_MAX_SRC || b->kind > MPX_SC_SENDS)
        return hipErrorInvalidValue;
    StArgs a{};
    a.items = b->items, a.effect = b->effect, a.perm = b->perm, a.d_n = b->d_n;
    a.n = n, a.n_inst = b->n_inst, a.cap = arena->cap;
    a.a_op = arena->op, a.a_key = arena->key, a.a_val = arena->val, a.used = arena->used;
    a.inst = inst, a.res = res, a.err = err;
    a.inst_base = b->inst_base, a.kind = b->kind, a.n_src = (uint32_t)b->n_src, a.store_mask = b->store_mask;
    uint64_t cmds;
    fill_cmd_sources(b->src, b->n_src, a.src, a.n_recs, cmds);
    if (!(b->flags & MPX_SC_GENERAL) && n <= MPX_SC_ONE_LAUNCH_ITEMS && cmds <= MPX_SC_ONE_LAUNCH_CMDS) {
        k_st_one<<<1, kStOneT, 0, stream>>>(a);
        return hipGetLastError();
    }
    if (!n) {  // nothing stores: the one kernel writes the result
        k_st_one<<<1, kStOneT, 0, stream>>>(a);
        return hipGetLastError();
    }
    Carver c(work);
    const StWork w(c, n);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n + kStT - 1) / kStT);
    k_st_mark<<<blocks, kStT, 0, stream>>>(a, w.st, w.pos, w.words, w.part);
    hipError_t r = device_scan(StFlagIn{w.st, n}, StListOut{w.list, w.words, n}, n, ScanSum32{},
                               (uint32_t)0, (uint32_t*)w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    k_st_win<<<blocks, kStT, 0, stream>>>(a, w.st, w.list, w.wl, w.words, w.part);
    r = device_scan(StLenIn{w.wl, n}, StOffOut{w.off}, n + 1, ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    k_st_copy<<<st_copy_grid(arena->cap, n), kStT, 0, stream>>>(a, w.list, w.wl, w.pos, w.off, w.words,
                                                               w.part, blocks);
    return hipGetLastError();
}

hipError_t launch_store_compact(mpx_inst_cmds* inst, uint64_t n_inst, const mpx_store_arena* from,
                                const mpx_store_arena* to, mpx_store_result* res, void* work,
                                uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    if (n_inst >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (!n_inst) {
        k_st_empty<<<1, kWave, 0, stream>>>(res, to->used);
        return hipGetLastError();
    }
    StArgs a{};
    a.from_used = from->used;
    a.n = a.n_inst = n_inst, a.cap = to->cap;
    a.a_op = to->op, a.a_key = to->key, a.a_val = to->val, a.used = to->used;
    a.inst = inst, a.res = res, a.err = err;
    a.kind = kStCompact, a.n_src = 1;
    a.src[0] = CmdSrc{nullptr, from->op, from->key, from->val, 0, from->cap, 0};
    Carver c(work);
    const StWork w(c, n_inst);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n_inst + kStT - 1) / kStT);
    // (a slot's length is its winner's length: the mark pass writes the lengths where the copy reads them)
    k_st_mark<<<blocks, kStT, 0, stream>>>(a, w.wl, w.pos, w.words, w.part);
    const hipError_t r = device_scan(StLenIn{w.wl, n_inst}, StOffOut{w.off}, n_inst + 1, ScanSum64{},
                                     (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    k_st_copy<<<st_copy_grid(to->cap, n_inst), kStT, 0, stream>>>(a, nullptr, w.wl, w.pos, w.off, w.words,
                                                                 w.part, blocks);
    return hipGetLastError();
}

}  // namespace mpx

// execute.hip — execute assembly: executeCommands' walk and the gather of its commands.
//
// Reference: executeCommands, bareminpaxos.go:1066-1098 / paxos.go:675-706 (the same code): per
// group, from the last executed instance up to committedUpTo, stop at the first instance whose
// Cmds is nil, Execute the others' commands in order. One replica is one group of up to 2^24
// slots, so the walk is not a lane per group: a group's stop is the MINIMUM window slot inside
// (executed, committed] that lacks MPX_IC_HAS_CMDS, and every slot below it in that range runs.
//   k_xg_stop    a tile of kXgTile slots per workgroup: the first such slot per group inside each
//                64-slot unit by ballots, the units of a tile settled in LDS, one atomic minimum
//                per (tile, group) into the group's stop word (kXgNoStop between calls)
//   k_xg_mark    the same tiles: mask, and the executed slots' lengths
//   scan.hpp     the lengths' exclusive scan: inst_first, and the total as item n_inst
//   k_xg_gather  balanced over OUTPUT positions: a tile of kXgTile commands per workgroup, four
//                consecutive positions per thread, the tile's first and last instance by frames.hpp's
//                holder; 16-byte key / val stores and a dword of op bytes where aligned; the pad tail
//   k_xg_groups  a group or a send per thread: executed_out, grp_cmd_off, ret_first, the stop
//                words put back, the blocks' counts
//   k_xg_finish  the result record
// Launches: 8. A call of at most MPX_XG_ONE_LAUNCH_INST slots and MPX_XG_ONE_LAUNCH_CMDS commands
// of capacity is one kernel in one workgroup: a slot per thread, stops and offsets in LDS.
// The pieces shared with the other assembly families are assemble.hpp's.
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

constexpr int kXgT = 256;       // threads of the tile workgroups
constexpr int kXgPer = 4;       // slots (k_xg_stop, k_xg_mark) or positions (k_xg_gather) per thread
constexpr int kXgTile = kXgT * kXgPer;   // 1024
constexpr int kXgUnits = kXgTile / kWave;  // 64-slot units of a tile, in array order
constexpr int kXgOneT = 1024;   // threads of the one-launch workgroup: a slot each
constexpr int kXgFinT = 1024;
static_assert(kXgT == kFrBlock, "holder() is for kFrBlock threads");
static_assert(MPX_XG_ONE_LAUNCH_INST == kXgOneT, "the one-launch kernel takes a slot per thread");
static_assert(sizeof(mpx_inst_cmds) == 16, "one vector load per slot");

// the call, by value to every kernel
struct XgArgs {
    const mpx_inst_cmds* inst;
    const int32_t *cu, *ex_in;
    int32_t* ex_out;
    const uint8_t* src_op;
    const int64_t *src_key, *src_val;
    const mpx_accept_send* sends;
    uint64_t n_inst, n_groups, n_src, n_sends, cap;
    int32_t inst_base;
    uint32_t ipg, pad;
    uint8_t* op;
    int64_t *key, *val;
    uint8_t* mask;
    uint64_t *inst_first, *ret_first, *grp_cmd_off;
    mpx_execute_result* res;
    uint32_t* err;
};

// group g's cursors: usable when both lie in [first_g - 1, first_g + ipg - 1]
struct XgGroup {
    int64_t cu, ex;
    bool ok;
};
__device__ __forceinline__ XgGroup xg_group(const XgArgs& a, uint32_t g) {
    const int64_t none = (int64_t)a.inst_base + (int64_t)((uint64_t)g * a.ipg) - 1;
    const int64_t cu = a.cu[g], ex = a.ex_in[g];
    return {cu, ex, cu >= none && cu <= none + a.ipg && ex >= none && ex <= none + a.ipg};
}

struct XgSlot {
    uint32_t g, n;
    uint64_t first;
    bool in_range;  // inside (executed, committed] of a usable group
    bool has;       // MPX_IC_HAS_CMDS
    bool bad_group; // the group's first slot, and the group is not usable
};
__device__ __forceinline__ XgSlot xg_slot(const XgArgs& a, uint32_t idx) {
    const uint4 h = *reinterpret_cast<const uint4*>(a.inst + idx);  // {first_cmd, n_cmds, flags}
    XgSlot s;
    s.g = idx / a.ipg;
    const XgGroup G = xg_group(a, s.g);
    const int64_t i = (int64_t)a.inst_base + idx;
    s.first = (uint64_t)h.x | ((uint64_t)h.y << 32);
    s.n = h.z;
    s.has = (h.w & MPX_IC_HAS_CMDS) != 0;
    s.in_range = G.ok && i > G.ex && i <= G.cu;
    s.bad_group = !G.ok && idx == s.g * a.ipg;
    return s;
}
// the commands an executed slot contributes: none when its range leaves the source
__device__ __forceinline__ uint32_t xg_len(const XgArgs& a, const XgSlot& s, uint32_t& ebits) {
    if (s.first > a.n_src || s.n > a.n_src - s.first) {
        ebits |= kErrInval;
        return 0;
    }
    return s.n;
}

// executed_out of group g given its stop word, and what the result record counts
__device__ __forceinline__ int64_t xg_cursor(const XgArgs& a, const XgGroup& G, uint32_t stop) {
    if (!G.ok || G.ex >= G.cu) return G.ex;
    return stop != kXgNoStop ? (int64_t)a.inst_base + stop - 1 : G.cu;
}

__device__ __forceinline__ uint64_t xg_ret_first(const XgArgs& a, uint64_t s, const uint64_t* off) {
    const int64_t rel = (int64_t)a.sends[s].instance - a.inst_base;
    return rel >= 0 && (uint64_t)rel < a.n_inst ? off[rel] : 0;
}

// the scanned offsets, in global memory (general path) or in LDS (one launch)
struct XgOff {
    const uint64_t* off;
    __device__ __forceinline__ uint64_t operator()(uint32_t i) const { return off[i]; }
};
// Positions p0 .. p0 + 3 (p0 a multiple of 4): the first n_real are gathered commands whose
// instances lie in [i_lo, i_hi], the others up to n_out pad commands {NONE, key p, 0}.
__device__ __forceinline__ void xg_emit4(const XgArgs& a, uint64_t p0, uint32_t n_real,
                                         uint32_t n_out, const XgOff off, uint32_t i_lo,
                                         uint32_t i_hi) {
    uint32_t o[kXgPer];
    uint64_t k[kXgPer], v[kXgPer];
    uint32_t inst = i_lo;
    uint64_t begin = 0, end = 0, first = 0;
#pragma unroll
    for (int j = 0; j < kXgPer; ++j) {
        const uint64_t p = p0 + j;
        o[j] = 0, k[j] = p, v[j] = 0;
        if ((uint32_t)j < n_real) {
            if (j == 0 || p >= end) {
                inst = last_at_or_before(off, p, j ? inst + 1 : i_lo, i_hi + 1);
                begin = off(inst), end = off(inst + 1);
                first = a.inst[inst].first_cmd;
            }
            const uint64_t src = first + (p - begin);
            o[j] = a.src_op[src];
            k[j] = (uint64_t)a.src_key[src];
            v[j] = (uint64_t)a.src_val[src];
        }
    }
    // (not assemble.hpp's store4_cmds: its test per array costs the gather 1-3 % on aligned arrays)
    uint8_t* const d_op = a.op + p0;
    int64_t *const d_key = a.key + p0, *const d_val = a.val + p0;
    if (n_out >= kXgPer) {
        if ((((uintptr_t)d_key | (uintptr_t)d_val) & 15) == 0) {
#pragma unroll
            for (int j = 0; j < kXgPer; j += 2) {
                reinterpret_cast<uint4*>(d_key)[j / 2] = make_uint4(
                    (uint32_t)k[j], (uint32_t)(k[j] >> 32), (uint32_t)k[j + 1], (uint32_t)(k[j + 1] >> 32));
                reinterpret_cast<uint4*>(d_val)[j / 2] = make_uint4(
                    (uint32_t)v[j], (uint32_t)(v[j] >> 32), (uint32_t)v[j + 1], (uint32_t)(v[j + 1] >> 32));
            }
        } else {
#pragma unroll
            for (int j = 0; j < kXgPer; ++j) d_key[j] = (int64_t)k[j], d_val[j] = (int64_t)v[j];
        }
        if (((uintptr_t)d_op & 3) == 0) {
            *reinterpret_cast<uint32_t*>(d_op) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < kXgPer; ++j) d_op[j] = (uint8_t)o[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < kXgPer; ++j)
            if ((uint32_t)j < n_out) d_op[j] = (uint8_t)o[j], d_key[j] = (int64_t)k[j], d_val[j] = (int64_t)v[j];
    }
}

// One tile of T * kXgPer output positions from lo (clipped to cap): what thread t writes of it.
// total: the gathered commands; the tile's instances lie in [i_lo, i_hi] when it holds any.
template <int T>
__device__ __forceinline__ void xg_emit_tile(const XgArgs& a, uint64_t lo, uint64_t total,
                                             const XgOff off, uint32_t i_lo, uint32_t i_hi) {
    const uint64_t p0 = lo + (uint64_t)threadIdx.x * kXgPer;
    const uint64_t real_end = total < a.cap ? total : a.cap;
    const uint64_t out_end = a.pad ? a.cap : real_end;
    if (p0 >= out_end) return;
    const uint32_t n_out = (uint32_t)(out_end - p0 < kXgPer ? out_end - p0 : kXgPer);
    const uint32_t n_real = p0 >= real_end ? 0u : (uint32_t)(real_end - p0 < kXgPer ? real_end - p0 : kXgPer);
    xg_emit4(a, p0, n_real, n_out, off, i_lo, i_hi);
}

// the scan's ends: item i is slot i's length (one more item, 0, so that off[n_inst] is the total)
struct XgLenIn {
    const uint32_t* len;
    uint64_t n;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return i < n ? len[i] : 0; }
};
struct XgOffOut {
    uint64_t *off, *inst_first;
    uint64_t n;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t ex, uint64_t) const {
        off[i] = ex;
        if (inst_first && i < n) inst_first[i] = ex;
    }
};

}  // namespace

// ---- pass 1: the groups' stops ------------------------------------------------------------------
__global__ __launch_bounds__(kXgT) void k_xg_stop(XgArgs a, uint32_t* __restrict__ stop) {
    // whether unit u holds a stopping slot of its LAST group (the one that may go on in u + 1)
    __shared__ uint32_t tail_bad[kXgUnits];
    const uint32_t l = (uint32_t)lane_id(), w = threadIdx.x / kWave;
    const uint64_t tile0 = (uint64_t)blockIdx.x * kXgTile;
    bool cand[kXgPer];
    uint32_t grp[kXgPer];
    uint32_t ebits = 0;
#pragma unroll
    for (int k = 0; k < kXgPer; ++k) {
        const uint32_t u = (uint32_t)k * (kXgT / kWave) + w;
        const uint64_t unit0 = tile0 + (uint64_t)u * kWave, idx = unit0 + l;
        bool bad = false;
        grp[k] = 0;
        if (idx < a.n_inst) {
            const XgSlot s = xg_slot(a, (uint32_t)idx);
            grp[k] = s.g;
            bad = s.in_range && !s.has;
            if (s.bad_group) ebits |= kErrInval;
        }
        const uint64_t bm = ballot(bad);
        // the first stopping slot of its group inside the unit: no lower lane of the group stops
        const uint64_t g0 = (uint64_t)grp[k] * a.ipg;
        const uint64_t mine = lanes_below((int)l) & ~lanes_below(g0 > unit0 ? (int)(g0 - unit0) : 0);
        cand[k] = bad && !(bm & mine);
        if (l == 0) {
            uint32_t tb = 0;
            if (unit0 < a.n_inst) {
                const uint64_t last = unit0 + kWave - 1 < a.n_inst ? unit0 + kWave - 1 : a.n_inst - 1;
                const uint64_t gl0 = (uint64_t)((uint32_t)last / a.ipg) * a.ipg;
                tb = (bm & ~lanes_below(gl0 > unit0 ? (int)(gl0 - unit0) : 0)) != 0;
            }
            tail_bad[u] = tb;
        }
    }
    raise_bits(a.err, ebits, kErrInval);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kXgPer; ++k) {
        if (!cand[k]) continue;
        const uint32_t u = (uint32_t)k * (kXgT / kWave) + w;
        // ... and no earlier unit of the tile does: those whose last slot is the group's
        bool earlier = false;
        for (int v = (int)u - 1; v >= 0 && !earlier; --v) {
            const uint64_t last = tile0 + (uint64_t)v * kWave + kWave - 1;
            if ((uint32_t)last / a.ipg != grp[k]) break;
            earlier = tail_bad[v] != 0;
        }
        if (!earlier) {
            const uint32_t idx = (uint32_t)(tile0 + (uint64_t)u * kWave + l);
            (void)__hip_atomic_fetch_min(&stop[grp[k]], idx, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- pass 2: the mask and the executed slots' lengths -------------------------------------------
__global__ __launch_bounds__(kXgT) void k_xg_mark(XgArgs a, const uint32_t* __restrict__ stop,
                                                  uint32_t* __restrict__ len) {
    const uint64_t tile0 = (uint64_t)blockIdx.x * kXgTile;
    uint32_t ebits = 0;
#pragma unroll
    for (int k = 0; k < kXgPer; ++k) {
        const uint64_t idx = tile0 + (uint64_t)k * kXgT + threadIdx.x;
        if (idx < a.n_inst) {
            const XgSlot s = xg_slot(a, (uint32_t)idx);
            const bool run = s.in_range && (uint32_t)idx < stop[s.g];
            a.mask[idx] = run ? 1 : 0;
            len[idx] = run ? xg_len(a, s, ebits) : 0u;
        }
    }
    raise_bits(a.err, ebits, kErrInval);
}

// ---- pass 4: a tile of output positions per workgroup -------------------------------------------
__global__ __launch_bounds__(kXgT) void k_xg_gather(XgArgs a, const uint64_t* __restrict__ off) {
    const uint64_t lo = (uint64_t)blockIdx.x * kXgTile;
    const uint64_t total = a.n_inst ? off[a.n_inst] : 0;
    const uint64_t real_end = total < a.cap ? total : a.cap;
    uint32_t i_lo = 0, i_hi = 0;
    if (lo < real_end) {  // (the same in every thread)
        const uint64_t hi = lo + kXgTile < real_end ? lo + kXgTile : real_end;
        i_lo = (uint32_t)holder(off, a.n_inst, 0, lo, (int)threadIdx.x);
        i_hi = (uint32_t)holder(off, a.n_inst, i_lo, hi - 1, (int)threadIdx.x);
    }
    xg_emit_tile<kXgT>(a, lo, total, XgOff{off}, i_lo, i_hi);
}

// ---- pass 5: a group and a send per thread ------------------------------------------------------
__global__ __launch_bounds__(kXgT) void k_xg_groups(XgArgs a, uint32_t* __restrict__ stop,
                                                    const uint64_t* __restrict__ off,
                                                    uint64_t* __restrict__ part_inst,
                                                    uint32_t* __restrict__ part_moved) {
    __shared__ uint64_t ws[kXgT / kWave];
    const uint64_t i = (uint64_t)blockIdx.x * kXgT + threadIdx.x;
    uint64_t ran = 0;
    if (i < a.n_groups) {
        const XgGroup G = xg_group(a, (uint32_t)i);
        const int64_t out = xg_cursor(a, G, stop[i]);
        stop[i] = kXgNoStop;  // as the next call expects it
        a.ex_out[i] = (int32_t)out;
        ran = (uint64_t)(out - G.ex);
        if (a.grp_cmd_off) a.grp_cmd_off[i] = off[i * a.ipg];
    }
    if (i == 0 && a.grp_cmd_off) a.grp_cmd_off[a.n_groups] = a.n_inst ? off[a.n_inst] : 0;
    if (i < a.n_sends && a.ret_first) a.ret_first[i] = a.n_inst ? xg_ret_first(a, i, off) : 0;
    const uint32_t moved = (uint32_t)__syncthreads_count(ran != 0);
    if ((uint64_t)blockIdx.x * kXgT >= a.n_groups) return;  // a block of sends only
    ran = block_sum<uint64_t, kXgT>(ran, ws);
    if (threadIdx.x == 0) {
        part_inst[blockIdx.x] = ran;
        part_moved[blockIdx.x] = moved;
    }
}

// ---- the result record (one workgroup) ----------------------------------------------------------
__global__ __launch_bounds__(kXgFinT) void k_xg_finish(const uint64_t* __restrict__ off,
                                                       uint64_t n_inst,
                                                       const uint64_t* __restrict__ part_inst,
                                                       const uint32_t* __restrict__ part_moved,
                                                       uint32_t nb, mpx_execute_result* __restrict__ res) {
    __shared__ uint64_t ws[2][kXgFinT / kWave];
    uint64_t ran = 0, moved = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += kXgFinT) ran += part_inst[i], moved += part_moved[i];
    // (not two of assemble.hpp's block_sum: the two values share the shuffles' rounds and one barrier)
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        ran += shfl_any(ran, lane_id() ^ d);
        moved += shfl_any(moved, lane_id() ^ d);
    }
    if (lane_id() == 0) ws[0][threadIdx.x / kWave] = ran, ws[1][threadIdx.x / kWave] = moved;
    __syncthreads();
    if (threadIdx.x == 0) {
        ran = moved = 0;
        for (int w = 0; w < kXgFinT / kWave; ++w) ran += ws[0][w], moved += ws[1][w];
        res->n_cmds = n_inst ? off[n_inst] : 0;
        res->n_inst = ran;
        res->n_groups = moved;
        res->reserved = 0;
    }
}

// ---- one launch: a replica-sized call in one workgroup, no scratch ------------------------------
__global__ __launch_bounds__(kXgOneT) void k_xg_one(XgArgs a) {
    __shared__ uint32_t s_stop[kXgOneT];
    __shared__ uint64_t s_off[kXgOneT + 1];
    __shared__ uint64_t ws[kXgOneT / kWave];
    __shared__ unsigned long long s_ran;
    const uint32_t t = threadIdx.x;
    s_stop[t] = kXgNoStop;
    if (t == 0) s_ran = 0;
    __syncthreads();
    XgSlot s{};
    uint32_t ebits = 0;
    if (t < a.n_inst) {
        s = xg_slot(a, t);
        if (s.bad_group) ebits |= kErrInval;
        if (s.in_range && !s.has) atomicMin(&s_stop[s.g], t);
    }
    __syncthreads();
    uint32_t len = 0;
    if (t < a.n_inst) {
        const bool run = s.in_range && t < s_stop[s.g];
        a.mask[t] = run ? 1 : 0;
        if (run) len = xg_len(a, s, ebits);
    }
    // (not assemble.hpp's raise_bits: testing the one bit costs this kernel two scalar registers)
    if (ballot(ebits != 0) != 0 && lane_id() == 0) raise_err(a.err, kErrInval);
    s_off[t + 1] = block_excl_scan<uint64_t, kXgOneT>((uint64_t)len, ws) + len;
    if (t == 0) s_off[0] = 0;
    __syncthreads();
    const uint64_t total = s_off[a.n_inst];
    if (t < a.n_inst && a.inst_first) a.inst_first[t] = s_off[t];
    bool moved = false;
    if (t < a.n_groups) {
        const XgGroup G = xg_group(a, t);
        const int64_t out = xg_cursor(a, G, s_stop[t]);
        a.ex_out[t] = (int32_t)out;
        moved = out != G.ex;
        if (moved) atomicAdd(&s_ran, (unsigned long long)(out - G.ex));
        if (a.grp_cmd_off) a.grp_cmd_off[t] = s_off[t * a.ipg];
    }
    if (t == 0 && a.grp_cmd_off) a.grp_cmd_off[a.n_groups] = total;
    const uint32_t n_moved = (uint32_t)__syncthreads_count(moved);
    if (t == 0) {
        a.res->n_cmds = total;
        a.res->n_inst = s_ran;
        a.res->n_groups = n_moved;
        a.res->reserved = 0;
    }
    if (a.ret_first)
        for (uint64_t x = t; x < a.n_sends; x += kXgOneT) a.ret_first[x] = xg_ret_first(a, x, s_off);
    for (uint64_t lo = 0; lo < a.cap; lo += kXgOneT * kXgPer)
        xg_emit_tile<kXgOneT>(a, lo, total, XgOff{s_off}, 0u, a.n_inst ? (uint32_t)a.n_inst - 1 : 0u);
}

namespace {
struct XgWork {
    uint32_t *stop, *len, *part_moved;
    uint64_t *off, *part_inst, *scan_tmp;
    XgWork(Carver& c, uint64_t n_inst, uint64_t group_cap) {
        const uint64_t gb = (group_cap + kXgT - 1) / kXgT;
        stop = c.take<uint32_t>(group_cap);  // first: at the base for every call's sizes
        len = c.take<uint32_t>(n_inst);
        off = c.take<uint64_t>(n_inst + 1);
        part_inst = c.take<uint64_t>(gb);
        part_moved = c.take<uint32_t>(gb);
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(n_inst + 1));
    }
};
}  // namespace

uint64_t execute_work_bytes(uint64_t n_inst, uint64_t group_cap, Carver&& c) {
    return XgWork(c, n_inst, group_cap), c.bytes();
}

hipError_t launch_execute_gather(const mpx_execute_batch* b, const mpx_execute_out* out,
                                 mpx_execute_result* res, void* work, uint64_t work_bytes,
                                 uint64_t group_cap, uint32_t* err, hipStream_t stream) {
    const uint64_t n = b->n_inst, cap = out->cap;
    const uint64_t tiles_in = (n + kXgTile - 1) / kXgTile, tiles_out = (cap + kXgTile - 1) / kXgTile;
    const uint64_t per = std::max<uint64_t>(b->n_groups, out->ret_first ? b->n_sends : 0);
    const uint64_t gblocks = std::max<uint64_t>((per + kXgT - 1) / kXgT, 1);
    if (n >= 0xFFFFFFFFull || b->n_groups > n || tiles_out >= (1ull << 31) || gblocks >= (1ull << 31))
        return hipErrorInvalidValue;
    const XgArgs a{b->inst, b->committed_upto, b->executed_in, b->executed_out, b->src_op,
                   b->src_key, b->src_val, b->sends, n, b->n_groups, b->n_src, b->n_sends, cap,
                   b->inst_base, b->ipg, b->flags & MPX_XG_PAD, out->op, out->key, out->val,
                   out->mask, out->inst_first, out->ret_first, out->grp_cmd_off, res, err};
    if (!(b->flags & MPX_XG_GENERAL) && n <= MPX_XG_ONE_LAUNCH_INST && cap <= MPX_XG_ONE_LAUNCH_CMDS) {
        k_xg_one<<<1, kXgOneT, 0, stream>>>(a);
        return hipGetLastError();
    }
    Carver c(work);
    const XgWork w(c, n, group_cap);
    if (work_bytes < c.bytes() || b->n_groups > group_cap) return hipErrorInvalidValue;
    const uint64_t* off = n ? w.off : nullptr;
    if (n) {
        k_xg_stop<<<(unsigned)tiles_in, kXgT, 0, stream>>>(a, w.stop);
        k_xg_mark<<<(unsigned)tiles_in, kXgT, 0, stream>>>(a, w.stop, w.len);
        const hipError_t r = device_scan(XgLenIn{w.len, n}, XgOffOut{w.off, out->inst_first, n}, n + 1,
                                         ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
        if (r != hipSuccess) return r;
    }
    if (tiles_out) k_xg_gather<<<(unsigned)tiles_out, kXgT, 0, stream>>>(a, off);
    k_xg_groups<<<(unsigned)gblocks, kXgT, 0, stream>>>(a, w.stop, off, w.part_inst, w.part_moved);
    k_xg_finish<<<1, kXgFinT, 0, stream>>>(off, n, w.part_inst, w.part_moved,
                                           (uint32_t)((b->n_groups + kXgT - 1) / kXgT), res);
    return hipGetLastError();
}

}  // namespace mpx

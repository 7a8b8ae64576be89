// assemble.hpp — the building blocks the assembly kernels share (replies.hip, execute.hip,
// store.hip, record.hip): the command sources and the resolution of an item's commands in them,
// the search for the holder of an output position, the workgroup sum and exclusive scan, the
// wave-aggregated error raise and the four-position command store (store.hip's alone so far).
// Plain inlined functions, no kernels and no state: every caller keeps its own passes, LDS,
// scratch and launchers.
#pragma once
#include "common.hpp"
#include "scan.hpp"

namespace mpx {

// ---- the command sources ---------------------------------------------------------------------------
// One mpx_store_src as the kernels read it. rec_end: the records of sources 0 .. s, so that
// record p of the merged batch lies in the first source whose rec_end is above p.
struct CmdSrc {
    const uint64_t* cmd_off;
    const uint8_t* op;
    const int64_t *key, *val;
    uint64_t n_frames, n_cmds, rec_end;
};

// the launchers' side: the call's sources into its argument table; recs and cmds are their totals
inline void fill_cmd_sources(const mpx_store_src* src, size_t n_src, CmdSrc* out, uint64_t& recs,
                             uint64_t& cmds) {
    recs = cmds = 0;
    for (size_t s = 0; s < n_src; ++s) {
        const mpx_store_src& x = src[s];
        recs += x.n_recs, cmds += x.n_cmds;
        out[s] = CmdSrc{x.cmd_off, x.op, x.key, x.val, x.n_frames, x.n_cmds, recs};
    }
}

// the sources into LDS (constant indices into the kernel arguments; the kernels index the table
// by a lane's own source). Every thread calls; one barrier inside.
__device__ __forceinline__ void cmd_sources(const CmdSrc (&src)[MPX_SC_MAX_SRC], uint32_t n_src, CmdSrc* S) {
#pragma unroll
    for (int s = 0; s < MPX_SC_MAX_SRC; ++s)
        if ((int)threadIdx.x == s && (uint32_t)s < n_src) S[s] = src[s];
    __syncthreads();
}

// the items of the call: n, or what the device-side count allows of them
__device__ __forceinline__ uint64_t n_eff(const uint64_t* d_n, uint64_t n) {
    if (!d_n) return n;
    const uint64_t d = *d_n;
    return d < n ? d : n;
}

// An item's commands: len of them from index lo of source src. ok == false: the item is faulty
// and kErrInval stands in the caller's ebits.
struct CmdRange {
    uint64_t src, lo, len;
    bool ok;
};
// ... of message item i with the given value_id: its record is p = perm[i] (i without perm), its
// source the one holding p, its commands frame value_id of that source
__device__ __forceinline__ CmdRange msg_cmds(const CmdSrc* S, uint32_t n_src, uint64_t n_recs,
                                             const uint32_t* perm, uint64_t i, uint32_t value_id,
                                             uint32_t& ebits) {
    CmdRange r{0, 0, 0, false};
    const uint64_t p = perm ? perm[i] : i;
    if (p >= n_recs) {
        ebits |= kErrInval;
        return r;
    }
    while (r.src + 1 < n_src && p >= S[r.src].rec_end) ++r.src;
    const CmdSrc& s = S[r.src];
    if (value_id >= s.n_frames) {
        ebits |= kErrInval;
        return r;
    }
    r.lo = s.cmd_off[value_id];
    const uint64_t hi = s.cmd_off[value_id + 1];
    if (hi < r.lo || hi > s.n_cmds || hi - r.lo >= 0xFFFFFFFFull) {
        ebits |= kErrInval;
        return r;
    }
    r.len = hi - r.lo, r.ok = true;
    return r;
}
// ... of an mpx_accept_send: [first_cmd, first_cmd + n_cmds) of the call's one source
__device__ __forceinline__ CmdRange send_cmds(const CmdSrc& S0, uint64_t first_cmd, uint32_t n_cmds,
                                              uint32_t& ebits) {
    if (first_cmd > S0.n_cmds || n_cmds > S0.n_cmds - first_cmd || n_cmds == 0xFFFFFFFFu) {
        ebits |= kErrInval;
        return {0, 0, 0, false};
    }
    return {0, first_cmd, n_cmds, true};
}

// where an item's commands start, in one word: the source in the top byte, the index below
constexpr uint64_t kCmdPosMask = (1ull << 56) - 1;
__device__ __forceinline__ uint64_t cmd_pos(uint64_t src, uint64_t lo) { return (src << 56) | lo; }
__device__ __forceinline__ uint64_t cmd_pos_src(uint64_t pos) { return pos >> 56; }
__device__ __forceinline__ uint64_t cmd_pos_lo(uint64_t pos) { return pos & kCmdPosMask; }

// ---- the holder of an output position --------------------------------------------------------------
// The entry holding output position p, given off(l) <= p < off(h): the last one that starts at or
// before p (the empty ones before it start there too and are passed over). off: the scanned
// offsets, in global memory or in LDS.
template <typename Off, typename I>
__device__ __forceinline__ I last_at_or_before(const Off& off, uint64_t p, I l, I h) {
    while (h - l > 1) {
        const I mid = l + ((h - l) >> 1);
        if (off(mid) <= p) l = mid;
        else h = mid;
    }
    return l;
}

// ---- over the workgroup ----------------------------------------------------------------------------
// Both are for workgroups of THREADS threads and a ws of THREADS / kWave words. Every thread
// calls; one barrier inside, after ws is written: the caller keeps ws unwritten until its own next
// barrier, and a second call on the same ws needs a barrier between the two.
// The sum of every thread's v: in thread 0 (0 in the others).
template <typename T, int THREADS>
__device__ __forceinline__ T block_sum(T v, T* ws) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v += shfl_any(v, lane_id() ^ d);
    if (lane_id() == 0) ws[threadIdx.x / kWave] = v;
    __syncthreads();
    T s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / kWave; ++w) s += ws[w];
    return s;
}
// The sum of the v of the threads below this one. ws is left holding the waves' sums. The loop
// runs to the thread's own wave (dependent LDS reads, most in the last wave): a caller that wants
// the total too does better with one fixed-trip select over all of ws, as k_st_one does.
template <typename T, int THREADS>
__device__ __forceinline__ T block_excl_scan(T v, T* ws) {
    static_assert(THREADS % kWave == 0, "whole waves");
    const T incl = wave_incl_scan(v, [](T a, T b) { return a + b; });
    if (lane_id() == kWave - 1) ws[threadIdx.x / kWave] = incl;
    __syncthreads();
    T before = 0;
    for (uint32_t w = 0; w < threadIdx.x / kWave; ++w) before += ws[w];
    return before + incl - v;
}

// ---- errors ----------------------------------------------------------------------------------------
// The bits of `mask` (a constant) that any lane of the wave holds in `bits`, raised in the error
// word: an atomic of lane 0 per bit. Every lane of the wave calls.
__device__ __forceinline__ void raise_bits(uint32_t* err, uint32_t bits, uint32_t mask) {
#pragma unroll
    for (uint32_t b = 1u << 31; b; b >>= 1)
        if ((mask & b) && ballot((bits & b) != 0) != 0 && lane_id() == 0) raise_err(err, b);
}

// ---- four commands ---------------------------------------------------------------------------------
// Positions 0 .. 3 of d_op / d_key / d_val, which lie a multiple of 4 into their arrays: those
// with in[j], a run without gaps, take {o[j], k[j], v[j]}. All four: the keys and the values as 16-byte
// stores whichever way their array lies mod 16 (the four start 0 or 8 bytes into a 16-byte line)
// and the op bytes as one dword; a ragged end: position by position. store.hip's only, for now.
__device__ __forceinline__ void store4_cmds(uint8_t* d_op, int64_t* d_key, int64_t* d_val, const uint32_t (&o)[4],
                                            const uint64_t (&k)[4], const uint64_t (&v)[4], const bool (&in)[4]) {
    if (in[0] && in[3]) {
        const auto four = [](int64_t* d, const uint64_t (&x)[4]) {
            if (((uintptr_t)d & 15) == 0) {
                reinterpret_cast<uint4*>(d)[0] =
                    make_uint4((uint32_t)x[0], (uint32_t)(x[0] >> 32), (uint32_t)x[1], (uint32_t)(x[1] >> 32));
                reinterpret_cast<uint4*>(d)[1] =
                    make_uint4((uint32_t)x[2], (uint32_t)(x[2] >> 32), (uint32_t)x[3], (uint32_t)(x[3] >> 32));
            } else {
                d[0] = (int64_t)x[0];
                *reinterpret_cast<uint4*>(d + 1) =
                    make_uint4((uint32_t)x[1], (uint32_t)(x[1] >> 32), (uint32_t)x[2], (uint32_t)(x[2] >> 32));
                d[3] = (int64_t)x[3];
            }
        };
        four(d_key, k);
        four(d_val, v);
        if (((uintptr_t)d_op & 3) == 0) {
            *reinterpret_cast<uint32_t*>(d_op) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) d_op[j] = (uint8_t)o[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (in[j]) d_op[j] = (uint8_t)o[j], d_key[j] = (int64_t)k[j], d_val[j] = (int64_t)v[j];
    }
}

}  // namespace mpx

// unmarshal.hip — the inverse of mpx_encode_accepts: from the mpx_var_frame ranges the stream
// decoder found to the records and SoA arrays the rest of the engine consumes.
//   Accept.Unmarshal        MIN minpaxosprotomarsh.go:470-507   CLASSIC paxosprotomarsh.go:244-268
//   Commit.Unmarshal        :648-672                            :403-430
//   PrepareReply.Unmarshal  :352-387 (Command, CatchUpLog)      :152-176 (Command)
//   Instance.Unmarshal      :126-153
//   Command.Unmarshal       statemarsh.go:21-39
// Stations, all plain launches in stream order (n_var is a device value when d_n_var is given, so
// every grid is sized by the host's bound and the lanes past the device count do nothing):
//   1. two scans (scan.hpp) over the frame records, no payload byte read. The first sums
//      (n_cmds, n_log) packed in one u64: cmd_off, log_inst_off and their totals. The second sums
//      (is Accept, is Commit): the exclusive prefix is the frame's slot in the compacted outputs,
//      so the stable ranks come out of the scan's own wave scans.
//   2. k_um_frames, a lane per frame. The head: the fields at offset + 1 go to accepts /
//      accept_last_committed / commits at the frame's rank. (As the output step of the rank scan
//      the header reads ran in 16 workgroups for 65,536 frames, 164 bytes apart: 50 us; here they
//      run in 256.) Then, MIN, the lane walks its frame's CatchUpLog, the chain pos' = pos + 8 +
//      |V(k)| + 17 k that stream.hip's parse_var walks for the length: log_recs, and per instance
//      its command count and the byte position of its first command in scratch. A scan of the
//      counts gives log_cmd_off.
//   3. k_um_gather, once over (cmd_off, var[].cmds_off) and once over (log_cmd_off, positions): a
//      workgroup per tile of kUmTile output commands finds the tile's first and last owner by a
//      256-ary search of the offsets (k_ab_emit's search), every lane finds its commands' owners
//      by bisection between them. A 17-byte command at byte phase f = p & 15 lies inside exactly
//      two aligned 16-byte vectors (f + 17 <= 32), so a lane takes its command with two 16-byte
//      loads from 16-byte aligned addresses straight into registers - the second vector holds the
//      command's last byte, so no load reaches the 16-byte rounding of len - and all of a lane's
//      kUmPer x 2 loads are issued before the first is used. No LDS image: staging runs through
//      LDS would save the second vector's overlap with the neighbour lane (the lines come from
//      L1 either way) at the price of a per-run layout pass. The fields sit at any byte phase:
//      a word select and v_alignbyte. key / val leave as coalesced 8-byte stores; op goes through
//      1 KB of LDS and leaves as dwords with bytewise ends.
#include "common.hpp"
#include "kernels.hpp"
#include "scan.hpp"

namespace mpx {
namespace {
constexpr int kUmBlock = 256;
constexpr int kUmPer = 4;                     // commands per lane
constexpr int kUmTile = kUmBlock * kUmPer;    // commands per gather workgroup
// the call's totals in scratch (u64 each), read by the later kernels
enum { kTotAcc = 0, kTotCom, kTotCmd, kTotLog, kTotLogCmd, kTotWords = 8 };

__device__ __forceinline__ uint64_t um_nv(const uint64_t* d_nv, uint64_t n) {
    if (!d_nv) return n;
    const uint64_t v = *d_nv;
    return v < n ? v : n;
}
// the little-endian u32 at byte p of the 16-byte aligned buf: the aligned dwords that hold it
__device__ __forceinline__ uint32_t um_u32(const uint8_t* buf, uint64_t p) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(buf) + (p >> 2);
    const uint32_t b = (uint32_t)(p & 3);
    const uint32_t lo = w[0];
    if (!b) return lo;
    return __builtin_amdgcn_alignbyte(w[1], lo, b);
}
// binary.ReadVarint at *pos (stream.hip read_varint restated for global bytes), never reading at
// or past `end`; false: the bytes ran out or the value overflows 64 bits
__device__ __forceinline__ bool um_varint(const uint8_t* buf, uint64_t end, uint64_t* pos,
                                          int64_t* out) {
    uint64_t x = 0;
    uint32_t s = 0;
    for (int i = 0; i < 10; ++i) {
        if (*pos >= end) return false;
        const uint32_t b = buf[(*pos)++];
        if (b < 0x80u) {
            if (i == 9 && b > 1u) return false;  // errOverflow
            x |= (uint64_t)b << s;
            *out = (int64_t)(x >> 1) ^ -(int64_t)(x & 1ull);
            return true;
        }
        x |= (uint64_t)(b & 0x7fu) << s;
        s += 7;
    }
    return false;
}

struct UmFrame {
    uint32_t offset, length, n_cmds, cmds_off, n_log, log_off, code;
};
__device__ __forceinline__ UmFrame um_frame(const mpx_var_frame* var, uint64_t i) {
    const uint4 a = reinterpret_cast<const uint4*>(var + i)[0];
    const uint4 b = reinterpret_cast<const uint4*>(var + i)[1];
    return UmFrame{a.x, a.y, a.z, a.w, b.x, b.y, b.z & 0xFFu};
}

// scan 1: (n_cmds, n_log << 32) per frame; only MIN Accepts and PrepareReplies carry a log
struct UmCountIn {
    const mpx_var_frame* var;
    const uint64_t* d_nv;
    uint64_t n;
    int mode;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        if (i >= um_nv(d_nv, n)) return 0;
        const UmFrame f = um_frame(var, i);
        const bool has_log = mode == MPX_MODE_MIN && f.code != MPX_PEER_COMMIT;
        return (uint64_t)f.n_cmds | (has_log ? (uint64_t)f.n_log << 32 : 0ull);
    }
};
struct UmCountOut {
    uint64_t* s_cmd_off;  // scratch copies: the later kernels read these
    uint64_t* s_log_off;
    uint64_t* cmd_off;    // the caller's (optional)
    uint64_t* log_off;
    uint64_t n;
    uint64_t* tot;
    mpx_unmarshal_result* res;
    __device__ __forceinline__ void put(uint64_t i, uint64_t s) const {
        const uint64_t c = s & 0xFFFFFFFFull, l = s >> 32;
        s_cmd_off[i] = c;
        s_log_off[i] = l;
        if (cmd_off) cmd_off[i] = c;
        if (log_off) log_off[i] = l;
    }
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t s, uint64_t x) const {
        put(i, s);
        if (i != n - 1) return;
        put(n, s + x);
        tot[kTotCmd] = res->n_cmds = (s + x) & 0xFFFFFFFFull;
        tot[kTotLog] = res->n_log_inst = (s + x) >> 32;
    }
};

// scan 2: (is Accept, is Commit << 32); the exclusive prefixes are the frames' ranks
struct UmCodeIn {
    const mpx_var_frame* var;
    const uint64_t* d_nv;
    uint64_t n;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        if (i >= um_nv(d_nv, n)) return 0;
        const uint32_t code = reinterpret_cast<const uint32_t*>(var + i)[6] & 0xFFu;
        return code == MPX_PEER_ACCEPT ? 1ull : code == MPX_PEER_COMMIT ? 1ull << 32 : 0ull;
    }
};
struct UmRankOut {
    uint64_t* rank;  // scratch: (Accepts, Commits << 32) before frame i
    uint64_t n;
    uint64_t* tot;
    mpx_unmarshal_result* res;
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t s, uint64_t x) const {
        rank[i] = s;
        if (i != n - 1) return;
        tot[kTotAcc] = res->n_accepts = (s + x) & 0xFFFFFFFFull;
        tot[kTotCom] = res->n_commits = (s + x) >> 32;
    }
};

// scan 3: the log instances' command counts (past the call's instances: 0)
struct UmLogIn {
    const uint32_t* cnt;
    const uint64_t* tot;
    uint64_t scratch_cap;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const {
        const uint64_t m = tot[kTotLog] < scratch_cap ? tot[kTotLog] : scratch_cap;
        return i < m ? cnt[i] : 0;
    }
};
struct UmLogOut {
    uint64_t* s_off;  // scratch: n + 1 entries, every one written
    uint64_t* off;    // the caller's log_cmd_off (optional): entries <= min(n_log_inst, cap)
    uint64_t cap, n;
    uint64_t* tot;
    mpx_unmarshal_result* res;
    __device__ __forceinline__ void put(uint64_t i, uint64_t s) const {
        s_off[i] = s;
        if (off && i <= cap && i <= tot[kTotLog]) off[i] = s;
    }
    __device__ __forceinline__ void operator()(uint64_t i, uint64_t s, uint64_t x) const {
        put(i, s);
        if (i != n - 1) return;
        put(n, s + x);
        tot[kTotLogCmd] = res->n_log_cmds = s + x;
    }
};

// where an owner's commands start: a frame's Command slice / a log instance's
struct UmVarPos {
    const mpx_var_frame* var;
    __device__ __forceinline__ uint64_t operator()(uint64_t o) const {
        return reinterpret_cast<const uint32_t*>(var + o)[3];
    }
};
struct UmArrPos {
    const uint32_t* pos;
    __device__ __forceinline__ uint64_t operator()(uint64_t o) const { return pos[o]; }
};

// the last i in [0, n) with off[i] <= c, for off[0] <= c < off[n] (all threads call; 256-ary,
// invariant off[lo] <= c < off[hi])
__device__ __forceinline__ uint64_t um_owner(const uint64_t* __restrict__ off, uint64_t n,
                                            uint64_t c) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + kUmBlock - 1) / kUmBlock;
        const uint64_t i = lo + (uint64_t)threadIdx.x * step;
        const int k = __syncthreads_count(i < hi && off[i] <= c);
        const uint64_t nh = lo + (uint64_t)k * step;
        lo += (uint64_t)(k - 1) * step;
        hi = nh < hi ? nh : hi;
    }
    return lo;
}
}  // namespace

__global__ void k_um_init(mpx_unmarshal_result* res, uint64_t* tot, uint64_t* s_log_cmd_off,
                          uint64_t* log_cmd_off, uint64_t* cmd_off, uint64_t* log_inst_off,
                          const uint64_t* d_nv, uint64_t n_var) {
    res->n_accepts = res->n_commits = res->n_cmds = res->n_log_inst = res->n_log_cmds = 0;
    res->n_var = um_nv(d_nv, n_var);
    for (int i = 0; i < kTotWords; ++i) tot[i] = 0;
    s_log_cmd_off[0] = 0;
    if (log_cmd_off) log_cmd_off[0] = 0;
    if (!n_var) {  // (the scans of an empty call launch nothing)
        if (cmd_off) cmd_off[0] = 0;
        if (log_inst_off) log_inst_off[0] = 0;
    }
}

// the compacted outputs of a call
struct UmHeads {
    mpx_accept_msg* accepts;
    int32_t* alc;
    uint64_t acc_cap;
    mpx_accept_msg* commits;
    uint64_t com_cap;
};

// a lane per frame. The head: an Accept's or Commit's fields at offset + 1 go to the slot its
// rank names. Then the CatchUpLog of a MIN Accept / PrepareReply: Instance.Unmarshal per record.
__global__ __launch_bounds__(kUmBlock) void k_um_frames(
    int mode, const uint8_t* __restrict__ buf, uint64_t len, const mpx_var_frame* __restrict__ var,
    uint64_t n_var, const uint64_t* d_nv, const uint64_t* __restrict__ rank, UmHeads h,
    const uint64_t* __restrict__ s_log_off, mpx_log_rec* log_recs, uint64_t log_inst_cap,
    uint32_t* __restrict__ cnt, uint32_t* __restrict__ cpos, uint64_t scratch_cap, uint32_t* err) {
    const uint64_t i = (uint64_t)blockIdx.x * kUmBlock + threadIdx.x;
    if (i >= um_nv(d_nv, n_var)) return;
    const UmFrame f = um_frame(var, i);
    const uint64_t fs = f.offset, fe = fs + f.length;
    const uint64_t lim = fe < len ? fe : len;  // no byte at or past it is read
    if (f.code == MPX_PEER_ACCEPT || f.code == MPX_PEER_COMMIT) {
        const bool acc = f.code == MPX_PEER_ACCEPT, min_acc = acc && mode == MPX_MODE_MIN;
        const uint64_t s = rank[i];
        const uint64_t slot = acc ? (s & 0xFFFFFFFFull) : (s >> 32);
        if (slot < (acc ? h.acc_cap : h.com_cap)) {
            if (fs + (min_acc ? 17 : 13) > lim) {
                raise_err(err, kErrInval);
            } else {
                // LeaderId, Instance, Ballot(, LastCommitted)
                const int32_t leader = (int32_t)um_u32(buf, fs + 1);
                const int32_t inst = (int32_t)um_u32(buf, fs + 5);
                const int32_t bal = (int32_t)um_u32(buf, fs + 9);
                int4* dst = reinterpret_cast<int4*>((acc ? h.accepts : h.commits) + slot);
                *dst = make_int4(inst, bal, leader, (int32_t)(uint32_t)i);
                if (acc) h.alc[slot] = min_acc ? (int32_t)um_u32(buf, fs + 13) : -1;
            }
        }
    }
    if (mode != MPX_MODE_MIN || !f.n_log || f.code == MPX_PEER_COMMIT) return;
    const uint64_t lc_at = fs + (f.code == MPX_PEER_ACCEPT ? 13 : 14);
    if (lc_at + 4 > lim) {
        raise_err(err, kErrInval);
        return;
    }
    // the sender's numbering: the log ends at the frame's LastCommitted
    const uint32_t first = um_u32(buf, lc_at) - f.n_log + 1u;
    const uint64_t r0 = s_log_off[i];
    uint64_t pos = f.log_off;
    bool bad = pos < fs;
    for (uint32_t j = 0; j < f.n_log; ++j) {
        const uint64_t r = r0 + j;
        if (r >= scratch_cap) {  // more log instances than mpx_unmarshal_frames_reserve was told
            bad = true;
            break;
        }
        uint32_t k = 0, at = 0;
        int32_t ballot = 0, status = 0;
        if (!bad) {
            int64_t kk = 0;
            if (pos + 9 > lim) {
                bad = true;
            } else {
                ballot = (int32_t)um_u32(buf, pos);      // :131
                status = (int32_t)um_u32(buf, pos + 4);  // :135
                pos += 8;
                if (!um_varint(buf, lim, &pos, &kk) || kk < 0 || (uint64_t)kk > (lim - pos) / 17) {
                    bad = true;
                } else {
                    k = (uint32_t)kk;
                    at = (uint32_t)pos;
                    pos += 17ull * k;
                }
            }
        }
        cnt[r] = bad ? 0u : k;
        cpos[r] = at;
        if (!bad && r < log_inst_cap)
            reinterpret_cast<int4*>(log_recs)[r] =
                make_int4(ballot, status, (int32_t)(first + j), 0);
    }
    if (bad || pos != fe) raise_err(err, kErrInval);
}

// commands [c0, c0 + kUmTile) of the concatenation of the owners' 17-byte AoS runs -> SoA
template <typename Pos>
__global__ __launch_bounds__(kUmBlock) void k_um_gather(
    const uint8_t* __restrict__ buf, uint64_t len, const uint64_t* __restrict__ off, uint64_t n_own,
    Pos pos, const uint64_t* __restrict__ total_p, uint8_t* __restrict__ op,
    int64_t* __restrict__ key, int64_t* __restrict__ val, uint64_t cap, uint32_t* err) {
    __shared__ uint8_t ops[kUmTile];
    const int t = threadIdx.x;
    const uint64_t total = *total_p;
    const uint64_t lim = total < cap ? total : cap;  // nothing at or past the capacity
    const uint64_t c0 = (uint64_t)blockIdx.x * kUmTile;
    if (c0 >= lim) return;  // (uniform)
    const uint64_t c1 = c0 + kUmTile < lim ? c0 + kUmTile : lim;
    const uint64_t o0 = um_owner(off, n_own, c0), o1 = um_owner(off, n_own, c1 - 1);
    uint4 v0[kUmPer], v1[kUmPer];
    uint32_t ph[kUmPer];
    bool ok[kUmPer];
#pragma unroll
    for (int r = 0; r < kUmPer; ++r) {
        const uint64_t c = c0 + (uint64_t)(t + r * kUmBlock);
        ok[r] = c < c1;
        ph[r] = 0;
        v0[r] = v1[r] = make_uint4(0, 0, 0, 0);
        if (!ok[r]) continue;
        uint64_t lo = o0, hi = o1 + 1;  // the last owner with off <= c
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (off[mid] <= c) lo = mid; else hi = mid;
        }
        const uint64_t p = pos(lo) + 17ull * (c - off[lo]);
        if (p + 17 > len) {  // (frames the caller vouched for never get here)
            raise_err(err, kErrInval);
            ok[r] = false;
            continue;
        }
        // bytes [p, p + 17) lie in the two aligned vectors from p & ~15; the second one holds
        // byte p + 16 < len, so neither reaches len rounded up to 16
        const uint4* v = reinterpret_cast<const uint4*>(buf + (p & ~15ull));
        v0[r] = ld_stream(v);
        v1[r] = ld_stream(v + 1);
        ph[r] = (uint32_t)(p & 15);
    }
#pragma unroll
    for (int r = 0; r < kUmPer; ++r) {
        uint32_t w[9] = {v0[r].x, v0[r].y, v0[r].z, v0[r].w, v1[r].x, v1[r].y, v1[r].z, v1[r].w, 0u};
        const uint32_t s = ph[r] >> 2, b = ph[r] & 3u;
        if (s & 2u) {
#pragma unroll
            for (int j = 0; j < 7; ++j) w[j] = w[j + 2];
        }
        if (s & 1u) {
#pragma unroll
            for (int j = 0; j < 6; ++j) w[j] = w[j + 1];
        }
        uint32_t x[5];  // the command's 17 bytes from byte 0 of x[0]
#pragma unroll
        for (int j = 0; j < 5; ++j) x[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], b);
        const uint64_t k8 = (uint64_t)__builtin_amdgcn_alignbyte(x[1], x[0], 1) |
                            ((uint64_t)__builtin_amdgcn_alignbyte(x[2], x[1], 1) << 32);
        const uint64_t v8 = (uint64_t)__builtin_amdgcn_alignbyte(x[3], x[2], 1) |
                            ((uint64_t)__builtin_amdgcn_alignbyte(x[4], x[3], 1) << 32);
        ops[t + r * kUmBlock] = ok[r] ? (uint8_t)(x[0] & 0xFFu) : (uint8_t)0;
        if (ok[r]) {
            const uint64_t c = c0 + (uint64_t)(t + r * kUmBlock);
            st_stream(key + c, (int64_t)k8);
            st_stream(val + c, (int64_t)v8);
        }
    }
    __syncthreads();
    // op: bytewise up to the first dword boundary of the destination, dwords, bytewise tail
    uint8_t* dst = op + c0;
    const uint32_t n = (uint32_t)(c1 - c0);
    uint32_t a = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
    a = a < n ? a : n;
    if ((uint32_t)t < a) dst[t] = ops[t];
    const uint32_t q = a + 4u * (uint32_t)t;
    if (q + 4 <= n) {
        const uint32_t v = (uint32_t)ops[q] | ((uint32_t)ops[q + 1] << 8) |
                           ((uint32_t)ops[q + 2] << 16) | ((uint32_t)ops[q + 3] << 24);
        *reinterpret_cast<uint32_t*>(dst + q) = v;
    } else {
        for (uint32_t i = q; i < n; ++i) dst[i] = ops[i];
    }
}

namespace {
struct UmWork {
    uint64_t* tot;          // kTotWords
    uint64_t* cmd_off;      // n_var + 1
    uint64_t* log_off;      // n_var + 1
    uint64_t* rank;         // n_var: (Accepts, Commits << 32) before each frame
    uint64_t* log_cmd_off;  // n_log + 1
    uint32_t* cnt;          // n_log: commands of each log instance
    uint32_t* pos;          // n_log: byte position of its first command
    uint64_t* scan_tmp;     // for the larger of the scans
    UmWork(Carver& c, uint64_t n_var, uint64_t n_log) {
        tot = c.take<uint64_t>(kTotWords);
        cmd_off = c.take<uint64_t>(n_var + 1);
        log_off = c.take<uint64_t>(n_var + 1);
        rank = c.take<uint64_t>(n_var);
        log_cmd_off = c.take<uint64_t>(n_log + 1);
        cnt = c.take<uint32_t>(n_log);
        pos = c.take<uint32_t>(n_log);
        const uint64_t big = n_var > n_log ? n_var : n_log;
        scan_tmp = (uint64_t*)c.take<char>(scan_scratch_bytes<uint64_t>(big ? big : 1));
    }
};

template <typename Pos>
hipError_t um_gather(const uint8_t* buf, uint64_t len, const uint64_t* off, uint64_t n_own, Pos pos,
                     const uint64_t* total, uint8_t* op, int64_t* key, int64_t* val, uint64_t cap,
                     uint32_t* err, hipStream_t stream) {
    const uint64_t most = len / 17 < cap ? len / 17 : cap;  // commands the call can write
    const uint64_t tiles = (most + kUmTile - 1) / kUmTile;
    if (!tiles || !n_own) return hipSuccess;
    k_um_gather<Pos><<<(unsigned)tiles, kUmBlock, 0, stream>>>(buf, len, off, n_own, pos, total, op,
                                                               key, val, cap, err);
    return hipGetLastError();
}
}  // namespace

uint64_t unmarshal_work_bytes(uint64_t n_var, uint64_t n_log, Carver&& c) {
    return UmWork(c, n_var, n_log), c.bytes();
}

hipError_t launch_unmarshal(int mode, const uint8_t* buf, uint64_t len, const mpx_var_frame* var,
                            uint64_t n_var, const uint64_t* d_n_var, const mpx_unmarshal_out* o,
                            mpx_unmarshal_result* res, uint64_t log_scratch, void* work,
                            uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    if (n_var >= (1ull << 32) || len > MPX_DECODE_MAX_BYTES) return hipErrorInvalidValue;
    // log instances the call can carry: 9 bytes each at least, and what the scratch holds
    uint64_t n_log = mode == MPX_MODE_MIN && n_var ? len / 9 : 0;
    n_log = n_log < log_scratch ? n_log : log_scratch;
    Carver c(work);
    const UmWork w(c, n_var, n_log);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    k_um_init<<<1, 1, 0, stream>>>(res, w.tot, w.log_cmd_off, o->log_cmd_off, o->cmd_off,
                                   o->log_inst_off, d_n_var, n_var);
    if (!n_var) return hipGetLastError();
    hipError_t r = device_scan(UmCountIn{var, d_n_var, n_var, mode},
                               UmCountOut{w.cmd_off, w.log_off, o->cmd_off, o->log_inst_off, n_var,
                                          w.tot, res},
                               n_var, ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    r = device_scan(UmCodeIn{var, d_n_var, n_var}, UmRankOut{w.rank, n_var, w.tot, res}, n_var,
                    ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
    if (r != hipSuccess) return r;
    k_um_frames<<<(unsigned)((n_var + kUmBlock - 1) / kUmBlock), kUmBlock, 0, stream>>>(
        mode, buf, len, var, n_var, d_n_var, w.rank,
        UmHeads{o->accepts, o->accept_last_committed, o->accept_cap, o->commits, o->commit_cap},
        w.log_off, o->log_recs, o->log_inst_cap, w.cnt, w.pos, n_log, err);
    if (mode == MPX_MODE_MIN) {
        r = device_scan(UmLogIn{w.cnt, w.tot, n_log},
                        UmLogOut{w.log_cmd_off, o->log_cmd_off, o->log_inst_cap, n_log, w.tot, res},
                        n_log, ScanSum64{}, (uint64_t)0, w.scan_tmp, stream);
        if (r != hipSuccess) return r;
        r = um_gather(buf, len, w.log_cmd_off, n_log, UmArrPos{w.pos}, w.tot + kTotLogCmd, o->log_op,
                      o->log_key, o->log_val, o->log_cmd_cap, err, stream);
        if (r != hipSuccess) return r;
    }
    return um_gather(buf, len, w.cmd_off, n_var, UmVarPos{var}, w.tot + kTotCmd, o->op, o->key,
                     o->val, o->cmd_cap, err, stream);
}

}  // namespace mpx

// order.hip — batch assembly (mpx_order_records): up to 16 record arrays, each in arrival order,
// as one array grouped by instance, the groups ascending, slot order = arrival order: the order
// every handler's contract asks for (what the Go shim's sort.SliceStable by Instance produces).
//
// key = (instance - inst_base) << arrival_bits | arrival, ceil(log2(n_inst)) + arrival_bits bits;
// the stable sort of the concatenation by that key is the output order (ties: source index, then
// index within the source = concatenation order). A record outside the window raises kErrNil and
// sorts as the window's first instance, so every index formed below comes from a permutation of
// [0, n) whatever the records hold.
//
// General path (three stations):
//   k_ord_keys    one thread per record of the concatenation: the key and the iota, out-of-window
//                 flags, the count of descents (key[i] < key[i-1]) for MPX_ORD_WAS_ORDERED
//   radix_sort    radix.hpp over exactly the key bits, values = the iota; its value output is the
//                 caller's perm when given
//   k_ord_gather  one thread per output slot: the 16-byte record through the permutation, the
//                 run heads (n_runs); the last workgroup writes *res and takes the counters back
//                 to zero
// One-launch path (n <= MPX_ORDER_ONE_LAUNCH_MAX = one radix tile): k_ord_one, one workgroup; the
// keys and the permutation stay in LDS, sorted by the ranking of radix.hpp's scatter kernel (a
// wave ranks a contiguous 1024-element run, 8 ballots a round), one pass per 8 key bits.
#include <algorithm>

#include "common.hpp"
#include "radix.hpp"

namespace mpx {

static_assert(MPX_ORDER_ONE_LAUNCH_MAX == kRsTile, "the one-launch path sorts one radix tile");
static_assert(sizeof(mpx_order_result) == 32, "mpx_order_result is 32 bytes");

namespace {

constexpr int kOrdT = 256;
// control words (uint32) at the start of the family's scratch
constexpr int kOrdDesc = 0, kOrdRuns = 1, kOrdTicket = 2;

// the call's sources, by value: end[s] = records in sources 0..s (0xFFFFFFFF past n_src)
struct OrdSrcs {
    const uint4* recs[MPX_ORDER_MAX_SRC];
    const uint32_t* arrival[MPX_ORDER_MAX_SRC];
    uint32_t end[MPX_ORDER_MAX_SRC];
};

struct OrdAt {
    const uint4* rec;
    const uint32_t* arr;  // nullptr: no arrival keys
};
// record i (< the total) of the concatenation: its address and its arrival key's. An empty
// source shares its bound with its neighbour, so it is never selected.
__device__ __forceinline__ OrdAt ord_at(const OrdSrcs& S, uint32_t i) {
    const uint4* r = S.recs[0];
    const uint32_t* a = S.arrival[0];
    uint32_t b = 0;
#pragma unroll
    for (int q = 1; q < MPX_ORDER_MAX_SRC; ++q)
        if (S.end[q - 1] <= i) {
            r = S.recs[q];
            a = S.arrival[q];
            b = S.end[q - 1];
        }
    return OrdAt{r + (i - b), a ? a + (i - b) : nullptr};
}

// the key of record i; oob: the record lies outside the window (its key is then the arrival alone)
template <typename K>
__device__ __forceinline__ K ord_key(const OrdSrcs& S, uint32_t i, uint64_t n_inst, int32_t base,
                                     uint32_t ab, bool& oob) {
    const OrdAt at = ord_at(S, i);
    const uint4 r = *at.rec;
    const int64_t rel = (int64_t)(int32_t)r.x - (int64_t)base;
    oob = rel < 0 || (uint64_t)rel >= n_inst;
    const uint32_t amask = ab >= 32 ? 0xFFFFFFFFu : (1u << ab) - 1u;
    const uint64_t arr = at.arr ? (uint64_t)(*at.arr & amask) : 0ull;
    return (K)(((oob ? 0ull : (uint64_t)rel) << ab) | arr);
}

template <typename K>
__device__ __forceinline__ uint64_t ord_inst(K key, uint32_t ab) {
    return (uint64_t)key >> ab;
}

__device__ __forceinline__ void ord_result(mpx_order_result* res, uint32_t n, uint32_t runs,
                                           uint32_t desc, uint64_t first, uint64_t last,
                                           int32_t base) {
    res->n = n;
    res->n_runs = runs;
    res->lo = n ? (int32_t)((int64_t)base + (int64_t)first) : 0;
    res->hi = n ? (int32_t)((int64_t)base + (int64_t)last) : -1;
    res->flags = desc ? 0u : MPX_ORD_WAS_ORDERED;
    res->pad = 0;
}

template <typename K>
__global__ __launch_bounds__(kOrdT) void k_ord_keys(OrdSrcs S, uint32_t n, uint64_t n_inst,
                                                    int32_t base, uint32_t ab,
                                                    K* __restrict__ keys,
                                                    uint32_t* __restrict__ iota,
                                                    uint32_t* __restrict__ ctl,
                                                    uint32_t* __restrict__ err) {
    __shared__ K sk[kOrdT];
    const int t = threadIdx.x;
    const uint64_t i64 = (uint64_t)blockIdx.x * kOrdT + t;
    const bool live = i64 < n;
    const uint32_t i = (uint32_t)i64;
    bool oob = false;
    K k = 0;
    if (live) {
        k = ord_key<K>(S, i, n_inst, base, ab, oob);
        keys[i] = k;
        iota[i] = i;
    }
    sk[t] = k;
    __syncthreads();
    bool desc = false;
    if (live && i > 0) {
        bool o2;
        const K prev = t > 0 ? sk[t - 1] : ord_key<K>(S, i - 1, n_inst, base, ab, o2);
        desc = k < prev;
    }
    const uint64_t md = ballot(desc), mo = ballot(live && oob);
    if (lane_id() == 0) {
        if (md) atomicAdd(&ctl[kOrdDesc], (uint32_t)popc(md));
        if (mo) raise_err(err, kErrNil);
    }
}

template <typename K>
__global__ __launch_bounds__(kOrdT) void k_ord_gather(OrdSrcs S, const K* __restrict__ skeys,
                                                      const uint32_t* __restrict__ perm,
                                                      uint32_t n, uint32_t ab, int32_t base,
                                                      uint4* __restrict__ out,
                                                      uint32_t* __restrict__ ctl,
                                                      mpx_order_result* __restrict__ res) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kOrdT + threadIdx.x;
    bool head = false;
    if (i64 < n) {
        const uint32_t i = (uint32_t)i64;
        const uint32_t p = perm[i];
        const uint4 r = ld_stream(ord_at(S, p).rec);
        st_stream(out + i, r);
        head = i == 0 || ord_inst(skeys[i], ab) != ord_inst(skeys[i - 1], ab);
    }
    const uint64_t mh = ballot(head);
    if (lane_id() == 0 && mh) atomic_add_done(&ctl[kOrdRuns], (uint32_t)popc(mh));
    if (last_workgroup(&ctl[kOrdTicket]) && threadIdx.x == 0) {
        const uint32_t desc = atomic_take(&ctl[kOrdDesc]), runs = atomic_take(&ctl[kOrdRuns]);
        ord_result(res, n, runs, desc, ord_inst(skeys[0], ab), ord_inst(skeys[n - 1], ab), base);
    }
}

// n <= kRsTile records (n == 0 included) in one workgroup
template <typename K>
__global__ __launch_bounds__(kRsT) void k_ord_one(OrdSrcs S, uint32_t n, uint64_t n_inst,
                                                  int32_t base, uint32_t ab, unsigned kbits,
                                                  uint4* __restrict__ out,
                                                  uint32_t* __restrict__ perm,
                                                  mpx_order_result* __restrict__ res,
                                                  uint32_t* __restrict__ err) {
    __shared__ uint32_t cnt[kRsWaves][kRsDigits];
    __shared__ uint32_t tst[kRsDigits];
    __shared__ uint32_t wtot[kRsWaves];
    __shared__ K sk[kRsTile];
    __shared__ uint16_t sv[kRsTile];
    __shared__ uint32_t s_desc, s_runs;
    const int t = threadIdx.x, l = lane_id(), w = t / kWave;
    const uint64_t below = lanes_below(l);
    if (t == 0) s_desc = s_runs = 0;
    bool any_oob = false;
    for (uint32_t i = t; i < n; i += kRsT) {  // the keys, in the concatenation's order
        bool oob;
        sk[i] = ord_key<K>(S, i, n_inst, base, ab, oob);
        sv[i] = (uint16_t)i;
        any_oob |= oob;
    }
    if (any_oob) raise_err(err, kErrNil);
    __syncthreads();
    {
        uint32_t desc = 0;
        for (uint32_t i = t; i < n; i += kRsT) desc += i > 0 && sk[i] < sk[i - 1];
        if (desc) atomicAdd(&s_desc, desc);
    }
    // a wave holds the contiguous run [w0, w0 + 1024), 64 consecutive elements a round
    const uint32_t w0 = (uint32_t)w * kRsWaveItems;
    K k[kRsRounds];
    uint32_t v[kRsRounds], rk[kRsRounds];
#pragma unroll
    for (int r = 0; r < kRsRounds; ++r) {
        const uint32_t i = w0 + (uint32_t)r * kWave + l;
        k[r] = i < n ? sk[i] : K{};
        v[r] = i;
    }
    for (unsigned sh = 0; sh < kbits; sh += 8) {  // one stable pass per digit, low to high
        const unsigned nb = kbits - sh < 8 ? kbits - sh : 8;
        const uint32_t mask = (1u << nb) - 1u;
#pragma unroll
        for (int x = 0; x < kRsWaves; ++x) cnt[x][t] = 0;
        __syncthreads();  // (also: every read of sk / sv of the round before is done)
#pragma unroll
        for (int r = 0; r < kRsRounds; ++r) {
            const bool live = w0 + (uint32_t)r * kWave + l < n;
            const uint32_t d = rs_digit(k[r], sh, mask);
            uint64_t peers = __ballot(live);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint64_t m = __ballot((d >> b) & 1u);
                peers &= ((d >> b) & 1u) ? m : ~m;
            }
            const uint32_t run = live ? cnt[w][d] : 0u;
            rk[r] = run + (uint32_t)popc(peers & below);
            if (live && !(peers >> l >> 1)) cnt[w][d] = run + (uint32_t)popc(peers);  // last lane
        }
        __syncthreads();
        uint32_t tot_d;  // this thread's digit: its count, and per wave the earlier waves' counts
        {
            uint32_t p = 0;
#pragma unroll
            for (int x = 0; x < kRsWaves; ++x) {
                const uint32_t c = cnt[x][t];
                cnt[x][t] = p;
                p += c;
            }
            tot_d = p;
        }
        {  // the digits' starts (block exclusive scan of the 256 counts)
            uint32_t x = tot_d;
#pragma unroll
            for (int d2 = 1; d2 < kWave; d2 <<= 1) {
                const uint32_t y = __shfl_up(x, d2);
                if (l >= d2) x += y;
            }
            if (l == kWave - 1) wtot[w] = x;
            __syncthreads();
            uint32_t before = 0;
#pragma unroll
            for (int x2 = 0; x2 < kRsWaves; ++x2) before += x2 < w ? wtot[x2] : 0u;
            tst[t] = before + x - tot_d;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRsRounds; ++r) {
            if (w0 + (uint32_t)r * kWave + l >= n) continue;
            const uint32_t d = rs_digit(k[r], sh, mask);
            const uint32_t pos = tst[d] + cnt[w][d] + rk[r];
            sk[pos] = k[r];
            sv[pos] = (uint16_t)v[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kRsRounds; ++r) {
            const uint32_t i = w0 + (uint32_t)r * kWave + l;
            if (i < n) {
                k[r] = sk[i];
                v[r] = sv[i];
            }
        }
    }
    // sk / sv hold the sorted keys and the permutation
    {
        uint32_t runs = 0;
        for (uint32_t i = t; i < n; i += kRsT) {
            const uint32_t p = sv[i];
            const uint4 r = ld_stream(ord_at(S, p).rec);
            st_stream(out + i, r);
            if (perm) perm[i] = p;
            runs += i == 0 || ord_inst(sk[i], ab) != ord_inst(sk[i - 1], ab);
        }
        if (runs) atomicAdd(&s_runs, runs);
    }
    __syncthreads();
    if (t == 0)
        ord_result(res, n, s_runs, s_desc, n ? ord_inst(sk[0], ab) : 0,
                   n ? ord_inst(sk[n - 1], ab) : 0, base);
}

struct OrdWork {
    uint32_t* ctl;
    void *kin, *kout;
    uint32_t *iota, *perm;
    void* sort_tmp;
    uint64_t sort_tmp_bytes;
    OrdWork(Carver& c, uint64_t n, bool wide) {
        const uint64_t m = n ? n : 1;
        ctl = (uint32_t*)c.take<char>(kOrderCtlBytes);
        kin = c.take<char>(m * (wide ? 8 : 4));
        kout = c.take<char>(m * (wide ? 8 : 4));
        iota = c.take<uint32_t>(m);
        perm = c.take<uint32_t>(m);
        sort_tmp_bytes = wide ? radix_scratch_bytes<uint64_t, uint32_t>(m)
                              : radix_scratch_bytes<uint32_t, uint32_t>(m);
        sort_tmp = c.take<char>(sort_tmp_bytes);
    }
};

template <typename K>
hipError_t order_general(const OrdSrcs& S, uint32_t n, uint64_t n_inst, int32_t base, uint32_t ab,
                         unsigned kbits, uint4* out, uint32_t* perm, mpx_order_result* res,
                         const OrdWork& w, uint32_t* err, hipStream_t stream) {
    const unsigned blocks = (unsigned)(((uint64_t)n + kOrdT - 1) / kOrdT);
    K* const kin = (K*)w.kin;
    K* const kout = (K*)w.kout;
    uint32_t* const pdst = perm ? perm : w.perm;
    k_ord_keys<K><<<blocks, kOrdT, 0, stream>>>(S, n, n_inst, base, ab, kin, w.iota, w.ctl, err);
    const hipError_t r = radix_sort<K, uint32_t>(kin, kout, w.iota, pdst, n, 0u, kbits, w.sort_tmp,
                                                 w.sort_tmp_bytes, stream);
    if (r != hipSuccess) return r;
    k_ord_gather<K><<<blocks, kOrdT, 0, stream>>>(S, kout, pdst, n, ab, base, out, w.ctl, res);
    return hipGetLastError();
}

}  // namespace

unsigned order_key_bits(uint64_t n_inst, uint32_t arrival_bits) {
    unsigned ib = 0;
    while (ib < 32 && (1ull << ib) < n_inst) ++ib;
    return ib + arrival_bits;
}

uint64_t order_work_bytes(uint64_t n, bool wide, Carver&& c) {
    return OrdWork(c, n, wide), c.bytes();
}

hipError_t launch_order_records(const mpx_order_src* src, uint32_t n_src, uint64_t n_inst,
                                int32_t base, uint32_t arrival_bits, bool general, void* out,
                                uint32_t* perm, mpx_order_result* res, void* work,
                                uint64_t work_bytes, uint32_t* err, hipStream_t stream) {
    if (n_src > MPX_ORDER_MAX_SRC || arrival_bits > 32 || !n_inst || n_inst > (1ull << 32))
        return hipErrorInvalidValue;
    OrdSrcs S;
    uint64_t total = 0;
    for (uint32_t s = 0; s < MPX_ORDER_MAX_SRC; ++s) {
        const bool has = s < n_src && src[s].n;
        S.recs[s] = has ? (const uint4*)src[s].recs : nullptr;
        S.arrival[s] = has ? src[s].arrival : nullptr;
        if (s < n_src) total += src[s].n;
        S.end[s] = s < n_src ? (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull) : 0xFFFFFFFFu;
    }
    if (total >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint32_t n = (uint32_t)total;
    const unsigned kbits = order_key_bits(n_inst, arrival_bits);
    const bool wide = kbits > 32;
    if (n <= (uint32_t)kRsTile && (!general || !n)) {
        if (wide)
            k_ord_one<uint64_t><<<1, kRsT, 0, stream>>>(S, n, n_inst, base, arrival_bits, kbits,
                                                        (uint4*)out, perm, res, err);
        else
            k_ord_one<uint32_t><<<1, kRsT, 0, stream>>>(S, n, n_inst, base, arrival_bits, kbits,
                                                        (uint4*)out, perm, res, err);
        return hipGetLastError();
    }
    Carver c(work);
    const OrdWork w(c, n, wide);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    return wide ? order_general<uint64_t>(S, n, n_inst, base, arrival_bits, kbits, (uint4*)out,
                                          perm, res, w, err, stream)
                : order_general<uint32_t>(S, n, n_inst, base, arrival_bits, kbits, (uint4*)out,
                                          perm, res, w, err, stream);
}

}  // namespace mpx

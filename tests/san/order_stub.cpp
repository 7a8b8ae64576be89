// tests/san/order_stub.cpp — TEST INFRASTRUCTURE ONLY: host-memory stand-ins for the launcher of
// order.hip, for the CPU build of engine.cpp + order.cpp over the stub runtime (hip_stub.cpp,
// where a "device" pointer is a host pointer). Unlike the pattern-filling stand-ins of hip_stub.cpp
// this one really sorts (std::stable_sort by the kernels' key), so the driver can compare what
// comes back through the staging of the host form with the order it expects. It reads every input
// byte, writes exactly the extents the kernels may write and scribbles over the scratch it was
// promised (never the control words), so a slot or a scratch size that is too small faults under
// ASan or shows in the results.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../minpaxos_amd/csrc/kernels.hpp"

namespace mpx {

unsigned order_key_bits(uint64_t n_inst, uint32_t arrival_bits) {
    unsigned ib = 0;
    while (ib < 32 && (1ull << ib) < n_inst) ++ib;
    return ib + arrival_bits;
}

uint64_t order_work_bytes(uint64_t n, bool wide, Carver&& c) {
    (void)c.take<char>(kOrderCtlBytes);
    (void)c.take<char>((n ? n : 1) * (wide ? 24 : 16));
    return c.bytes();
}

hipError_t launch_order_records(const mpx_order_src* src, uint32_t n_src, uint64_t n_inst,
                                int32_t base, uint32_t arrival_bits, bool, void* out,
                                uint32_t* perm, mpx_order_result* res, void* work,
                                uint64_t work_bytes, uint32_t* err, hipStream_t) {
    if (n_src > MPX_ORDER_MAX_SRC || arrival_bits > 32 || !n_inst) return hipErrorInvalidValue;
    struct Rec {
        uint8_t b[16];
    };
    std::vector<Rec> cat;
    std::vector<uint64_t> key;
    const uint32_t amask = arrival_bits >= 32 ? 0xFFFFFFFFu : (1u << arrival_bits) - 1u;
    for (uint32_t s = 0; s < n_src; ++s)
        for (size_t i = 0; i < src[s].n; ++i) {
            Rec r;
            memcpy(r.b, (const char*)src[s].recs + 16 * i, 16);
            int32_t inst;
            memcpy(&inst, r.b, 4);
            const int64_t rel = (int64_t)inst - base;
            const bool oob = rel < 0 || (uint64_t)rel >= n_inst;
            if (oob) *err |= kErrNil;
            const uint64_t a = src[s].arrival ? (src[s].arrival[i] & amask) : 0;
            cat.push_back(r);
            key.push_back(((oob ? 0ull : (uint64_t)rel) << arrival_bits) | a);
        }
    const size_t n = cat.size();
    if (n) {
        const uint64_t need = order_work_bytes(n, order_key_bits(n_inst, arrival_bits) > 32);
        if (work_bytes < need) return hipErrorInvalidValue;
        for (uint64_t i = 0; i < kOrderCtlBytes; ++i)
            if (((const uint8_t*)work)[i]) return hipErrorInvalidValue;  // zero between calls
        memset((char*)work + kOrderCtlBytes, 0xEE, need - kOrderCtlBytes);
    }
    std::vector<uint32_t> p(n);
    for (size_t i = 0; i < n; ++i) p[i] = (uint32_t)i;
    std::stable_sort(p.begin(), p.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    uint64_t runs = 0;
    bool ordered = true;
    for (size_t i = 0; i < n; ++i) {
        memcpy((char*)out + 16 * i, cat[p[i]].b, 16);
        if (perm) perm[i] = p[i];
        runs += i == 0 || (key[p[i]] >> arrival_bits) != (key[p[i - 1]] >> arrival_bits);
        ordered &= p[i] == i;
    }
    res->n = n;
    res->n_runs = runs;
    res->lo = n ? (int32_t)(base + (int64_t)(key[p[0]] >> arrival_bits)) : 0;
    res->hi = n ? (int32_t)(base + (int64_t)(key[p[n - 1]] >> arrival_bits)) : -1;
    res->flags = ordered ? MPX_ORD_WAS_ORDERED : 0u;
    res->pad = 0;
    return hipSuccess;
}

}  // namespace mpx

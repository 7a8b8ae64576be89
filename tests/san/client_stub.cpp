// tests/san/client_stub.cpp — TEST INFRASTRUCTURE ONLY: host-memory stand-ins for the launcher of
// client.hip, for the CPU build of engine.cpp + client.cpp over the stub runtime (hip_stub.cpp,
// where a "device" pointer is a host pointer). Like order_stub.cpp this one really does the work (a
// sequential framing loop per connection, with the device form's treatment of faulty
// connections), so the driver can compare what comes back through the staging of the host form
// with what it expects. It reads every input byte of every connection, writes exactly the extents
// the kernels may write and scribbles over the scratch it was promised, so a slot or a scratch
// size that is too small faults under ASan or shows in the results.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../minpaxos_amd/csrc/kernels.hpp"

namespace mpx {

uint64_t client_work_bytes(uint64_t len, uint64_t n_conns, uint64_t n_groups, Carver&& c) {
    (void)c.take<char>(len / 3 + 16 * n_conns + 4 * (n_groups + 1) + 64);
    return c.bytes();
}

hipError_t launch_decode_client_streams(const uint8_t* buf, uint64_t len,
                                        const mpx_client_conn* conns, uint64_t n_conns,
                                        uint64_t n_groups, const mpx_client_out* out,
                                        mpx_client_conn_result* conn_res, mpx_client_result* res,
                                        void* work, uint64_t work_bytes, uint32_t* err, hipStream_t) {
    if (len > (uint64_t)MPX_DECODE_MAX_BYTES || n_conns > MPX_CLIENT_MAX_CONNS ||
        n_groups > MPX_CLIENT_MAX_GROUPS)
        return hipErrorInvalidValue;
    if (n_conns) {
        const uint64_t need = client_work_bytes(len, n_conns, n_groups);
        if (work_bytes < need) return hipErrorInvalidValue;
        memset(work, 0xEE, need);
    }
    uint64_t end = 0, total = 0, dropped = 0, partial = 0;
    uint32_t grp = 0;
    std::vector<uint64_t> first_of(n_groups + 1, ~0ull);  // first proposal of the first connection
    for (uint64_t k = 0; k < n_conns; ++k) {              // with group >= g
        const mpx_client_conn c = conns[k];
        const bool self_ok = !(c.offset & (MPX_CLIENT_ALIGN - 1)) && c.offset <= len &&
                             c.length <= len - c.offset && c.group < n_groups;
        const bool valid = self_ok && c.offset >= end && c.group >= grp;
        if (!valid) *err |= kErrInval;
        if (self_ok) {
            end = std::max(end, c.offset + c.length);
            grp = std::max(grp, c.group);
        }
        const uint32_t gkey = valid ? c.group : grp;
        for (uint64_t g = 0; g <= gkey && g < n_groups; ++g)
            if (first_of[g] == ~0ull) first_of[g] = total;
        mpx_client_conn_result r{};
        r.first = total;
        r.stop_reason = MPX_DECODE_END;
        r.stop_code = -1;
        const uint8_t* b = buf + c.offset;
        uint32_t p = 0;
        const uint32_t n = valid ? c.length : 0;
        while (p < n) {
            const uint8_t code = b[p];
            const uint32_t fl = code == MPX_CLIENT_PROPOSE || code == MPX_CLIENT_PROPOSE_AND_READ
                                    ? MPX_CLIENT_PROPOSE_FRAME
                                    : code == MPX_CLIENT_READ ? MPX_CLIENT_READ_FRAME : 1;
            if (p + fl > n) {
                r.stop_reason = MPX_DECODE_PARTIAL;
                r.stop_code = code;
                ++partial;
                break;
            }
            unsigned sum = 0;
            for (uint32_t i = 0; i < fl; ++i) sum += b[p + i];  // every byte of the frame is read
            if (code == MPX_CLIENT_PROPOSE) {
                if (total < out->prop_cap) {
                    out->op[total] = b[p + 5];
                    memcpy(&out->key[total], b + p + 6, 8);
                    memcpy(&out->val[total], b + p + 14, 8);
                    mpx_proposal m;
                    memcpy(&m.command_id, b + p + 1, 4);
                    memcpy(&m.timestamp, b + p + 22, 8);
                    m.client = (uint32_t)k + (sum & 0u);
                    out->meta[total] = m;
                }
                ++total;
                ++r.n_proposals;
            } else {
                ++dropped;
                ++r.n_dropped;
            }
            p += fl;
        }
        r.consumed = p;
        conn_res[k] = r;
    }
    uint64_t sends = 0;
    for (uint64_t g = 0; g <= n_groups; ++g) {
        const uint64_t at = g < n_groups && first_of[g] != ~0ull ? first_of[g] : total;
        const uint64_t nx = g + 1 < n_groups && first_of[g + 1] != ~0ull ? first_of[g + 1] : total;
        if (out->prop_off) out->prop_off[g] = at;
        if (out->send_off) out->send_off[g] = sends;
        if (g < n_groups)
            sends += (nx - at + MPX_PROPOSE_MAX_BATCH - 1) / MPX_PROPOSE_MAX_BATCH;
    }
    res->n_proposals = total;
    res->n_dropped = dropped;
    res->n_partial = partial;
    res->n_sends = sends;
    return hipSuccess;
}

}  // namespace mpx

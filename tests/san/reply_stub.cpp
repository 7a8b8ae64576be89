// tests/san/reply_stub.cpp — TEST INFRASTRUCTURE ONLY: host-memory stand-ins for the launcher of
// replies.hip, for the CPU build of engine.cpp + replies.cpp over the stub runtime (hip_stub.cpp,
// where a "device" pointer is a host pointer). Like order_stub.cpp and client_stub.cpp this one
// really does the work (a sequential expansion over the slots, with the device form's treatment
// of faulty slots), so the driver can compare what comes back through the staging of the host
// form with what it expects. It reads every input byte the kernels may read, writes exactly the
// extents the kernels may write and scribbles over the scratch it was promised, so a slot or a
// scratch size that is too small faults under ASan or shows in the results.
#include <algorithm>
#include <cstring>

#include "../../minpaxos_amd/csrc/kernels.hpp"

namespace mpx {

uint64_t reply_work_bytes(uint64_t n_sends, Carver&& c) {
    (void)c.take<char>(12 * n_sends + 8);
    (void)c.take<char>(n_sends / 64 + 64);
    return c.bytes();
}

hipError_t launch_build_replies(const mpx_reply_batch* b, mpx_reply_rec* recs, uint64_t cap,
                                mpx_commit_send* commit_sends, mpx_reply_result* res, void* work,
                                uint64_t work_bytes, uint32_t* err, hipStream_t) {
    const uint64_t n = b->n_sends;
    if (n >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    const bool one = !(b->flags & MPX_RB_GENERAL) && n <= MPX_RB_ONE_LAUNCH_SLOTS &&
                     cap <= MPX_RB_ONE_LAUNCH_REPLIES;
    if (n && !one) {
        const uint64_t need = reply_work_bytes(n);
        if (work_bytes < need) return hipErrorInvalidValue;
        memset(work, 0xEE, need);
    }
    // every byte of the inputs is read (a staging slot that is too small faults here)
    unsigned sum = 0;
    for (uint64_t i = 0; i < b->n_props * sizeof(mpx_proposal); ++i) sum += ((const uint8_t*)b->meta)[i];
    for (uint64_t i = 0; b->mask && i < b->n_inst; ++i) sum += b->mask[i];
    for (uint64_t i = 0; b->ret && i < b->n_ret * 8; ++i) sum += ((const uint8_t*)b->ret)[i];
    const bool refusals = b->kind == MPX_RB_FALSE;
    const uint32_t eligible =
        refusals ? MPX_PH_NOT_LEADER | MPX_PH_REFUSED : MPX_PH_ACCEPT | MPX_PH_PREPARE;
    uint64_t total = 0, slots = 0;
    for (uint64_t s = 0; s < n; ++s) {
        const mpx_accept_send x = b->sends[s];
        bool sel = false;
        uint32_t cnt = 0;
        if (x.flags & eligible) {
            uint32_t bits = 0;
            if (x.first_cmd > b->n_props || x.n_cmds > b->n_props - x.first_cmd) bits |= kErrInval;
            const uint64_t rf = b->ret_first ? b->ret_first[s] : x.first_cmd;
            sel = true;
            if (b->mask) {
                const int64_t rel = (int64_t)x.instance - b->inst_base;
                if (rel < 0 || (uint64_t)rel >= b->n_inst) bits |= kErrNil;
                else sel = b->mask[rel] != 0;
            }
            if (sel && b->kind == MPX_RB_EXECUTED && (rf > b->n_ret || x.n_cmds > b->n_ret - rf))
                bits |= kErrInval;  // only a selected slot reads results
            if (bits) {
                *err |= bits;
                sel = false;
            }
            if (sel) cnt = refusals && !(x.flags & MPX_PH_NOT_LEADER) ? std::min(x.n_cmds, 1u) : x.n_cmds;
            for (uint32_t k = 0; k < cnt; ++k, ++total) {
                if (total >= cap) continue;
                const mpx_proposal m = b->meta[x.first_cmd + k];
                mpx_reply_rec r{0, m.timestamp, m.command_id, m.client + (sum & 0u)};
                if (refusals) r.timestamp = 0, r.command_id = -1;
                if (b->kind == MPX_RB_EXECUTED) r.value = b->ret[rf + k];
                recs[total] = r;
            }
            slots += sel;
        }
        if (commit_sends)
            commit_sends[s] = mpx_commit_send{x.instance, x.ballot, x.first_cmd, x.n_cmds,
                                              sel ? MPX_CS_SEND : 0u, {0, 0}};
    }
    if (b->pad_client != MPX_RB_NO_PAD)
        for (uint64_t i = std::min(total, cap); i < cap; ++i) recs[i] = mpx_reply_rec{0, 0, 0, b->pad_client};
    res->n_replies = total;
    res->n_slots = slots;
    return hipSuccess;
}

}  // namespace mpx

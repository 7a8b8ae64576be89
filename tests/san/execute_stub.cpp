// tests/san/execute_stub.cpp — TEST INFRASTRUCTURE ONLY: host-memory stand-ins for the launcher of
// execute.hip, for the CPU build of engine.cpp + execute.cpp over the stub runtime (hip_stub.cpp,
// where a "device" pointer is a host pointer). Like reply_stub.cpp this one really does the work
// (executeCommands' walk per group and a sequential gather, with the device form's treatment of
// faulty groups and instances), so the driver can compare what comes back through the staging of
// the host form with what it expects. It reads every input byte the kernels may read, writes
// exactly the extents the kernels may write, requires the groups' stop words as the engine must
// leave them between calls and scribbles over the rest of the scratch it was promised, so a slot
// or a scratch size that is too small faults under ASan or shows in the results.
#include <algorithm>
#include <cstring>

#include "../../minpaxos_amd/csrc/kernels.hpp"

namespace mpx {

uint64_t execute_work_bytes(uint64_t n_inst, uint64_t group_cap, Carver&& c) {
    (void)c.take<uint32_t>(group_cap);
    (void)c.take<char>(12 * n_inst + 8);
    (void)c.take<char>(group_cap / 16 + 64);
    return c.bytes();
}

hipError_t launch_execute_gather(const mpx_execute_batch* b, const mpx_execute_out* out,
                                 mpx_execute_result* res, void* work, uint64_t work_bytes,
                                 uint64_t group_cap, uint32_t* err, hipStream_t) {
    const uint64_t n = b->n_inst, G = b->n_groups, cap = out->cap;
    if (n >= 0xFFFFFFFFull || G > n) return hipErrorInvalidValue;
    const bool one = !(b->flags & MPX_XG_GENERAL) && n <= MPX_XG_ONE_LAUNCH_INST &&
                     cap <= MPX_XG_ONE_LAUNCH_CMDS;
    if (!one) {
        const uint64_t need = execute_work_bytes(n, group_cap);
        if (work_bytes < need || G > group_cap) return hipErrorInvalidValue;
        const uint32_t* stop = (const uint32_t*)work;
        for (uint64_t g = 0; g < group_cap; ++g)
            if (stop[g] != kXgNoStop) return hipErrorInvalidValue;  // the engine initialises them
        const uint64_t keep = (group_cap * 4 + 255) & ~255ull;
        memset((char*)work + keep, 0xEE, need - keep);
    }
    // every byte of the inputs is read (a staging slot that is too small faults here)
    unsigned sum = 0;
    for (uint64_t i = 0; i < b->n_src; ++i)
        sum += b->src_op[i] + ((const uint8_t*)b->src_key)[8 * i + 7] + ((const uint8_t*)b->src_val)[8 * i + 7];
    for (uint64_t i = 0; i < n * sizeof(mpx_inst_cmds); ++i) sum += ((const uint8_t*)b->inst)[i];
    for (uint64_t i = 0; b->sends && i < b->n_sends * sizeof(mpx_accept_send); ++i)
        sum += ((const uint8_t*)b->sends)[i];
    uint64_t total = 0, ran = 0, moved = 0;
    for (uint64_t i = 0; i < n; ++i) out->mask[i] = 0;
    for (uint64_t i = 0; out->inst_first && i < n; ++i) out->inst_first[i] = 0;
    std::vector<uint64_t> first(n + 1, 0);
    for (uint64_t g = 0; g < G; ++g) {
        const int64_t none = (int64_t)b->inst_base + (int64_t)(g * b->ipg) - 1;
        const int64_t cu = b->committed_upto[g], ex = b->executed_in[g];
        if (out->grp_cmd_off) out->grp_cmd_off[g] = total;
        int64_t i = ex + 1;
        if (cu < none || cu > none + b->ipg || ex < none || ex > none + b->ipg) {
            *err |= kErrInval;
            b->executed_out[g] = (int32_t)ex;
            continue;
        }
        for (; i <= cu; ++i) {
            const mpx_inst_cmds x = b->inst[i - b->inst_base];
            if (!(x.flags & MPX_IC_HAS_CMDS)) break;
            uint32_t k = x.n_cmds;
            if (x.first_cmd > b->n_src || k > b->n_src - x.first_cmd) *err |= kErrInval, k = 0;
            out->mask[i - b->inst_base] = 1;
            first[i - b->inst_base + 1] = k;
            ++ran;
            for (uint32_t j = 0; j < k; ++j, ++total) {
                if (total >= cap) continue;
                out->op[total] = b->src_op[x.first_cmd + j] + (uint8_t)(sum & 0u);
                out->key[total] = b->src_key[x.first_cmd + j];
                out->val[total] = b->src_val[x.first_cmd + j];
            }
        }
        b->executed_out[g] = (int32_t)(i - 1);
        moved += i - 1 != ex;
    }
    for (uint64_t i = 0; i < n; ++i) first[i + 1] += first[i];
    for (uint64_t i = 0; out->inst_first && i < n; ++i) out->inst_first[i] = first[i];
    if (out->grp_cmd_off) out->grp_cmd_off[G] = total;
    for (uint64_t s = 0; out->ret_first && s < b->n_sends; ++s) {
        const int64_t rel = (int64_t)b->sends[s].instance - b->inst_base;
        out->ret_first[s] = rel >= 0 && (uint64_t)rel < n ? first[rel] : 0;
    }
    if (b->flags & MPX_XG_PAD)
        for (uint64_t j = std::min(total, cap); j < cap; ++j)
            out->op[j] = 0, out->key[j] = (int64_t)j, out->val[j] = 0;
    *res = mpx_execute_result{total, ran, moved, 0};
    return hipSuccess;
}

}  // namespace mpx

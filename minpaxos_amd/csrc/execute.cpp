// execute.cpp — the C ABI of execute assembly (mpx_execute_gather[_reserve|_dev], include/mpx.h)
// over the launcher of execute.hip: validation, then, for the host form, Stage staging around the
// _dev form, like the other host-pointer entry points (engine.cpp, order.cpp, client.cpp,
// replies.cpp). The kernels' pieces shared with the other assembly families are assemble.hpp's.
#include <algorithm>
#include <cstdint>
#include <string>

#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {

// what both forms check
int execute_args(mpx_engine* e, const mpx_execute_batch* b, const mpx_execute_out* out,
                 const void* res) {
    if (!b || !out || !res) return fail(e, MPX_E_INVAL, "null argument");
    if ((b->n_inst && (!b->inst || !out->mask)) ||
        (b->n_groups && (!b->committed_upto || !b->executed_in || !b->executed_out)) ||
        (b->n_src && (!b->src_op || !b->src_key || !b->src_val)) ||
        (out->cap && (!out->op || !out->key || !out->val)) || (b->n_sends && !b->sends))
        return fail(e, MPX_E_INVAL, "null argument");
    if (b->flags & ~(MPX_XG_PAD | MPX_XG_GENERAL)) return fail(e, MPX_E_INVAL, "unknown flags");
    if (b->reserved) return fail(e, MPX_E_INVAL, "reserved is not 0");
    if (out->ret_first && !b->sends) return fail(e, MPX_E_INVAL, "ret_first needs sends");
    if ((b->n_groups && !b->ipg) || (uint64_t)b->n_inst != (uint64_t)b->n_groups * b->ipg)
        return fail(e, MPX_E_INVAL, "n_inst is not n_groups * ipg");
    if ((uint64_t)b->n_inst >= 0xFFFFFFFFull)
        return fail(e, MPX_E_UNSUPPORTED, "2^32-1 window slots or more");
    return MPX_OK;
}

// grow the family's scratch to calls of n_inst slots in n_groups groups and (re)initialise the
// groups' stop words: the region of them grows with the group capacity, over bytes that were
// other scratch before
int execute_grow(mpx_engine* e, size_t n_inst, size_t n_groups) {
    const size_t inst = std::max(e->xg_inst_cap, n_inst), groups = std::max(e->xg_group_cap, n_groups);
    if (e->xg_work.p && inst == e->xg_inst_cap && groups == e->xg_group_cap) return MPX_OK;
    // (the stream's earlier calls may still use the words)
    GROW(e, e->xg_work, mpx::execute_work_bytes(inst, groups));
    e->xg_inst_cap = inst, e->xg_group_cap = groups;
    if (groups)
        HIPCHK(e, hipMemsetAsync(e->xg_work.p, 0xFF, groups * sizeof(uint32_t), e->stream));
    return MPX_OK;
}

}  // namespace

extern "C" {

int mpx_execute_gather_reserve(mpx_engine* e, size_t max_n_inst, size_t max_n_groups) {
    if (!e) return MPX_E_INVAL;
    if ((uint64_t)max_n_inst >= 0xFFFFFFFFull || (uint64_t)max_n_groups >= 0xFFFFFFFFull)
        return fail(e, MPX_E_UNSUPPORTED, "2^32-1 window slots or more");
    CK(begin(e));
    CK(execute_grow(e, max_n_inst, max_n_groups));
    return finish(e);
}

int mpx_execute_gather_dev(mpx_engine* e, const mpx_execute_batch* b, const mpx_execute_out* out,
                           mpx_execute_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(execute_args(e, b, out, d_res));
    if ((((uintptr_t)b->inst | (uintptr_t)b->sends) & 15) ||
        (((uintptr_t)b->src_key | (uintptr_t)b->src_val | (uintptr_t)out->key | (uintptr_t)out->val |
          (uintptr_t)out->inst_first | (uintptr_t)out->ret_first | (uintptr_t)out->grp_cmd_off |
          (uintptr_t)d_res) & 7) ||
        (((uintptr_t)b->committed_upto | (uintptr_t)b->executed_in | (uintptr_t)b->executed_out) & 3))
        return fail(e, MPX_E_INVAL, "mpx_execute_gather_dev: inst and sends must be 16-byte "
                                    "aligned, the 8-byte arrays and d_res 8, committed_upto and "
                                    "executed_in / executed_out 4");
    if (!e->xg_work.p || b->n_groups > e->xg_group_cap || b->n_inst > e->xg_inst_cap)
        return fail(e, MPX_E_INVAL, "mpx_execute_gather_dev: call mpx_execute_gather_reserve("
                                    "max_n_inst, max_n_groups) first (the dev entry point never "
                                    "allocates)");
    HIPCHK(e, mpx::launch_execute_gather(b, out, d_res, e->xg_work.p, e->xg_work.cap,
                                         e->xg_group_cap, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_execute_gather(mpx_engine* e, const mpx_execute_batch* b, const mpx_execute_out* out,
                       mpx_execute_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(execute_args(e, b, out, res));
    // the device kernels report these through the error word; here they answer before any launch:
    // the walk itself, as executeCommands makes it
    uint64_t total = 0;
    for (size_t g = 0; g < b->n_groups; ++g) {
        const int64_t none = (int64_t)b->inst_base + (int64_t)((uint64_t)g * b->ipg) - 1;
        const int64_t cu = b->committed_upto[g], ex = b->executed_in[g];
        if (cu < none || cu > none + b->ipg || ex < none || ex > none + b->ipg)
            return fail(e, MPX_E_INVAL, "committed_upto or executed_in outside its group's window");
        for (int64_t i = ex + 1; i <= cu; ++i) {
            const mpx_inst_cmds& x = b->inst[i - b->inst_base];
            if (!(x.flags & MPX_IC_HAS_CMDS)) break;
            if (x.first_cmd > (uint64_t)b->n_src || x.n_cmds > (uint64_t)b->n_src - x.first_cmd)
                return fail(e, MPX_E_INVAL, "an instance's command range leaves [0, n_src)");
            total += x.n_cmds;
            if (total >= 0xFFFFFFFFull)
                return fail(e, MPX_E_UNSUPPORTED, "2^32-1 commands or more");
        }
    }
    CK(begin(e));
    CK(execute_grow(e, b->n_inst, b->n_groups));
    // the commands the call writes: those below cap, and with padding the whole of cap
    const size_t n_out =
        b->flags & MPX_XG_PAD ? out->cap : (size_t)std::min<uint64_t>(total, out->cap);
    Stage L(e);
    const Slot s_inst = L.add(b->n_inst * sizeof(mpx_inst_cmds)),
               s_cu = L.add(b->n_groups * sizeof(int32_t)),
               s_ex = L.add(b->n_groups * sizeof(int32_t)),
               s_sop = L.add(b->n_src), s_skey = L.add(b->n_src * sizeof(int64_t)),
               s_sval = L.add(b->n_src * sizeof(int64_t)),
               s_sends = L.add(b->sends ? b->n_sends * sizeof(mpx_accept_send) : 0),
               s_op = L.add(n_out), s_key = L.add(n_out * sizeof(int64_t)),
               s_val = L.add(n_out * sizeof(int64_t)), s_mask = L.add(b->n_inst),
               s_if = L.add(out->inst_first ? b->n_inst * sizeof(uint64_t) : 0),
               s_rf = L.add(out->ret_first ? b->n_sends * sizeof(uint64_t) : 0),
               s_go = L.add(out->grp_cmd_off ? (b->n_groups + 1) * sizeof(uint64_t) : 0),
               s_res = L.add(sizeof(mpx_execute_result));
    CK(L.commit());
    CK(L.in(s_inst, b->inst));
    CK(L.in(s_cu, b->committed_upto));
    CK(L.in(s_ex, b->executed_in));
    CK(L.in(s_sop, b->src_op));
    CK(L.in(s_skey, b->src_key));
    CK(L.in(s_sval, b->src_val));
    if (b->sends) CK(L.in(s_sends, b->sends));
    mpx_execute_batch d = *b;
    d.inst = L.at<mpx_inst_cmds>(s_inst, b->inst);
    d.committed_upto = L.at<int32_t>(s_cu, b->committed_upto);
    d.executed_in = d.executed_out = L.at<int32_t>(s_ex, b->executed_in);  // in place
    d.src_op = L.at<uint8_t>(s_sop, b->src_op);
    d.src_key = L.at<int64_t>(s_skey, b->src_key);
    d.src_val = L.at<int64_t>(s_sval, b->src_val);
    d.sends = L.at<mpx_accept_send>(s_sends, b->sends);
    mpx_execute_out o = *out;
    o.cap = n_out;
    o.op = L.at<uint8_t>(s_op, n_out ? out->op : nullptr);
    o.key = L.at<int64_t>(s_key, n_out ? out->key : nullptr);
    o.val = L.at<int64_t>(s_val, n_out ? out->val : nullptr);
    o.mask = L.at<uint8_t>(s_mask, out->mask);
    o.inst_first = L.at<uint64_t>(s_if, out->inst_first);
    o.ret_first = L.at<uint64_t>(s_rf, out->ret_first);
    o.grp_cmd_off = L.at<uint64_t>(s_go, out->grp_cmd_off);
    CK(mpx_execute_gather_dev(e, &d, &o, L.at<mpx_execute_result>(s_res), e->stream));
    CK(L.out(s_op, out->op));
    CK(L.out(s_key, out->key));
    CK(L.out(s_val, out->val));
    CK(L.out(s_mask, out->mask));
    CK(L.out(s_ex, b->executed_out));
    if (out->inst_first) CK(L.out(s_if, out->inst_first));
    if (out->ret_first) CK(L.out(s_rf, out->ret_first));
    if (out->grp_cmd_off) CK(L.out(s_go, out->grp_cmd_off));
    CK(L.out(s_res, res));
    return finish(e);
}

}  // extern "C"

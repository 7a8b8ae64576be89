// replies.cpp — the C ABI of reply assembly (mpx_build_replies[_reserve|_dev], include/mpx.h)
// over the launcher of replies.hip: validation, then, for the host form, Stage staging around the
// _dev form, like the other host-pointer entry points (engine.cpp, order.cpp, client.cpp). The
// kernels' pieces shared with the other assembly families are assemble.hpp's.
#include <algorithm>
#include <cstdint>
#include <string>

#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {

// what both forms check
int reply_args(mpx_engine* e, const mpx_reply_batch* b, const void* recs, size_t cap,
               const void* commit_sends, const void* res) {
    if (!b || !res || (b->n_sends && !b->sends) || (cap && !recs) || (b->n_props && !b->meta))
        return fail(e, MPX_E_INVAL, "null argument");
    if (b->kind != MPX_RB_FALSE && b->kind != MPX_RB_DECIDED && b->kind != MPX_RB_EXECUTED)
        return fail(e, MPX_E_INVAL, "unknown kind");
    if (b->flags & ~MPX_RB_GENERAL) return fail(e, MPX_E_INVAL, "unknown flags");
    if (b->reserved) return fail(e, MPX_E_INVAL, "reserved is not 0");
    if (b->kind == MPX_RB_FALSE && (b->mask || b->ret || b->ret_first || commit_sends))
        return fail(e, MPX_E_INVAL,
                    "MPX_RB_FALSE takes no mask, ret, ret_first or commit_sends");
    if (b->kind == MPX_RB_DECIDED && (b->ret || b->ret_first))
        return fail(e, MPX_E_INVAL, "MPX_RB_DECIDED takes no ret or ret_first");
    if (b->kind == MPX_RB_EXECUTED && !b->ret)
        return fail(e, MPX_E_INVAL, "MPX_RB_EXECUTED needs ret");
    if ((uint64_t)b->n_sends >= 0xFFFFFFFFull)
        return fail(e, MPX_E_UNSUPPORTED, "2^32-1 slots or more");
    return MPX_OK;
}

}  // namespace

extern "C" {

int mpx_build_replies_reserve(mpx_engine* e, size_t max_sends) {
    if (!e) return MPX_E_INVAL;
    if ((uint64_t)max_sends >= 0xFFFFFFFFull)
        return fail(e, MPX_E_UNSUPPORTED, "2^32-1 slots or more");
    return reserve(e, e->rp_work, mpx::reply_work_bytes(max_sends));
}

int mpx_build_replies_dev(mpx_engine* e, const mpx_reply_batch* b, mpx_reply_rec* d_recs,
                          size_t cap, mpx_commit_send* d_commit_sends, mpx_reply_result* d_res,
                          void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(reply_args(e, b, d_recs, cap, d_commit_sends, d_res));
    if (((uintptr_t)b->sends & 15) || ((uintptr_t)b->meta & 15) ||
        ((uintptr_t)d_commit_sends & 15) || ((uintptr_t)d_recs & 7) || ((uintptr_t)b->ret & 7) ||
        ((uintptr_t)b->ret_first & 7) || ((uintptr_t)d_res & 7))
        return fail(e, MPX_E_INVAL, "mpx_build_replies_dev: sends, meta and d_commit_sends must be "
                                    "16-byte aligned, d_recs, ret, ret_first and d_res 8");
    // (a call of no slot uses no scratch)
    CK(reserved(e, e->rp_work, b->n_sends ? mpx::reply_work_bytes(b->n_sends) : 0,
                "mpx_build_replies_dev", "mpx_build_replies_reserve(max_sends)"));
    HIPCHK(e, mpx::launch_build_replies(b, d_recs, cap, d_commit_sends, d_res, e->rp_work.p,
                                        e->rp_work.cap, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_build_replies(mpx_engine* e, const mpx_reply_batch* b, mpx_reply_rec* recs, size_t cap,
                      mpx_commit_send* commit_sends, mpx_reply_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(reply_args(e, b, recs, cap, commit_sends, res));
    // the device kernels report these through the error word; here they answer before any launch
    const bool refusals = b->kind == MPX_RB_FALSE;
    const uint32_t eligible = refusals ? MPX_PH_NOT_LEADER | MPX_PH_REFUSED
                                       : MPX_PH_ACCEPT | MPX_PH_PREPARE;
    uint64_t total = 0;
    for (size_t s = 0; s < b->n_sends; ++s) {
        const mpx_accept_send& x = b->sends[s];
        if (!(x.flags & eligible)) continue;
        if (x.first_cmd > (uint64_t)b->n_props || x.n_cmds > (uint64_t)b->n_props - x.first_cmd)
            return fail(e, MPX_E_INVAL, "a slot's command range leaves [0, n_props)");
        bool selected = true;
        if (b->mask) {
            const int64_t rel = (int64_t)x.instance - b->inst_base;
            if (rel < 0 || (uint64_t)rel >= (uint64_t)b->n_inst)
                return fail(e, MPX_E_NIL_INSTANCE, "a slot names an instance outside the window");
            selected = b->mask[rel] != 0;
        }
        if (!selected) continue;
        // only a selected slot reads results: an instance that did not execute in this call has none,
        // and mpx_execute_gather's ret_first puts it wherever the executed ones before it end
        if (b->kind == MPX_RB_EXECUTED) {
            const uint64_t rf = b->ret_first ? b->ret_first[s] : x.first_cmd;
            if (rf > (uint64_t)b->n_ret || x.n_cmds > (uint64_t)b->n_ret - rf)
                return fail(e, MPX_E_INVAL, "a selected slot's result range leaves [0, n_ret)");
        }
        total += refusals && !(x.flags & MPX_PH_NOT_LEADER) ? std::min(x.n_cmds, 1u) : x.n_cmds;
        if (total >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 replies or more");
    }
    CK(begin(e));
    if (b->n_sends) GROW(e, e->rp_work, mpx::reply_work_bytes(b->n_sends));
    // the records the call writes: the replies below cap, and with padding the whole of cap
    const size_t n_out =
        b->pad_client != MPX_RB_NO_PAD ? cap : (size_t)std::min<uint64_t>(total, cap);
    Stage L(e);
    const Slot s_sends = L.add(b->n_sends * sizeof(mpx_accept_send)),
               s_meta = L.add(b->n_props * sizeof(mpx_proposal)),
               s_mask = L.add(b->mask ? b->n_inst : 0),
               s_ret = L.add(b->ret ? b->n_ret * sizeof(int64_t) : 0),
               s_rf = L.add(b->ret_first ? b->n_sends * sizeof(uint64_t) : 0),
               s_recs = L.add(n_out * sizeof(mpx_reply_rec)),
               s_cs = L.add(commit_sends ? b->n_sends * sizeof(mpx_commit_send) : 0),
               s_res = L.add(sizeof(mpx_reply_result));
    CK(L.commit());
    CK(L.in(s_sends, b->sends));
    CK(L.in(s_meta, b->meta));
    if (b->mask) CK(L.in(s_mask, b->mask));
    if (b->ret) CK(L.in(s_ret, b->ret));
    if (b->ret_first) CK(L.in(s_rf, b->ret_first));
    mpx_reply_batch d = *b;
    d.sends = L.at<mpx_accept_send>(s_sends, b->sends);
    d.meta = L.at<mpx_proposal>(s_meta, b->meta);
    d.mask = L.at<uint8_t>(s_mask, b->mask);
    d.ret = L.at<int64_t>(s_ret, b->ret);
    d.ret_first = L.at<uint64_t>(s_rf, b->ret_first);
    CK(mpx_build_replies_dev(e, &d, L.at<mpx_reply_rec>(s_recs, n_out ? recs : nullptr), n_out,
                             L.at<mpx_commit_send>(s_cs, commit_sends),
                             L.at<mpx_reply_result>(s_res), e->stream));
    CK(L.out(s_recs, recs));
    if (commit_sends) CK(L.out(s_cs, commit_sends));
    CK(L.out(s_res, res));
    return finish(e);
}

}  // extern "C"

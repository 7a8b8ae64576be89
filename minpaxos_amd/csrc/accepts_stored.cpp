// accepts_stored.cpp — the C ABI of the Accept encoder that reads the catch-up log from the
// instance store (mpx_encode_accepts_stored[_reserve|_dev], include/mpx.h) over the launcher of
// accepts_stored.hip: validation, then, for the host form, Stage staging around the _dev form, like
// the other host-pointer entry points. A file of its own so that the units that link engine.cpp
// alone keep their set of launchers. It shares the dense encoder's scratch (mpx_engine::ab_work).
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {
// what the host and _dev forms of the stored Accept encoder check alike (accept_batch_args' list)
int accept_store_args(mpx_engine* e, const mpx_accept_store_batch* b, const void* out,
                      size_t out_cap, const void* dest_off) {
    if (!b || !dest_off || (out_cap && !out) || (b->n_sends && (!b->sends || !b->groups)))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    if (b->reserved) return fail(e, MPX_E_INVAL, "reserved is not 0");
    CK(propose_shape(e, b->n_groups, b->n_groups * (size_t)b->ipg, b->ipg));
    if (b->n_sends >= (1ull << 32))
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 sends per call");
    if (b->n_sends && !b->n_groups) return fail(e, MPX_E_INVAL, "sends without a window");
    if (e->cfg.mode == MPX_MODE_MIN && b->n_sends && (!b->peer_commits || !b->st || !b->inst))
        return fail(e, MPX_E_INVAL, "MIN needs peer_commits, st and inst");
    return MPX_OK;
}
}  // namespace

extern "C" {

int mpx_encode_accepts_stored_reserve(mpx_engine* e, size_t max_sends, size_t max_n_inst) {
    if (!e) return MPX_E_INVAL;
    if (max_sends >= (1ull << 32) || max_n_inst > (1ull << 32))
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 sends over 2^32 instances per call");
    return reserve(e, e->ab_work, mpx::accepts_stored_work_bytes((uint32_t)e->cfg.n_replicas,
                                                                 max_sends, max_n_inst));
}

int mpx_encode_accepts_stored_dev(mpx_engine* e, const mpx_accept_store_batch* b, uint8_t* d_out,
                                  size_t out_cap, uint64_t* d_dest_off, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(accept_store_args(e, b, d_out, out_cap, d_dest_off));
    if ((((uintptr_t)b->sends | (uintptr_t)b->groups | (uintptr_t)b->st | (uintptr_t)b->lb |
          (uintptr_t)b->inst) & 15) ||
        (((uintptr_t)b->cmd_key | (uintptr_t)b->cmd_val | (uintptr_t)b->src_key |
          (uintptr_t)b->src_val | (uintptr_t)d_dest_off) & 7) ||
        ((uintptr_t)b->peer_commits & 3))
        return fail(e, MPX_E_INVAL, "mpx_encode_accepts_stored_dev: sends, groups, st, lb and inst "
                                    "must be 16-byte aligned, keys, values and d_dest_off 8, "
                                    "peer_commits 4");
    const size_t n_inst = b->n_groups * (size_t)b->ipg;
    // (an empty call uses no scratch)
    CK(reserved(e, e->ab_work,
                b->n_sends ? mpx::accepts_stored_work_bytes((uint32_t)e->cfg.n_replicas, b->n_sends,
                                                            n_inst)
                           : 0,
                "mpx_encode_accepts_stored_dev", "mpx_encode_accepts_stored_reserve(n_sends, n_inst)"));
    HIPCHK(e, mpx::launch_encode_accepts_stored(e->cfg.mode, e->cfg.n_replicas, b, d_out, out_cap,
                                                d_dest_off, e->ab_work.p, e->ab_work.cap, e->d_err,
                                                pick(e, stream)));
    return MPX_OK;
}

int mpx_encode_accepts_stored(mpx_engine* e, const mpx_accept_store_batch* b, uint8_t* out,
                              size_t out_cap, uint64_t* dest_off) {
    if (!e) return MPX_E_INVAL;
    CK(accept_store_args(e, b, out, out_cap, dest_off));
    const size_t n_inst = b->n_groups * (size_t)b->ipg;
    const bool min = e->cfg.mode == MPX_MODE_MIN;
    const int32_t N = e->cfg.n_replicas;
    const bool thrifty = (b->flags & MPX_AB_THRIFTY) != 0;
    // the sends, as mpx_encode_accepts judges them. in: a difference array over the window; its
    // running sum at slot i is the number of catch-up ranges the slot lies in
    std::vector<int64_t> in;
    if (min && b->n_sends) in.assign(n_inst + 1, 0);
    for (size_t s = 0; s < b->n_sends; ++s) {
        const mpx_accept_send& x = b->sends[s];
        if (!(x.flags & MPX_PH_ACCEPT)) continue;
        const int64_t idx = (int64_t)x.instance - b->inst_base;
        if (idx < 0 || (uint64_t)idx >= n_inst)
            return fail(e, MPX_E_INVAL, "a send names an instance outside the window");
        if (x.first_cmd > b->n_cmds || x.n_cmds > b->n_cmds - x.first_cmd ||
            (x.n_cmds && (!b->cmd_op || !b->cmd_key || !b->cmd_val)))
            return fail(e, MPX_E_INVAL, "a send's commands are outside the command arrays");
        const size_t g = (size_t)idx / b->ipg;
        const int32_t self = b->groups[g].self_id;
        if (self < 0 || self >= N) return fail(e, MPX_E_INVAL, "self_id outside [0, N)");
        if (!min) continue;
        const int64_t first = (int64_t)(g * b->ipg), lc = (int64_t)x.last_committed - b->inst_base;
        if (lc >= idx || lc < first - 1)
            return fail(e, MPX_E_INVAL, "last_committed must lie in [first_g - 1, instance)");
        const uint32_t dests = accept_dests(e->cfg.mode, N, self, thrifty, b->alive_mask);
        for (int32_t q = 0; q < N; ++q) {
            if (!((dests >> q) & 1u)) continue;
            const int64_t pc = (int64_t)b->peer_commits[g * N + q] - b->inst_base;
            const int64_t lo = pc < first ? first : pc + 1;
            if (lo <= lc) ++in[lo], --in[lc + 1];
        }
    }
    // the slots inside some range: judged, and theirs alone are the commands that are staged, as
    // a compact arena the staged slots' first_cmd is rewritten for
    size_t w_lo = 0, w_hi = 0;  // the span [w_lo, w_hi) of the window the ranges touch
    std::vector<mpx_inst_cmds> sinst;
    std::vector<uint8_t> sop;
    std::vector<int64_t> skey, sval;
    if (!in.empty()) {
        bool nil_hit = false, arena_hit = false, any = false;
        int64_t depth = 0;
        for (size_t i = 0; i < n_inst; ++i) {
            depth += in[i];
            if (!depth) continue;
            if (!any) w_lo = i;
            any = true;
            w_hi = i + 1;
            const mpx_inst_cmds& x = b->inst[i];
            if (b->st[i].status == MPX_STATUS_NIL) nil_hit = true;
            else if ((x.flags & MPX_IC_HAS_CMDS) &&
                     (x.first_cmd > (uint64_t)b->n_src || x.n_cmds > (uint64_t)b->n_src - x.first_cmd ||
                      (x.n_cmds && (!b->src_op || !b->src_key || !b->src_val))))
                arena_hit = true;
        }
        if (nil_hit)
            return fail(e, MPX_E_NIL_INSTANCE, "a nil instance inside a catch-up range");
        if (arena_hit)
            return fail(e, MPX_E_INVAL, "an instance's command range leaves [0, n_src)");
        sinst.assign(w_hi - w_lo, mpx_inst_cmds{0, 0, 0});
        depth = 0;
        for (size_t i = 0; i < w_hi; ++i) {
            depth += in[i];
            if (!depth || !(b->inst[i].flags & MPX_IC_HAS_CMDS)) continue;
            const mpx_inst_cmds& x = b->inst[i];
            sinst[i - w_lo] = mpx_inst_cmds{(uint64_t)sop.size(), x.n_cmds, x.flags};
            if (!x.n_cmds) continue;
            sop.insert(sop.end(), b->src_op + x.first_cmd, b->src_op + x.first_cmd + x.n_cmds);
            skey.insert(skey.end(), b->src_key + x.first_cmd, b->src_key + x.first_cmd + x.n_cmds);
            sval.insert(sval.end(), b->src_val + x.first_cmd, b->src_val + x.first_cmd + x.n_cmds);
        }
    }
    CK(begin(e));
    if (b->n_sends)
        GROW(e, e->ab_work, mpx::accepts_stored_work_bytes((uint32_t)N, b->n_sends, n_inst));
    Stage L(e);
    // st and inst are staged at the window's size (the scans walk it) but filled from the host
    // over the span only: the rest is nil, which no range reads (lb is read inside ranges alone)
    const size_t m = b->n_cmds, li = min && b->n_sends ? n_inst : 0, span = w_hi - w_lo,
                 sm = sop.size();
    const Slot s_snd = L.add(b->n_sends * sizeof(mpx_accept_send)),
               s_grp = L.add(b->n_sends ? b->n_groups * sizeof(mpx_proposer_group) : 0),
               s_pc = L.add(min && b->n_sends ? b->n_groups * (size_t)N * 4 : 0),
               s_op = L.add(b->cmd_op ? m : 0), s_key = L.add(b->cmd_key ? m * 8 : 0),
               s_val = L.add(b->cmd_val ? m * 8 : 0), s_st = L.add(li * sizeof(mpx_acceptor_state)),
               s_lb = L.add(b->lb ? li * sizeof(mpx_inst_state) : 0),
               s_inst = L.add(li * sizeof(mpx_inst_cmds)), s_sop = L.add(sm),
               s_skey = L.add(sm * 8), s_sval = L.add(sm * 8), s_out = L.add(out_cap),
               s_off = L.add(((size_t)N + 1) * 8);
    CK(L.commit());
    CK(L.in(s_snd, b->sends));
    CK(L.in(s_grp, b->groups));
    CK(L.in(s_pc, b->peer_commits));
    CK(L.in(s_op, b->cmd_op));
    CK(L.in(s_key, b->cmd_key));
    CK(L.in(s_val, b->cmd_val));
    if (li) {
        HIPCHK(e, hipMemsetAsync(L.at<void>(s_st), 0xFF, s_st.bytes, e->stream));
        HIPCHK(e, hipMemsetAsync(L.at<void>(s_inst), 0, s_inst.bytes, e->stream));
        CK(h2d(e, L.at<mpx_acceptor_state>(s_st) + w_lo, b->st + w_lo,
               span * sizeof(mpx_acceptor_state)));
        if (b->lb)
            CK(h2d(e, L.at<mpx_inst_state>(s_lb) + w_lo, b->lb + w_lo,
                   span * sizeof(mpx_inst_state)));
        CK(h2d(e, L.at<mpx_inst_cmds>(s_inst) + w_lo, sinst.data(), span * sizeof(mpx_inst_cmds)));
        CK(L.in(s_sop, sop.data()));
        CK(L.in(s_skey, skey.data()));
        CK(L.in(s_sval, sval.data()));
    }
    mpx_accept_store_batch d = *b;
    d.sends = L.at<mpx_accept_send>(s_snd);
    d.groups = L.at<mpx_proposer_group>(s_grp);
    d.peer_commits = L.at<int32_t>(s_pc);
    d.cmd_op = L.at<uint8_t>(s_op);
    d.cmd_key = L.at<int64_t>(s_key);
    d.cmd_val = L.at<int64_t>(s_val);
    d.st = L.at<mpx_acceptor_state>(s_st);
    d.lb = L.at<mpx_inst_state>(s_lb, b->lb);
    d.inst = L.at<mpx_inst_cmds>(s_inst);
    d.src_op = L.at<uint8_t>(s_sop);
    d.src_key = L.at<int64_t>(s_skey);
    d.src_val = L.at<int64_t>(s_sval);
    d.n_src = sm;
    CK(mpx_encode_accepts_stored_dev(e, &d, L.at<uint8_t>(s_out), out_cap, L.at<uint64_t>(s_off),
                                     e->stream));
    CK(L.out(s_off, dest_off));
    CK(finish(e));
    if (dest_off[N] > out_cap) return fail(e, MPX_E_INVAL, "out_cap is smaller than the frames");
    CK(L.out(s_out, out, dest_off[N]));
    return finish(e);
}

}  // extern "C"

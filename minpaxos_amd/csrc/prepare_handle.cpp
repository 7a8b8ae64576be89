// prepare_handle.cpp — the C ABI of the prepare side (mpx_gather_prepares, mpx_prepare_handle,
// mpx_encode_prepare_replies and their _reserve / _dev forms, include/mpx.h) over the launchers
// of prepare_handle.hip: validation, then, for the host forms, Stage staging around the _dev
// forms, like the other host-pointer entry points. A file of its own so that the units that link
// engine.cpp alone keep their set of launchers. The family's scratch is mpx_engine::pr_work.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {
inline bool is_min(const mpx_engine* e) { return e->cfg.mode == MPX_MODE_MIN; }
inline size_t reply_bytes(const mpx_engine* e) {
    return is_min(e) ? sizeof(mpx_prepare_reply_min) : sizeof(mpx_prepare_reply);
}
inline size_t value_id_at(const mpx_engine* e) {
    return is_min(e) ? offsetof(mpx_prepare_reply_min, value_id)
                     : offsetof(mpx_prepare_reply, value_id);
}

// what the two forms of the gather check alike (the CommitShort gather's list)
int gather_args(mpx_engine* e, const void* buf, size_t len, const void* other, size_t n_other,
                const void* msgs, const void* frame_index, size_t cap, const void* n_prepares) {
    if (!n_prepares || (len && !buf) || (n_other && !other) || (cap && (!msgs || !frame_index)))
        return fail(e, MPX_E_INVAL, "null argument");
    if (len > MPX_DECODE_MAX_BYTES)
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^31-1 bytes per call");
    if (n_other >= (1ull << 32))
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 frames per call");
    return MPX_OK;
}

// ... of the handler
int handle_args(mpx_engine* e, const void* msgs, size_t n, const void* st, size_t n_inst,
                const void* groups, size_t n_groups, uint32_t ipg, const void* replies,
                const void* reply_to, const void* effect, const void* log_from) {
    if (n && (!msgs || !st || !groups || !replies || !reply_to || !effect ||
              (is_min(e) && !log_from)))
        return fail(e, MPX_E_INVAL, "null argument");
    CK(propose_shape(e, n_groups, n_inst, ipg));
    if (n >= (1ull << 32)) return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 messages per call");
    if (n && !n_groups) return fail(e, MPX_E_INVAL, "messages without a window");
    return MPX_OK;
}

// ... of the encoder
int encode_args(mpx_engine* e, const mpx_prepare_reply_batch* b, const void* out, size_t out_cap,
                const void* dest_off) {
    if (!b || !dest_off || (out_cap && !out))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    if (b->reserved) return fail(e, MPX_E_INVAL, "reserved is not 0");
    if (b->n_dest < 1 || b->n_dest > MPX_MAX_REPLICAS)
        return fail(e, MPX_E_INVAL, "n_dest must lie in [1, MPX_MAX_REPLICAS]");
    if (b->n >= (1ull << 32) || b->n_inst > (1ull << 32))
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 replies over 2^32 instances per call");
    if (b->n && (!b->replies || !b->reply_to)) return fail(e, MPX_E_INVAL, "null replies");
    if (is_min(e) && b->n && (!b->log_from || (b->n_inst && (!b->st || !b->inst))))
        return fail(e, MPX_E_INVAL, "MIN needs log_from, st and inst");
    return MPX_OK;
}
}  // namespace

extern "C" {

// ---- mpx_gather_prepares ---------------------------------------------------------------------------
int mpx_gather_prepares_dev(mpx_engine* e, const uint8_t* d_buf, size_t len,
                            const mpx_peer_frame* d_other, size_t n_other,
                            const uint64_t* d_n_other, int32_t group, mpx_prepare_msg* d_msgs,
                            uint32_t* d_frame_index, size_t cap, uint64_t* d_n_prepares,
                            void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(gather_args(e, d_buf, len, d_other, n_other, d_msgs, d_frame_index, cap, d_n_prepares));
    if (((uintptr_t)d_buf | (uintptr_t)d_msgs) & 15)
        return fail(e, MPX_E_INVAL, "mpx_gather_prepares_dev: d_buf and d_msgs must be 16-byte "
                                    "aligned");
    CK(reserved(e, e->pr_work, n_other ? mpx::prepare_replies_work_bytes(1, n_other, 0) : 0,
                "mpx_gather_prepares_dev", "mpx_encode_prepare_replies_reserve(n_other, 0, 1)"));
    HIPCHK(e, mpx::launch_gather_prepares(e->cfg.mode, d_buf, len, d_other, n_other, d_n_other,
                                          group, d_msgs, d_frame_index, cap, d_n_prepares,
                                          e->pr_work.p, e->pr_work.cap, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_gather_prepares(mpx_engine* e, const uint8_t* buf, size_t len, const mpx_peer_frame* other,
                        size_t n_other, int32_t group, mpx_prepare_msg* msgs, uint32_t* frame_index,
                        size_t cap, uint64_t* n_prepares) {
    if (!e) return MPX_E_INVAL;
    CK(gather_args(e, buf, len, other, n_other, msgs, frame_index, cap, n_prepares));
    const uint64_t frame = is_min(e) ? 13 : 14;  // the code byte and the body
    uint64_t want = 0;  // the device kernel reports a frame outside the buffer and skips it
    for (size_t i = 0; i < n_other; ++i) {
        if (other[i].code != MPX_PEER_PREPARE) continue;
        if ((uint64_t)other[i].offset + frame > len)
            return fail(e, MPX_E_INVAL, "a Prepare frame lies outside [0, len)");
        ++want;
    }
    CK(begin(e));
    if (n_other) GROW(e, e->pr_work, mpx::prepare_replies_work_bytes(1, n_other, 0));
    const size_t k = std::min<uint64_t>(cap, want);
    Stage L(e);
    const Slot s_buf = L.add(len), s_oth = L.add(n_other * sizeof(mpx_peer_frame)),
               s_msg = L.add(k * sizeof(mpx_prepare_msg)), s_idx = L.add(k * 4),
               s_n = L.add(sizeof(uint64_t));
    CK(L.commit());
    CK(L.in(s_buf, buf));
    CK(L.in(s_oth, other));
    CK(mpx_gather_prepares_dev(e, L.at<uint8_t>(s_buf), len, L.at<mpx_peer_frame>(s_oth), n_other,
                               nullptr, group, L.at<mpx_prepare_msg>(s_msg),
                               L.at<uint32_t>(s_idx), k, L.at<uint64_t>(s_n), e->stream));
    CK(L.out(s_n, n_prepares));
    CK(L.out(s_msg, msgs));
    CK(L.out(s_idx, frame_index));
    return finish(e);
}

// ---- mpx_prepare_handle ----------------------------------------------------------------------------
int mpx_prepare_handle_dev(mpx_engine* e, const mpx_prepare_msg* d_msgs, size_t n,
                           const mpx_acceptor_state* d_st, size_t n_inst, int32_t inst_base,
                           mpx_proposer_group* d_groups, size_t n_groups, uint32_t ipg,
                           mpx_group_prep_state* d_gps, int32_t* d_peer_commits, void* d_replies,
                           int32_t* d_reply_to, uint8_t* d_effect, int32_t* d_log_from,
                           void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(handle_args(e, d_msgs, n, d_st, n_inst, d_groups, n_groups, ipg, d_replies, d_reply_to,
                   d_effect, d_log_from));
    if ((((uintptr_t)d_msgs | (uintptr_t)d_st | (uintptr_t)d_groups | (uintptr_t)d_gps) & 15) ||
        ((uintptr_t)d_replies & (is_min(e) ? 7 : 15)) ||
        (((uintptr_t)d_peer_commits | (uintptr_t)d_reply_to | (uintptr_t)d_log_from) & 3))
        return fail(e, MPX_E_INVAL, "mpx_prepare_handle_dev: d_msgs, d_st, d_groups and d_gps must "
                                    "be 16-byte aligned, d_replies 8 (MIN) or 16 (CLASSIC), "
                                    "d_peer_commits, d_reply_to and d_log_from 4");
    HIPCHK(e, mpx::launch_prepare_handle(e->cfg.mode, d_msgs, n, d_st, n_inst, inst_base, d_groups,
                                         n_groups, ipg, e->cfg.n_replicas, d_gps, d_peer_commits,
                                         d_replies, d_reply_to, d_effect, d_log_from, e->d_err,
                                         pick(e, stream)));
    return MPX_OK;
}

int mpx_prepare_handle(mpx_engine* e, const mpx_prepare_msg* msgs, size_t n,
                       const mpx_acceptor_state* st, size_t n_inst, int32_t inst_base,
                       mpx_proposer_group* groups, size_t n_groups, uint32_t ipg,
                       mpx_group_prep_state* gps, int32_t* peer_commits, void* replies,
                       int32_t* reply_to, uint8_t* effect, int32_t* log_from) {
    if (!e) return MPX_E_INVAL;
    CK(handle_args(e, msgs, n, st, n_inst, groups, n_groups, ipg, replies, reply_to, effect,
                   log_from));
    if (!n) return MPX_OK;
    const bool min = is_min(e);
    const int32_t N = e->cfg.n_replicas;
    // the batch's own faults, before anything is staged, and the groups [g_lo, g_hi] it touches
    size_t g_lo = n_groups, g_hi = 0;
    for (size_t i = 0; i < n; ++i) {
        if (i && msgs[i - 1].key > msgs[i].key)
            return fail(e, MPX_E_INVAL, "messages are not grouped in ascending key order");
        size_t g;
        if (min) {
            if (msgs[i].key < 0 || (uint64_t)msgs[i].key >= n_groups)
                return fail(e, MPX_E_INVAL, "a message's group lies outside [0, n_groups)");
            g = (size_t)msgs[i].key;
        } else {
            const int64_t idx = (int64_t)msgs[i].key - inst_base;
            if (idx < 0 || (uint64_t)idx >= n_inst)
                return fail(e, MPX_E_NIL_INSTANCE, "a message names an instance outside the window");
            g = (size_t)idx / ipg;
        }
        if (msgs[i].leader_id < 0 || msgs[i].leader_id >= N)
            return fail(e, MPX_E_BAD_ID, "leader_id outside [0, N)");
        g_lo = std::min(g_lo, g);
        g_hi = std::max(g_hi, g);
    }
    // only those groups and their span of the window are staged: the device form runs on the
    // window [g_lo, g_hi], so MIN's keys and the replies' value_id move by the span's start
    const size_t ng = g_hi - g_lo + 1, w_lo = g_lo * (size_t)ipg, span = ng * (size_t)ipg;
    std::vector<mpx_prepare_msg> moved;
    if (min && g_lo) {
        moved.assign(msgs, msgs + n);
        for (mpx_prepare_msg& m : moved) m.key -= (int32_t)g_lo;
    }
    CK(begin(e));
    Stage L(e);
    const size_t rb = reply_bytes(e);
    const Slot s_msg = L.add(n * sizeof(mpx_prepare_msg)),
               s_st = L.add(span * sizeof(mpx_acceptor_state)),
               s_grp = L.add(ng * sizeof(mpx_proposer_group)),
               s_gps = L.add(min && gps ? ng * sizeof(mpx_group_prep_state) : 0),
               s_pc = L.add(min && peer_commits ? ng * (size_t)N * 4 : 0), s_rep = L.add(n * rb),
               s_to = L.add(n * 4), s_eff = L.add(n), s_lf = L.add(min ? n * 4 : 0);
    CK(L.commit());
    CK(L.in(s_msg, moved.empty() ? msgs : moved.data()));
    CK(L.in(s_st, st + w_lo));
    CK(L.in(s_grp, groups + g_lo));
    if (s_gps.bytes) CK(L.in(s_gps, gps + g_lo));
    if (s_pc.bytes) CK(L.in(s_pc, peer_commits + g_lo * (size_t)N));
    CK(mpx_prepare_handle_dev(
        e, L.at<mpx_prepare_msg>(s_msg), n, L.at<mpx_acceptor_state>(s_st), span,
        (int32_t)(inst_base + (int64_t)w_lo), L.at<mpx_proposer_group>(s_grp), ng, ipg,
        s_gps.bytes ? L.at<mpx_group_prep_state>(s_gps) : nullptr,
        s_pc.bytes ? L.at<int32_t>(s_pc) : nullptr, L.at<void>(s_rep), L.at<int32_t>(s_to),
        L.at<uint8_t>(s_eff), min ? L.at<int32_t>(s_lf) : nullptr, e->stream));
    CK(L.out(s_grp, groups + g_lo));
    if (s_gps.bytes) CK(L.out(s_gps, gps + g_lo));
    if (s_pc.bytes) CK(L.out(s_pc, peer_commits + g_lo * (size_t)N));
    CK(L.out(s_rep, replies));
    CK(L.out(s_to, reply_to));
    CK(L.out(s_eff, effect));
    if (min) CK(L.out(s_lf, log_from));
    const int rc = finish(e);
    if (w_lo) {  // value_id back to the caller's window
        uint8_t* p = (uint8_t*)replies + value_id_at(e);
        for (size_t i = 0; i < n; ++i, p += rb) {
            uint32_t v;
            memcpy(&v, p, 4);
            if (v == MPX_VALUE_KEEP) continue;
            v += (uint32_t)w_lo;
            memcpy(p, &v, 4);
        }
    }
    return rc;
}

// ---- mpx_encode_prepare_replies --------------------------------------------------------------------
int mpx_encode_prepare_replies_reserve(mpx_engine* e, size_t max_n, size_t max_n_inst,
                                       uint32_t n_dest) {
    if (!e) return MPX_E_INVAL;
    if (n_dest < 1 || n_dest > MPX_MAX_REPLICAS)
        return fail(e, MPX_E_INVAL, "n_dest must lie in [1, MPX_MAX_REPLICAS]");
    if (max_n >= (1ull << 32) || max_n_inst > (1ull << 32))
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 replies over 2^32 instances per call");
    return reserve(e, e->pr_work, mpx::prepare_replies_work_bytes(n_dest, max_n, max_n_inst));
}

int mpx_encode_prepare_replies_dev(mpx_engine* e, const mpx_prepare_reply_batch* b, uint8_t* d_out,
                                   size_t out_cap, uint64_t* d_dest_off, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(encode_args(e, b, d_out, out_cap, d_dest_off));
    if ((((uintptr_t)b->st | (uintptr_t)b->lb | (uintptr_t)b->inst) & 15) ||
        ((uintptr_t)b->replies & (is_min(e) ? 7 : 15)) ||
        (((uintptr_t)b->src_key | (uintptr_t)b->src_val | (uintptr_t)d_dest_off) & 7) ||
        (((uintptr_t)b->reply_to | (uintptr_t)b->log_from) & 3))
        return fail(e, MPX_E_INVAL, "mpx_encode_prepare_replies_dev: st, lb and inst must be "
                                    "16-byte aligned, replies 8 (MIN) or 16 (CLASSIC), keys, values "
                                    "and d_dest_off 8, reply_to and log_from 4");
    // (an empty call uses no scratch)
    CK(reserved(e, e->pr_work,
                b->n ? mpx::prepare_replies_work_bytes(b->n_dest, b->n, b->n_inst) : 0,
                "mpx_encode_prepare_replies_dev",
                "mpx_encode_prepare_replies_reserve(n, n_inst, n_dest)"));
    HIPCHK(e, mpx::launch_encode_prepare_replies(e->cfg.mode, b, d_out, out_cap, d_dest_off,
                                                 e->pr_work.p, e->pr_work.cap, e->d_err,
                                                 pick(e, stream)));
    return MPX_OK;
}

int mpx_encode_prepare_replies(mpx_engine* e, const mpx_prepare_reply_batch* b, uint8_t* out,
                               size_t out_cap, uint64_t* dest_off) {
    if (!e) return MPX_E_INVAL;
    CK(encode_args(e, b, out, out_cap, dest_off));
    const bool min = is_min(e);
    const size_t rb = reply_bytes(e), vat = value_id_at(e), n_inst = b->n_inst;
    const uint8_t* reps = (const uint8_t*)b->replies;
    // the slots the frames read: ref bit 0 inside some log range (judged nil), bit 1 a Command
    std::vector<int64_t> in;   // a difference array over the window for the ranges
    std::vector<uint8_t> ref;
    if (b->n) in.assign(n_inst + 1, 0), ref.assign(n_inst, 0);
    for (size_t i = 0; i < b->n; ++i) {
        const int32_t to = b->reply_to[i];
        if (to < 0) continue;
        if ((uint32_t)to >= b->n_dest) return fail(e, MPX_E_INVAL, "reply_to outside [0, n_dest)");
        uint32_t vid;
        memcpy(&vid, reps + i * rb + vat, 4);
        if (vid != MPX_VALUE_KEEP) {
            if (vid >= n_inst || !b->inst)
                return fail(e, MPX_E_INVAL, "a value_id outside [0, n_inst)");
            ref[vid] |= 2;
        }
        if (!min) continue;
        mpx_prepare_reply_min r;
        memcpy(&r, reps + i * rb, sizeof(r));
        const int64_t lf = (int64_t)b->log_from[i] - b->inst_base,
                      lc = (int64_t)r.last_committed - b->inst_base;
        if (lf > lc) continue;
        if (lf < 0 || (uint64_t)lc >= n_inst)
            return fail(e, MPX_E_INVAL, "a log range leaves the window");
        ++in[lf], --in[lc + 1];
    }
    // judged, and theirs alone are the commands that are staged, as a compact arena the staged
    // slots' first_cmd is rewritten for
    size_t w_lo = 0, w_hi = 0;  // the span [w_lo, w_hi) of the window the frames touch
    std::vector<mpx_inst_cmds> sinst;
    std::vector<uint8_t> sop;
    std::vector<int64_t> skey, sval;
    {
        bool nil_hit = false, arena_hit = false, any = false;
        int64_t depth = 0;
        for (size_t i = 0; i < ref.size(); ++i) {
            depth += in[i];
            if (depth) ref[i] |= 1;
            if (!ref[i]) continue;
            if (!any) w_lo = i;
            any = true;
            w_hi = i + 1;
            const mpx_inst_cmds& x = b->inst[i];
            if ((ref[i] & 1) && b->st[i].status == MPX_STATUS_NIL) nil_hit = true;
            else if ((x.flags & MPX_IC_HAS_CMDS) &&
                     (x.first_cmd > (uint64_t)b->n_src || x.n_cmds > (uint64_t)b->n_src - x.first_cmd ||
                      (x.n_cmds && (!b->src_op || !b->src_key || !b->src_val))))
                arena_hit = true;
        }
        if (nil_hit) return fail(e, MPX_E_NIL_INSTANCE, "a nil instance inside a log range");
        if (arena_hit)
            return fail(e, MPX_E_INVAL, "an instance's command range leaves [0, n_src)");
        sinst.assign(w_hi - w_lo, mpx_inst_cmds{0, 0, 0});
        for (size_t i = w_lo; i < w_hi; ++i) {
            if (!ref[i] || !(b->inst[i].flags & MPX_IC_HAS_CMDS)) continue;
            const mpx_inst_cmds& x = b->inst[i];
            sinst[i - w_lo] = mpx_inst_cmds{(uint64_t)sop.size(), x.n_cmds, x.flags};
            if (!x.n_cmds) continue;
            sop.insert(sop.end(), b->src_op + x.first_cmd, b->src_op + x.first_cmd + x.n_cmds);
            skey.insert(skey.end(), b->src_key + x.first_cmd, b->src_key + x.first_cmd + x.n_cmds);
            sval.insert(sval.end(), b->src_val + x.first_cmd, b->src_val + x.first_cmd + x.n_cmds);
        }
    }
    // the device form runs on the window [w_lo, w_hi): the replies' value_id moves by its start
    // (instance numbers stay: inst_base moves with it)
    const size_t span = w_hi - w_lo, sm = sop.size();
    std::vector<uint8_t> moved;
    if (w_lo) {
        moved.assign(reps, reps + b->n * rb);
        for (size_t i = 0; i < b->n; ++i) {
            uint32_t vid;
            memcpy(&vid, &moved[i * rb + vat], 4);
            if (vid == MPX_VALUE_KEEP) continue;
            // (a skipped reply's value_id was not judged: it may lie anywhere and is not read)
            vid -= (uint32_t)w_lo;
            memcpy(&moved[i * rb + vat], &vid, 4);
        }
    }
    CK(begin(e));
    if (b->n) GROW(e, e->pr_work, mpx::prepare_replies_work_bytes(b->n_dest, b->n, span));
    Stage L(e);
    const bool with_st = min && span;
    const Slot s_rep = L.add(b->n * rb), s_to = L.add(b->n * 4), s_lf = L.add(min ? b->n * 4 : 0),
               s_st = L.add(with_st ? span * sizeof(mpx_acceptor_state) : 0),
               s_lb = L.add(with_st && b->lb ? span * sizeof(mpx_inst_state) : 0),
               s_inst = L.add(span * sizeof(mpx_inst_cmds)), s_sop = L.add(sm),
               s_skey = L.add(sm * 8), s_sval = L.add(sm * 8), s_out = L.add(out_cap),
               s_off = L.add(((size_t)b->n_dest + 1) * 8);
    CK(L.commit());
    CK(L.in(s_rep, moved.empty() ? reps : moved.data()));
    CK(L.in(s_to, b->reply_to));
    CK(L.in(s_lf, b->log_from));
    if (s_st.bytes) CK(L.in(s_st, b->st + w_lo));
    if (s_lb.bytes) CK(L.in(s_lb, b->lb + w_lo));
    CK(L.in(s_inst, sinst.data()));
    CK(L.in(s_sop, sop.data()));
    CK(L.in(s_skey, skey.data()));
    CK(L.in(s_sval, sval.data()));
    mpx_prepare_reply_batch d = *b;
    d.replies = L.at<void>(s_rep);
    d.reply_to = L.at<int32_t>(s_to);
    d.log_from = min ? L.at<int32_t>(s_lf) : nullptr;
    d.inst_base = (int32_t)(b->inst_base + (int64_t)w_lo);
    d.n_inst = span;
    d.st = s_st.bytes ? L.at<mpx_acceptor_state>(s_st) : nullptr;
    d.lb = s_lb.bytes ? L.at<mpx_inst_state>(s_lb) : nullptr;
    d.inst = L.at<mpx_inst_cmds>(s_inst);
    d.src_op = L.at<uint8_t>(s_sop);
    d.src_key = L.at<int64_t>(s_skey);
    d.src_val = L.at<int64_t>(s_sval);
    d.n_src = sm;
    CK(mpx_encode_prepare_replies_dev(e, &d, L.at<uint8_t>(s_out), out_cap, L.at<uint64_t>(s_off),
                                      e->stream));
    CK(L.out(s_off, dest_off));
    CK(finish(e));
    if (dest_off[b->n_dest] > out_cap)
        return fail(e, MPX_E_INVAL, "out_cap is smaller than the frames");
    CK(L.out(s_out, out, dest_off[b->n_dest]));
    return finish(e);
}

}  // extern "C"

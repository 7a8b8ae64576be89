// record.cpp — the C ABI of record assembly (mpx_record_log[_reserve|_dev], mpx_record_bound,
// include/mpx.h) over the launcher of record.hip: validation, then, for the host form, Stage staging
// around the _dev form, like the other host-pointer entry points (engine.cpp, order.cpp, client.cpp,
// replies.cpp, execute.cpp, store.cpp). The command sources' checks, the pre-check of an item's
// commands and their staging are cmd_src_host.hpp's, shared with store.cpp.
#include <algorithm>
#include <cstdint>
#include <string>

#include "cmd_src_host.hpp"
#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {

bool msgs(const mpx_record_batch* b) { return b->kind == MPX_LR_ACCEPTS || b->kind == MPX_LR_COMMITS; }
size_t item_bytes(const mpx_record_batch* b) {
    return msgs(b) ? sizeof(mpx_accept_msg) : sizeof(mpx_accept_send);
}
// the sources the call reads (MPX_LR_DECIDED: none)
size_t n_src(const mpx_record_batch* b) { return b->kind == MPX_LR_DECIDED ? 0 : b->n_src; }

// what both forms check
int record_args(mpx_engine* e, const mpx_record_batch* b, const uint8_t* out, size_t out_cap,
                const void* res) {
    if (!b || !res || (out_cap && !out)) return fail(e, MPX_E_INVAL, "null argument");
    if (b->kind > MPX_LR_DECIDED) return fail(e, MPX_E_INVAL, "unknown kind");
    if (b->format != MPX_LOG_DURABLE && b->format != MPX_LOG_DURABLE_CLASSIC)
        return fail(e, MPX_E_INVAL, "unknown format");
    if (b->flags & ~MPX_LR_GENERAL) return fail(e, MPX_E_INVAL, "unknown flags");
    if (b->reserved) return fail(e, MPX_E_INVAL, "reserved is not 0");
    if (b->kind == MPX_LR_ACCEPTS && b->format == MPX_LOG_DURABLE_CLASSIC)
        return fail(e, MPX_E_UNSUPPORTED, "MPX_LR_ACCEPTS has no MPX_LOG_DURABLE_CLASSIC form: CLASSIC's "
                                          "handleAccept records a status the batch does not carry");
    if (b->kind == MPX_LR_DECIDED) {
        if (b->n_src > MPX_SC_MAX_SRC) return fail(e, MPX_E_INVAL, "n_src above MPX_SC_MAX_SRC");
    } else if (!b->src || b->n_src < 1 || b->n_src > MPX_SC_MAX_SRC ||
               (b->kind == MPX_LR_SENDS && b->n_src != 1)) {
        return fail(e, MPX_E_INVAL, "n_src outside [1, MPX_SC_MAX_SRC] (MPX_LR_SENDS: 1)");
    }
    if ((uint64_t)b->n >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 items or more");
    if (b->n && (!b->items || (msgs(b) && !b->effect) ||
                 (b->kind == MPX_LR_DECIDED && b->n_inst && !b->mask)))
        return fail(e, MPX_E_INVAL, "null argument");
    if (msgs(b) && b->n_src > 1 && !b->perm) return fail(e, MPX_E_INVAL, "more than one source needs perm");
    uint64_t recs;
    CK(src_args(e, b->src, n_src(b), &recs));
    if (b->kind != MPX_LR_DECIDED && recs < b->n)
        return fail(e, MPX_E_INVAL, "the sources hold fewer records than n");
    return MPX_OK;
}

}  // namespace

extern "C" {

size_t mpx_record_bound(size_t n, size_t m) { return 12 * n + 17 * m; }

int mpx_record_log_reserve(mpx_engine* e, size_t max_n) {
    if (!e) return MPX_E_INVAL;
    if ((uint64_t)max_n >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 items or more");
    return reserve(e, e->lr_work, mpx::record_work_bytes(max_n));
}

int mpx_record_log_dev(mpx_engine* e, const mpx_record_batch* b, uint8_t* d_out, size_t out_cap,
                       uint64_t* d_item_off, mpx_record_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(record_args(e, b, d_out, out_cap, d_res));
    uintptr_t a8 = (uintptr_t)d_res | (uintptr_t)b->d_n | (uintptr_t)d_item_off;
    for (size_t s = 0; s < n_src(b); ++s)
        a8 |= (uintptr_t)b->src[s].cmd_off | (uintptr_t)b->src[s].key | (uintptr_t)b->src[s].val;
    if (((uintptr_t)b->items & 15) || (a8 & 7) || ((uintptr_t)b->perm & 3))
        return fail(e, MPX_E_INVAL, "mpx_record_log_dev: items must be 16-byte aligned, the 8-byte "
                                    "arrays, d_item_off, d_n and d_res 8, perm 4");
    CK(reserved(e, e->lr_work, b->n ? mpx::record_work_bytes(b->n) : 0, "mpx_record_log_dev",
                "mpx_record_log_reserve(max_n)"));
    HIPCHK(e, mpx::launch_record_log(b, d_out, out_cap, d_item_off, d_res, e->lr_work.p, e->lr_work.cap,
                                     e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_record_log(mpx_engine* e, const mpx_record_batch* b, uint8_t* out, size_t out_cap,
                   uint64_t* item_off, mpx_record_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(record_args(e, b, out, out_cap, res));
    if (b->d_n) return fail(e, MPX_E_INVAL, "d_n is for mpx_record_log_dev");
    // the device kernels report these through the error word; here they answer before any launch:
    // the recording items, judged in array order as the kernels judge each
    const size_t ns = n_src(b);
    const SrcIndex idx(b->src, ns);
    if (msgs(b)) CK(perm_args(e, idx, b->perm, b->n));
    const uint64_t hdr = b->format == MPX_LOG_DURABLE ? 12 : 5;
    bool any = false;
    uint64_t total = 0, rel_lo = 0, rel_hi = 0;
    for (size_t i = 0; i < b->n; ++i) {
        uint64_t len = 0;
        if (msgs(b)) {
            const mpx_accept_msg& m = ((const mpx_accept_msg*)b->items)[i];
            bool cmds = true;
            if (b->kind == MPX_LR_ACCEPTS) {
                if (!(b->effect[i] & MPX_AH_STORED)) continue;
            } else {
                cmds = (b->effect[i] & MPX_CH_CMDS) && m.value_id != MPX_VALUE_KEEP;
            }
            if (cmds) CK(resolve_msg(e, idx, b->perm ? b->perm[i] : i, m.value_id, "recording", &len));
        } else {
            const mpx_accept_send& x = ((const mpx_accept_send*)b->items)[i];
            if (!(x.flags & MPX_PH_ACCEPT)) continue;
            if (b->kind == MPX_LR_SENDS) {
                CK(resolve_send(e, b->src[0], x, "recording", &len));
            } else {
                const int64_t rel = (int64_t)x.instance - b->inst_base;
                if (rel < 0 || (uint64_t)rel >= b->n_inst)
                    return fail(e, MPX_E_NIL_INSTANCE, "an accepted slot names an instance outside the window");
                rel_lo = any ? std::min<uint64_t>(rel_lo, rel) : (uint64_t)rel;
                rel_hi = any ? std::max<uint64_t>(rel_hi, rel) : (uint64_t)rel;
                any = true;
                if (!b->mask[rel]) continue;
            }
        }
        total += hdr + 17 * len;
        if (total >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 bytes or more");
    }
    CK(begin(e));
    if (b->n) GROW(e, e->lr_work, mpx::record_work_bytes(b->n));
    const bool fits = total <= out_cap;
    // only what the call reads and writes is staged: the run, and the span of mask between the
    // first and the last accepted slot (the kernels index it from the window's start)
    const size_t n_out = fits ? (size_t)total : 0, n_span = any ? (size_t)(rel_hi - rel_lo + 1) : 0;
    Stage L(e);
    const Slot s_items = L.add(b->n * item_bytes(b)), s_eff = L.add(msgs(b) ? b->n : 0),
               s_perm = L.add(b->perm && msgs(b) ? b->n * sizeof(uint32_t) : 0), s_mask = L.add(n_span),
               s_out = L.add(n_out), s_ioff = L.add(item_off ? (b->n + 1) * sizeof(uint64_t) : 0),
               s_res = L.add(sizeof(mpx_record_result));
    StagedSrcs srcs(L, b->src, ns);
    CK(L.commit());
    CK(L.in(s_items, b->items));
    if (msgs(b)) CK(L.in(s_eff, b->effect));
    if (b->perm && msgs(b)) CK(L.in(s_perm, b->perm));
    if (n_span) CK(L.in(s_mask, b->mask + rel_lo));
    CK(srcs.in());
    mpx_record_batch d = *b;
    d.items = L.at<char>(s_items, b->n ? b->items : nullptr);
    d.effect = msgs(b) ? L.at<uint8_t>(s_eff, b->effect) : nullptr;
    d.perm = msgs(b) ? L.at<uint32_t>(s_perm, b->perm) : nullptr;
    d.mask = n_span ? L.at<uint8_t>(s_mask) - rel_lo : b->mask;  // (no accepted slot: not read)
    d.src = srcs.dev(), d.n_src = ns;
    // (a run that does not fit writes nothing: the device form gets the caller's capacity and an
    // empty slot)
    CK(mpx_record_log_dev(e, &d, L.at<uint8_t>(s_out), out_cap, L.at<uint64_t>(s_ioff, item_off),
                          L.at<mpx_record_result>(s_res), e->stream));
    if (fits) CK(L.out(s_out, out));
    if (item_off) CK(L.out(s_ioff, item_off));
    CK(L.out(s_res, res));
    return finish(e);
}

}  // extern "C"

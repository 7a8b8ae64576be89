// order.cpp — the C ABI of batch assembly (mpx_order_records[_reserve|_dev], include/mpx.h) over
// the launcher of order.hip: validation, then, for the host form, Stage staging around the _dev
// form, like the other host-pointer entry points (engine.cpp).
#include <cstdint>
#include <cstring>
#include <string>

#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {

// the family's scratch holds its control words first: zero when allocated, zero after every call
int ord_grow(mpx_engine* e, uint64_t bytes) {
    if (bytes <= e->ord_work.cap) return MPX_OK;
    GROW(e, e->ord_work, bytes);
    HIPCHK(e, hipMemsetAsync(e->ord_work.p, 0, mpx::kOrderCtlBytes, e->stream));
    return MPX_OK;
}

// what both forms check; *total = the records of the call, *keyed = it gives arrival keys
int order_args(mpx_engine* e, const mpx_order_src* src, size_t n_src, size_t n_inst,
               int32_t inst_base, uint32_t arrival_bits, uint32_t flags, const void* out,
               const void* res, uint64_t* total, bool* keyed) {
    if (!res || (n_src && !src)) return fail(e, MPX_E_INVAL, "null argument");
    if (n_src > MPX_ORDER_MAX_SRC)
        return fail(e, MPX_E_INVAL, "more than MPX_ORDER_MAX_SRC sources");
    if (flags & ~MPX_ORDER_GENERAL) return fail(e, MPX_E_INVAL, "unknown flags");
    if (!n_inst || (uint64_t)n_inst > (1ull << 32) ||
        (int64_t)inst_base + (int64_t)(n_inst - 1) > INT32_MAX)
        return fail(e, MPX_E_INVAL, "the window [inst_base, inst_base + n_inst) is not int32");
    if (arrival_bits > 32) return fail(e, MPX_E_INVAL, "arrival_bits above 32");
    uint64_t n = 0;
    size_t with = 0, without = 0;
    for (size_t s = 0; s < n_src; ++s) {
        if (!src[s].n) continue;
        if (!src[s].recs) return fail(e, MPX_E_INVAL, "a source with records has no recs");
        if (src[s].n >= 0xFFFFFFFFull || (n += src[s].n) >= 0xFFFFFFFFull)
            return fail(e, MPX_E_UNSUPPORTED, "2^32-1 records or more");
        ++(src[s].arrival ? with : without);
    }
    if (with && without)
        return fail(e, MPX_E_INVAL, "arrival keys given for some sources and not for others");
    if (arrival_bits && !with && n)
        return fail(e, MPX_E_INVAL, "arrival_bits set without arrival keys");
    if (with && !arrival_bits)
        return fail(e, MPX_E_INVAL, "arrival keys given with arrival_bits == 0");
    if (n && !out) return fail(e, MPX_E_INVAL, "null argument");
    *total = n;
    *keyed = with != 0;
    return MPX_OK;
}

}  // namespace

extern "C" {

int mpx_order_records_reserve(mpx_engine* e, size_t max_n, size_t max_n_inst) {
    if (!e) return MPX_E_INVAL;
    if ((uint64_t)max_n >= 0xFFFFFFFFull)
        return fail(e, MPX_E_UNSUPPORTED, "2^32-1 records or more");
    if ((uint64_t)max_n_inst > (1ull << 32))
        return fail(e, MPX_E_INVAL, "a window of more than 2^32 instances");
    // (any arrival_bits: the 64-bit keys' carve-up, which holds the 32-bit one)
    CK(begin(e));
    CK(ord_grow(e, mpx::order_work_bytes(max_n, true)));
    return finish(e);
}

int mpx_order_records_dev(mpx_engine* e, const mpx_order_src* src, size_t n_src, size_t n_inst,
                          int32_t inst_base, uint32_t arrival_bits, uint32_t flags, void* d_out,
                          uint32_t* d_perm, mpx_order_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    uint64_t n = 0;
    bool keyed = false;
    CK(order_args(e, src, n_src, n_inst, inst_base, arrival_bits, flags, d_out, d_res, &n, &keyed));
    bool aligned = !((uintptr_t)d_out & 15) && !((uintptr_t)d_perm & 3) && !((uintptr_t)d_res & 7);
    for (size_t s = 0; s < n_src; ++s)
        if (src[s].n && (((uintptr_t)src[s].recs & 15) || ((uintptr_t)src[s].arrival & 3)))
            aligned = false;
    if (!aligned)
        return fail(e, MPX_E_INVAL, "mpx_order_records_dev: recs and d_out must be 16-byte aligned, "
                                    "d_perm and arrival 4, d_res 8");
    const bool wide = mpx::order_key_bits(n_inst, arrival_bits) > 32;
    // (a call of no record uses no scratch)
    CK(reserved(e, e->ord_work, n ? mpx::order_work_bytes(n, wide) : 0, "mpx_order_records_dev",
                "mpx_order_records_reserve(n, n_inst)"));
    HIPCHK(e, mpx::launch_order_records(src, (uint32_t)n_src, n_inst, inst_base, arrival_bits,
                                        (flags & MPX_ORDER_GENERAL) != 0, d_out, d_perm, d_res,
                                        e->ord_work.p, e->ord_work.cap, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_order_records(mpx_engine* e, const mpx_order_src* src, size_t n_src, size_t n_inst,
                      int32_t inst_base, uint32_t arrival_bits, uint32_t flags, void* out,
                      uint32_t* perm, mpx_order_result* res) {
    if (!e) return MPX_E_INVAL;
    uint64_t n = 0;
    bool keyed = false;
    CK(order_args(e, src, n_src, n_inst, inst_base, arrival_bits, flags, out, res, &n, &keyed));
    // the device kernels mask the keys and report the window through the error word; here both
    // answer before any launch
    for (size_t s = 0; s < n_src; ++s)
        for (size_t i = 0; i < src[s].n; ++i) {
            int32_t inst;
            memcpy(&inst, (const char*)src[s].recs + 16 * i, sizeof(inst));
            const int64_t rel = (int64_t)inst - inst_base;
            if (rel < 0 || (uint64_t)rel >= (uint64_t)n_inst)
                return fail(e, MPX_E_NIL_INSTANCE, "a record names an instance outside the window");
            if (keyed && arrival_bits < 32 && (src[s].arrival[i] >> arrival_bits))
                return fail(e, MPX_E_INVAL, "an arrival key has bits at or above arrival_bits");
        }
    CK(begin(e));
    if (n) CK(ord_grow(e, mpx::order_work_bytes(n, mpx::order_key_bits(n_inst, arrival_bits) > 32)));
    Stage L(e);
    Slot s_rec[MPX_ORDER_MAX_SRC], s_arr[MPX_ORDER_MAX_SRC];
    for (size_t s = 0; s < n_src; ++s) {
        s_rec[s] = L.add(src[s].n * 16);
        s_arr[s] = L.add(keyed ? src[s].n * sizeof(uint32_t) : 0);
    }
    const Slot s_out = L.add(n * 16), s_perm = L.add(perm ? n * sizeof(uint32_t) : 0),
               s_res = L.add(sizeof(mpx_order_result));
    CK(L.commit());
    mpx_order_src d[MPX_ORDER_MAX_SRC];
    for (size_t s = 0; s < n_src; ++s) {
        CK(L.in(s_rec[s], src[s].recs));
        if (keyed && src[s].n) CK(L.in(s_arr[s], src[s].arrival));
        d[s].recs = L.at<char>(s_rec[s]);
        d[s].arrival = L.at<uint32_t>(s_arr[s], keyed && src[s].n ? src[s].arrival : nullptr);
        d[s].n = src[s].n;
    }
    CK(mpx_order_records_dev(e, d, n_src, n_inst, inst_base, arrival_bits, flags,
                             L.at<char>(s_out), L.at<uint32_t>(s_perm, perm),
                             L.at<mpx_order_result>(s_res), e->stream));
    CK(L.out(s_out, out));
    if (perm) CK(L.out(s_perm, perm));
    CK(L.out(s_res, res));
    return finish(e);
}

}  // extern "C"

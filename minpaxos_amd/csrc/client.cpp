// client.cpp — the C ABI of the client side (mpx_decode_client_streams[_reserve|_dev],
// include/mpx.h) over the launcher of client.hip: validation, then, for the host form, Stage
// staging around the _dev form, like the other host-pointer entry points (engine.cpp, order.cpp).
#include <algorithm>
#include <cstdint>
#include <string>

#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {

// what both forms check
int client_args(mpx_engine* e, const void* buf, size_t len, const void* conns, size_t n_conns,
                size_t n_groups, const mpx_client_out* out, const void* conn_res, const void* res) {
    if (!out || !res || (len && !buf) || (n_conns && (!conns || !conn_res)))
        return fail(e, MPX_E_INVAL, "null argument");
    if (out->prop_cap && (!out->op || !out->key || !out->val || !out->meta))
        return fail(e, MPX_E_INVAL, "prop_cap > 0 with a null output array");
    if (!n_groups && (out->prop_off || out->send_off))
        return fail(e, MPX_E_INVAL, "prop_off / send_off given with n_groups == 0");
    if ((uint64_t)len > (uint64_t)MPX_DECODE_MAX_BYTES)
        return fail(e, MPX_E_UNSUPPORTED, "more than MPX_DECODE_MAX_BYTES bytes");
    if ((uint64_t)n_conns > MPX_CLIENT_MAX_CONNS)
        return fail(e, MPX_E_UNSUPPORTED, "more than MPX_CLIENT_MAX_CONNS connections");
    if ((uint64_t)n_groups > MPX_CLIENT_MAX_GROUPS)
        return fail(e, MPX_E_UNSUPPORTED, "more than MPX_CLIENT_MAX_GROUPS groups");
    return MPX_OK;
}

// no more proposals than this can come out of len bytes: what the host form stages
size_t staged_cap(const mpx_client_out* out, size_t len) {
    return std::min(out->prop_cap, len / MPX_CLIENT_PROPOSE_FRAME);
}

}  // namespace

extern "C" {

int mpx_decode_client_streams_reserve(mpx_engine* e, size_t max_len, size_t max_conns,
                                      size_t max_groups) {
    if (!e) return MPX_E_INVAL;
    if ((uint64_t)max_len > (uint64_t)MPX_DECODE_MAX_BYTES)
        return fail(e, MPX_E_UNSUPPORTED, "more than MPX_DECODE_MAX_BYTES bytes");
    if ((uint64_t)max_conns > MPX_CLIENT_MAX_CONNS)
        return fail(e, MPX_E_UNSUPPORTED, "more than MPX_CLIENT_MAX_CONNS connections");
    if ((uint64_t)max_groups > MPX_CLIENT_MAX_GROUPS)
        return fail(e, MPX_E_UNSUPPORTED, "more than MPX_CLIENT_MAX_GROUPS groups");
    return reserve(e, e->cl_work, mpx::client_work_bytes(max_len, max_conns, max_groups));
}

int mpx_decode_client_streams_dev(mpx_engine* e, const uint8_t* d_buf, size_t len,
                                  const mpx_client_conn* d_conns, size_t n_conns, size_t n_groups,
                                  const mpx_client_out* out, mpx_client_conn_result* d_conn_res,
                                  mpx_client_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(client_args(e, d_buf, len, d_conns, n_conns, n_groups, out, d_conn_res, d_res));
    if (((uintptr_t)d_buf & 15) || ((uintptr_t)d_conns & 15) || ((uintptr_t)out->meta & 15) ||
        ((uintptr_t)d_conn_res & 15) || ((uintptr_t)out->key & 7) || ((uintptr_t)out->val & 7) ||
        ((uintptr_t)out->prop_off & 7) || ((uintptr_t)out->send_off & 7) || ((uintptr_t)d_res & 7))
        return fail(e, MPX_E_INVAL, "mpx_decode_client_streams_dev: d_buf, d_conns, meta and "
                                    "d_conn_res must be 16-byte aligned, keys, values, offsets "
                                    "and d_res 8");
    // (a call of no connection uses no scratch)
    CK(reserved(e, e->cl_work, n_conns ? mpx::client_work_bytes(len, n_conns, n_groups) : 0,
                "mpx_decode_client_streams_dev",
                "mpx_decode_client_streams_reserve(max_len, max_conns, max_groups)"));
    HIPCHK(e, mpx::launch_decode_client_streams(d_buf, len, d_conns, n_conns, n_groups, out,
                                                d_conn_res, d_res, e->cl_work.p, e->cl_work.cap,
                                                e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_decode_client_streams(mpx_engine* e, const uint8_t* buf, size_t len,
                              const mpx_client_conn* conns, size_t n_conns, size_t n_groups,
                              const mpx_client_out* out, mpx_client_conn_result* conn_res,
                              mpx_client_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(client_args(e, buf, len, conns, n_conns, n_groups, out, conn_res, res));
    // the device kernels report these through the error word; here they answer before any launch
    uint64_t end = 0;
    uint32_t grp = 0;
    for (size_t k = 0; k < n_conns; ++k) {
        const mpx_client_conn& c = conns[k];
        if (c.offset & (MPX_CLIENT_ALIGN - 1))
            return fail(e, MPX_E_INVAL, "a connection's offset is not a multiple of MPX_CLIENT_ALIGN");
        if (c.offset > (uint64_t)len || (uint64_t)c.length > (uint64_t)len - c.offset)
            return fail(e, MPX_E_INVAL, "a connection lies outside [0, len]");
        if (c.offset < end)
            return fail(e, MPX_E_INVAL, "connections overlap or are not ascending by offset");
        if (c.group >= n_groups) return fail(e, MPX_E_INVAL, "a connection's group is >= n_groups");
        if (c.group < grp) return fail(e, MPX_E_INVAL, "the connections' groups decrease");
        end = c.offset + c.length;
        grp = c.group;
    }
    CK(begin(e));
    if (n_conns) GROW(e, e->cl_work, mpx::client_work_bytes(len, n_conns, n_groups));
    const size_t cap = staged_cap(out, len);
    Stage L(e);
    const Slot s_buf = L.add((len + 15) & ~(size_t)15),
               s_conns = L.add(n_conns * sizeof(mpx_client_conn)), s_op = L.add(cap),
               s_key = L.add(cap * sizeof(int64_t)), s_val = L.add(cap * sizeof(int64_t)),
               s_meta = L.add(cap * sizeof(mpx_proposal)),
               s_po = L.add(out->prop_off ? (n_groups + 1) * sizeof(uint64_t) : 0),
               s_so = L.add(out->send_off ? (n_groups + 1) * sizeof(uint64_t) : 0),
               s_cr = L.add(n_conns * sizeof(mpx_client_conn_result)),
               s_res = L.add(sizeof(mpx_client_result));
    CK(L.commit());
    CK(h2d(e, L.at<char>(s_buf), buf, len));
    CK(L.in(s_conns, conns));
    mpx_client_out d;
    d.op = L.at<uint8_t>(s_op);
    d.key = L.at<int64_t>(s_key);
    d.val = L.at<int64_t>(s_val);
    d.meta = L.at<mpx_proposal>(s_meta);
    d.prop_cap = cap;
    d.prop_off = L.at<uint64_t>(s_po, out->prop_off);
    d.send_off = L.at<uint64_t>(s_so, out->send_off);
    CK(mpx_decode_client_streams_dev(e, L.at<uint8_t>(s_buf), len,
                                     L.at<mpx_client_conn>(s_conns), n_conns, n_groups, &d,
                                     L.at<mpx_client_conn_result>(s_cr),
                                     L.at<mpx_client_result>(s_res), e->stream));
    // the total first: only the proposals the call produced are copied out
    CK(L.out(s_res, res));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t n = (size_t)std::min<uint64_t>(res->n_proposals, cap);
    CK(L.out(s_op, out->op, n));
    CK(L.out(s_key, out->key, n * sizeof(int64_t)));
    CK(L.out(s_val, out->val, n * sizeof(int64_t)));
    CK(L.out(s_meta, out->meta, n * sizeof(mpx_proposal)));
    if (out->prop_off) CK(L.out(s_po, out->prop_off));
    if (out->send_off) CK(L.out(s_so, out->send_off));
    CK(L.out(s_cr, conn_res));
    return finish(e);
}

}  // extern "C"

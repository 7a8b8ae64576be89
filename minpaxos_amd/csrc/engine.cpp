// engine.cpp — the C ABI (include/mpx.h) over the gfx950 kernels.
//
// *_dev entry points enqueue on the caller's stream with device pointers, never allocate and never
// synchronise. A host-pointer entry point is a staging wrapper over its _dev form: host-only
// checks, begin, lay the call out in the engine's staging arena (Stage) and copy in, the _dev form
// on the engine's stream, copy out, finish; it returns when results are back in caller memory.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>

#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {

constexpr size_t kPinHdr = 128;
struct PinView {
    volatile uint32_t* err;
    uint8_t* op;
    int64_t* key;
    int64_t* val;
    int64_t* ret;
    uint8_t* conf;
};
PinView pin_view_at(uint8_t* base, size_t cap) {
    const size_t a16 = (cap + 15) & ~(size_t)15;
    PinView v;
    v.err = (volatile uint32_t*)base;
    v.op = base + kPinHdr;
    v.key = (int64_t*)(v.op + a16);
    v.val = v.key + cap;
    v.ret = v.val + cap;
    v.conf = (uint8_t*)(v.ret + cap);
    return v;
}
PinView pin_view(const PinIo& p) { return pin_view_at(p.p, p.cap); }
size_t pin_bytes(size_t cap) { return kPinHdr + ((cap + 15) & ~(size_t)15) + cap * 25; }

}  // namespace

namespace {

// size limits the host and _dev forms of a family share
int record_limit(mpx_engine* e, size_t n) {
    if (n >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "more than 2^32-2 records");
    return MPX_OK;
}
int reply_limit(mpx_engine* e, size_t n) {
    if (n >= (1ull << 32)) return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 replies per call");
    return MPX_OK;
}
int decode_limit(mpx_engine* e, size_t len) {
    if (len > MPX_DECODE_MAX_BYTES)
        return fail(e, MPX_E_UNSUPPORTED, "decode buffers are limited to 2^31-1 bytes per call");
    return MPX_OK;
}

void free_kv(mpx::KvTable& t) {
    if (t.keys) (void)hipFree(t.keys);
    if (t.vals) (void)hipFree(t.vals);
    if (t.state) (void)hipFree(t.state);
    if (t.n_present) (void)hipFree(t.n_present);
    if (t.epoch) (void)hipFree(t.epoch);
    if (t.probe) (void)hipFree(t.probe);
    if (t.lhead) (void)hipFree(t.lhead);
    t = mpx::KvTable{};
}

int ensure_kv(mpx_engine* e) {
    if (e->kv_ready) return MPX_OK;
    uint64_t want = e->cfg.kv_capacity ? e->cfg.kv_capacity : (1ull << 20);
    uint64_t cap = 1024;
    while (cap < 2 * want) cap <<= 1;
    mpx::KvTable t{};
    t.cap = cap;
    t.lgnb = 0;
    while ((1ull << (t.lgnb + 8)) < cap) ++t.lgnb;
    // cap hash slots + one side slot for the key INT64_MIN (the empty-slot sentinel)
    if (hipMalloc(&t.keys, (cap + 1) * 8) != hipSuccess ||
        hipMalloc(&t.vals, (cap + 1) * 8) != hipSuccess ||
        hipMalloc(&t.state, (cap + 1) * 4) != hipSuccess ||
        hipMalloc(&t.n_present, sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&t.epoch, 2 * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&t.probe, mpx::kSmallScratchWords * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&t.lhead, (cap + 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        free_kv(t);
        return fail(e, MPX_E_NOMEM, "KV table allocation failed");
    }
    hipError_t r0 = hipMemsetAsync(t.epoch, 0, 2 * sizeof(uint32_t), e->stream);
    if (r0 == hipSuccess)
        r0 = hipMemsetAsync(t.probe, 0, mpx::kSmallScratchWords * sizeof(uint32_t), e->stream);
    if (r0 == hipSuccess) r0 = hipMemsetAsync(t.lhead, 0, (cap + 1) * 4, e->stream);
    const hipError_t r1 = r0 == hipSuccess ? mpx::launch_kv_clear(t, e->stream) : r0;
    if (r1 != hipSuccess) {
        (void)hipGetLastError();
        free_kv(t);
        return hip_fail(e, "KV table initialisation", r1);
    }
    e->kv = t;
    e->kv_ready = true;
    return MPX_OK;
}

int pin_grow(mpx_engine* e, PinIo& p, size_t m) {
    if (p.cap >= m && p.p) return MPX_OK;
    if (p.p) (void)hipHostFree(p.p);
    p.p = nullptr;
    p.cap = 0;
    const size_t cap = m < 1024 ? 1024 : m;
    void* hp = nullptr;
    if (hipHostMalloc(&hp, pin_bytes(cap), hipHostMallocDefault) != hipSuccess || !hp) {
        (void)hipGetLastError();
        return fail(e, MPX_E_NOMEM, "pinned staging for the replica-batch apply");
    }
    p.p = (uint8_t*)hp;
    p.cap = cap;
    return MPX_OK;
}

// the replica-batch kernels on m commands in pinned staging p, results back in it; returns once
// the stream is done (DESIGN section 9 records the rejected alternative to the stream wait)
int run_pinned(mpx_engine* e, const PinIo& p, size_t m, bool want_conf) {
    const PinView v = pin_view(p);
    *v.err = 0u;
    void* dp = nullptr;
    HIPCHK(e, hipHostGetDevicePointer(&dp, p.p, 0));
    const PinView d = pin_view_at((uint8_t*)dp, p.cap);
    HIPCHK(e, mpx::launch_apply_small(e->kv, d.op, d.key, d.val, m, d.ret,
                                      want_conf ? d.conf : nullptr, (uint32_t*)d.err, e->stream,
                                      /*host_io=*/true));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return check_errword(e, *v.err);
}

}  // namespace

extern "C" {

int mpx_abi_version(void) { return MPX_ABI_VERSION; }

int mpx_device_count(int* count) {
    if (!count) return MPX_E_INVAL;
    int c = 0;
    hipError_t r = hipGetDeviceCount(&c);
    if (r != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return MPX_OK;
    }
    *count = c;
    return MPX_OK;
}

int mpx_open(int device, const mpx_config* cfg, mpx_engine** out) {
    if (!cfg || !out) return MPX_E_INVAL;
    *out = nullptr;
    if (cfg->n_replicas < 1 || cfg->n_replicas > MPX_MAX_REPLICAS) return MPX_E_INVAL;
    if (cfg->mode != MPX_MODE_MIN && cfg->mode != MPX_MODE_CLASSIC) return MPX_E_INVAL;
    if (cfg->apply_path > MPX_APPLY_SMALL || (cfg->flags & ~MPX_FLAG_KNOWN) || cfg->reserved)
        return MPX_E_INVAL;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || device < 0 || device >= c) {
        (void)hipGetLastError();
        return MPX_E_NODEV;
    }
    mpx_engine* e = new (std::nothrow) mpx_engine();
    if (!e) return MPX_E_NOMEM;
    e->device = device;
    e->cfg = *cfg;
    if (!e->cfg.kv_per_group) e->cfg.kv_per_group = 512;
    e->apply = mpx::ApplyOpts{cfg->apply_chunk, cfg->apply_path, cfg->apply_fast_min,
                              cfg->apply_hot_min};
    if (!e->cfg.max_groups) e->cfg.max_groups = 1ull << 20;
    if (e->cfg.kv_per_group > 1024) {
        delete e;
        return MPX_E_UNSUPPORTED;
    }
    e->worklist.cap = e->cfg.max_groups * sizeof(uint32_t);
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&e->d_err, sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&e->d_red, mpx::kRedWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&e->d_tctl, mpx::kTileCtlWords * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(e->d_tctl, 0, mpx::kTileCtlWords * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(e->d_red, 0, mpx::kRedWords * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&e->d_wcount, mpx::kStepCtlWords * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(e->d_wcount, 0, mpx::kStepCtlWords * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&e->worklist.p, e->worklist.cap) != hipSuccess ||
        // (one-launch steps keep their packed totals slots there, zero between steps)
        hipMemset(e->worklist.p, 0, e->worklist.cap) != hipSuccess ||
        hipMemset(e->d_err, 0, sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        mpx_close(e);
        return MPX_E_HIP;
    }
    *out = e;
    return MPX_OK;
}

int mpx_close(mpx_engine* e) {
    if (!e) return MPX_E_INVAL;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->comm) ncclCommDestroy(e->comm);
    for (DevBuf* x : {&e->arena, &e->apply_work, &e->decode_work, &e->stream_work, &e->fan_work,
                      &e->log_work, &e->replay_work, &e->are_work, &e->ab_work, &e->um_work,
                      &e->cm_work, &e->ord_work, &e->cl_work, &e->rp_work, &e->xg_work,
                      &e->st_work, &e->lr_work, &e->pr_work, &e->worklist})
        if (x->p) (void)hipFree(x->p);
    if (e->pin_io.p) (void)hipHostFree(e->pin_io.p);
    if (e->pin_staged.p) (void)hipHostFree(e->pin_staged.p);
    if (e->d_wcount) (void)hipFree(e->d_wcount);
    if (e->kv_ready) free_kv(e->kv);
    if (e->d_err) (void)hipFree(e->d_err);
    if (e->d_red) (void)hipFree(e->d_red);
    if (e->d_tctl) (void)hipFree(e->d_tctl);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return MPX_OK;
}

const char* mpx_last_error(mpx_engine* e) { return e ? e->err.c_str() : "null engine"; }

void* mpx_stream(mpx_engine* e) { return e ? (void*)e->stream : nullptr; }

int mpx_synchronize(mpx_engine* e) {
    if (!e) return MPX_E_INVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipDeviceSynchronize());
    return finish(e);
}

// ---- A1 / A2 --------------------------------------------------------------------------------
int mpx_accept_tally(mpx_engine* e, const mpx_accept_reply* recs, size_t n, mpx_inst_state* st,
                     size_t n_inst, int32_t inst_base, int32_t* committed_upto,
                     int32_t* peer_commits, uint8_t* decided_out) {
    if (!e) return MPX_E_INVAL;
    if ((n && !recs) || (n_inst && !st) || !committed_upto || !peer_commits)
        return fail(e, MPX_E_INVAL, "null argument");
    CK(record_limit(e, n));
    const int N = e->cfg.n_replicas;
    int32_t sc[1 + MPX_MAX_REPLICAS];
    sc[0] = *committed_upto;
    memcpy(sc + 1, peer_commits, N * sizeof(int32_t));
    CK(begin(e));
    Stage L(e);
    const Slot s_rec = L.add(n * sizeof(mpx_accept_reply)),
               s_st = L.add(n_inst * sizeof(mpx_inst_state)),
               s_sc = L.add((1 + N) * sizeof(int32_t)), s_dec = L.add(decided_out ? n_inst : 0);
    CK(L.commit());
    CK(L.in(s_rec, recs));
    CK(L.in(s_st, st));
    CK(L.in(s_sc, sc));
    mpx_inst_state* d_st = L.at<mpx_inst_state>(s_st);
    CK(mpx_accept_tally_dev(e, L.at<mpx_accept_reply>(s_rec), n, d_st, d_st, n_inst, inst_base,
                            L.at<int32_t>(s_sc), L.at<uint8_t>(s_dec, decided_out), e->stream));
    CK(L.out(s_st, st));
    CK(L.out(s_sc, sc));
    CK(L.out(s_dec, decided_out));
    CK(finish(e));
    *committed_upto = sc[0];
    memcpy(peer_commits, sc + 1, N * sizeof(int32_t));
    return MPX_OK;
}

int mpx_accept_tally_dev(mpx_engine* e, const mpx_accept_reply* d_recs, size_t n,
                         const mpx_inst_state* d_st_in, mpx_inst_state* d_st_out, size_t n_inst,
                         int32_t inst_base, int32_t* d_scalars, uint8_t* d_decided,
                         void* stream) {
    if (!e) return MPX_E_INVAL;
    if ((n && !d_recs) || (n_inst && (!d_st_in || !d_st_out)) || !d_scalars)
        return fail(e, MPX_E_INVAL, "null argument");
    CK(record_limit(e, n));
    HIPCHK(e, mpx::launch_accept_tally(e->cfg.mode, d_recs, n, d_st_in, d_st_out, n_inst,
                                       inst_base, e->cfg.n_replicas, d_scalars, d_decided,
                                       e->d_red, e->d_tctl, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_committed_prefix(mpx_engine* e, const mpx_inst_state* st, size_t n_inst,
                         int32_t inst_base, int32_t* committed_upto) {
    if (!e) return MPX_E_INVAL;
    if ((n_inst && !st) || !committed_upto) return fail(e, MPX_E_INVAL, "null argument");
    CK(begin(e));
    Stage L(e);
    const Slot s_st = L.add(n_inst * sizeof(mpx_inst_state)), s_cu = L.add(sizeof(int32_t));
    CK(L.commit());
    CK(L.in(s_st, st));
    CK(L.in(s_cu, committed_upto));
    HIPCHK(e, mpx::launch_committed_prefix(L.at<mpx_inst_state>(s_st), n_inst, inst_base,
                                           L.at<int32_t>(s_cu), e->d_red, e->stream));
    CK(L.out(s_cu, committed_upto));
    return finish(e);
}

// ---- A4 ---------------------------------------------------------------------------------------
int mpx_prepare_select(mpx_engine* e, const mpx_prepare_reply* recs, size_t n, mpx_prep_state* st,
                       size_t n_inst, int32_t inst_base, int32_t* default_ballot,
                       uint8_t* prepared_out) {
    if (!e) return MPX_E_INVAL;
    if ((n && !recs) || (n_inst && !st) || !default_ballot)
        return fail(e, MPX_E_INVAL, "null argument");
    CK(begin(e));
    Stage L(e);
    const Slot s_rec = L.add(n * sizeof(mpx_prepare_reply)),
               s_st = L.add(n_inst * sizeof(mpx_prep_state)), s_db = L.add(sizeof(int32_t)),
               s_prep = L.add(prepared_out ? n_inst : 0);
    CK(L.commit());
    CK(L.in(s_rec, recs));
    CK(L.in(s_st, st));
    CK(L.in(s_db, default_ballot));
    mpx_prep_state* d_st = L.at<mpx_prep_state>(s_st);
    CK(mpx_prepare_select_dev(e, L.at<mpx_prepare_reply>(s_rec), n, d_st, d_st, n_inst, inst_base,
                              L.at<int32_t>(s_db), L.at<uint8_t>(s_prep, prepared_out),
                              e->stream));
    CK(L.out(s_st, st));
    CK(L.out(s_db, default_ballot));
    CK(L.out(s_prep, prepared_out));
    return finish(e);
}

int mpx_prepare_select_dev(mpx_engine* e, const mpx_prepare_reply* d_recs, size_t n,
                           const mpx_prep_state* d_st_in, mpx_prep_state* d_st_out, size_t n_inst,
                           int32_t inst_base, int32_t* d_default_ballot, uint8_t* d_prepared,
                           void* stream) {
    if (!e) return MPX_E_INVAL;
    if ((n && !d_recs) || (n_inst && (!d_st_in || !d_st_out)) || !d_default_ballot)
        return fail(e, MPX_E_INVAL, "null argument");
    HIPCHK(e, mpx::launch_prepare_classic(d_recs, n, d_st_in, d_st_out, n_inst, inst_base,
                                          e->cfg.n_replicas, d_default_ballot, d_prepared,
                                          e->d_tctl, e->d_err, pick(e, stream)));
    return MPX_OK;
}

// ---- A3 ---------------------------------------------------------------------------------------
int mpx_prepare_select_min(mpx_engine* e, const mpx_prepare_reply_min* recs, size_t n,
                           const uint64_t* grp_rec_off, mpx_group_prep_state* gst,
                           size_t n_groups, int32_t* peer_commits, mpx_prepare_effect* eff) {
    if (!e) return MPX_E_INVAL;
    if ((n && !recs) || !grp_rec_off || (n_groups && (!gst || !peer_commits)))
        return fail(e, MPX_E_INVAL, "null argument");
    if (grp_rec_off[0] != 0 || grp_rec_off[n_groups] != n)
        return fail(e, MPX_E_INVAL, "grp_rec_off must start at 0 and end at n");
    for (size_t g = 0; g < n_groups; ++g)
        if (grp_rec_off[g + 1] < grp_rec_off[g])
            return fail(e, MPX_E_INVAL, "grp_rec_off must be non-decreasing");
    const int N = e->cfg.n_replicas;
    CK(begin(e));
    Stage L(e);
    const Slot s_rec = L.add(n * sizeof(mpx_prepare_reply_min)),
               s_off = L.add((n_groups + 1) * sizeof(uint64_t)),
               s_gst = L.add(n_groups * sizeof(mpx_group_prep_state)),
               s_pc = L.add(n_groups * N * sizeof(int32_t)),
               s_eff = L.add(eff ? n * sizeof(mpx_prepare_effect) : 0);
    CK(L.commit());
    CK(L.in(s_rec, recs));
    CK(L.in(s_off, grp_rec_off));
    CK(L.in(s_gst, gst));
    CK(L.in(s_pc, peer_commits));
    CK(mpx_prepare_select_min_dev(e, L.at<mpx_prepare_reply_min>(s_rec), n, L.at<uint64_t>(s_off),
                                  L.at<mpx_group_prep_state>(s_gst), n_groups,
                                  L.at<int32_t>(s_pc), L.at<mpx_prepare_effect>(s_eff, eff),
                                  e->stream));
    CK(L.out(s_gst, gst));
    CK(L.out(s_pc, peer_commits));
    CK(L.out(s_eff, eff));
    return finish(e);
}

int mpx_prepare_select_min_dev(mpx_engine* e, const mpx_prepare_reply_min* d_recs, size_t n,
                               const uint64_t* d_grp_rec_off, mpx_group_prep_state* d_gst,
                               size_t n_groups, int32_t* d_peer_commits,
                               mpx_prepare_effect* d_eff, void* stream) {
    if (!e) return MPX_E_INVAL;
    if ((n && !d_recs) || !d_grp_rec_off || (n_groups && (!d_gst || !d_peer_commits)))
        return fail(e, MPX_E_INVAL, "null argument");
    HIPCHK(e, mpx::launch_prepare_min(d_recs, n, d_grp_rec_off, d_gst, n_groups,
                                      e->cfg.n_replicas, d_peer_commits, d_eff, e->d_err,
                                      pick(e, stream)));
    return MPX_OK;
}

// ---- A5 / A6 ----------------------------------------------------------------------------------
int mpx_apply(mpx_engine* e, const uint8_t* op, const int64_t* key, const int64_t* val, size_t m,
              int64_t* ret, uint8_t* conf_prev) {
    if (!e) return MPX_E_INVAL;
    if (m && (!op || !key || !val || !ret)) return fail(e, MPX_E_INVAL, "null argument");
    if (m >= (1ull << 31)) return fail(e, MPX_E_UNSUPPORTED, "more than 2^31-1 commands per call");
    if (mpx::apply_is_one_launch(e->apply, m)) {
        // one drained executeCommands batch: the commands go into pinned host memory the kernels
        // read over the link, the results and the call's error word come back the same way (no
        // DMA, no memset, no copy of the error word: the host clears and reads it in place); a
        // CPU copy on each side (mpx_apply_staged: none)
        HIPCHK(e, hipSetDevice(e->device));
        CK(ensure_kv(e));
        CK(pin_grow(e, e->pin_io, m));
        const PinView v = pin_view(e->pin_io);
        std::memcpy(v.op, op, m);
        std::memcpy(v.key, key, m * 8);
        std::memcpy(v.val, val, m * 8);
        const int rc = run_pinned(e, e->pin_io, m, conf_prev != nullptr);
        std::memcpy(ret, v.ret, m * 8);
        if (conf_prev) std::memcpy(conf_prev, v.conf, m);
        return rc;
    }
    CK(begin(e));
    CK(ensure_kv(e));
    GROW(e, e->apply_work, mpx::apply_work_bytes(e->kv, e->apply, m));
    Stage L(e);
    const Slot s_op = L.add(m), s_key = L.add(m * 8), s_val = L.add(m * 8), s_ret = L.add(m * 8),
               s_conf = L.add(conf_prev ? m : 0);
    CK(L.commit());
    CK(L.in(s_op, op));
    CK(L.in(s_key, key));
    CK(L.in(s_val, val));
    CK(mpx_apply_dev(e, L.at<uint8_t>(s_op), L.at<int64_t>(s_key), L.at<int64_t>(s_val), m,
                     L.at<int64_t>(s_ret), L.at<uint8_t>(s_conf, conf_prev), e->stream));
    CK(L.out(s_ret, ret));
    CK(L.out(s_conf, conf_prev));
    return finish(e);
}

int mpx_apply_buffers(mpx_engine* e, size_t max_m, mpx_apply_io* io) {
    if (!e) return MPX_E_INVAL;
    if (!io) return fail(e, MPX_E_INVAL, "null io");
    if (!max_m || max_m > MPX_APPLY_SMALL_MAX)
        return fail(e, MPX_E_INVAL, "max_m must lie in [1, MPX_APPLY_SMALL_MAX]");
    if (!mpx::apply_is_one_launch(e->apply, max_m))
        return fail(e, MPX_E_INVAL, "the staged apply needs apply_path AUTO or SMALL");
    HIPCHK(e, hipSetDevice(e->device));
    CK(ensure_kv(e));
    if (e->pin_staged.cap < max_m) {
        HIPCHK(e, hipStreamSynchronize(e->stream));  // (no call may still use the old buffers)
        CK(pin_grow(e, e->pin_staged, max_m));
    }
    const PinView v = pin_view(e->pin_staged);
    io->op = v.op;
    io->key = v.key;
    io->val = v.val;
    io->ret = v.ret;
    io->conf = v.conf;
    io->cap = e->pin_staged.cap;
    return MPX_OK;
}

int mpx_apply_staged(mpx_engine* e, size_t m) {
    if (!e) return MPX_E_INVAL;
    if (!m) return MPX_OK;
    if (!e->pin_staged.p || m > e->pin_staged.cap)
        return fail(e, MPX_E_INVAL, "m exceeds the buffers of mpx_apply_buffers");
    HIPCHK(e, hipSetDevice(e->device));
    return run_pinned(e, e->pin_staged, m, true);
}

int mpx_apply_reserve(mpx_engine* e, size_t max_cmds) {
    if (!e) return MPX_E_INVAL;
    if (max_cmds >= (1ull << 31)) return fail(e, MPX_E_UNSUPPORTED, "more than 2^31-1 commands");
    HIPCHK(e, hipSetDevice(e->device));
    CK(ensure_kv(e));  // (its size enters the scratch's)
    return reserve(e, e->apply_work, mpx::apply_reserve_bytes(e->kv, e->apply, max_cmds));
}

int mpx_apply_dev(mpx_engine* e, const uint8_t* d_op, const int64_t* d_key, const int64_t* d_val,
                  size_t m, int64_t* d_ret, uint8_t* d_conf_prev, void* stream) {
    if (!e) return MPX_E_INVAL;
    if (m && (!d_op || !d_key || !d_val || !d_ret)) return fail(e, MPX_E_INVAL, "null argument");
    if (m >= (1ull << 31)) return fail(e, MPX_E_UNSUPPORTED, "more than 2^31-1 commands per call");
    // (no table yet: no scratch is enough)
    CK(reserved(e, e->apply_work,
                e->kv_ready ? mpx::apply_work_bytes(e->kv, e->apply, m) : UINT64_MAX,
                "mpx_apply_dev", "mpx_apply_reserve(m)"));
    mpx::ApplyWork w{e->apply_work.p, e->apply_work.cap};
    HIPCHK(e, mpx::launch_apply(e->kv, d_op, d_key, d_val, m, d_ret, d_conf_prev,
                                e->apply, w, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_kv_size(mpx_engine* e, size_t* n) {
    if (!e) return MPX_E_INVAL;
    if (!n) return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(begin(e));
    CK(ensure_kv(e));
    unsigned long long c = 0;
    CK(d2h(e, &c, e->kv.n_present, sizeof(c)));
    CK(finish(e));
    *n = (size_t)c;
    return MPX_OK;
}

int mpx_kv_export(mpx_engine* e, int64_t* keys, int64_t* vals, size_t cap, size_t* n) {
    if (!e) return MPX_E_INVAL;
    if (!n || (cap && (!keys || !vals))) return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(begin(e));
    CK(ensure_kv(e));
    unsigned long long c = 0;
    CK(d2h(e, &c, e->kv.n_present, sizeof(c)));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t want = (size_t)c;
    Stage L(e);
    const Slot s_keys = L.add(want * 8), s_vals = L.add(want * 8);
    CK(L.commit());
    HIPCHK(e, mpx::launch_kv_export(e->kv, L.at<int64_t>(s_keys), L.at<int64_t>(s_vals), want,
                                    (unsigned long long*)e->d_red, e->stream));
    const size_t k = std::min(cap, want);
    CK(L.out(s_keys, keys, k * 8));
    CK(L.out(s_vals, vals, k * 8));
    CK(finish(e));
    *n = want;
    return MPX_OK;
}

int mpx_kv_import(mpx_engine* e, const int64_t* keys, const int64_t* vals, size_t n) {
    if (!e) return MPX_E_INVAL;
    if ((n && (!keys || !vals))) return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(begin(e));
    CK(ensure_kv(e));
    Stage L(e);
    const Slot s_keys = L.add(n * 8), s_vals = L.add(n * 8);
    CK(L.commit());
    CK(L.in(s_keys, keys));
    CK(L.in(s_vals, vals));
    HIPCHK(e, mpx::launch_kv_import(e->kv, L.at<int64_t>(s_keys), L.at<int64_t>(s_vals), n,
                                    e->d_err, e->stream));
    return finish(e);
}

int mpx_kv_clear(mpx_engine* e) {
    if (!e) return MPX_E_INVAL;
    CK(begin(e));
    CK(ensure_kv(e));
    HIPCHK(e, mpx::launch_kv_clear(e->kv, e->stream));
    return finish(e);
}

int mpx_conflict_batch(mpx_engine* e, const uint8_t* op, const int64_t* key,
                       const uint64_t* inst_off, size_t n_inst, uint8_t* out) {
    if (!e) return MPX_E_INVAL;
    if (n_inst < 2) return MPX_OK;
    if (!op || !key || !inst_off || !out) return fail(e, MPX_E_INVAL, "null argument");
    const uint64_t m = inst_off[n_inst];
    if (inst_off[0] != 0) return fail(e, MPX_E_INVAL, "inst_off[0] must be 0");
    for (size_t i = 0; i < n_inst; ++i)
        if (inst_off[i + 1] < inst_off[i]) return fail(e, MPX_E_INVAL, "inst_off not sorted");
    CK(begin(e));
    Stage L(e);
    const Slot s_op = L.add(m), s_key = L.add(m * 8), s_off = L.add((n_inst + 1) * 8),
               s_out = L.add(n_inst - 1);
    CK(L.commit());
    CK(L.in(s_op, op));
    CK(L.in(s_key, key));
    CK(L.in(s_off, inst_off));
    CK(mpx_conflict_batch_dev(e, L.at<uint8_t>(s_op), L.at<int64_t>(s_key), L.at<uint64_t>(s_off),
                              n_inst, L.at<uint8_t>(s_out), e->stream));
    CK(L.out(s_out, out));
    return finish(e);
}

int mpx_conflict_batch_dev(mpx_engine* e, const uint8_t* d_op, const int64_t* d_key,
                           const uint64_t* d_inst_off, size_t n_inst, uint8_t* d_out,
                           void* stream) {
    if (!e) return MPX_E_INVAL;
    if (n_inst < 2) return MPX_OK;
    if (!d_op || !d_key || !d_inst_off || !d_out) return fail(e, MPX_E_INVAL, "null argument");
    HIPCHK(e, mpx::launch_conflict_batch(d_op, d_key, d_inst_off, n_inst, d_out, pick(e, stream)));
    return MPX_OK;
}

// ---- fused group step -------------------------------------------------------------------------
namespace {
bool one_launch(const mpx_engine* e) { return (e->cfg.flags & MPX_FLAG_STEP_ONE_LAUNCH) != 0; }
// one-launch steps: the packed totals slots (one u64 per 64 groups) live in the work list's
// memory, which such a handle never uses as a list
unsigned long long* pslots(const mpx_engine* e) {
    return one_launch(e) ? reinterpret_cast<unsigned long long*>(e->worklist.p) : nullptr;
}
// the batch shapes the kernels take (the host form checks them before it stages anything)
int step_shape(mpx_engine* e, const mpx_group_batch* b) {
    if (b->ipg == 0 && b->n_groups) return fail(e, MPX_E_INVAL, "ipg must be > 0");
    if (b->ipg > 8192) return fail(e, MPX_E_UNSUPPORTED, "more than 8192 instances per group");
    return MPX_OK;
}
// the device-pointer group step; d_totals (optional) gets the step totals from the same kernels.
// timed: record the mpx_group_step_events pair around the fast kernel (the _dev forms do, the
// host form does not)
int group_step_dev(mpx_engine* e, const mpx_group_batch* b, int64_t* d_totals, void* stream,
                   bool timed = true) {
    if (!e) return MPX_E_INVAL;
    if (!b) return fail(e, MPX_E_INVAL, "null or invalid argument");
    if (b->n_groups && (!b->recs || !b->grp_rec_off || !b->st_in || !b->st_out ||
                        !b->committed_in || !b->committed_out || !b->executed_in ||
                        !b->executed_out || !b->peer_in || !b->peer_out || !b->op || !b->key ||
                        !b->val || !b->cmd_off || !b->ret || !b->kv_cnt_in || !b->kv_key_in ||
                        !b->kv_val_in || !b->kv_cnt_out || !b->kv_key_out || !b->kv_val_out))
        return fail(e, MPX_E_INVAL, "null field in mpx_group_batch");
    CK(step_shape(e, b));
    if ((uint64_t)b->n_groups * sizeof(uint32_t) > e->worklist.cap)
        return fail(e, MPX_E_INVAL, "n_groups exceeds mpx_config.max_groups");
    if (one_launch(e) && !mpx::step_one_launch_fits(e->cfg.n_replicas, b->ipg, e->cfg.kv_per_group))
        return fail(e, MPX_E_INVAL, "MPX_FLAG_STEP_ONE_LAUNCH: the batch shape fits no fast variant");
    if (one_launch(e) && e->slots_dirty) {
        HIPCHK(e, hipMemsetAsync(e->worklist.p, 0, e->worklist.cap, pick(e, stream)));
        e->slots_dirty = false;
    }
    HIPCHK(e, mpx::launch_group_step(e->cfg.mode, e->cfg.n_replicas, e->cfg.kv_per_group, b,
                                     (uint32_t*)e->worklist.p, e->d_wcount, d_totals, e->d_err,
                                     pick(e, stream), timed ? e->ev_fast0 : nullptr,
                                     timed ? e->ev_fast1 : nullptr, pslots(e)));
    return MPX_OK;
}
}  // namespace

int mpx_group_step_dev(mpx_engine* e, const mpx_group_batch* b, void* stream) {
    return group_step_dev(e, b, nullptr, stream);
}

int mpx_group_step_totals_dev(mpx_engine* e, const mpx_group_batch* b, int64_t* d_totals,
                              void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!d_totals) return fail(e, MPX_E_INVAL, "null d_totals");
    if (b && b->n_groups && !b->n_decided)
        return fail(e, MPX_E_INVAL, "mpx_group_step_totals_dev needs n_decided");
    return group_step_dev(e, b, d_totals, stream);
}

int mpx_group_step_events(mpx_engine* e, void* ev_fast_start, void* ev_fast_end) {
    if (!e) return MPX_E_INVAL;
    if (!ev_fast_start != !ev_fast_end) return fail(e, MPX_E_INVAL, "give both events or neither");
    e->ev_fast0 = (hipEvent_t)ev_fast_start;
    e->ev_fast1 = (hipEvent_t)ev_fast_end;
    return MPX_OK;
}

int mpx_step_totals_dev(mpx_engine* e, const mpx_group_batch* b, int64_t* d_totals,
                        void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!b || !d_totals) return fail(e, MPX_E_INVAL, "null argument");
    if (b->n_groups && (!b->n_decided || !b->executed_in || !b->executed_out || !b->cmd_off))
        return fail(e, MPX_E_INVAL, "mpx_step_totals_dev needs n_decided, executed_in/out, cmd_off");
    HIPCHK(e, mpx::launch_step_totals(b, d_totals, e->d_wcount, pick(e, stream)));
    return MPX_OK;
}

int mpx_group_step(mpx_engine* e, const mpx_group_batch* hb) {
    if (!e) return MPX_E_INVAL;
    if (!hb) return fail(e, MPX_E_INVAL, "null or invalid argument");
    const uint64_t G = hb->n_groups, ipg = hb->ipg, ni = G * ipg;
    const int N = e->cfg.n_replicas;
    const uint64_t K = e->cfg.kv_per_group;
    if (!G) return MPX_OK;
    if (!hb->grp_rec_off || !hb->cmd_off) return fail(e, MPX_E_INVAL, "null offsets");
    const uint64_t nr = hb->grp_rec_off[G];
    const uint64_t m = hb->cmd_off[ni];
    if (hb->grp_rec_off[0] != 0) return fail(e, MPX_E_INVAL, "grp_rec_off[0] must be 0");
    for (uint64_t g = 0; g < G; ++g)
        if (hb->grp_rec_off[g + 1] < hb->grp_rec_off[g])
            return fail(e, MPX_E_INVAL, "grp_rec_off not sorted");
    for (uint64_t i = 0; i < ni; ++i)
        if (hb->cmd_off[i + 1] < hb->cmd_off[i]) return fail(e, MPX_E_INVAL, "cmd_off not sorted");
    CK(step_shape(e, hb));
    CK(begin(e));
    // unlike the _dev form, the host form takes more groups than mpx_config.max_groups
    if (G * sizeof(uint32_t) > e->worklist.cap) {
        GROW(e, e->worklist, G * sizeof(uint32_t));
        HIPCHK(e, hipMemsetAsync(e->worklist.p, 0, e->worklist.cap, e->stream));  // (slots)
    }
    // in-place state (st, the KV tables) is one slot, in and out
    Stage L(e);
    const Slot s_recs = L.add(nr * sizeof(mpx_accept_reply)), s_roff = L.add((G + 1) * 8),
               s_st = L.add(ni * sizeof(mpx_inst_state)), s_ci = L.add(G * 4),
               s_co = L.add(G * 4), s_ei = L.add(G * 4), s_eo = L.add(G * 4),
               s_pi = L.add(G * N * 4), s_po = L.add(G * N * 4), s_op = L.add(m),
               s_key = L.add(m * 8), s_val = L.add(m * 8), s_coff = L.add((ni + 1) * 4),
               s_has = L.add(hb->has_cmds ? ni : 0), s_ret = L.add(m * 8),
               s_conf = L.add(hb->conf_prev ? m : 0), s_kc = L.add(G * 4),
               s_kk = L.add(G * K * 8), s_kv = L.add(G * K * 8),
               s_dec = L.add(hb->decided ? ni : 0), s_nd = L.add(hb->n_decided ? G * 4 : 0);
    CK(L.commit());
    mpx_group_batch db{};
    db.n_groups = (uint32_t)G;
    db.ipg = (uint32_t)ipg;
    db.recs = L.at<mpx_accept_reply>(s_recs);
    db.grp_rec_off = L.at<uint64_t>(s_roff);
    db.st_in = db.st_out = L.at<mpx_inst_state>(s_st);
    db.committed_in = L.at<int32_t>(s_ci);
    db.committed_out = L.at<int32_t>(s_co);
    db.executed_in = L.at<int32_t>(s_ei);
    db.executed_out = L.at<int32_t>(s_eo);
    db.peer_in = L.at<int32_t>(s_pi);
    db.peer_out = L.at<int32_t>(s_po);
    db.op = L.at<uint8_t>(s_op);
    db.key = L.at<int64_t>(s_key);
    db.val = L.at<int64_t>(s_val);
    db.cmd_off = L.at<uint32_t>(s_coff);
    db.has_cmds = L.at<uint8_t>(s_has, hb->has_cmds);
    db.ret = L.at<int64_t>(s_ret);
    db.conf_prev = L.at<uint8_t>(s_conf, hb->conf_prev);
    db.kv_cnt_in = db.kv_cnt_out = L.at<uint32_t>(s_kc);
    db.kv_key_in = db.kv_key_out = L.at<int64_t>(s_kk);
    db.kv_val_in = db.kv_val_out = L.at<int64_t>(s_kv);
    db.decided = L.at<uint8_t>(s_dec, hb->decided);
    db.n_decided = L.at<uint32_t>(s_nd, hb->n_decided);
    CK(L.in(s_recs, hb->recs));
    CK(L.in(s_roff, hb->grp_rec_off));
    CK(L.in(s_st, hb->st_in));
    CK(L.in(s_ci, hb->committed_in));
    CK(L.in(s_ei, hb->executed_in));
    CK(L.in(s_pi, hb->peer_in));
    CK(L.in(s_op, hb->op));
    CK(L.in(s_key, hb->key));
    CK(L.in(s_val, hb->val));
    CK(L.in(s_coff, hb->cmd_off));
    CK(L.in(s_has, hb->has_cmds));
    CK(L.in(s_ret, hb->ret));  // unexecuted commands keep the caller's values
    CK(L.in(s_conf, hb->conf_prev));
    CK(L.in(s_kc, hb->kv_cnt_in));
    CK(L.in(s_kk, hb->kv_key_in));
    CK(L.in(s_kv, hb->kv_val_in));
    CK(group_step_dev(e, &db, nullptr, e->stream, /*timed=*/false));
    CK(L.out(s_st, hb->st_out));
    CK(L.out(s_co, hb->committed_out));
    CK(L.out(s_eo, hb->executed_out));
    CK(L.out(s_po, hb->peer_out));
    CK(L.out(s_ret, hb->ret));
    CK(L.out(s_conf, hb->conf_prev));
    CK(L.out(s_kc, hb->kv_cnt_out));
    CK(L.out(s_kk, hb->kv_key_out));
    CK(L.out(s_kv, hb->kv_val_out));
    CK(L.out(s_dec, hb->decided));
    CK(L.out(s_nd, hb->n_decided));
    return finish(e);
}

// ---- RCCL -------------------------------------------------------------------------------------
int mpx_comm_unique_id(void* out128) {
    if (!out128) return MPX_E_INVAL;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return MPX_E_RCCL;
    memcpy(out128, &id, sizeof(id));
    return MPX_OK;
}

int mpx_comm_init(mpx_engine* e, int nranks, int rank, const void* unique_id128) {
    if (!e) return MPX_E_INVAL;
    if (!unique_id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(e, MPX_E_INVAL, "null or invalid argument");
    HIPCHK(e, hipSetDevice(e->device));
    if (e->comm) {
        ncclCommDestroy(e->comm);
        e->comm = nullptr;
    }
    ncclUniqueId id;
    memcpy(&id, unique_id128, sizeof(id));
    ncclResult_t r = ncclCommInitRank(&e->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        e->comm = nullptr;
        return fail(e, MPX_E_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    }
    e->nranks = nranks;
    e->rank = rank;
    return MPX_OK;
}

int mpx_watermarks_allreduce_dev(mpx_engine* e, int32_t* d_wm, size_t n_groups, void* stream) {
    if (!e) return MPX_E_INVAL;
    if (n_groups && !d_wm) return fail(e, MPX_E_INVAL, "null d_watermarks");
    if (!e->comm) return fail(e, MPX_E_INVAL, "mpx_comm_init has not been called");
    ncclResult_t r = ncclAllReduce(d_wm, d_wm, 2 * n_groups, ncclInt32, ncclMax, e->comm,
                                   pick(e, stream));
    if (r != ncclSuccess) return fail(e, MPX_E_RCCL, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    return MPX_OK;
}

int mpx_step_allreduce_dev(mpx_engine* e, int32_t* d_wm, size_t n_groups, int64_t* d_totals,
                           size_t n_totals, void* stream) {
    if (!e) return MPX_E_INVAL;
    if ((n_groups && !d_wm) || (n_totals && !d_totals)) return fail(e, MPX_E_INVAL, "null argument");
    if (!e->comm) return fail(e, MPX_E_INVAL, "mpx_comm_init has not been called");
    const hipStream_t s = pick(e, stream);
    ncclResult_t r = ncclGroupStart();
    if (r == ncclSuccess && n_groups)
        r = ncclAllReduce(d_wm, d_wm, 2 * n_groups, ncclInt32, ncclMax, e->comm, s);
    if (r == ncclSuccess && n_totals)
        r = ncclAllReduce(d_totals, d_totals, n_totals, ncclInt64, ncclSum, e->comm, s);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess)
        return fail(e, MPX_E_RCCL, std::string("step all-reduce: ") + ncclGetErrorString(r));
    return MPX_OK;
}

int mpx_step_allreduce_oop_dev(mpx_engine* e, const int32_t* d_wm_send, int32_t* d_wm_recv,
                               size_t n_groups, int64_t* d_totals, size_t n_totals, void* stream) {
    if (!e) return MPX_E_INVAL;
    if ((n_groups && (!d_wm_send || !d_wm_recv)) || (n_totals && !d_totals))
        return fail(e, MPX_E_INVAL, "null argument");
    if (n_groups && d_wm_send == d_wm_recv)
        return fail(e, MPX_E_INVAL, "d_wm_send and d_wm_recv must differ (mpx_step_allreduce_dev "
                                    "is the in-place form)");
    if (!e->comm) return fail(e, MPX_E_INVAL, "mpx_comm_init has not been called");
    const hipStream_t s = pick(e, stream);
    ncclResult_t r = ncclGroupStart();
    if (r == ncclSuccess && n_groups)
        r = ncclAllReduce(d_wm_send, d_wm_recv, 2 * n_groups, ncclInt32, ncclMax, e->comm, s);
    if (r == ncclSuccess && n_totals)
        r = ncclAllReduce(d_totals, d_totals, n_totals, ncclInt64, ncclSum, e->comm, s);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess)
        return fail(e, MPX_E_RCCL, std::string("step all-reduce: ") + ncclGetErrorString(r));
    return MPX_OK;
}

int mpx_watermarks_allreduce(mpx_engine* e, int32_t* committed, int32_t* executed,
                             size_t n_groups) {
    if (!e) return MPX_E_INVAL;
    if ((n_groups && (!committed || !executed))) return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(begin(e));
    Stage L(e);
    const Slot s_wm = L.add(2 * n_groups * 4);  // committed, then executed
    CK(L.commit());
    int32_t* d = L.at<int32_t>(s_wm);
    CK(h2d(e, d, committed, n_groups * 4));
    CK(h2d(e, d + n_groups, executed, n_groups * 4));
    CK(mpx_watermarks_allreduce_dev(e, d, n_groups, e->stream));
    CK(d2h(e, committed, d, n_groups * 4));
    CK(d2h(e, executed, d + n_groups, n_groups * 4));
    return finish(e);
}

// ---- §8(f) rank 1: peer stream framing + AcceptReply decode --------------------------------
int mpx_decode_reserve(mpx_engine* e, size_t max_len) {
    if (!e) return MPX_E_INVAL;
    CK(decode_limit(e, max_len));
    return reserve(e, e->decode_work, mpx::decode_work_bytes(max_len));
}

int mpx_decode_peer_stream_dev(mpx_engine* e, const uint8_t* d_buf, size_t len,
                               mpx_accept_reply* d_ar, size_t ar_cap, mpx_peer_frame* d_other,
                               size_t other_cap, mpx_decode_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!d_res || (len && !d_buf) || (ar_cap && !d_ar) || (other_cap && !d_other))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(decode_limit(e, len));
    if ((uintptr_t)d_buf % 16)
        return fail(e, MPX_E_INVAL, "d_buf must be 16-byte aligned (tiles load 16 B vectors)");
    CK(reserved(e, e->decode_work, mpx::decode_work_bytes(len), "mpx_decode_peer_stream_dev",
                "mpx_decode_reserve(len)"));
    HIPCHK(e, mpx::launch_decode_peer_stream(d_buf, len, d_ar, ar_cap, d_other, other_cap, d_res,
                                             e->decode_work.p, e->decode_work.cap,
                                             pick(e, stream)));
    return MPX_OK;
}

int mpx_decode_peer_stream(mpx_engine* e, const uint8_t* buf, size_t len, mpx_accept_reply* ar,
                           size_t ar_cap, mpx_peer_frame* other, size_t other_cap,
                           mpx_decode_result* res) {
    if (!e) return MPX_E_INVAL;
    if (!res || (len && !buf) || (ar_cap && !ar) || (other_cap && !other))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(decode_limit(e, len));
    CK(begin(e));
    GROW(e, e->decode_work, mpx::decode_work_bytes(len));
    Stage L(e);
    const Slot s_buf = L.add(len), s_ar = L.add(ar_cap * sizeof(mpx_accept_reply)),
               s_oth = L.add(other_cap * sizeof(mpx_peer_frame)),
               s_res = L.add(sizeof(mpx_decode_result));
    CK(L.commit());
    CK(L.in(s_buf, buf));
    CK(mpx_decode_peer_stream_dev(e, L.at<uint8_t>(s_buf), len, L.at<mpx_accept_reply>(s_ar),
                                  ar_cap, L.at<mpx_peer_frame>(s_oth), other_cap,
                                  L.at<mpx_decode_result>(s_res), e->stream));
    CK(L.out(s_res, res));
    CK(finish(e));
    // the records the call wrote (the result counts past the caller's capacities)
    CK(L.out(s_ar, ar, std::min<uint64_t>(res->n_accept_replies, ar_cap) *
                           sizeof(mpx_accept_reply)));
    CK(L.out(s_oth, other, std::min<uint64_t>(res->n_other, other_cap) * sizeof(mpx_peer_frame)));
    return finish(e);
}

// ---- §8(f) rank 1, full: fixed and variable-length frames -------------------------------------
namespace {
size_t prep_rec_bytes(const mpx_engine* e) {
    return e->cfg.mode == MPX_MODE_MIN ? sizeof(mpx_prepare_reply_min) : sizeof(mpx_prepare_reply);
}
// the argument rules both forms share (buf / res: host or device pointers alike)
int decode_stream_args(mpx_engine* e, const uint8_t* buf, size_t len, const mpx_decode_out* out,
                       const mpx_stream_result* res) {
    if (!out || !res || (len && !buf) || (out->ar_cap && !out->ar) ||
        (out->prep_cap && !out->prep) || (out->var_cap && !out->var) ||
        (out->other_cap && !out->other))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    return decode_limit(e, len);
}
}  // namespace

int mpx_decode_stream_reserve(mpx_engine* e, size_t max_len) {
    if (!e) return MPX_E_INVAL;
    CK(decode_limit(e, max_len));
    return reserve(e, e->stream_work, mpx::stream_work_bytes(max_len));
}

int mpx_decode_stream_dev(mpx_engine* e, const uint8_t* d_buf, size_t len, size_t start,
                          const mpx_decode_out* out, mpx_stream_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(decode_stream_args(e, d_buf, len, out, d_res));
    if (start > len) return fail(e, MPX_E_INVAL, "start is past the end of the buffer");
    if ((uintptr_t)d_buf % 16)
        return fail(e, MPX_E_INVAL, "d_buf must be 16-byte aligned (tiles load 16 B vectors)");
    CK(reserved(e, e->stream_work, mpx::stream_work_bytes(len), "mpx_decode_stream_dev",
                "mpx_decode_stream_reserve(len)"));
    const mpx::StreamOuts o{out->ar, out->ar_cap, out->prep, out->prep_cap, out->var,
                            out->var_cap, out->other, out->other_cap};
    HIPCHK(e, mpx::launch_decode_stream(e->cfg.mode, d_buf, len, start, o, d_res,
                                        e->stream_work.p, e->stream_work.cap, pick(e, stream)));
    return MPX_OK;
}

int mpx_decode_stream(mpx_engine* e, const uint8_t* buf, size_t len, const mpx_decode_out* out,
                      mpx_stream_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(decode_stream_args(e, buf, len, out, res));
    const size_t pb = prep_rec_bytes(e);
    CK(begin(e));
    GROW(e, e->stream_work, mpx::stream_work_bytes(len));
    Stage L(e);
    const Slot s_buf = L.add(len), s_ar = L.add(out->ar_cap * sizeof(mpx_accept_reply)),
               s_prep = L.add(out->prep_cap * pb),
               s_var = L.add(out->var_cap * sizeof(mpx_var_frame)),
               s_oth = L.add(out->other_cap * sizeof(mpx_peer_frame)),
               s_res = L.add(sizeof(mpx_stream_result));
    CK(L.commit());
    CK(L.in(s_buf, buf));
    const mpx_decode_out d{L.at<mpx_accept_reply>(s_ar), out->ar_cap, L.at<void>(s_prep),
                           out->prep_cap, L.at<mpx_var_frame>(s_var), out->var_cap,
                           L.at<mpx_peer_frame>(s_oth), out->other_cap};
    mpx_stream_result r;
    memset(&r, 0, sizeof(r));
    CK(L.in(s_res, &r));
    // one call per frame longer than the in-map window (MPX_DECODE_LONG); after one, windows
    // of the buffer (a PARTIAL stop at a window's end just continues) keep each call short
    size_t start = 0, window = len;
    for (;;) {
        const size_t end = std::min(len, start + window);
        CK(mpx_decode_stream_dev(e, L.at<uint8_t>(s_buf), end, start, &d,
                                 L.at<mpx_stream_result>(s_res), e->stream));
        CK(L.out(s_res, &r));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (r.stop_reason == MPX_DECODE_LONG && r.next <= len) {
            start = r.next;
            window = 1u << 18;
        } else if ((r.stop_reason == MPX_DECODE_PARTIAL || r.stop_reason == MPX_DECODE_END) &&
                   end < len) {
            // the window ended inside the buffer: a frame that runs past it (PARTIAL) or one
            // that ends exactly at it (END) - both continue from there
            start = r.consumed;
            window = std::min<size_t>(window * 2, len);
        } else {
            break;
        }
    }
    *res = r;
    CK(L.out(s_ar, out->ar, std::min<uint64_t>(r.n_accept_replies, out->ar_cap) *
                                sizeof(mpx_accept_reply)));
    CK(L.out(s_prep, out->prep, std::min<uint64_t>(r.n_prepare_replies, out->prep_cap) * pb));
    CK(L.out(s_var, out->var, std::min<uint64_t>(r.n_var, out->var_cap) * sizeof(mpx_var_frame)));
    CK(L.out(s_oth, out->other, std::min<uint64_t>(r.n_other, out->other_cap) *
                                    sizeof(mpx_peer_frame)));
    return finish(e);
}

// ---- §8(f) rank 2: client reply fan-out -----------------------------------------------------
int mpx_encode_replies_reserve(mpx_engine* e, size_t max_n) {
    if (!e) return MPX_E_INVAL;
    CK(reply_limit(e, max_n));
    return reserve(e, e->fan_work, mpx::fanout_work_bytes(max_n));
}

int mpx_encode_replies_dev(mpx_engine* e, const mpx_reply_rec* d_recs, size_t n,
                           uint32_t n_clients, uint8_t ok, int32_t leader, uint8_t* d_out,
                           uint64_t* d_client_off, void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!n_clients || !d_client_off || (n && (!d_recs || !d_out))) return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(reply_limit(e, n));
    CK(reserved(e, e->fan_work, mpx::fanout_work_bytes(n), "mpx_encode_replies_dev",
                "mpx_encode_replies_reserve(n)"));
    HIPCHK(e, mpx::launch_encode_replies(d_recs, n, n_clients, ok, leader, d_out, d_client_off,
                                         e->fan_work.p, e->fan_work.cap, e->d_err,
                                         pick(e, stream)));
    return MPX_OK;
}

int mpx_encode_replies(mpx_engine* e, const mpx_reply_rec* recs, size_t n, uint32_t n_clients,
                       uint8_t ok, int32_t leader, uint8_t* out, uint64_t* client_off) {
    if (!e) return MPX_E_INVAL;
    if (!n_clients || !client_off || (n && (!recs || !out))) return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(reply_limit(e, n));
    CK(begin(e));
    GROW(e, e->fan_work, mpx::fanout_work_bytes(n));
    Stage L(e);
    const Slot s_rec = L.add(n * sizeof(mpx_reply_rec)), s_out = L.add(n * MPX_PROPOSE_REPLY_BYTES),
               s_off = L.add(((size_t)n_clients + 1) * sizeof(uint64_t));
    CK(L.commit());
    CK(L.in(s_rec, recs));
    CK(mpx_encode_replies_dev(e, L.at<mpx_reply_rec>(s_rec), n, n_clients, ok, leader,
                              L.at<uint8_t>(s_out), L.at<uint64_t>(s_off), e->stream));
    CK(L.out(s_out, out));
    CK(L.out(s_off, client_off));
    int rc = finish(e);
    if (rc == MPX_E_INVAL) return fail(e, MPX_E_INVAL, "a reply names a client >= n_clients");
    return rc;
}

// ---- the acceptor side: handleAccept and the AcceptReply bytes ------------------------------
namespace {
// the sizes the host and _dev forms of the acceptor and commit handlers take (the host forms check
// them before they allocate)
int window_limits(mpx_engine* e, size_t n, size_t n_inst, size_t n_groups, uint32_t ipg) {
    if (!ipg || !n_groups || n_groups > (1ull << 32) || n_groups * (uint64_t)ipg != n_inst ||
        n_inst > (1ull << 32))
        return fail(e, MPX_E_INVAL, "n_inst must equal n_groups * ipg (at most 2^32)");
    return record_limit(e, n);
}
}  // namespace

int mpx_accept_handle_dev(mpx_engine* e, const mpx_accept_msg* d_msgs, size_t n,
                          const mpx_acceptor_state* d_st_in, mpx_acceptor_state* d_st_out,
                          size_t n_inst, int32_t inst_base, const mpx_acceptor_group* d_groups,
                          size_t n_groups, uint32_t ipg, mpx_accept_reply* d_replies,
                          int32_t* d_reply_to, uint8_t* d_effect, void* stream) {
    if (!e) return MPX_E_INVAL;
    if ((n && (!d_msgs || !d_replies || !d_reply_to || !d_effect)) ||
        (n_inst && (!d_st_in || !d_st_out)) || !d_groups)
        return fail(e, MPX_E_INVAL, "null argument");
    CK(window_limits(e, n, n_inst, n_groups, ipg));
    HIPCHK(e, mpx::launch_accept_handle(e->cfg.mode, d_msgs, n, d_st_in, d_st_out, n_inst,
                                        inst_base, d_groups, n_groups, ipg, e->cfg.n_replicas,
                                        d_replies, d_reply_to, d_effect, e->d_err,
                                        pick(e, stream)));
    return MPX_OK;
}

int mpx_accept_handle(mpx_engine* e, const mpx_accept_msg* msgs, size_t n, mpx_acceptor_state* st,
                      size_t n_inst, int32_t inst_base, const mpx_acceptor_group* groups,
                      size_t n_groups, uint32_t ipg, mpx_accept_reply* replies, int32_t* reply_to,
                      uint8_t* effect) {
    if (!e) return MPX_E_INVAL;
    if ((n && (!msgs || !replies || !reply_to || !effect)) || (n_inst && !st) || !groups)
        return fail(e, MPX_E_INVAL, "null argument");
    CK(window_limits(e, n, n_inst, n_groups, ipg));
    CK(begin(e));
    Stage L(e);
    const Slot s_msg = L.add(n * sizeof(mpx_accept_msg)),
               s_st = L.add(n_inst * sizeof(mpx_acceptor_state)),
               s_grp = L.add(n_groups * sizeof(mpx_acceptor_group)),
               s_rep = L.add(n * sizeof(mpx_accept_reply)), s_to = L.add(n * sizeof(int32_t)),
               s_eff = L.add(n);
    CK(L.commit());
    CK(L.in(s_msg, msgs));
    CK(L.in(s_st, st));
    CK(L.in(s_grp, groups));
    mpx_acceptor_state* d_st = L.at<mpx_acceptor_state>(s_st);
    CK(mpx_accept_handle_dev(e, L.at<mpx_accept_msg>(s_msg), n, d_st, d_st, n_inst, inst_base,
                             L.at<mpx_acceptor_group>(s_grp), n_groups, ipg,
                             L.at<mpx_accept_reply>(s_rep), L.at<int32_t>(s_to),
                             L.at<uint8_t>(s_eff), e->stream));
    CK(L.out(s_st, st));
    CK(L.out(s_rep, replies));
    CK(L.out(s_to, reply_to));
    CK(L.out(s_eff, effect));
    return finish(e);
}

static size_t accept_reply_frame(const mpx_engine* e) {
    return e->cfg.mode == MPX_MODE_MIN ? MPX_ACCEPT_REPLY_FRAME_MIN : MPX_ACCEPT_REPLY_FRAME_CLASSIC;
}

int mpx_encode_accept_replies_reserve(mpx_engine* e, size_t max_n) {
    if (!e) return MPX_E_INVAL;
    CK(reply_limit(e, max_n));
    return reserve(e, e->are_work, mpx::accept_replies_work_bytes(max_n));
}

int mpx_encode_accept_replies_dev(mpx_engine* e, const mpx_accept_reply* d_replies,
                                  const int32_t* d_reply_to, size_t n, uint32_t n_dest,
                                  uint8_t* d_out, uint64_t* d_dest_off, void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!n_dest || n_dest > MPX_MAX_REPLICAS || !d_dest_off ||
        (n && (!d_replies || !d_reply_to || !d_out)))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(reply_limit(e, n));
    // (an empty call uses no scratch)
    CK(reserved(e, e->are_work, n ? mpx::accept_replies_work_bytes(n) : 0,
                "mpx_encode_accept_replies_dev", "mpx_encode_accept_replies_reserve(n)"));
    HIPCHK(e, mpx::launch_encode_accept_replies(e->cfg.mode, d_replies, d_reply_to, n, n_dest,
                                                d_out, d_dest_off, e->are_work.p,
                                                e->are_work.cap, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_encode_accept_replies(mpx_engine* e, const mpx_accept_reply* replies,
                              const int32_t* reply_to, size_t n, uint32_t n_dest, uint8_t* out,
                              uint64_t* dest_off) {
    if (!e) return MPX_E_INVAL;
    if (!n_dest || n_dest > MPX_MAX_REPLICAS || !dest_off || (n && (!replies || !reply_to || !out)))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(reply_limit(e, n));
    const size_t frame = accept_reply_frame(e);
    CK(begin(e));
    if (n) GROW(e, e->are_work, mpx::accept_replies_work_bytes(n));
    Stage L(e);
    const Slot s_rep = L.add(n * sizeof(mpx_accept_reply)), s_to = L.add(n * sizeof(int32_t)),
               s_out = L.add(n * frame), s_off = L.add(((size_t)n_dest + 1) * sizeof(uint64_t));
    CK(L.commit());
    CK(L.in(s_rep, replies));
    CK(L.in(s_to, reply_to));
    CK(mpx_encode_accept_replies_dev(e, L.at<mpx_accept_reply>(s_rep), L.at<int32_t>(s_to), n,
                                     n_dest, L.at<uint8_t>(s_out), L.at<uint64_t>(s_off),
                                     e->stream));
    CK(L.out(s_off, dest_off));
    const int rc = finish(e);
    if (rc == MPX_E_INVAL) return fail(e, MPX_E_INVAL, "a reply names a destination >= n_dest");
    if (rc) return rc;
    // the frames written: skipped slots leave the rest of out untouched
    const uint64_t total = dest_off[n_dest];
    if (total > n * frame) return fail(e, MPX_E_HIP, "mpx_encode_accept_replies: bad offsets");
    CK(L.out(s_out, out, total));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MPX_OK;
}

// ---- the proposer side: handlePropose and the Accept bytes -----------------------------------
namespace {
// what the host and _dev forms of the Accept encoder check alike
int accept_batch_args(mpx_engine* e, const mpx_accept_batch* b, const void* out, size_t out_cap,
                      const void* dest_off) {
    if (!b || !dest_off || (out_cap && !out) || (b->n_sends && (!b->sends || !b->groups)))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(propose_shape(e, b->n_groups, b->n_groups * (size_t)b->ipg, b->ipg));
    if (b->n_sends >= (1ull << 32))
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 sends per call");
    if (b->n_sends && !b->n_groups) return fail(e, MPX_E_INVAL, "sends without a window");
    if (e->cfg.mode == MPX_MODE_MIN && b->n_sends &&
        (!b->peer_commits || !b->log_recs || !b->log_cmd_off))
        return fail(e, MPX_E_INVAL, "MIN needs peer_commits and the log");
    return MPX_OK;
}
}  // namespace

int mpx_propose_handle_dev(mpx_engine* e, mpx_proposer_group* d_groups, size_t n_groups,
                           const uint64_t* d_prop_off, const uint64_t* d_send_off,
                           mpx_acceptor_state* d_st, mpx_inst_state* d_lb, size_t n_inst,
                           int32_t inst_base, uint32_t ipg, mpx_accept_send* d_sends,
                           void* stream) {
    if (!e) return MPX_E_INVAL;
    if (n_groups && (!d_groups || !d_prop_off || !d_send_off || !d_st || !d_sends))
        return fail(e, MPX_E_INVAL, "null argument");
    CK(propose_shape(e, n_groups, n_inst, ipg));
    HIPCHK(e, mpx::launch_propose_handle(e->cfg.mode, d_groups, n_groups, d_prop_off, d_send_off,
                                         d_st, d_lb, n_inst, inst_base, ipg, e->cfg.n_replicas,
                                         d_sends, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_propose_handle(mpx_engine* e, mpx_proposer_group* groups, size_t n_groups,
                       const uint64_t* prop_off, mpx_acceptor_state* st, mpx_inst_state* lb,
                       size_t n_inst, int32_t inst_base, uint32_t ipg, uint64_t* send_off,
                       mpx_accept_send* sends, size_t sends_cap) {
    if (!e) return MPX_E_INVAL;
    if (!send_off || (n_groups && (!groups || !prop_off || !st)))
        return fail(e, MPX_E_INVAL, "null argument");
    CK(propose_shape(e, n_groups, n_inst, ipg));
    send_off[0] = 0;
    for (size_t g = 0; g < n_groups; ++g) {
        if (prop_off[g] > prop_off[g + 1])
            return fail(e, MPX_E_INVAL, "prop_off must be non-decreasing");
        const uint64_t n_g = prop_off[g + 1] - prop_off[g];
        send_off[g + 1] = send_off[g] + (n_g + MPX_PROPOSE_MAX_BATCH - 1) / MPX_PROPOSE_MAX_BATCH;
    }
    const uint64_t n_sends = send_off[n_groups];
    if (n_sends > sends_cap || (n_sends && !sends))
        return fail(e, MPX_E_INVAL, "sends_cap is smaller than send_off[n_groups]");
    const int32_t N = e->cfg.n_replicas;
    for (size_t g = 0; g < n_groups; ++g) {  // a leader whose crtInstance is outside its window
        const mpx_proposer_group& G = groups[g];
        const bool leads = G.leader == G.self_id &&
                           (e->cfg.mode != MPX_MODE_MIN || G.prepare_oks > (N >> 1));
        const int64_t first = (int64_t)inst_base + (int64_t)g * ipg;
        if (leads && prop_off[g + 1] > prop_off[g] &&
            (G.crt_instance < first || G.crt_instance >= first + (int64_t)ipg))
            return fail(e, MPX_E_NIL_INSTANCE, "crt_instance is outside its group's window");
    }
    CK(begin(e));
    Stage L(e);
    const Slot s_grp = L.add(n_groups * sizeof(mpx_proposer_group)),
               s_poff = L.add(n_groups ? (n_groups + 1) * 8 : 0),
               s_soff = L.add(n_groups ? (n_groups + 1) * 8 : 0),
               s_st = L.add(n_inst * sizeof(mpx_acceptor_state)),
               s_lb = L.add(lb ? n_inst * sizeof(mpx_inst_state) : 0),
               s_snd = L.add(n_sends * sizeof(mpx_accept_send));
    CK(L.commit());
    CK(L.in(s_grp, groups));
    CK(L.in(s_poff, prop_off));
    CK(L.in(s_soff, send_off));
    CK(L.in(s_st, st));
    if (lb) CK(L.in(s_lb, lb));
    CK(mpx_propose_handle_dev(e, L.at<mpx_proposer_group>(s_grp), n_groups,
                              L.at<uint64_t>(s_poff), L.at<uint64_t>(s_soff),
                              L.at<mpx_acceptor_state>(s_st), L.at<mpx_inst_state>(s_lb, lb),
                              n_inst, inst_base, ipg, L.at<mpx_accept_send>(s_snd), e->stream));
    CK(L.out(s_grp, groups));
    CK(L.out(s_st, st));
    if (lb) CK(L.out(s_lb, lb));
    CK(L.out(s_snd, sends));
    return finish(e);
}

int mpx_encode_accepts_reserve(mpx_engine* e, size_t max_sends, size_t max_n_inst,
                               size_t max_log_cmds) {
    if (!e) return MPX_E_INVAL;
    (void)max_log_cmds;  // (the built form keeps offsets only, no catch-up bytes)
    if (max_sends >= (1ull << 32) || max_n_inst > (1ull << 32))
        return fail(e, MPX_E_UNSUPPORTED, "at most 2^32-1 sends over 2^32 instances per call");
    return reserve(e, e->ab_work,
                   mpx::accepts_work_bytes((uint32_t)e->cfg.n_replicas, max_sends, max_n_inst));
}

int mpx_encode_accepts_dev(mpx_engine* e, const mpx_accept_batch* b, uint8_t* d_out,
                           size_t out_cap, uint64_t* d_dest_off, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(accept_batch_args(e, b, d_out, out_cap, d_dest_off));
    const size_t n_inst = b->n_groups * (size_t)b->ipg;
    // (an empty call uses no scratch)
    CK(reserved(e, e->ab_work,
                b->n_sends ? mpx::accepts_work_bytes((uint32_t)e->cfg.n_replicas, b->n_sends, n_inst)
                           : 0,
                "mpx_encode_accepts_dev", "mpx_encode_accepts_reserve(n_sends, n_inst, m)"));
    HIPCHK(e, mpx::launch_encode_accepts(e->cfg.mode, e->cfg.n_replicas, b, d_out, out_cap,
                                         d_dest_off, e->ab_work.p, e->ab_work.cap, e->d_err,
                                         pick(e, stream)));
    return MPX_OK;
}

int mpx_encode_accepts(mpx_engine* e, const mpx_accept_batch* b, uint8_t* out, size_t out_cap,
                       uint64_t* dest_off) {
    if (!e) return MPX_E_INVAL;
    CK(accept_batch_args(e, b, out, out_cap, dest_off));
    const size_t n_inst = b->n_groups * (size_t)b->ipg;
    const bool min = e->cfg.mode == MPX_MODE_MIN;
    const int32_t N = e->cfg.n_replicas;
    const bool thrifty = (b->flags & MPX_AB_THRIFTY) != 0;
    // the device kernels trust the offsets and the ranges
    std::vector<uint32_t> nils;  // nils[i] = nil records among window records [0, i)
    if (min && b->n_sends) {
        nils.assign(n_inst + 1, 0);
        for (size_t i = 0; i < n_inst; ++i) {
            if (b->log_cmd_off[i] > b->log_cmd_off[i + 1] || b->log_cmd_off[i + 1] > b->n_log_cmds)
                return fail(e, MPX_E_INVAL, "log_cmd_off must be non-decreasing and <= n_log_cmds");
            nils[i + 1] = nils[i] + (b->log_recs[i].status == MPX_STATUS_NIL ? 1u : 0u);
        }
        if (b->n_log_cmds && (!b->log_op || !b->log_key || !b->log_val))
            return fail(e, MPX_E_INVAL, "null log command arrays");
    }
    bool nil_hit = false;
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
            if (lo <= lc && nils[lc + 1] != nils[lo]) nil_hit = true;
        }
    }
    if (nil_hit)
        return fail(e, MPX_E_NIL_INSTANCE, "a nil instance inside a catch-up range");
    CK(begin(e));
    if (b->n_sends)
        GROW(e, e->ab_work, mpx::accepts_work_bytes((uint32_t)N, b->n_sends, n_inst));
    Stage L(e);
    const size_t m = b->n_cmds, lm = min ? b->n_log_cmds : 0, li = min && b->n_sends ? n_inst : 0;
    const Slot s_snd = L.add(b->n_sends * sizeof(mpx_accept_send)),
               s_grp = L.add(b->n_sends ? b->n_groups * sizeof(mpx_proposer_group) : 0),
               s_pc = L.add(min && b->n_sends ? b->n_groups * (size_t)N * 4 : 0),
               s_op = L.add(b->cmd_op ? m : 0), s_key = L.add(b->cmd_key ? m * 8 : 0),
               s_val = L.add(b->cmd_val ? m * 8 : 0), s_lrec = L.add(li * sizeof(mpx_log_rec)),
               s_lcoff = L.add(li ? (li + 1) * 8 : 0), s_lop = L.add(b->log_op ? lm : 0),
               s_lkey = L.add(b->log_key ? lm * 8 : 0), s_lval = L.add(b->log_val ? lm * 8 : 0),
               s_out = L.add(out_cap), s_off = L.add(((size_t)N + 1) * 8);
    CK(L.commit());
    CK(L.in(s_snd, b->sends));
    CK(L.in(s_grp, b->groups));
    CK(L.in(s_pc, b->peer_commits));
    CK(L.in(s_op, b->cmd_op));
    CK(L.in(s_key, b->cmd_key));
    CK(L.in(s_val, b->cmd_val));
    CK(L.in(s_lrec, b->log_recs));
    CK(L.in(s_lcoff, b->log_cmd_off));
    CK(L.in(s_lop, b->log_op));
    CK(L.in(s_lkey, b->log_key));
    CK(L.in(s_lval, b->log_val));
    mpx_accept_batch d = *b;
    d.sends = L.at<mpx_accept_send>(s_snd);
    d.groups = L.at<mpx_proposer_group>(s_grp);
    d.peer_commits = L.at<int32_t>(s_pc);
    d.cmd_op = L.at<uint8_t>(s_op);
    d.cmd_key = L.at<int64_t>(s_key);
    d.cmd_val = L.at<int64_t>(s_val);
    d.log_recs = L.at<mpx_log_rec>(s_lrec);
    d.log_cmd_off = L.at<uint64_t>(s_lcoff);
    d.log_op = L.at<uint8_t>(s_lop);
    d.log_key = L.at<int64_t>(s_lkey);
    d.log_val = L.at<int64_t>(s_lval);
    CK(mpx_encode_accepts_dev(e, &d, L.at<uint8_t>(s_out), out_cap, L.at<uint64_t>(s_off),
                              e->stream));
    CK(L.out(s_off, dest_off));
    CK(finish(e));
    if (dest_off[N] > out_cap) return fail(e, MPX_E_INVAL, "out_cap is smaller than the frames");
    CK(L.out(s_out, out, dest_off[N]));
    return finish(e);
}

// ---- Accept / Commit / PrepareReply payloads: Unmarshal in a batch ---------------------------
namespace {
int unmarshal_args(mpx_engine* e, const void* buf, size_t len, const void* var, size_t n_var,
                   const mpx_unmarshal_out* o, const void* res) {
    if (!o || !res || (len && !buf) || (n_var && (!var || !len)))
        return fail(e, MPX_E_INVAL, "null argument");
    if ((o->accept_cap && (!o->accepts || !o->accept_last_committed)) ||
        (o->commit_cap && !o->commits) || (o->cmd_cap && (!o->op || !o->key || !o->val)) ||
        (o->log_inst_cap && !o->log_recs) ||
        (o->log_cmd_cap && (!o->log_op || !o->log_key || !o->log_val)))
        return fail(e, MPX_E_INVAL, "a capacity above 0 needs its arrays");
    CK(decode_limit(e, len));
    return record_limit(e, n_var);
}
// catch-up instances the scratch of a call on len bytes is carved for (an Instance is 9 bytes at
// least); launch_unmarshal takes the same minimum
uint64_t unmarshal_log_slots(const mpx_engine* e, size_t n_var, size_t len) {
    if (e->cfg.mode != MPX_MODE_MIN || !n_var) return 0;
    return std::min<uint64_t>(len / 9, e->um_log_cap);
}
// bytes from the code byte to V(len(Command))
uint32_t var_header(int mode, uint32_t code) {
    if (mode == MPX_MODE_MIN)
        return code == MPX_PEER_ACCEPT ? 17 : code == MPX_PEER_COMMIT ? 13 : 18;
    return code == MPX_PEER_PREPARE_REPLY ? 10 : 13;
}
}  // namespace

int mpx_unmarshal_frames_reserve(mpx_engine* e, size_t max_var, size_t max_log_inst) {
    if (!e) return MPX_E_INVAL;
    CK(record_limit(e, max_var));
    CK(record_limit(e, max_log_inst));
    e->um_var_cap = std::max(e->um_var_cap, max_var);
    e->um_log_cap = std::max(e->um_log_cap, max_log_inst);
    return reserve(e, e->um_work, mpx::unmarshal_work_bytes(e->um_var_cap, e->um_log_cap));
}

int mpx_unmarshal_frames_dev(mpx_engine* e, const uint8_t* d_buf, size_t len,
                             const mpx_var_frame* d_var, size_t n_var, const uint64_t* d_n_var,
                             const mpx_unmarshal_out* out, mpx_unmarshal_result* d_res,
                             void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(unmarshal_args(e, d_buf, len, d_var, n_var, out, d_res));
    if ((uintptr_t)d_buf & 15)
        return fail(e, MPX_E_INVAL, "mpx_unmarshal_frames_dev: d_buf must be 16-byte aligned");
    CK(reserved(e, e->um_work,
                mpx::unmarshal_work_bytes(n_var, unmarshal_log_slots(e, n_var, len)),
                "mpx_unmarshal_frames_dev", "mpx_unmarshal_frames_reserve(n_var, n_log_inst)"));
    HIPCHK(e, mpx::launch_unmarshal(e->cfg.mode, d_buf, len, d_var, n_var, d_n_var, out, d_res,
                                    e->um_log_cap, e->um_work.p, e->um_work.cap, e->d_err,
                                    pick(e, stream)));
    return MPX_OK;
}

int mpx_unmarshal_frames(mpx_engine* e, const uint8_t* buf, size_t len, const mpx_var_frame* var,
                         size_t n_var, const mpx_unmarshal_out* out, mpx_unmarshal_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(unmarshal_args(e, buf, len, var, n_var, out, res));
    // the device kernels trust the frames
    const bool min = e->cfg.mode == MPX_MODE_MIN;
    uint64_t prev_end = 0, n_acc = 0, n_com = 0, n_cmds = 0, n_log = 0;
    for (size_t i = 0; i < n_var; ++i) {
        const mpx_var_frame& f = var[i];
        if (f.code != MPX_PEER_ACCEPT && f.code != MPX_PEER_COMMIT &&
            f.code != MPX_PEER_PREPARE_REPLY)
            return fail(e, MPX_E_INVAL, "a frame's code is not Accept, Commit or PrepareReply");
        const uint64_t end = (uint64_t)f.offset + f.length;
        if (!f.length || f.offset >= len || end > len)
            return fail(e, MPX_E_INVAL, "a frame lies outside [0, len)");
        if (f.offset < prev_end)
            return fail(e, MPX_E_INVAL, "frames overlap or are not ascending by offset");
        prev_end = end;
        const uint64_t cmds_end = (uint64_t)f.cmds_off + 17ull * f.n_cmds;
        if (f.cmds_off < (uint64_t)f.offset + var_header(e->cfg.mode, f.code) || cmds_end > end)
            return fail(e, MPX_E_INVAL, "a frame's Command slice lies outside the frame");
        if (f.log_off < cmds_end || f.log_off > end)
            return fail(e, MPX_E_INVAL, "a frame's log_off lies outside the frame");
        const bool has_log = min && f.code != MPX_PEER_COMMIT;
        if (has_log ? f.n_log > (end - f.log_off) / 9 : f.n_log != 0)
            return fail(e, MPX_E_INVAL, "a frame's n_log does not fit the frame");
        n_acc += f.code == MPX_PEER_ACCEPT;
        n_com += f.code == MPX_PEER_COMMIT;
        n_cmds += f.n_cmds;
        n_log += f.n_log;
    }
    CK(begin(e));
    e->um_log_cap = std::max<size_t>(e->um_log_cap, n_log);
    GROW(e, e->um_work, mpx::unmarshal_work_bytes(n_var, unmarshal_log_slots(e, n_var, len)));
    const size_t na = std::min<uint64_t>(out->accept_cap, n_acc),
                 nc = std::min<uint64_t>(out->commit_cap, n_com),
                 m = std::min<uint64_t>(out->cmd_cap, n_cmds),
                 li = std::min<uint64_t>(out->log_inst_cap, n_log),
                 lm = n_log ? std::min<uint64_t>(out->log_cmd_cap, len / 17) : 0;
    Stage L(e);
    const Slot s_buf = L.add(len), s_var = L.add(n_var * sizeof(mpx_var_frame)),
               s_acc = L.add(na * sizeof(mpx_accept_msg)), s_alc = L.add(na * 4),
               s_com = L.add(nc * sizeof(mpx_accept_msg)),
               s_coff = L.add(out->cmd_off ? (n_var + 1) * 8 : 0), s_op = L.add(m),
               s_key = L.add(m * 8), s_val = L.add(m * 8),
               s_loff = L.add(out->log_inst_off ? (n_var + 1) * 8 : 0),
               s_lrec = L.add(li * sizeof(mpx_log_rec)),
               s_lcoff = L.add(out->log_cmd_off ? (li + 1) * 8 : 0), s_lop = L.add(lm),
               s_lkey = L.add(lm * 8), s_lval = L.add(lm * 8),
               s_res = L.add(sizeof(mpx_unmarshal_result));
    CK(L.commit());
    CK(L.in(s_buf, buf));
    CK(L.in(s_var, var));
    mpx_unmarshal_out d{};
    d.accepts = L.at<mpx_accept_msg>(s_acc);
    d.accept_last_committed = L.at<int32_t>(s_alc);
    d.accept_cap = na;
    d.commits = L.at<mpx_accept_msg>(s_com);
    d.commit_cap = nc;
    d.cmd_off = L.at<uint64_t>(s_coff, out->cmd_off);
    d.op = L.at<uint8_t>(s_op);
    d.key = L.at<int64_t>(s_key);
    d.val = L.at<int64_t>(s_val);
    d.cmd_cap = m;
    d.log_inst_off = L.at<uint64_t>(s_loff, out->log_inst_off);
    d.log_recs = L.at<mpx_log_rec>(s_lrec);
    d.log_cmd_off = L.at<uint64_t>(s_lcoff, out->log_cmd_off);
    d.log_inst_cap = li;
    d.log_op = L.at<uint8_t>(s_lop);
    d.log_key = L.at<int64_t>(s_lkey);
    d.log_val = L.at<int64_t>(s_lval);
    d.log_cmd_cap = lm;
    CK(mpx_unmarshal_frames_dev(e, L.at<uint8_t>(s_buf), len, L.at<mpx_var_frame>(s_var), n_var,
                                nullptr, &d, L.at<mpx_unmarshal_result>(s_res), e->stream));
    CK(L.out(s_res, res));
    const int rc = finish(e);
    if (rc == MPX_E_INVAL)
        return fail(e, MPX_E_INVAL, "a CatchUpLog does not end at its frame's end");
    if (rc) return rc;
    const size_t lc = std::min<uint64_t>(res->n_log_cmds, lm);
    CK(L.out(s_acc, out->accepts, na * sizeof(mpx_accept_msg)));
    CK(L.out(s_alc, out->accept_last_committed, na * 4));
    CK(L.out(s_com, out->commits, nc * sizeof(mpx_accept_msg)));
    if (out->cmd_off) CK(L.out(s_coff, out->cmd_off));
    CK(L.out(s_op, out->op, m));
    CK(L.out(s_key, out->key, m * 8));
    CK(L.out(s_val, out->val, m * 8));
    if (out->log_inst_off) CK(L.out(s_loff, out->log_inst_off));
    CK(L.out(s_lrec, out->log_recs, li * sizeof(mpx_log_rec)));
    if (out->log_cmd_off) CK(L.out(s_lcoff, out->log_cmd_off));
    CK(L.out(s_lop, out->log_op, lc));
    CK(L.out(s_lkey, out->log_key, lc * 8));
    CK(L.out(s_lval, out->log_val, lc * 8));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MPX_OK;
}

// ---- the commit side: handleCommit[Short], the Commit bytes, CommitShort records --------------
namespace {
int commit_batch_args(mpx_engine* e, const mpx_commit_batch* b, const void* out, size_t out_cap,
                      const void* dest_off) {
    if (!b || !dest_off || (out_cap && !out) || (b->n_sends && (!b->sends || !b->groups)))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    if (b->n_sends || b->n_groups)
        CK(window_limits(e, b->n_sends, b->n_groups * (size_t)b->ipg, b->n_groups, b->ipg));
    return MPX_OK;
}
int gather_args(mpx_engine* e, const void* buf, size_t len, const void* other, size_t n_other,
                const void* msgs, const void* count, const void* fidx, size_t cap,
                const void* n_shorts) {
    if (!n_shorts || (len && !buf) || (n_other && (!other || !len)) ||
        (cap && (!msgs || !count || !fidx)))
        return fail(e, MPX_E_INVAL, "null argument");
    CK(decode_limit(e, len));
    return record_limit(e, n_other);
}
}  // namespace

int mpx_commit_handle_dev(mpx_engine* e, const mpx_accept_msg* d_msgs, size_t n,
                          mpx_acceptor_state* d_st, size_t n_inst, int32_t inst_base,
                          int32_t* d_committed_upto, size_t n_groups, uint32_t ipg,
                          uint8_t* d_effect, mpx_log_rec* d_log_recs, void* stream) {
    if (!e) return MPX_E_INVAL;
    if ((n && (!d_msgs || !d_effect)) || !d_st || !d_committed_upto)
        return fail(e, MPX_E_INVAL, "null argument");
    CK(window_limits(e, n, n_inst, n_groups, ipg));
    HIPCHK(e, mpx::launch_commit_handle(d_msgs, n, d_st, n_inst, inst_base, d_committed_upto,
                                        n_groups, ipg, d_effect, d_log_recs, e->d_err,
                                        pick(e, stream)));
    return MPX_OK;
}

int mpx_commit_handle(mpx_engine* e, const mpx_accept_msg* msgs, size_t n, mpx_acceptor_state* st,
                      size_t n_inst, int32_t inst_base, int32_t* committed_upto, size_t n_groups,
                      uint32_t ipg, uint8_t* effect, mpx_log_rec* log_recs) {
    if (!e) return MPX_E_INVAL;
    if ((n && (!msgs || !effect)) || !st || !committed_upto)
        return fail(e, MPX_E_INVAL, "null argument");
    CK(window_limits(e, n, n_inst, n_groups, ipg));
    for (size_t g = 0; g < n_groups; ++g) {
        const int64_t first = (int64_t)inst_base + (int64_t)(g * ipg);
        if (committed_upto[g] < first - 1 || committed_upto[g] > first + (int64_t)ipg - 1)
            return fail(e, MPX_E_INVAL, "committed_upto[g] outside [first_g - 1, first_g + ipg - 1]");
    }
    CK(begin(e));
    Stage L(e);
    const Slot s_msg = L.add(n * sizeof(mpx_accept_msg)),
               s_st = L.add(n_inst * sizeof(mpx_acceptor_state)),
               s_cu = L.add(n_groups * sizeof(int32_t)), s_eff = L.add(n),
               s_log = L.add(log_recs ? n * sizeof(mpx_log_rec) : 0);
    CK(L.commit());
    CK(L.in(s_msg, msgs));
    CK(L.in(s_st, st));
    CK(L.in(s_cu, committed_upto));
    CK(mpx_commit_handle_dev(e, L.at<mpx_accept_msg>(s_msg), n, L.at<mpx_acceptor_state>(s_st),
                             n_inst, inst_base, L.at<int32_t>(s_cu), n_groups, ipg,
                             L.at<uint8_t>(s_eff), L.at<mpx_log_rec>(s_log, log_recs), e->stream));
    CK(L.out(s_st, st));
    CK(L.out(s_cu, committed_upto));
    CK(L.out(s_eff, effect));
    if (log_recs) CK(L.out(s_log, log_recs));
    return finish(e);
}

int mpx_encode_commits_reserve(mpx_engine* e, size_t max_sends, size_t max_other) {
    if (!e) return MPX_E_INVAL;
    CK(record_limit(e, max_sends));
    CK(record_limit(e, max_other));
    e->cm_send_cap = std::max(e->cm_send_cap, max_sends);
    e->cm_other_cap = std::max(e->cm_other_cap, max_other);
    return reserve(e, e->cm_work, mpx::commits_work_bytes((uint32_t)e->cfg.n_replicas,
                                                          e->cm_send_cap, e->cm_other_cap));
}

int mpx_encode_commits_dev(mpx_engine* e, const mpx_commit_batch* b, uint8_t* d_out, size_t out_cap,
                           uint64_t* d_dest_off, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(commit_batch_args(e, b, d_out, out_cap, d_dest_off));
    // (an empty call uses no scratch)
    CK(reserved(e, e->cm_work,
                b->n_sends ? mpx::commits_work_bytes((uint32_t)e->cfg.n_replicas, b->n_sends, 0) : 0,
                "mpx_encode_commits_dev", "mpx_encode_commits_reserve(n_sends, 0)"));
    HIPCHK(e, mpx::launch_encode_commits(e->cfg.n_replicas, b, d_out, out_cap, d_dest_off,
                                         e->cm_work.p, e->cm_work.cap, e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_encode_commits(mpx_engine* e, const mpx_commit_batch* b, uint8_t* out, size_t out_cap,
                       uint64_t* dest_off) {
    if (!e) return MPX_E_INVAL;
    CK(commit_batch_args(e, b, out, out_cap, dest_off));
    const int32_t N = e->cfg.n_replicas;
    const size_t n_inst = b->n_groups * (size_t)b->ipg;
    // the device kernels report these through the error word; here they answer before any launch
    for (size_t s = 0; s < b->n_sends; ++s) {
        const mpx_commit_send& x = b->sends[s];
        if (!(x.flags & MPX_CS_SEND)) continue;
        const int64_t idx = (int64_t)x.instance - b->inst_base;
        if (idx < 0 || (uint64_t)idx >= n_inst)
            return fail(e, MPX_E_INVAL, "a send names an instance outside the window");
        if (x.first_cmd > b->n_cmds || x.n_cmds > b->n_cmds - x.first_cmd ||
            (x.n_cmds && (!b->cmd_op || !b->cmd_key || !b->cmd_val)))
            return fail(e, MPX_E_INVAL, "a send's commands are outside the command arrays");
        const int32_t self = b->groups[(size_t)idx / b->ipg].self_id;
        if (self < 0 || self >= N) return fail(e, MPX_E_INVAL, "self_id outside [0, N)");
    }
    CK(begin(e));
    if (b->n_sends) GROW(e, e->cm_work, mpx::commits_work_bytes((uint32_t)N, b->n_sends, 0));
    Stage L(e);
    const size_t m = b->n_cmds;
    const Slot s_snd = L.add(b->n_sends * sizeof(mpx_commit_send)),
               s_grp = L.add(b->n_sends ? b->n_groups * sizeof(mpx_proposer_group) : 0),
               s_op = L.add(b->cmd_op ? m : 0), s_key = L.add(b->cmd_key ? m * 8 : 0),
               s_val = L.add(b->cmd_val ? m * 8 : 0), s_out = L.add(out_cap),
               s_off = L.add(((size_t)N + 1) * 8);
    CK(L.commit());
    CK(L.in(s_snd, b->sends));
    CK(L.in(s_grp, b->groups));
    CK(L.in(s_op, b->cmd_op));
    CK(L.in(s_key, b->cmd_key));
    CK(L.in(s_val, b->cmd_val));
    mpx_commit_batch d = *b;
    d.sends = L.at<mpx_commit_send>(s_snd);
    d.groups = L.at<mpx_proposer_group>(s_grp);
    d.cmd_op = L.at<uint8_t>(s_op);
    d.cmd_key = L.at<int64_t>(s_key);
    d.cmd_val = L.at<int64_t>(s_val);
    CK(mpx_encode_commits_dev(e, &d, L.at<uint8_t>(s_out), out_cap, L.at<uint64_t>(s_off),
                              e->stream));
    CK(L.out(s_off, dest_off));
    CK(finish(e));
    if (dest_off[N] > out_cap) return fail(e, MPX_E_INVAL, "out_cap is smaller than the frames");
    CK(L.out(s_out, out, dest_off[N]));
    return finish(e);
}

int mpx_gather_commit_shorts_dev(mpx_engine* e, const uint8_t* d_buf, size_t len,
                                 const mpx_peer_frame* d_other, size_t n_other,
                                 const uint64_t* d_n_other, mpx_accept_msg* d_msgs, int32_t* d_count,
                                 uint32_t* d_frame_index, size_t cap, uint64_t* d_n_shorts,
                                 void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(gather_args(e, d_buf, len, d_other, n_other, d_msgs, d_count, d_frame_index, cap,
                   d_n_shorts));
    if ((uintptr_t)d_buf & 15)
        return fail(e, MPX_E_INVAL, "mpx_gather_commit_shorts_dev: d_buf must be 16-byte aligned");
    CK(reserved(e, e->cm_work, n_other ? mpx::commits_work_bytes(1, 0, n_other) : 0,
                "mpx_gather_commit_shorts_dev", "mpx_encode_commits_reserve(0, n_other)"));
    HIPCHK(e, mpx::launch_gather_commit_shorts(d_buf, len, d_other, n_other, d_n_other, d_msgs,
                                               d_count, d_frame_index, cap, d_n_shorts,
                                               e->cm_work.p, e->cm_work.cap, e->d_err,
                                               pick(e, stream)));
    return MPX_OK;
}

int mpx_gather_commit_shorts(mpx_engine* e, const uint8_t* buf, size_t len,
                             const mpx_peer_frame* other, size_t n_other, mpx_accept_msg* msgs,
                             int32_t* count, uint32_t* frame_index, size_t cap, uint64_t* n_shorts) {
    if (!e) return MPX_E_INVAL;
    CK(gather_args(e, buf, len, other, n_other, msgs, count, frame_index, cap, n_shorts));
    uint64_t want = 0;  // the device kernel reports a frame outside the buffer and skips it
    for (size_t i = 0; i < n_other; ++i) {
        if (other[i].code != MPX_PEER_COMMIT_SHORT) continue;
        if ((uint64_t)other[i].offset + MPX_COMMIT_SHORT_FRAME > len)
            return fail(e, MPX_E_INVAL, "a CommitShort frame lies outside [0, len)");
        ++want;
    }
    CK(begin(e));
    if (n_other) GROW(e, e->cm_work, mpx::commits_work_bytes(1, 0, n_other));
    const size_t k = std::min<uint64_t>(cap, want);
    Stage L(e);
    const Slot s_buf = L.add(len), s_oth = L.add(n_other * sizeof(mpx_peer_frame)),
               s_msg = L.add(k * sizeof(mpx_accept_msg)), s_cnt = L.add(k * 4),
               s_idx = L.add(k * 4), s_n = L.add(sizeof(uint64_t));
    CK(L.commit());
    CK(L.in(s_buf, buf));
    CK(L.in(s_oth, other));
    CK(mpx_gather_commit_shorts_dev(e, L.at<uint8_t>(s_buf), len, L.at<mpx_peer_frame>(s_oth),
                                    n_other, nullptr, L.at<mpx_accept_msg>(s_msg),
                                    L.at<int32_t>(s_cnt), L.at<uint32_t>(s_idx), k,
                                    L.at<uint64_t>(s_n), e->stream));
    CK(L.out(s_n, n_shorts));
    CK(L.out(s_msg, msgs));
    CK(L.out(s_cnt, count));
    CK(L.out(s_idx, frame_index));
    return finish(e);
}

// ---- §8(f) ranks 3/4: instance-log encoding -------------------------------------------------
size_t mpx_encode_log_bound(size_t n, size_t m) { return (size_t)mpx::logenc_max_bytes(n, m); }

static int log_format(mpx_engine* e, int format) {
    if (format != MPX_LOG_CATCHUP && format != MPX_LOG_DURABLE)
        return fail(e, MPX_E_INVAL, "unknown log format");
    return MPX_OK;
}

int mpx_encode_log_reserve(mpx_engine* e, size_t max_n, size_t max_m) {
    if (!e) return MPX_E_INVAL;
    return reserve(e, e->log_work, mpx::logenc_work_bytes(max_n, max_m));
}

int mpx_encode_log_dev(mpx_engine* e, int format, const mpx_log_rec* d_recs, size_t n,
                       const uint64_t* d_cmd_off, const uint8_t* d_op, const int64_t* d_key,
                       const int64_t* d_val, size_t m, uint8_t* d_out, uint64_t* d_rec_off,
                       void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!d_rec_off || (n && (!d_recs || !d_cmd_off || !d_out)) || (m && (!d_op || !d_key || !d_val)))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(log_format(e, format));
    CK(reserved(e, e->log_work, mpx::logenc_work_bytes(n, m), "mpx_encode_log_dev",
                "mpx_encode_log_reserve(n, m)"));
    HIPCHK(e, mpx::launch_encode_log(format, d_recs, n, d_cmd_off, d_op, d_key, d_val, m, d_out,
                                     d_rec_off, e->log_work.p, e->log_work.cap, pick(e, stream)));
    return MPX_OK;
}

int mpx_encode_log(mpx_engine* e, int format, const mpx_log_rec* recs, size_t n,
                   const uint64_t* cmd_off, const uint8_t* op, const int64_t* key,
                   const int64_t* val, size_t m, uint8_t* out, size_t out_cap,
                   uint64_t* rec_off) {
    if (!e) return MPX_E_INVAL;
    if (!rec_off || (n && (!recs || !cmd_off)) || (m && (!op || !key || !val)) || (out_cap && !out))
        return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(log_format(e, format));
    for (size_t i = 0; i < n; ++i)  // the device kernels trust the offsets
        if (cmd_off[i] > cmd_off[i + 1] || cmd_off[i + 1] > m)
            return fail(e, MPX_E_INVAL, "cmd_off must be non-decreasing and <= m");
    const size_t bound = mpx::logenc_max_bytes(n, m);
    CK(begin(e));
    GROW(e, e->log_work, mpx::logenc_work_bytes(n, m));
    Stage L(e);
    // (cmd_off may be null when n == 0: nothing of it is read then)
    const Slot s_rec = L.add(n * sizeof(mpx_log_rec)), s_coff = L.add(n ? (n + 1) * 8 : 0),
               s_op = L.add(m), s_key = L.add(m * 8), s_val = L.add(m * 8), s_out = L.add(bound),
               s_roff = L.add((n + 1) * 8);
    CK(L.commit());
    CK(L.in(s_rec, recs));
    CK(L.in(s_coff, cmd_off));
    CK(L.in(s_op, op));
    CK(L.in(s_key, key));
    CK(L.in(s_val, val));
    CK(mpx_encode_log_dev(e, format, L.at<mpx_log_rec>(s_rec), n, L.at<uint64_t>(s_coff),
                          L.at<uint8_t>(s_op), L.at<int64_t>(s_key), L.at<int64_t>(s_val), m,
                          L.at<uint8_t>(s_out), L.at<uint64_t>(s_roff), e->stream));
    CK(L.out(s_roff, rec_off));
    CK(finish(e));
    if (rec_off[n] > out_cap) return fail(e, MPX_E_INVAL, "out_cap is smaller than the encoding");
    CK(L.out(s_out, out, rec_off[n]));
    return finish(e);
}

// ---- §8(f) rank 3, read side: durable-log replay --------------------------------------------
namespace {
// shared argument checks of both forms; *n_out = number of records
int replay_args(mpx_engine* e, size_t len, int32_t inst_cap, int32_t rec_base, size_t* n_out) {
    if (inst_cap < 0) return fail(e, MPX_E_INVAL, "inst_cap must be >= 0");
    if (rec_base < 0) return fail(e, MPX_E_INVAL, "rec_base must be >= 0");
    if (len % MPX_DURABLE_REC_BYTES)
        return fail(e, MPX_E_INVAL, "durable log ends in a partial record");
    const size_t n = len / MPX_DURABLE_REC_BYTES;
    if ((uint64_t)rec_base + n > (uint64_t)INT32_MAX)
        return fail(e, MPX_E_UNSUPPORTED, "rec_base + records must stay below 2^31");
    // every record indexes instanceSpace[instNo]: with no instance space, the first one panics
    if (n && inst_cap == 0)
        return fail(e, MPX_E_NIL_INSTANCE, "a durable record's instNo is outside [0, inst_cap)");
    *n_out = n;
    return MPX_OK;
}
}  // namespace

int mpx_replay_durable_dev(mpx_engine* e, const uint8_t* d_log, size_t len, int32_t inst_cap,
                           int32_t rec_base, mpx_log_rec* d_recs, uint8_t* d_op, int64_t* d_key,
                           int64_t* d_val, int32_t* d_last_rec, int32_t* d_scalars, void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!d_scalars) return fail(e, MPX_E_INVAL, "null d_scalars");
    size_t n = 0;
    CK(replay_args(e, len, inst_cap, rec_base, &n));
    if (n && (!d_log || !d_recs || !d_op || !d_key || !d_val || !d_last_rec))
        return fail(e, MPX_E_INVAL, "null device buffer");
    if ((uintptr_t)d_log % 16)
        return fail(e, MPX_E_INVAL, "d_log must be 16-byte aligned (the tiles load 16 B vectors)");
    HIPCHK(e, mpx::launch_replay_durable(d_log, n, inst_cap, rec_base, d_recs, d_op, d_key, d_val,
                                         d_last_rec, d_scalars, e->d_err, e->replay_work.p,
                                         e->replay_work.cap, pick(e, stream)));
    return MPX_OK;
}

int mpx_replay_durable_reserve(mpx_engine* e, size_t max_len, int32_t inst_cap) {
    if (!e) return MPX_E_INVAL;
    if (inst_cap < 0) return fail(e, MPX_E_INVAL, "inst_cap must be >= 0");
    const size_t n = max_len / MPX_DURABLE_REC_BYTES;
    return reserve(e, e->replay_work, mpx::replay_work_bytes(n, inst_cap));
}

int mpx_replay_durable(mpx_engine* e, const uint8_t* log, size_t len, int32_t inst_cap,
                       int32_t rec_base, mpx_log_rec* recs, uint8_t* op, int64_t* key, int64_t* val,
                       int32_t* last_rec, int32_t* scalars) {
    if (!e) return MPX_E_INVAL;
    if (!scalars || (inst_cap > 0 && !last_rec)) return fail(e, MPX_E_INVAL, "null argument");
    size_t n = 0;
    CK(replay_args(e, len, inst_cap, rec_base, &n));
    if (n && (!log || !recs || !op || !key || !val)) return fail(e, MPX_E_INVAL, "null argument");
    CK(begin(e));
    GROW(e, e->replay_work, mpx::replay_work_bytes(n, inst_cap));
    Stage L(e);
    const Slot s_log = L.add(len), s_rec = L.add(n * sizeof(mpx_log_rec)), s_op = L.add(n),
               s_key = L.add(n * 8), s_val = L.add(n * 8), s_last = L.add((size_t)inst_cap * 4),
               s_sc = L.add(2 * sizeof(int32_t));
    CK(L.commit());
    CK(L.in(s_log, log));
    CK(L.in(s_last, last_rec));
    CK(L.in(s_sc, scalars));
    if (n)  // (an empty log still round-trips last_rec and scalars)
        CK(mpx_replay_durable_dev(e, L.at<uint8_t>(s_log), len, inst_cap, rec_base,
                                  L.at<mpx_log_rec>(s_rec), L.at<uint8_t>(s_op),
                                  L.at<int64_t>(s_key), L.at<int64_t>(s_val),
                                  L.at<int32_t>(s_last), L.at<int32_t>(s_sc), e->stream));
    CK(L.out(s_rec, recs));
    CK(L.out(s_op, op));
    CK(L.out(s_key, key));
    CK(L.out(s_val, val));
    CK(L.out(s_last, last_rec));
    CK(L.out(s_sc, scalars));
    int rc = finish(e);
    if (rc == MPX_E_NIL_INSTANCE)
        return fail(e, rc, "a durable record's instNo is outside [0, inst_cap)");
    return rc;
}

// ---- diagnostics (test-only; never called on the product path) -----------------------------
int mpx_debug_kv_set_epoch(mpx_engine* e, uint32_t epoch) {
    if (!e) return MPX_E_INVAL;
    if (epoch < 1 || epoch >= mpx::kKvEpochMax)
        return fail(e, MPX_E_INVAL, "epoch must lie in [1, 2^30)");
    CK(begin(e));
    CK(ensure_kv(e));
    HIPCHK(e, hipMemcpyAsync(e->kv.epoch, &epoch, sizeof epoch, hipMemcpyHostToDevice, e->stream));
    return finish(e);
}

int mpx_debug_kv_set_small_tag(mpx_engine* e, uint32_t tag) {
    if (!e) return MPX_E_INVAL;
    if (tag >= mpx::kSmallTagMax - 1) return fail(e, MPX_E_INVAL, "tag must lie in [0, 2^18 - 1)");
    CK(begin(e));
    CK(ensure_kv(e));
    // the heads carry the tags of earlier calls: a tag moved backwards would let a later call
    // follow one of them, so every head is cleared with the move (as at the wrap)
    HIPCHK(e, hipMemsetAsync(e->kv.lhead, 0, (e->kv.cap + 1) * 4, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->kv.probe + mpx::kSmallCtl + 1, &tag, sizeof tag,
                             hipMemcpyHostToDevice, e->stream));
    return finish(e);
}

int mpx_debug_kv_state(mpx_engine* e, uint32_t* state, size_t cap, size_t* n) {
    if (!e) return MPX_E_INVAL;
    if (!n || (cap && !state)) return fail(e, MPX_E_INVAL, "null or invalid argument");
    CK(begin(e));
    CK(ensure_kv(e));
    *n = (size_t)e->kv.cap + 1;
    CK(d2h(e, state, e->kv.state, std::min<size_t>(cap, *n) * sizeof(uint32_t)));
    return finish(e);
}

// ---- device memory, streams, events (the engine's HIP runtime) --------------------------------
int mpx_dev_alloc(mpx_engine* e, size_t bytes, void** out) {
    if (!e) return MPX_E_INVAL;
    if (!out) return fail(e, MPX_E_INVAL, "null or invalid argument");
    *out = nullptr;
    HIPCHK(e, hipSetDevice(e->device));
    if (hipMalloc(out, bytes ? bytes : 1) != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return fail(e, MPX_E_NOMEM, "device allocation of " + std::to_string(bytes) + " bytes failed");
    }
    return MPX_OK;
}

int mpx_dev_free(mpx_engine* e, void* d) {
    if (!e) return MPX_E_INVAL;
    if (!d) return MPX_OK;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipFree(d));
    return MPX_OK;
}

int mpx_memcpy_async(mpx_engine* e, void* dst, const void* src, size_t bytes, int kind,
                     void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!bytes) return MPX_OK;
    if (!dst || !src) return fail(e, MPX_E_INVAL, "null copy pointer");
    hipMemcpyKind k;
    switch (kind) {
        case MPX_COPY_H2D: k = hipMemcpyHostToDevice; break;
        case MPX_COPY_D2H: k = hipMemcpyDeviceToHost; break;
        case MPX_COPY_D2D: k = hipMemcpyDeviceToDevice; break;
        default: return fail(e, MPX_E_INVAL, "unknown copy kind");
    }
    HIPCHK(e, hipMemcpyAsync(dst, src, bytes, k, pick(e, stream)));
    return MPX_OK;
}

int mpx_memset_async(mpx_engine* e, void* d, int byte_value, size_t bytes, void* stream) {
    if (!e) return MPX_E_INVAL;
    if (!bytes) return MPX_OK;
    if (!d) return fail(e, MPX_E_INVAL, "null memset pointer");
    HIPCHK(e, hipMemsetAsync(d, byte_value, bytes, pick(e, stream)));
    return MPX_OK;
}

int mpx_stream_create(mpx_engine* e, void** out) {
    if (!e) return MPX_E_INVAL;
    if (!out) return fail(e, MPX_E_INVAL, "null or invalid argument");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = nullptr;
    HIPCHK(e, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = (void*)s;
    return MPX_OK;
}

int mpx_stream_destroy(mpx_engine* e, void* s) {
    if (!e) return MPX_E_INVAL;
    if (!s || s == (void*)e->stream) return fail(e, MPX_E_INVAL, "not a stream of mpx_stream_create");
    HIPCHK(e, hipStreamDestroy((hipStream_t)s));
    return MPX_OK;
}

int mpx_stream_synchronize(mpx_engine* e, void* s) {
    if (!e) return MPX_E_INVAL;
    HIPCHK(e, hipStreamSynchronize(pick(e, s)));
    return MPX_OK;
}

int mpx_event_create(mpx_engine* e, int timing, void** out) {
    if (!e) return MPX_E_INVAL;
    if (!out) return fail(e, MPX_E_INVAL, "null or invalid argument");
    HIPCHK(e, hipSetDevice(e->device));
    hipEvent_t ev = nullptr;
    HIPCHK(e, hipEventCreateWithFlags(&ev, timing ? hipEventDefault : hipEventDisableTiming));
    *out = (void*)ev;
    return MPX_OK;
}

int mpx_event_destroy(mpx_engine* e, void* ev) {
    if (!e) return MPX_E_INVAL;
    if (!ev) return fail(e, MPX_E_INVAL, "null or invalid argument");
    // a destroyed event never stays registered as the group step's timing hook: the pair is
    // unregistered together (the hook records both or neither)
    if ((hipEvent_t)ev == e->ev_fast0 || (hipEvent_t)ev == e->ev_fast1)
        e->ev_fast0 = e->ev_fast1 = nullptr;
    HIPCHK(e, hipEventDestroy((hipEvent_t)ev));
    return MPX_OK;
}

int mpx_event_record(mpx_engine* e, void* ev, void* s) {
    if (!e) return MPX_E_INVAL;
    if (!ev) return fail(e, MPX_E_INVAL, "null or invalid argument");
    HIPCHK(e, hipEventRecord((hipEvent_t)ev, pick(e, s)));
    return MPX_OK;
}

int mpx_stream_wait_event(mpx_engine* e, void* s, void* ev) {
    if (!e) return MPX_E_INVAL;
    if (!ev) return fail(e, MPX_E_INVAL, "null or invalid argument");
    HIPCHK(e, hipStreamWaitEvent(pick(e, s), (hipEvent_t)ev, 0));
    return MPX_OK;
}

int mpx_event_elapsed_ms(mpx_engine* e, void* ev0, void* ev1, float* ms) {
    if (!e) return MPX_E_INVAL;
    if (!ev0 || !ev1 || !ms) return fail(e, MPX_E_INVAL, "null or invalid argument");
    HIPCHK(e, hipEventElapsedTime(ms, (hipEvent_t)ev0, (hipEvent_t)ev1));
    return MPX_OK;
}

// ---- hipGraph capture ----------------------------------------------------------------------------
int mpx_graph_begin(mpx_engine* e, void* s) {
    if (!e) return MPX_E_INVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamBeginCapture(pick(e, s), hipStreamCaptureModeRelaxed));
    return MPX_OK;
}

int mpx_graph_end(mpx_engine* e, void* s, void** exec_out) {
    if (!e) return MPX_E_INVAL;
    if (!exec_out) return fail(e, MPX_E_INVAL, "null exec_out");
    *exec_out = nullptr;
    hipGraph_t g = nullptr;
    HIPCHK(e, hipStreamEndCapture(pick(e, s), &g));
    hipGraphExec_t x = nullptr;
    const hipError_t r = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (r != hipSuccess) return hip_fail(e, "hipGraphInstantiate", r);
    *exec_out = (void*)x;
    return MPX_OK;
}

int mpx_graph_launch(mpx_engine* e, void* exec, void* s) {
    if (!e) return MPX_E_INVAL;
    if (!exec) return fail(e, MPX_E_INVAL, "null graph");
    HIPCHK(e, hipGraphLaunch((hipGraphExec_t)exec, pick(e, s)));
    return MPX_OK;
}

int mpx_graph_destroy(mpx_engine* e, void* exec) {
    if (!e) return MPX_E_INVAL;
    if (!exec) return fail(e, MPX_E_INVAL, "null graph");
    HIPCHK(e, hipGraphExecDestroy((hipGraphExec_t)exec));
    return MPX_OK;
}

int mpx_runtime_info(char* buf, size_t cap) {
    int rt = 0, drv = 0, nv = 0;
    (void)hipRuntimeGetVersion(&rt);
    (void)hipDriverGetVersion(&drv);
    (void)ncclGetVersion(&nv);
    (void)hipGetLastError();
    auto path_of = [](const void* sym) {
        Dl_info info{};
        return (sym && dladdr(sym, &info) && info.dli_fname) ? std::string(info.dli_fname)
                                                              : std::string("?");
    };
    const std::string s = "{\"hip_runtime\": " + std::to_string(rt) +
                          ", \"hip_driver\": " + std::to_string(drv) +
                          ", \"rccl\": " + std::to_string(nv) + ", \"hip_path\": \"" +
                          path_of((const void*)&hipRuntimeGetVersion) + "\", \"rccl_path\": \"" +
                          path_of((const void*)&ncclAllReduce) + "\"}";
    if (buf && cap) {
        const size_t k = std::min(cap - 1, s.size());
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return (int)s.size();
}

}  // extern "C"

// store.cpp — the C ABI of store assembly (mpx_store_commands[_reserve|_dev],
// mpx_store_compact[_reserve|_dev], include/mpx.h) over the launchers of store.hip: validation,
// then, for the host forms, Stage staging around the _dev forms, like the other host-pointer entry
// points (engine.cpp, order.cpp, client.cpp, replies.cpp, execute.cpp). The command sources' checks,
// the pre-check of an item's commands and their staging are cmd_src_host.hpp's, shared with record.cpp.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "cmd_src_host.hpp"
#include "engine_host.hpp"
#include "kernels.hpp"

using namespace mpx_host;

namespace {

size_t item_bytes(const mpx_store_batch* b) {
    return b->kind == MPX_SC_SENDS ? sizeof(mpx_accept_send) : sizeof(mpx_accept_msg);
}

int arena_args(mpx_engine* e, const mpx_store_arena* a) {
    if (!a || !a->used || (a->cap && (!a->op || !a->key || !a->val)))
        return fail(e, MPX_E_INVAL, "null argument");
    return MPX_OK;
}

// what both forms of mpx_store_commands check
int store_args(mpx_engine* e, const mpx_store_batch* b, const mpx_store_arena* arena,
               const mpx_inst_cmds* inst, const void* res) {
    if (!b || !res) return fail(e, MPX_E_INVAL, "null argument");
    CK(arena_args(e, arena));
    if (b->kind != MPX_SC_MSGS && b->kind != MPX_SC_SENDS) return fail(e, MPX_E_INVAL, "unknown kind");
    if (b->flags & ~MPX_SC_GENERAL) return fail(e, MPX_E_INVAL, "unknown flags");
    if (b->reserved) return fail(e, MPX_E_INVAL, "reserved is not 0");
    if (!b->src || b->n_src < 1 || b->n_src > MPX_SC_MAX_SRC || (b->kind == MPX_SC_SENDS && b->n_src != 1))
        return fail(e, MPX_E_INVAL, "n_src outside [1, MPX_SC_MAX_SRC] (MPX_SC_SENDS: 1)");
    if ((uint64_t)b->n >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 items or more");
    if (b->n && (!b->items || (b->kind == MPX_SC_MSGS && !b->effect) || (b->n_inst && !inst)))
        return fail(e, MPX_E_INVAL, "null argument");
    if (b->kind == MPX_SC_MSGS && b->n_src > 1 && !b->perm)
        return fail(e, MPX_E_INVAL, "more than one source needs perm");
    uint64_t recs;
    CK(src_args(e, b->src, b->n_src, &recs));
    if (recs < b->n) return fail(e, MPX_E_INVAL, "the sources hold fewer records than n");
    return MPX_OK;
}

bool misaligned(const mpx_store_arena* a) {
    return (((uintptr_t)a->key | (uintptr_t)a->val | (uintptr_t)a->used) & 7) != 0;
}

int store_grow(mpx_engine* e, size_t n) {
    GROW(e, e->st_work, mpx::store_work_bytes(n));
    return MPX_OK;
}

// [p, p + n * size) of two arrays overlap
bool overlap(const void* p, size_t n, const void* q, size_t m, size_t size) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return n && m && a < b + m * size && b < a + n * size;
}

// what both forms of mpx_store_compact check
int compact_args(mpx_engine* e, const mpx_inst_cmds* inst, size_t n_inst, const mpx_store_arena* from,
                 const mpx_store_arena* to, const void* res) {
    if (!res || (n_inst && !inst)) return fail(e, MPX_E_INVAL, "null argument");
    CK(arena_args(e, from));
    CK(arena_args(e, to));
    if ((uint64_t)n_inst >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 window slots or more");
    if (overlap(from->op, from->cap, to->op, to->cap, 1) ||
        overlap(from->key, from->cap, to->key, to->cap, 8) ||
        overlap(from->val, from->cap, to->val, to->cap, 8) ||
        overlap(from->key, from->cap, to->val, to->cap, 8) ||
        overlap(from->val, from->cap, to->key, to->cap, 8) || from->used == to->used)
        return fail(e, MPX_E_INVAL, "from and to overlap");
    return MPX_OK;
}

}  // namespace

extern "C" {

int mpx_store_commands_reserve(mpx_engine* e, size_t max_n) {
    if (!e) return MPX_E_INVAL;
    if ((uint64_t)max_n >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 items or more");
    return reserve(e, e->st_work, mpx::store_work_bytes(max_n));
}

int mpx_store_compact_reserve(mpx_engine* e, size_t max_n_inst) {
    if (!e) return MPX_E_INVAL;
    if ((uint64_t)max_n_inst >= 0xFFFFFFFFull)
        return fail(e, MPX_E_UNSUPPORTED, "2^32-1 window slots or more");
    return reserve(e, e->st_work, mpx::store_work_bytes(max_n_inst));
}

int mpx_store_commands_dev(mpx_engine* e, const mpx_store_batch* b, const mpx_store_arena* arena,
                           mpx_inst_cmds* d_inst, mpx_store_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(store_args(e, b, arena, d_inst, d_res));
    uintptr_t a8 = (uintptr_t)d_res | (uintptr_t)b->d_n;
    for (size_t s = 0; s < b->n_src; ++s)
        a8 |= (uintptr_t)b->src[s].cmd_off | (uintptr_t)b->src[s].key | (uintptr_t)b->src[s].val;
    if ((((uintptr_t)b->items | (uintptr_t)d_inst) & 15) || (a8 & 7) || misaligned(arena) ||
        ((uintptr_t)b->perm & 3))
        return fail(e, MPX_E_INVAL, "mpx_store_commands_dev: items and d_inst must be 16-byte "
                                    "aligned, the 8-byte arrays, used, d_n and d_res 8, perm 4");
    CK(reserved(e, e->st_work, b->n ? mpx::store_work_bytes(b->n) : 0, "mpx_store_commands_dev",
                "mpx_store_commands_reserve(max_n)"));
    HIPCHK(e, mpx::launch_store_commands(b, arena, d_inst, d_res, e->st_work.p, e->st_work.cap,
                                         e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_store_commands(mpx_engine* e, const mpx_store_batch* b, const mpx_store_arena* arena,
                       mpx_inst_cmds* inst, mpx_store_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(store_args(e, b, arena, inst, res));
    if (b->d_n) return fail(e, MPX_E_INVAL, "d_n is for mpx_store_commands_dev");
    const uint64_t used = *arena->used;
    if (used > arena->cap) return fail(e, MPX_E_INVAL, "*used is past cap");
    // the device kernels report these through the error word; here they answer before any launch:
    // the storing items, judged in array order as the kernels judge each
    const SrcIndex idx(b->src, b->n_src);
    CK(perm_args(e, idx, b->perm, b->n));
    bool any = false;
    int32_t prev = 0;
    uint32_t prev_len = 0;
    uint64_t total = 0, rel_lo = 0, rel_hi = 0;
    for (size_t i = 0; i < b->n; ++i) {
        int32_t instance;
        uint64_t len;
        if (b->kind == MPX_SC_MSGS) {
            const mpx_accept_msg& m = ((const mpx_accept_msg*)b->items)[i];
            if (!(b->effect[i] & b->store_mask) || m.value_id == MPX_VALUE_KEEP) continue;
            instance = m.instance;
            CK(resolve_msg(e, idx, b->perm ? b->perm[i] : i, m.value_id, "storing", &len));
        } else {
            const mpx_accept_send& x = ((const mpx_accept_send*)b->items)[i];
            if (!(x.flags & (MPX_PH_ACCEPT | MPX_PH_PREPARE))) continue;
            instance = x.instance;
            CK(resolve_send(e, b->src[0], x, "storing", &len));
        }
        const int64_t rel = (int64_t)instance - b->inst_base;
        if (rel < 0 || (uint64_t)rel >= b->n_inst)
            return fail(e, MPX_E_NIL_INSTANCE, "a storing item names an instance outside the window");
        if (any && prev == instance) total -= prev_len;  // superseded
        rel_lo = any ? std::min<uint64_t>(rel_lo, rel) : (uint64_t)rel;
        rel_hi = any ? std::max<uint64_t>(rel_hi, rel) : (uint64_t)rel;
        any = true, prev = instance, prev_len = (uint32_t)len;
        total += len;
        if (total >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 commands or more");
    }
    CK(begin(e));
    if (b->n) CK(store_grow(e, b->n));
    const bool fits = total <= arena->cap - used;
    const size_t n_out = fits ? (size_t)total : 0, n_span = any ? (size_t)(rel_hi - rel_lo + 1) : 0;
    Stage L(e);
    const Slot s_items = L.add(b->n * item_bytes(b)), s_eff = L.add(b->effect ? b->n : 0),
               s_perm = L.add(b->perm ? b->n * sizeof(uint32_t) : 0),
               s_op = L.add(n_out), s_key = L.add(n_out * sizeof(int64_t)),
               s_val = L.add(n_out * sizeof(int64_t)), s_inst = L.add(n_span * sizeof(mpx_inst_cmds)),
               s_used = L.add(sizeof(uint64_t)), s_res = L.add(sizeof(mpx_store_result));
    StagedSrcs srcs(L, b->src, b->n_src);
    CK(L.commit());
    CK(L.in(s_items, b->items));
    if (b->effect) CK(L.in(s_eff, b->effect));
    if (b->perm) CK(L.in(s_perm, b->perm));
    if (n_span) CK(L.in(s_inst, inst + rel_lo));
    CK(L.in(s_used, arena->used));
    CK(srcs.in());
    mpx_store_batch d = *b;
    d.items = L.at<char>(s_items, b->n ? b->items : nullptr);
    d.effect = L.at<uint8_t>(s_eff, b->effect);
    d.perm = L.at<uint32_t>(s_perm, b->perm);
    d.src = srcs.dev();
    // the arena's appended range and the window's written span alone are staged: the kernels index
    // them from the arena's and the window's starts
    mpx_store_arena da{};
    da.op = L.at<uint8_t>(s_op) - used, da.key = L.at<int64_t>(s_key) - used;
    da.val = L.at<int64_t>(s_val) - used, da.cap = arena->cap, da.used = L.at<uint64_t>(s_used);
    mpx_inst_cmds* const d_inst = L.at<mpx_inst_cmds>(s_inst) - rel_lo;
    CK(mpx_store_commands_dev(e, &d, &da, d_inst, L.at<mpx_store_result>(s_res), e->stream));
    if (fits) {
        CK(L.out(s_op, arena->op + used));
        CK(L.out(s_key, arena->key + used));
        CK(L.out(s_val, arena->val + used));
        if (n_span) CK(L.out(s_inst, inst + rel_lo));
        CK(L.out(s_used, arena->used));
    }
    CK(L.out(s_res, res));
    return finish(e);
}

int mpx_store_compact_dev(mpx_engine* e, mpx_inst_cmds* d_inst, size_t n_inst,
                          const mpx_store_arena* from, const mpx_store_arena* to,
                          mpx_store_result* d_res, void* stream) {
    if (!e) return MPX_E_INVAL;
    CK(compact_args(e, d_inst, n_inst, from, to, d_res));
    if (((uintptr_t)d_inst & 15) || ((uintptr_t)d_res & 7) || misaligned(from) || misaligned(to))
        return fail(e, MPX_E_INVAL, "mpx_store_compact_dev: d_inst must be 16-byte aligned, the "
                                    "8-byte arrays, used and d_res 8");
    CK(reserved(e, e->st_work, n_inst ? mpx::store_work_bytes(n_inst) : 0, "mpx_store_compact_dev",
                "mpx_store_compact_reserve(max_n_inst)"));
    HIPCHK(e, mpx::launch_store_compact(d_inst, n_inst, from, to, d_res, e->st_work.p, e->st_work.cap,
                                        e->d_err, pick(e, stream)));
    return MPX_OK;
}

int mpx_store_compact(mpx_engine* e, mpx_inst_cmds* inst, size_t n_inst, const mpx_store_arena* from,
                      const mpx_store_arena* to, mpx_store_result* res) {
    if (!e) return MPX_E_INVAL;
    CK(compact_args(e, inst, n_inst, from, to, res));
    const uint64_t f_used = *from->used;
    if (f_used > from->cap) return fail(e, MPX_E_INVAL, "*from->used is past cap");
    uint64_t total = 0;
    for (size_t i = 0; i < n_inst; ++i) {
        if (!(inst[i].flags & MPX_IC_HAS_CMDS)) continue;
        if (inst[i].first_cmd > f_used || inst[i].n_cmds > f_used - inst[i].first_cmd ||
            inst[i].n_cmds == 0xFFFFFFFFu)
            return fail(e, MPX_E_INVAL, "an instance's command range leaves [0, *from->used)");
        total += inst[i].n_cmds;
        if (total >= 0xFFFFFFFFull) return fail(e, MPX_E_UNSUPPORTED, "2^32-1 commands or more");
    }
    CK(begin(e));
    if (n_inst) CK(store_grow(e, n_inst));
    const bool fits = total <= to->cap;
    const size_t n_out = fits ? (size_t)total : 0, n_in = (size_t)f_used;
    Stage L(e);
    const Slot s_inst = L.add(n_inst * sizeof(mpx_inst_cmds)), s_fop = L.add(n_in),
               s_fkey = L.add(n_in * sizeof(int64_t)), s_fval = L.add(n_in * sizeof(int64_t)),
               s_fused = L.add(sizeof(uint64_t)), s_op = L.add(n_out),
               s_key = L.add(n_out * sizeof(int64_t)), s_val = L.add(n_out * sizeof(int64_t)),
               s_used = L.add(sizeof(uint64_t)), s_res = L.add(sizeof(mpx_store_result));
    CK(L.commit());
    CK(L.in(s_inst, inst));
    CK(L.in(s_fop, from->op));
    CK(L.in(s_fkey, from->key));
    CK(L.in(s_fval, from->val));
    CK(L.in(s_fused, from->used));
    const mpx_store_arena df{L.at<uint8_t>(s_fop), L.at<int64_t>(s_fkey), L.at<int64_t>(s_fval), n_in,
                             L.at<uint64_t>(s_fused)};
    const mpx_store_arena dt{L.at<uint8_t>(s_op), L.at<int64_t>(s_key), L.at<int64_t>(s_val), to->cap,
                             L.at<uint64_t>(s_used)};
    CK(mpx_store_compact_dev(e, L.at<mpx_inst_cmds>(s_inst, inst), n_inst, &df, &dt,
                             L.at<mpx_store_result>(s_res), e->stream));
    if (fits) {
        CK(L.out(s_op, to->op));
        CK(L.out(s_key, to->key));
        CK(L.out(s_val, to->val));
        CK(L.out(s_inst, inst));
        CK(L.out(s_used, to->used));
    }
    CK(L.out(s_res, res));
    return finish(e);
}

}  // extern "C"

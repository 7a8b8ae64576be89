// tests/san/store_stub.cpp — TEST INFRASTRUCTURE ONLY: host-memory stand-ins for the launchers of
// store.hip, for the CPU build of engine.cpp + store.cpp over the stub runtime (hip_stub.cpp, where a
// "device" pointer is a host pointer). Like execute_stub.cpp these really do the work (the storing
// items, their winners, the append and the slots; the compaction), sequentially and with the device
// form's treatment of faulty items, so the driver can compare what comes back through the staging of
// the host forms with what it expects. They read every input byte the kernels may read, write exactly
// the extents the kernels may write and scribble over the scratch they were promised, so a slot or a
// scratch size that is too small faults under ASan or shows in the results.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../minpaxos_amd/csrc/kernels.hpp"

namespace mpx {

uint64_t store_work_bytes(uint64_t n, Carver&& c) {
    (void)c.take<char>(32);
    (void)c.take<char>(28 * n + 24);
    (void)c.take<char>(n / 64 + 64);
    return c.bytes();
}

namespace {
unsigned touch(const void* p, uint64_t bytes) {
    unsigned sum = 0;
    for (uint64_t i = 0; i < bytes; ++i) sum += ((const uint8_t*)p)[i];
    return sum;
}
}  // namespace

hipError_t launch_store_commands(const mpx_store_batch* b, const mpx_store_arena* arena,
                                 mpx_inst_cmds* inst, mpx_store_result* res, void* work,
                                 uint64_t work_bytes, uint32_t* err, hipStream_t) {
    const uint64_t n = b->n;
    if (n >= 0xFFFFFFFFull || !b->n_src || b->n_src > MPX_SC_MAX_SRC) return hipErrorInvalidValue;
    uint64_t cmds = 0, rec_end[MPX_SC_MAX_SRC], recs = 0;
    unsigned sum = 0;
    for (size_t s = 0; s < b->n_src; ++s) {
        const mpx_store_src& x = b->src[s];
        cmds += x.n_cmds, rec_end[s] = recs += x.n_recs;
        // every byte of the sources is read (a staging slot that is too small faults here)
        sum += touch(x.op, x.n_cmds) + touch(x.key, 8 * x.n_cmds) + touch(x.val, 8 * x.n_cmds);
        if (x.n_frames) sum += touch(x.cmd_off, 8 * (x.n_frames + 1));
    }
    const bool one = (!(b->flags & MPX_SC_GENERAL) && n <= MPX_SC_ONE_LAUNCH_ITEMS &&
                      cmds <= MPX_SC_ONE_LAUNCH_CMDS) || !n;
    if (!one) {
        const uint64_t need = store_work_bytes(n);
        if (work_bytes < need) return hipErrorInvalidValue;
        memset(work, 0xEE, need);
    }
    const uint64_t n_eff = b->d_n ? std::min<uint64_t>(*b->d_n, n) : n;
    const size_t stride = b->kind == MPX_SC_SENDS ? sizeof(mpx_accept_send) : sizeof(mpx_accept_msg);
    sum += touch(b->items, n_eff * stride);
    if (b->effect) sum += touch(b->effect, n_eff);
    if (b->perm) sum += touch(b->perm, 4 * n_eff);
    struct W {
        int32_t instance;
        uint64_t src, lo, len;
    };
    std::vector<W> storing;
    for (uint64_t i = 0; i < n_eff; ++i) {
        W w{0, 0, 0, 0};
        if (b->kind == MPX_SC_MSGS) {
            const mpx_accept_msg& m = ((const mpx_accept_msg*)b->items)[i];
            if (!(b->effect[i] & b->store_mask) || m.value_id == MPX_VALUE_KEEP) continue;
            w.instance = m.instance;
            const uint64_t p = b->perm ? b->perm[i] : i;
            if (p >= recs) {
                *err |= kErrInval;
                continue;
            }
            while (w.src + 1 < b->n_src && p >= rec_end[w.src]) ++w.src;
            const mpx_store_src& x = b->src[w.src];
            if (m.value_id >= x.n_frames) {
                *err |= kErrInval;
                continue;
            }
            w.lo = x.cmd_off[m.value_id];
            const uint64_t hi = x.cmd_off[m.value_id + 1];
            if (hi < w.lo || hi > x.n_cmds || hi - w.lo >= 0xFFFFFFFFull) {
                *err |= kErrInval;
                continue;
            }
            w.len = hi - w.lo;
        } else {
            const mpx_accept_send& x = ((const mpx_accept_send*)b->items)[i];
            if (!(x.flags & (MPX_PH_ACCEPT | MPX_PH_PREPARE))) continue;
            w.instance = x.instance, w.lo = x.first_cmd, w.len = x.n_cmds;
            if (w.lo > b->src[0].n_cmds || w.len > b->src[0].n_cmds - w.lo || w.len == 0xFFFFFFFFull) {
                *err |= kErrInval;
                continue;
            }
        }
        const int64_t rel = (int64_t)w.instance - b->inst_base;
        if (rel < 0 || (uint64_t)rel >= b->n_inst) {
            *err |= kErrNil;
            continue;
        }
        storing.push_back(w);
    }
    std::vector<W> won;
    for (size_t k = 0; k < storing.size(); ++k)
        if (k + 1 == storing.size() || storing[k + 1].instance != storing[k].instance) won.push_back(storing[k]);
    uint64_t total = 0;
    for (const W& w : won) total += w.len;
    const uint64_t used = *arena->used;
    const bool bad = used > arena->cap, full = bad || total > arena->cap - used;
    if (bad) *err |= kErrInval;
    *res = mpx_store_result{won.size(), total, storing.size() - won.size(), full ? (uint64_t)MPX_SC_FULL : 0};
    if (full) return hipSuccess;
    uint64_t at = used;
    for (const W& w : won) {
        const mpx_store_src& x = b->src[w.src];
        for (uint64_t j = 0; j < w.len; ++j) {
            arena->op[at + j] = x.op[w.lo + j] + (uint8_t)(sum & 0u);
            arena->key[at + j] = x.key[w.lo + j];
            arena->val[at + j] = x.val[w.lo + j];
        }
        inst[(int64_t)w.instance - b->inst_base] = mpx_inst_cmds{at, (uint32_t)w.len, MPX_IC_HAS_CMDS};
        at += w.len;
    }
    *arena->used = at;
    return hipSuccess;
}

hipError_t launch_store_compact(mpx_inst_cmds* inst, uint64_t n_inst, const mpx_store_arena* from,
                                const mpx_store_arena* to, mpx_store_result* res, void* work,
                                uint64_t work_bytes, uint32_t* err, hipStream_t) {
    if (n_inst >= 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n_inst) {
        const uint64_t need = store_work_bytes(n_inst);
        if (work_bytes < need) return hipErrorInvalidValue;
        memset(work, 0xEE, need);
    }
    const uint64_t bound = std::min<uint64_t>(*from->used, from->cap);
    unsigned sum = touch(inst, n_inst * sizeof(mpx_inst_cmds)) + touch(from->op, bound) +
                   touch(from->key, 8 * bound) + touch(from->val, 8 * bound);
    std::vector<mpx_inst_cmds> rows(inst, inst + n_inst);
    uint64_t total = 0, flagged = 0;
    for (mpx_inst_cmds& x : rows) {
        if (!(x.flags & MPX_IC_HAS_CMDS)) continue;
        if (x.first_cmd > bound || x.n_cmds > bound - x.first_cmd || x.n_cmds == 0xFFFFFFFFu)
            *err |= kErrInval, x.first_cmd = 0, x.n_cmds = 0;
        total += x.n_cmds, ++flagged;
    }
    const bool full = total > to->cap;
    *res = mpx_store_result{flagged, total, 0, full ? (uint64_t)MPX_SC_FULL : 0};
    if (full) return hipSuccess;
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_inst; ++i) {
        const mpx_inst_cmds& x = rows[i];
        if (!(x.flags & MPX_IC_HAS_CMDS)) continue;
        for (uint64_t j = 0; j < x.n_cmds; ++j) {
            to->op[at + j] = from->op[x.first_cmd + j] + (uint8_t)(sum & 0u);
            to->key[at + j] = from->key[x.first_cmd + j];
            to->val[at + j] = from->val[x.first_cmd + j];
        }
        inst[i] = mpx_inst_cmds{at, x.n_cmds, MPX_IC_HAS_CMDS};
        at += x.n_cmds;
    }
    *to->used = at;
    return hipSuccess;
}

}  // namespace mpx
